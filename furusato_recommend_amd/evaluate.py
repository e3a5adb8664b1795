"""Recall@k / NDCG@k evaluation (Trainer.test, trainer.py:115-187).

The layer-mean embeddings are propagated ONCE per evaluation with the HIP
engine (the reference re-propagates per 10 000-user batch through
getUsersRating, model/lgcn.py:120-125).  Per batch of users, for a model
with ``eval_embeddings`` (LightGCN, MF) and k <= 32: mirec_score_topk streams
the scores U_b · Iᵀ through MFMA tiles straight into per-user top-k
candidates, the train positives at -1024 (trainer.py:132-138) — the
[batch, M] rating matrix is never written (MF's sigmoid ratings rank like
its raw scores: sigmoid is monotone).  Otherwise (k > 32, or a width
outside STREAM_DIMS): rating = U_b · Iᵀ (library GEMM, as the reference's
torch.matmul), then mirec_topk_masked masks in place and selects.  Metric
sums on the host with the reference formulas (metric.py:60-103).

evaluate_ranked is the full-rank form: mirec_score_rank counts, on the same
score stream, the exact rank of every test item among its user's non-train
items, which gives the same four metrics at any k plus MRR and AUC
(DESIGN.md §20).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from .metric import test_one_batch


@torch.no_grad()
def topk_masked(rating: torch.Tensor, users: torch.Tensor, graph, k: int,
                mask: bool = True):
    """In-place mask of train positives + top-k of each rating row (HIP)."""
    if rating.dtype != torch.float32 or not rating.is_contiguous():
        raise ValueError("rating must be contiguous float32")
    n_eval, m = rating.shape
    users = users.to(torch.int32).contiguous()
    idx = torch.empty(n_eval, k, dtype=torch.int32, device=rating.device)
    val = torch.empty(n_eval, k, dtype=torch.float32, device=rating.device)
    check(lib.mirec_topk_masked(rating.data_ptr(), n_eval, m, users.data_ptr(),
                                graph.csr_ptr() if mask else None, graph.n_users, int(k),
                                idx.data_ptr(), val.data_ptr(), _lib.stream_handle()),
          "topk_masked")
    return val, idx


STREAM_DIMS = (16, 32, 64, 128, 256)
STREAM_MAX_K = 32


@torch.no_grad()
def score_topk(user_rows: torch.Tensor, items: torch.Tensor, users: torch.Tensor, graph,
               k: int, mask: bool = True):
    """Top-k of user_rows · itemsᵀ per row with the users' train positives
    at -1024, streamed (mirec_score_topk): (values, item ids) [n, k]."""
    n, d = user_rows.shape
    user_rows, items = user_rows.contiguous(), items.contiguous()
    users = users.to(torch.int32).contiguous()
    idx = torch.empty(n, k, dtype=torch.int32, device=user_rows.device)
    val = torch.empty(n, k, dtype=torch.float32, device=user_rows.device)
    ws = torch.empty(max(int(lib.mirec_score_topk_workspace(n, items.shape[0], k)), 1),
                     dtype=torch.uint8, device=user_rows.device)
    check(lib.mirec_score_topk(user_rows.data_ptr(), n, items.data_ptr(), items.shape[0], d,
                               users.data_ptr(), graph.csr_ptr() if mask else None,
                               graph.n_users, int(k), idx.data_ptr(), val.data_ptr(),
                               ws.data_ptr(), ws.numel(), _lib.stream_handle()), "score_topk")
    return val, idx


@torch.no_grad()
def evaluate(model, test_dict: dict, topks=(10, 20), batch: int = 10000,
             return_topk: bool = False, stream: bool | None = None):
    users = np.array(sorted(test_dict.keys()), dtype=np.int64)
    res = {m: np.zeros(len(topks)) for m in ("precision", "recall", "ndcg", "hr")}
    if users.size == 0:
        return res
    kmax = max(topks)
    if getattr(model, "device", None) is not None and torch.device(model.device).type == "cpu":
        return _evaluate_host(model, test_dict, users, topks, batch, return_topk, res)
    emb = None
    if stream is not False and hasattr(model, "eval_embeddings") and kmax <= STREAM_MAX_K:
        emb = model.eval_embeddings()   # propagates once
        if emb[0].shape[1] not in STREAM_DIMS:
            emb = None
    if emb is None:
        ratings = model.eval_ratings()   # propagates once, returns users -> rating rows
    tops = []
    for i in range(0, len(users), batch):
        bu = torch.from_numpy(users[i:i + batch]).to(model.device)
        if emb is not None:
            _, top = score_topk(emb[0][bu], emb[1], bu, model.graph, kmax)
        else:
            rating = ratings(bu).contiguous()
            _, top = topk_masked(rating, bu, model.graph, kmax)
        top = top.cpu().numpy()
        if return_topk:
            tops.append(top)
        gt = [test_dict[int(u)] for u in users[i:i + batch]]
        r = test_one_batch(top, gt, topks)
        for m in res:
            res[m] += r[m]
    for m in res:
        res[m] /= float(len(users))
    if return_topk:
        return res, np.concatenate(tops)
    return res


@torch.no_grad()
def _evaluate_host(model, test_dict, users, topks, batch, return_topk, res):
    """A CPU model (configuration C1): the reference's own arithmetic on the
    host — rating = model.eval_ratings() rows, the train positives set to
    -1024, torch.topk (trainer.py:115-138) — and the same metric sums."""
    kmax = max(topks)
    ratings = model.eval_ratings()
    g = model.graph
    rp, col, nu = g.rowptr_host, g.col_host, g.n_users
    tops = []
    for i in range(0, len(users), batch):
        bu = users[i:i + batch]
        rating = ratings(torch.from_numpy(bu)).clone()
        for r, u in enumerate(bu.tolist()):
            items = col[rp[u]:rp[u + 1]].astype(np.int64) - nu
            rating[r, torch.from_numpy(items[(items >= 0) & (items < rating.shape[1])])] = -1024.0
        top = torch.topk(rating, kmax).indices.numpy()
        if return_topk:
            tops.append(top)
        r_ = test_one_batch(top, [test_dict[int(u)] for u in bu], topks)
        for m in res:
            res[m] += r_[m]
    for m in res:
        res[m] /= float(len(users))
    if return_topk:
        return res, np.concatenate(tops)
    return res


# ---------------------------------------------------------------- exact ranks
@torch.no_grad()
def score_rank(user_rows: torch.Tensor, items: torch.Tensor, users: torch.Tensor, tptr,
               targets: torch.Tensor, graph, mask: bool = True):
    """Exact rank counts of held-out (user, item) pairs, streamed
    (mirec_score_rank).  Row r of ``user_rows`` (user id
    users[r]) owns the item ids targets[tptr[r] : tptr[r + 1]], distinct per
    user.  Returns (score, gt, eq, eq_lower, masked), one entry per pair:
    with s_j = <user_rows[r], items[j]> over the items J that are not train
    positives of the user (``mask=False``: all items), gt = #{s_j > s_t},
    eq = #{s_j == s_t} (t included), eq_lower = #{j < t : s_j == s_t}, and
    masked = 1 for a target outside J (its counts are then meaningless).
    rank = 1 + gt + eq_lower is the target's place in score_topk's order."""
    n, d = user_rows.shape
    if d not in STREAM_DIMS:
        raise ValueError(f"score_rank: width {d} not in {STREAM_DIMS}")
    dev = user_rows.device
    user_rows, items = user_rows.contiguous(), items.contiguous()
    users = users.to(device=dev, dtype=torch.int32).contiguous()
    tptr = np.ascontiguousarray(torch.as_tensor(tptr).cpu().numpy(), dtype=np.int64)
    if tptr.shape != (n + 1,) or users.shape != (n,):
        raise ValueError("score_rank: users [n] and tptr [n + 1] must match user_rows [n, d]")
    targets = torch.as_tensor(targets).to(device=dev, dtype=torch.int32).contiguous()
    nt = int(targets.numel())
    if int(tptr[-1]) != nt:
        raise ValueError("score_rank: tptr[-1] must be the number of targets")
    score = torch.empty(nt, dtype=torch.float32, device=dev)
    gt, eq, eql = (torch.empty(nt, dtype=torch.int32, device=dev) for _ in range(3))
    masked = torch.empty(nt, dtype=torch.uint8, device=dev)
    m = items.shape[0]
    ws = torch.empty(max(int(lib.mirec_score_rank_workspace(n, nt, m, d)), 16),
                     dtype=torch.uint8, device=dev)
    check(lib.mirec_score_rank(user_rows.data_ptr(), n, items.data_ptr(), m, d,
                               users.data_ptr(), tptr.ctypes.data, targets.data_ptr(),
                               graph.csr_ptr() if mask else None, graph.n_users,
                               score.data_ptr(), gt.data_ptr(), eq.data_ptr(), eql.data_ptr(),
                               masked.data_ptr(), ws.data_ptr(), ws.numel(),
                               _lib.stream_handle()), "score_rank")
    return score, gt, eq, eql, masked


def _train_pairs(graph, users: np.ndarray, m_items: int):
    """(row in ``users``, item) of every distinct train positive, host."""
    rp, col = graph.rowptr_host, graph.col_host
    beg = rp[users]
    cnt = rp[users + 1] - beg
    rows = np.repeat(np.arange(len(users)), cnt)
    off = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    it = col[np.repeat(beg, cnt) + off].astype(np.int64) - graph.n_users
    ok = (it >= 0) & (it < m_items)
    key = np.unique(rows[ok] * int(m_items) + it[ok])
    return key // int(m_items), key % int(m_items)


@torch.no_grad()
def _score_rank_dense(user_rows, items, users: np.ndarray, tptr, targets: np.ndarray, graph,
                      mask: bool = True):
    """score_rank's definitions on a dense [n, M] rating block in torch: the
    path of a CPU model or of a width outside STREAM_DIMS (as _evaluate_host
    and the k > 32 path of evaluate())."""
    dev = user_rows.device
    s = user_rows @ items.t()
    n, m = s.shape
    train = torch.zeros(n, m, dtype=torch.bool, device=dev)
    if mask:
        r, it = _train_pairs(graph, np.asarray(users, dtype=np.int64), m)
        train[torch.from_numpy(r).to(dev), torch.from_numpy(it).to(dev)] = True
    tptr = np.asarray(tptr, dtype=np.int64)
    slot = torch.from_numpy(np.repeat(np.arange(n), np.diff(tptr))).to(dev)
    t = torch.from_numpy(np.asarray(targets, dtype=np.int64)).to(dev)
    nt = int(t.numel())
    score = s[slot, t]
    masked = train[slot, t].to(torch.uint8)
    gt = torch.empty(nt, dtype=torch.int32, device=dev)
    eq, eql = torch.empty_like(gt), torch.empty_like(gt)
    ids = torch.arange(m, device=dev)[None, :]
    step = max(1, (1 << 24) // m)
    for a in range(0, nt, step):
        rows = slot[a:a + step]
        sr, live = s[rows], ~train[rows]
        th = score[a:a + step, None]
        tie = (sr == th) & live
        gt[a:a + step] = ((sr > th) & live).sum(1)
        eq[a:a + step] = tie.sum(1)
        eql[a:a + step] = (tie & (ids < t[a:a + step, None])).sum(1)
    return score, gt, eq, eql, masked


@torch.no_grad()
def evaluate_ranked(model, test_dict: dict, topks=(10, 20), batch: int = 10000,
                    return_ranks: bool = False):
    """Full-rank evaluation: the exact rank of every test
    item among its user's non-train items, from one propagation
    (``eval_embeddings``) and one score_rank call per batch of users — no
    [batch, M] rating matrix and no limit on k.  Returns precision / recall /
    ndcg / hr at every k of ``topks`` (evaluate()'s values, for any k), the
    mean reciprocal rank "mrr" and the per-user "auc" (metric.rank_metrics);
    with ``return_ranks`` also "ranks": the rank of every (user, test item)
    in sorted(test_dict) order, each user's items ascending, 0 for a test
    item that is a train positive.  A CPU model or a width outside
    STREAM_DIMS ranks a dense per-batch rating block in torch."""
    from .metric import rank_metrics
    users = np.array(sorted(test_dict.keys()), dtype=np.int64)
    res = {m: np.zeros(len(topks)) for m in ("precision", "recall", "ndcg", "hr")}
    res["mrr"], res["auc"] = 0.0, 0.0
    if return_ranks:
        res["ranks"] = np.zeros(0, dtype=np.int64)
    if users.size == 0:
        return res
    if not hasattr(model, "eval_embeddings"):
        raise TypeError("evaluate_ranked needs a model with eval_embeddings()")
    U, I = model.eval_embeddings()   # propagates once
    m_items = int(I.shape[0])
    streamed = U.device.type != "cpu" and U.shape[1] in STREAM_DIMS
    g = model.graph
    auc_users, ranks = 0, []
    for i in range(0, len(users), batch):
        bu = users[i:i + batch]
        lists = [np.unique(np.asarray(test_dict[int(u)], dtype=np.int64)) for u in bu]
        n_gt = np.array([len(test_dict[int(u)]) for u in bu], dtype=np.int64)
        tptr = np.zeros(len(bu) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in lists], out=tptr[1:])
        targets = np.concatenate(lists) if lists else np.zeros(0, np.int64)
        but = torch.from_numpy(bu).to(U.device)
        if streamed:
            out = score_rank(U[but], I, but, tptr, torch.from_numpy(targets), g)
        else:
            out = _score_rank_dense(U[but], I, bu, tptr, targets, g)
        score, gt, eq, eql, masked = (x.cpu().numpy() for x in out)
        n_train = np.bincount(_train_pairs(g, bu, m_items)[0], minlength=len(bu))
        r = rank_metrics(tptr, score, gt, eq, eql, masked, n_gt, n_train, m_items, topks,
                         return_ranks)
        for m in ("precision", "recall", "ndcg", "hr", "mrr", "auc"):
            res[m] += r[m]
        auc_users += r["auc_users"]
        if return_ranks:
            ranks.append(r["ranks"])
    for m in ("precision", "recall", "ndcg", "hr"):
        res[m] /= float(len(users))
    res["mrr"] /= float(len(users))
    res["auc"] = res["auc"] / auc_users if auc_users else 0.0
    if return_ranks:
        res["ranks"] = np.concatenate(ranks)
    return res
