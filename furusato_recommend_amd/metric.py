"""Top-k ranking metrics with the reference's exact semantics.

utils.py:40-48 (getLabel), metric.py:60-103 (RecallPrecision_ATk, NDCGatK_r):
recall sums hits/(|gt| + 1e-6) per user, precision sums hits/k, NDCG uses the
binary-relevance DCG with an ideal DCG over min(k, |gt|) positions.  Sums are
per batch; the caller divides by the number of evaluated users
(trainer.py:166-170).  rank_metrics computes the same four from exact ranks
(any k) and adds the mean reciprocal rank and the per-user AUC.
"""
from __future__ import annotations

import numpy as np


def getLabel(test_data, pred_data) -> np.ndarray:
    r = np.zeros((len(test_data), pred_data.shape[1] if len(test_data) else 0))
    for i, gt in enumerate(test_data):
        r[i] = np.isin(pred_data[i], np.asarray(list(gt)))
    return r.astype("float")


def RecallPrecision_ATk(test_data, r, k):
    right_pred = r[:, :k].sum(1)
    recall_n = np.array([len(test_data[i]) for i in range(len(test_data))])
    recall = np.sum(right_pred / (recall_n + 1e-6))
    precis = np.sum(right_pred) / k
    hr = np.sum(right_pred >= 1)
    return {"recall": recall, "precision": precis, "hr": hr}


def NDCGatK_r(test_data, r, k):
    assert len(r) == len(test_data)
    pred_data = r[:, :k]
    test_matrix = np.zeros((len(pred_data), k))
    for i, items in enumerate(test_data):
        length = k if k <= len(items) else len(items)
        test_matrix[i, :length] = 1
    idcg = np.sum(test_matrix * 1.0 / np.log2(np.arange(2, k + 2)), axis=1)
    dcg = np.sum(pred_data * (1.0 / np.log2(np.arange(2, k + 2))), axis=1)
    idcg[idcg == 0.0] = 1.0
    ndcg = dcg / idcg
    ndcg[np.isnan(ndcg)] = 0.0
    return np.sum(ndcg)


def test_one_batch(sorted_items: np.ndarray, groundTrue, topks=(10, 20)) -> dict:
    """trainer.py:263-280 without the proprietary-data Diversity term."""
    r = getLabel(groundTrue, sorted_items)
    out = {"recall": [], "precision": [], "ndcg": [], "hr": []}
    for k in topks:
        ret = RecallPrecision_ATk(groundTrue, r, k)
        out["precision"].append(ret["precision"])
        out["recall"].append(ret["recall"])
        out["hr"].append(ret["hr"])
        out["ndcg"].append(NDCGatK_r(groundTrue, r, k))
    return {k: np.array(v) for k, v in out.items()}


def rank_metrics(tptr, score, gt, eq, eq_lower, masked, n_gt, n_train, m_items,
                 topks=(10, 20), return_ranks=False) -> dict:
    """The metric sums of one batch of users from exact ranks (the five
    arrays of evaluate.score_rank; user slot u owns pairs tptr[u] ..
    tptr[u + 1] - 1).  rank = 1 + gt + eq_lower is a target's place among
    the user's non-train items, score descending, ties to the lower id; a
    masked target (a test item that is a train positive) has no rank and is
    never a hit.  ``n_gt[u]`` counts all of u's test items, masked ones
    included; ``n_train[u]`` its distinct train items.

    precision / recall / ndcg / hr at every k (any k): the formulas above on
    the hit flags r[u, rank - 1] = 1 — built in row blocks, reduced per row
    as RecallPrecision_ATk / NDCGatK_r reduce them, summed once per batch, so
    the sums are the ones test_one_batch gives for the sorted lists.
    mrr: Σ_u 1 / min_t rank_t (0 without an unmasked target).  The
    reference's MRRatK_r divides by log2(1 / arange(1, k + 1)) — 0 at rank 1
    and negative after — and cannot be reproduced; this is the textbook mean
    reciprocal rank.
    auc: the reference's AUC, roc_auc_score of one user over the items that
    are not train positives, as the Mann-Whitney statistic with ties at ½:
    P = the unmasked targets, N = M - n_train - |P| negatives,
    AUC_u = Σ_{t in P} (N - neg_above_t - ½ neg_tied_t) / (|P| N), where the
    counts over J lose the other positives (found from the returned scores).
    Users with |P| = 0 or N = 0 are left out: "auc" is the sum over the
    others and "auc_users" their number.
    Sums, as test_one_batch returns; the caller divides."""
    tptr = np.asarray(tptr, dtype=np.int64)
    n = len(tptr) - 1
    score = np.asarray(score)
    gt = np.asarray(gt, dtype=np.int64)
    eq = np.asarray(eq, dtype=np.int64)
    eq_lower = np.asarray(eq_lower, dtype=np.int64)
    live = ~np.asarray(masked).astype(bool)
    n_gt = np.asarray(n_gt, dtype=np.int64)
    n_train = np.asarray(n_train, dtype=np.int64)
    slot = np.repeat(np.arange(n), np.diff(tptr))
    rank = np.where(live, 1 + gt + eq_lower, 0)

    kmax = int(max(topks))
    right = {k: np.zeros(n) for k in topks}
    dcg = {k: np.zeros(n) for k in topks}
    idcg = {k: np.zeros(n) for k in topks}
    step = max(1, (1 << 22) // kmax)
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        a, b = tptr[lo], tptr[hi]
        sel = live[a:b] & (rank[a:b] <= kmax)
        r = np.zeros((hi - lo, kmax))
        r[slot[a:b][sel] - lo, rank[a:b][sel] - 1] = 1.0
        for k in topks:
            pred = r[:, :k]
            right[k][lo:hi] = pred.sum(1)
            dcg[k][lo:hi] = np.sum(pred * (1.0 / np.log2(np.arange(2, k + 2))), axis=1)
            ideal = (np.arange(k)[None, :] < np.minimum(k, n_gt[lo:hi])[:, None]).astype("float")
            idcg[k][lo:hi] = np.sum(ideal * 1.0 / np.log2(np.arange(2, k + 2)), axis=1)
    out = {"recall": [], "precision": [], "ndcg": [], "hr": []}
    for k in topks:
        out["precision"].append(np.sum(right[k]) / k)
        out["recall"].append(np.sum(right[k] / (n_gt + 1e-6)))
        out["hr"].append(np.sum(right[k] >= 1))
        d = idcg[k]
        d[d == 0.0] = 1.0
        ndcg = dcg[k] / d
        ndcg[np.isnan(ndcg)] = 0.0
        out["ndcg"].append(np.sum(ndcg))
    out = {k: np.array(v) for k, v in out.items()}

    idx = np.nonzero(live)[0]
    sl = slot[idx]
    best = np.full(n, np.inf)
    np.minimum.at(best, sl, rank[idx].astype(np.float64))
    out["mrr"] = float(np.sum(np.where(np.isfinite(best), 1.0 / best, 0.0)))

    # the other positives above / tied with each target: pairs sorted by
    # (user, score descending); a run of equal scores inside a user starts
    # run_start - grp_start places after the user's first pair
    sc = score[idx].astype(np.float64)
    order = np.lexsort((-sc, sl))
    sl_o, sc_o = sl[order], sc[order]
    m = len(order)
    pos = np.arange(m)
    new_grp = np.ones(m, dtype=bool)
    new_grp[1:] = sl_o[1:] != sl_o[:-1]
    new_run = new_grp.copy()
    new_run[1:] |= sc_o[1:] != sc_o[:-1]
    grp_start = np.maximum.accumulate(np.where(new_grp, pos, 0))
    run_start = np.maximum.accumulate(np.where(new_run, pos, 0))
    run_id = np.cumsum(new_run) - 1
    run_len = np.bincount(run_id)[run_id] if m else np.zeros(0, dtype=np.int64)
    neg_above = gt[idx][order] - (run_start - grp_start)
    neg_tied = eq[idx][order] - 1 - (run_len - 1)
    n_pos = np.bincount(sl, minlength=n)
    n_neg = int(m_items) - n_train - n_pos
    wins = np.bincount(sl_o, weights=n_neg[sl_o] - neg_above - 0.5 * neg_tied, minlength=n)
    ok = (n_pos > 0) & (n_neg > 0)
    out["auc"] = float(np.sum(wins[ok] / (n_pos[ok] * n_neg[ok])))
    out["auc_users"] = int(ok.sum())
    if return_ranks:
        out["ranks"] = rank
    return out
