"""mirec_score_rank on the device: exact counts against the
float64 brute force, the derived f32 bracket, bitwise agreement with the
streamed top-k, edge shapes, and evaluate_ranked end to end."""
import functools

import numpy as np
import pytest
import torch

from tests.rank_common import (bracket, brute_counts, make_targets, pair_slots, train_mask)

pytestmark = pytest.mark.gpu
DIMS = [16, 32, 64, 128, 256]


@functools.lru_cache(maxsize=None)
def _small():
    """The shapes of test_score_topk_streaming_matches_exact_topk."""
    from furusato_recommend_amd import SyntheticBipartite
    from furusato_recommend_amd.graph import Graph
    ds = SyntheticBipartite(2000, 1337, 30_000, seed=7, test_frac=0)
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    return ds, g, np.arange(3, 2000, 11)


def _run(U, I, users, tptr, targets, g, mask=True):
    from furusato_recommend_amd.evaluate import score_rank
    out = score_rank(U.cuda(), I.cuda(), torch.from_numpy(np.asarray(users)).cuda(), tptr,
                     torch.from_numpy(np.asarray(targets, dtype=np.int64)), g, mask=mask)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


def _assert_exact(got, ref):
    score, gt, eq, eql, masked = got
    rs, rgt, req, reql, rmasked = ref
    assert np.array_equal(score, rs.astype(np.float32))
    assert np.array_equal(masked.astype(bool), rmasked)
    live = ~rmasked
    assert np.array_equal(gt[live], rgt[live])
    assert np.array_equal(eq[live], req[live])
    assert np.array_equal(eql[live], reql[live])


def _check_exact(ds, g, users, U, I, lists):
    tptr, targets = make_targets(lists)
    s = U.double().numpy() @ I.double().numpy().T
    for mask in (True, False):
        train = train_mask(ds.allPos if mask else None, users, I.shape[0])
        _assert_exact(_run(U, I, users, tptr, targets, g, mask),
                      brute_counts(s, train, tptr, targets))


def _target_lists(ds, users, m, rng):
    """0 to 5 distinct targets per slot; among them item 0, item M - 1, an
    item of the ragged last tile, train positives of their own user, and
    slots with none (slot 0 and every sixth)."""
    lists = []
    for r, u in enumerate(users.tolist()):
        t = rng.choice(m, size=r % 6, replace=False).tolist()
        if r == 1:
            t.append(0)
        if r == 2:
            t.append(m - 1)
        if r == 3:
            t.append(m - 1 - (m % 32) // 2)
        if r % 5 == 4:
            t.append(int(ds.allPos[u][0]))
        lists.append(np.unique(np.asarray(t, dtype=np.int64))[:5])
    assert len(lists[0]) == 0 and any(0 in x for x in lists) and any(m - 1 in x for x in lists)
    return lists


@pytest.mark.parametrize("d", DIMS)
def test_score_rank_exact_counts(d):
    """Integer embeddings in [-3, 3]: every score is exact in f32 and ties
    are common, so score, masked and (for unmasked targets) gt, eq, eq_lower
    equal the float64 brute force exactly, with and without the train mask,
    at ragged user and item counts."""
    ds, g, users = _small()
    gen = torch.Generator().manual_seed(d)
    U = torch.randint(-3, 4, (len(users), d), generator=gen).float()
    I = torch.randint(-3, 4, (ds.m_items, d), generator=gen).float()
    lists = _target_lists(ds, users, ds.m_items, np.random.default_rng(d))
    _check_exact(ds, g, users, U, I, lists)


@pytest.mark.parametrize("d", [16, 64])
def test_score_rank_exact_past_65536_items(d):
    """70 003 items: several item chunks whose partial counts meet in integer
    atomics, and counts above 65 535 (embeddings in [-2, 2], two targets
    each), exact as above."""
    from furusato_recommend_amd import SyntheticBipartite
    from furusato_recommend_amd.graph import Graph
    ds = SyntheticBipartite(1500, 70_003, 120_000, seed=9, test_frac=0)
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    users = np.arange(5, 1500, 13)
    gen = torch.Generator().manual_seed(d + 1)
    U = torch.randint(-2, 3, (len(users), d), generator=gen).float()
    I = torch.randint(-2, 3, (ds.m_items, d), generator=gen).float()
    rng = np.random.default_rng(d)
    lists = [np.sort(rng.choice(ds.m_items, size=2, replace=False)) for _ in users]
    tptr, targets = make_targets(lists)
    s = U.double().numpy() @ I.double().numpy().T
    train = train_mask(ds.allPos, users, ds.m_items)
    ref = brute_counts(s, train, tptr, targets)
    assert ref[1].max() > 65_535
    _assert_exact(_run(U, I, users, tptr, targets, g), ref)


@functools.lru_cache(maxsize=None)
def _floats(d):
    """U, I ~ 0.1 N(0, 1): 300 user rows x 1337 items."""
    ds, g, _ = _small()
    gen = torch.Generator().manual_seed(100 + d)
    users = np.arange(1, 1800, 6)
    U = 0.1 * torch.randn(len(users), d, generator=gen)
    I = 0.1 * torch.randn(ds.m_items, d, generator=gen)
    return ds, g, users, U, I


@pytest.mark.parametrize("d", DIMS)
def test_score_rank_floats_inside_f32_bracket(d):
    """Float embeddings against float64: with e_j = γ_d Σ_k |u_k||i_jk| (the
    f32 dot-product bound in any order) the counts lie in the derived
    bracket lower <= gt, gt + eq - 1 <= upper; the bracket pins the rank
    (lower == upper) for at least half the pairs, so it can fail; and every
    unmasked target finds itself (eq >= 1: its threshold is bitwise its
    score in the stream).  Measured shares of pinned pairs, d = 16 .. 256:
    0.991, 0.993, 0.984, 0.917, 0.799; widest bracket 1, 1, 1, 2, 4."""
    ds, g, users, U, I = _floats(d)
    rng = np.random.default_rng(d)
    lists = [np.sort(rng.choice(ds.m_items, size=1 + r % 2, replace=False))
             for r in range(len(users))]
    tptr, targets = make_targets(lists)
    train = train_mask(ds.allPos, users, ds.m_items)
    score, gt, eq, eql, masked = _run(U, I, users, tptr, targets, g)
    slot = pair_slots(tptr)
    assert np.array_equal(masked.astype(bool), train[slot, targets])
    live = ~masked.astype(bool)
    lower, upper = bracket(U.numpy(), I.numpy(), train, tptr, targets)
    pinned = float(np.mean(lower[live] == upper[live]))
    print(f"d={d}: pinned share {pinned:.3f}, widest {int((upper - lower)[live].max())}")
    assert pinned >= 0.5
    assert np.all(eq[live] >= 1)
    assert np.all(lower[live] <= gt[live])
    assert np.all(gt[live] + eq[live] - 1 <= upper[live])
    assert np.all((eql[live] >= 0) & (eql[live] <= eq[live] - 1))


@pytest.mark.parametrize("d", DIMS)
def test_score_rank_same_scores_as_streamed_topk(d):
    """On the float data: a target stands at position p of score_topk's
    k = 32 list iff its rank is p + 1, its score is bitwise the list's value,
    and for k = 1, 20, 32 the targets with rank <= k are the targets among
    the first k entries."""
    from furusato_recommend_amd.evaluate import score_topk
    ds, g, users, U, I = _floats(d)
    val, idx = score_topk(U.cuda(), I.cuda(), torch.from_numpy(users).cuda(), g, 32)
    val, idx = val.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
    lists, ids = [], np.arange(ds.m_items)
    for r in range(len(users)):
        out = np.setdiff1d(ids, idx[r])[[3, 700]]  # two items outside the list
        lists.append(np.concatenate([idx[r, [0, 5, 19, 31]], out]))
    tptr, targets = make_targets(lists)
    score, gt, eq, eql, masked = _run(U, I, users, tptr, targets, g)
    rank = 1 + gt.astype(np.int64) + eql
    slot = pair_slots(tptr)
    live = ~masked.astype(bool)
    for p in range(len(targets)):
        if not live[p]:
            continue
        where = np.nonzero(idx[slot[p]] == targets[p])[0]
        if where.size:
            assert rank[p] == where[0] + 1, (p, rank[p], where)
            assert score[p].tobytes() == val[slot[p], where[0]].tobytes()
        else:
            assert rank[p] > 32, (p, rank[p])
    for k in (1, 20, 32):
        for r in range(len(users)):
            sel = (slot == r) & live
            assert set(targets[sel & (rank <= k)]) == set(targets[sel]) & set(idx[r, :k])


def _tiny_case(n_users, m, d, seed, empty_user):
    """A small graph of its own (user ``empty_user`` has no train row)."""
    from furusato_recommend_amd.graph import Graph
    rng = np.random.default_rng(seed)
    tu = rng.integers(0, n_users, 6 * n_users)
    ti = rng.integers(0, m, 6 * n_users)
    keep = tu != empty_user
    tu, ti = tu[keep], ti[keep]
    g = Graph.from_interactions(tu, ti, n_users, m, "cuda:0")

    class DS:
        rows = [ti[tu == u] for u in range(n_users)]
        allPos = [np.unique(x) for x in rows]
    gen = torch.Generator().manual_seed(seed)
    return DS, g, gen


@pytest.mark.parametrize("n_eval,m", [(1, 1337), (65, 7), (65, 33), (1, 7)])
def test_score_rank_edge_shapes(n_eval, m):
    """One user row, 65 user rows, fewer items than a tile, one item past a
    tile; a user with an empty train row among them; exact with integer
    embeddings at d = 16 and 64."""
    n_users = 80
    for d in (16, 64):
        DS, g, gen = _tiny_case(n_users, m, d, seed=m + d, empty_user=4)
        users = np.arange(4, 4 + n_eval)
        assert len(DS.allPos[4]) == 0
        U = torch.randint(-3, 4, (n_eval, d), generator=gen).float()
        I = torch.randint(-3, 4, (m, d), generator=gen).float()
        rng = np.random.default_rng(m)
        lists = [np.sort(rng.choice(m, size=min(m, 1 + r % 4), replace=False))
                 for r in range(n_eval)]
        _check_exact(DS, g, users, U, I, lists)
        if m == 33:
            # without the sorted copy of the user rows the mask pass finds a
            # multi-edge's repeats by scanning the row
            assert any(len(np.unique(x)) < len(x) for x in DS.rows)
            g.csr.col_sorted, g.csr.n_sorted = None, 0
            _check_exact(DS, g, users, U, I, lists)


def test_score_rank_no_targets_launches_nothing():
    """Every user slot without targets: empty outputs, and the library
    returns before it reads an array (null device pointers pass)."""
    from furusato_recommend_amd._lib import lib
    ds, g, users = _small()
    U = torch.zeros(len(users), 32)
    I = torch.zeros(ds.m_items, 32)
    tptr = np.zeros(len(users) + 1, dtype=np.int64)
    out = _run(U, I, users, tptr, np.zeros(0, dtype=np.int64), g)
    assert all(x.shape == (0,) for x in out)
    assert lib.mirec_score_rank(None, len(users), None, ds.m_items, 32, None, tptr.ctypes.data,
                                None, None, ds.n_users, None, None, None, None, None, None, 0,
                                None) == 0


def test_evaluate_ranked_end_to_end():
    """LightGCN trained as in test_evaluate_matches_oracle.  At (10, 20) the
    four shared metrics of evaluate_ranked are evaluate()'s, exactly (same
    scores, same order).  At (50, 100), with mrr and auc, against
    rank_metrics fed the float64 ranks of the oracle's propagated
    embeddings: a user is a near-tie if a target of its has lower != upper
    in the f32 bracket; with n_tie such users of n every metric agrees
    within (n_tie + 0.5) / n, the AUC within n_tie / n + 1e-6."""
    from furusato_recommend_amd import LightGCN, SyntheticBipartite
    from furusato_recommend_amd.evaluate import evaluate, evaluate_ranked
    from furusato_recommend_amd.metric import rank_metrics
    from oracle.lightgcn_oracle import OracleLightGCN
    ds = SyntheticBipartite(4000, 900, 50_000, seed=6, test_frac=0.3)
    m = LightGCN({"recdim": 32, "layer": 2, "lr": 1e-3, "decay": 1e-4, "device": "cuda:0",
                  "bpr_batch_size": 512}, ds)
    for _ in range(3):
        m.OneEpoch(*m.sample(2048, seed=1))
    a = evaluate(m, ds.testDict, (10, 20), batch=1000)
    b = evaluate_ranked(m, ds.testDict, (10, 20), batch=1000)
    for key in ("precision", "recall", "ndcg", "hr"):
        assert np.array_equal(a[key], b[key]), (key, a[key], b[key])
    topks = (50, 100)
    c = evaluate_ranked(m, ds.testDict, topks, batch=1000)
    o = OracleLightGCN(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, 32, 2, 1e-3, 1e-4,
                       emb=m.all_embedding.weight.detach().cpu())
    out = o.propagated().double().numpy()
    users = np.array(sorted(ds.testDict), dtype=np.int64)
    n = len(users)
    Uo, Io = out[users], out[ds.n_users:]
    lists = [np.unique(np.asarray(ds.testDict[int(u)], dtype=np.int64)) for u in users]
    tptr, targets = make_targets(lists)
    train = train_mask(ds.allPos, users, ds.m_items)
    ref = brute_counts(Uo @ Io.T, train, tptr, targets)
    r = rank_metrics(tptr, *ref, np.array([len(ds.testDict[int(u)]) for u in users]),
                     train.sum(1), ds.m_items, topks)
    lower, upper = bracket(Uo, Io, train, tptr, targets)
    live = ~ref[4]
    n_tie = len(np.unique(pair_slots(tptr)[live & (lower != upper)]))
    print(f"near-tie users {n_tie} of {n}")
    assert n_tie <= n / 10
    for key in ("precision", "recall", "ndcg", "hr"):
        assert np.all(np.abs(c[key] - r[key] / n) <= (n_tie + 0.5) / n), (key, c[key], r[key] / n)
    assert abs(c["mrr"] - r["mrr"] / n) <= (n_tie + 0.5) / n
    assert abs(c["auc"] - r["auc"] / r["auc_users"]) <= n_tie / n + 1e-6
