"""HIP path vs the reference (golden fixtures) and vs the CPU oracle.

Tolerance (north_star): outputs match the reference CPU path within 1e-4
relative in fp32, measured as max|a-b| / max|b| over the tensor.  All calls go
through libmirec.so (the C ABI).  Marked gpu: needs an MI355X.
"""
import glob
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
TOL = 1e-4
LGCN = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "lgcn_*.npz")))
# sage_d16_L2 (fanout [4,3]) and sage_d128_L2_f25x10 (C3: d=128, fanout [25,10])
SAGE = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "sage_*.npz")))


def rel(a, b):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


class DS:
    def __init__(self, u, i, n_users, m_items):
        self.trainUser = np.asarray(u, np.int64)
        self.trainItem = np.asarray(i, np.int64)
        self.n_users, self.m_items = int(n_users), int(m_items)
        self.trainDataSize = len(u)
        self.allPos = [self.trainItem[self.trainUser == k] for k in range(self.n_users)]
        self.testDict = {}


def lgcn_from(f, split=None, batch=64, prune=True):
    from furusato_recommend_amd import LightGCN
    ds = DS(f["train_user"], f["train_item"], f["n_users"], f["m_items"])
    cfg = {"recdim": int(f["dim"]), "layer": int(f["n_layers"]), "lr": float(f["lr"]),
           "decay": float(f["decay"]), "device": "cuda:0", "bpr_batch_size": batch,
           "prune": prune}
    if split is not None:
        cfg["csr_split"] = split
    m = LightGCN(cfg, ds)
    with torch.no_grad():
        m.all_embedding.weight.copy_(torch.from_numpy(f["emb0"]))
    return m


@pytest.mark.parametrize("narrow_max", [0, 64, 1 << 30])
@pytest.mark.parametrize("split", [None, 4])
@pytest.mark.parametrize("name", LGCN)
def test_forward(golden, name, split, narrow_max):
    f = golden(name)
    m = lgcn_from(f, split)
    m.engine.narrow_max = narrow_max  # 0: wave-per-row only; huge: group-per-row only
    if split is not None:
        assert m.graph.n_long > 0  # long-row segments exercised
    out = m.propagated()
    torch.cuda.synchronize()
    assert rel(out, f["out"]) < TOL
    assert rel(out, f["out_radj"]) < TOL
    # one LGConv call == reference layer 1
    y = torch.empty_like(out)
    m.engine.propagate_once(m.all_embedding.weight, y)
    assert rel(y, f["layers"][1]) < TOL


@pytest.mark.parametrize("narrow_max", [0, 64])
@pytest.mark.parametrize("prune", [True, False])
@pytest.mark.parametrize("split", [None, 4])
@pytest.mark.parametrize("name", LGCN)
def test_train_steps(golden, name, split, prune, narrow_max):
    f = golden(name)
    m = lgcn_from(f, split, prune=prune)
    m.engine.narrow_max = narrow_max
    t = torch.from_numpy(f["triples"])
    l1 = float(m.stageOne(t[:, 0], t[:, 1], t[:, 2]))
    assert rel(m.all_embedding.weight, f["emb_step1"]) < TOL
    l2 = float(m.stageOne(t[:, 0], t[:, 1], t[:, 2]))
    assert rel(m.all_embedding.weight, f["emb_step2"]) < TOL
    assert np.allclose([l1, l2], f["step_losses"], rtol=TOL)


@pytest.mark.parametrize("name", LGCN)
def test_autograd_path(golden, name):
    f = golden(name)
    m = lgcn_from(f)
    t = torch.from_numpy(f["triples"]).cuda()
    loss, reg = m.bpr_loss(t[:, 0], t[:, 1], t[:, 2])
    assert abs(float(loss) - float(f["loss"])) < TOL * abs(float(f["loss"]))
    assert abs(float(reg) - float(f["reg"])) < TOL * abs(float(f["reg"]))
    (loss + float(f["decay"]) * reg).backward()
    assert rel(m.all_embedding.weight.grad, f["grad"]) < TOL
    # the torch.optim-style step on the HIP Adam kernel
    m.optim.step()
    assert rel(m.all_embedding.weight, f["emb_step1"]) < TOL


@pytest.mark.parametrize("sparse_filter", ["slot", "bytemap", "dense"])
@pytest.mark.parametrize("prune", [True, False])
@pytest.mark.parametrize("name", LGCN)
def test_engine_gradient_matches_reference(golden, name, prune, sparse_filter):
    """Dense-gradient (data-parallel) variant of the fused backward: every
    fixture's width and depth, pruned and full, each way of feeding the
    first backward layer."""
    f = golden(name)
    m = lgcn_from(f, prune=prune)
    m.engine.sparse_filter = sparse_filter
    t = torch.from_numpy(f["triples"]).cuda().int()
    w = m.all_embedding.weight
    out = m.engine.forward(w)
    m.engine.bpr(out, w, t[:, 0].contiguous(), t[:, 1].contiguous(), t[:, 2].contiguous(),
                 float(f["decay"]))
    g = torch.empty_like(w)
    m.engine.backward(w, grad_out=g)
    assert rel(g, f["grad"]) < TOL
    assert int((m.engine.slot != -1).sum()) == 0  # seeds reset


@pytest.mark.parametrize("dim", [4, 16, 64, 256])
def test_engine_gradient_repeated_nodes_vs_oracle(golden, dim):
    """A batch where one item is the positive of 90 % of the triples, one
    user appears 40 times and another LPR + 1 = dim / 4 + 1 times (a
    Zipf-popular item: its seed run spans many rounds of the seed
    accumulation's LPR-entry walk; LPR + 1 entries: one full round and one
    entry of the next): the fused backward's table gradient == the CPU
    oracle's autograd gradient.  dim 64 on the fixture graph, the other
    widths on a synthetic one."""
    from furusato_recommend_amd import LightGCN, SyntheticBipartite
    from oracle.lightgcn_oracle import OracleLightGCN
    B = 200
    if dim == 64:
        f = golden("lgcn_d64_L3.npz")
        m = lgcn_from(f, batch=B)
        n_users, m_items = int(f["n_users"]), int(f["m_items"])
        train, lr, decay = (f["train_user"], f["train_item"]), float(f["lr"]), float(f["decay"])
        emb0 = torch.from_numpy(f["emb0"])
    else:
        ds = SyntheticBipartite(500, 120, 6000, seed=dim, test_frac=0.0)
        torch.manual_seed(dim)
        lr, decay = 1e-3, 1e-4
        m = LightGCN({"recdim": dim, "layer": 3, "lr": lr, "decay": decay, "device": "cuda:0",
                      "bpr_batch_size": B}, ds)
        n_users, m_items = ds.n_users, ds.m_items
        train = (ds.trainUser, ds.trainItem)
        emb0 = m.all_embedding.weight.detach().cpu().clone()
    lpr = dim // 4
    rng = np.random.default_rng(7)
    users = rng.integers(0, n_users, B)
    users[users == 4] = 6
    users[:40] = 3
    users[40:40 + lpr + 1] = 4
    assert int((users == 4).sum()) == lpr + 1
    pos = np.where(rng.random(B) < 0.9, 5, rng.integers(0, m_items, B))
    neg = rng.integers(0, m_items, B)
    o = OracleLightGCN(train[0], train[1], n_users, m_items, dim, 3, lr, decay, emb=emb0)
    ref = o.grad(torch.from_numpy(users), torch.from_numpy(pos), torch.from_numpy(neg))
    w = m.all_embedding.weight
    out = m.engine.forward(w)
    tc = [torch.from_numpy(a).cuda().int().contiguous() for a in (users, pos, neg)]
    m.engine.bpr(out, w, *tc, decay)
    g = torch.empty_like(w)
    m.engine.backward(w, grad_out=g)
    assert rel(g, ref) < TOL


def test_mf(golden):
    from furusato_recommend_amd import MF
    f = golden("mf_d32.npz")
    ds = DS(f["train_user"], f["train_item"], f["n_users"], f["m_items"])
    m = MF({"latent_dim_rec": 32, "lr": float(f["lr"]), "decay": float(f["decay"]),
            "device": "cuda:0", "bpr_batch_size": 64}, ds)
    m.load_table(torch.from_numpy(f["user_w0"]), torch.from_numpy(f["item_w0"]))
    t = torch.from_numpy(f["triples"])
    sl = float(m.stageOne(t[:, 0], t[:, 1], t[:, 2]))
    assert abs(sl - float(f["step_loss"])) < TOL * abs(float(f["step_loss"]))
    assert rel(m.embedding_user.weight, f["user_w1"]) < TOL
    assert rel(m.embedding_item.weight, f["item_w1"]) < TOL
    # reference getUsersRating after the step (make_golden.py): sigmoid(U Iᵀ)
    assert rel(m.getUsersRating(torch.arange(5, device="cuda")), f["rating5"]) < TOL


def test_one_epoch_vs_oracle(golden):
    """OneEpoch (minibatch loop incl. a ragged last batch) vs the CPU oracle."""
    from oracle.lightgcn_oracle import OracleLightGCN
    f = golden("lgcn_d64_L3.npz")
    m = lgcn_from(f, batch=64)
    o = OracleLightGCN(f["train_user"], f["train_item"], int(f["n_users"]), int(f["m_items"]),
                       64, 3, float(f["lr"]), float(f["decay"]),
                       emb=torch.from_numpy(f["emb0"]))
    rng = np.random.default_rng(0)
    S = 300  # 4 full batches + one of 44
    u = rng.integers(0, int(f["n_users"]), S)
    p = rng.integers(0, int(f["m_items"]), S)
    n = rng.integers(0, int(f["m_items"]), S)
    lg = float(m.OneEpoch(torch.from_numpy(u), torch.from_numpy(p), torch.from_numpy(n)))
    lo = o.OneEpoch(u, p, n, 64)
    assert abs(lg - lo) < TOL * abs(lo)
    assert rel(m.all_embedding.weight, o.emb.detach()) < TOL


def test_deterministic(golden):
    f = golden("lgcn_d64_L3.npz")
    t = torch.from_numpy(f["triples"])
    res = []
    for _ in range(2):
        m = lgcn_from(f)
        a = m.propagated().clone()
        m.stageOne(t[:, 0], t[:, 1], t[:, 2])
        res.append((a, m.all_embedding.weight.detach().clone()))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


def test_prescale_reuse_tracks_table_writes(golden):
    """The fused update emits the next step's dinv ⊙ E; the engine reuses it
    only while the table is untouched (version counter, raw kernel writes)."""
    f = golden("lgcn_d64_L3.npz")
    t = torch.from_numpy(f["triples"])
    tc = t.cuda()

    def run(force):
        m = lgcn_from(f)
        w = m.all_embedding.weight

        def step():
            if force:
                m.engine.invalidate_prescaled()
            m.stageOne(t[:, 0], t[:, 1], t[:, 2])
        step()
        step()
        with torch.no_grad():
            w.mul_(0.5)                      # torch in-place: version bump
        step()
        m.optim.zero_grad()
        loss, reg = m.bpr_loss(tc[:, 0], tc[:, 1], tc[:, 2])
        (loss + float(f["decay"]) * reg).backward()
        m.optim.step()                       # HIP Adam kernel: raw write
        step()
        w.data.add_(0.01)                    # invisible to the version counter
        m.engine.invalidate_prescaled()
        step()
        return w.detach().clone()
    assert torch.equal(run(False), run(True))


@pytest.mark.parametrize("split", [None, 64])
def test_frontier_sets_and_lists(split):
    """S / F1 byte maps, the deduplicated S list and the F1 row list vs host
    set arithmetic (triples and key-list forms, sentinel keys, long rows)."""
    from furusato_recommend_amd import Graph
    from furusato_recommend_amd.engine import PropagationEngine
    rng = np.random.default_rng(3)
    n_users, m_items, E = 5000, 700, 60000
    u = rng.integers(0, n_users, E)
    i = np.minimum(rng.zipf(1.3, E) - 1, m_items - 1)  # hot items -> long rows
    g = Graph.from_interactions(u, i, n_users, m_items, device="cuda:0",
                                **({} if split is None else {"split": split}))
    if split is not None:
        assert g.n_long > 0
    eng = PropagationEngine(g, 32, 3, max_batch=700, prune=True)
    rowptr = g.rowptr.cpu().numpy()
    col = g.col.cpu().numpy()
    N = g.n_nodes

    def check_sets(S):
        S = set(int(x) for x in S)
        F1 = set(S)
        for x in S:
            F1.update(int(c) for c in col[rowptr[x]:rowptr[x + 1]])
        bs = eng.bm_self.view(torch.uint8)[:N].cpu().numpy()
        bh = eng.bm_hop.view(torch.uint8)[:N].cpu().numpy()
        assert set(np.nonzero(bs)[0].tolist()) == S
        assert set(np.nonzero(bh)[0].tolist()) == F1
        ns = int(eng.self_count.item())
        sl = eng.self_list[:ns].cpu().numpy()
        assert ns == len(S) and set(sl.tolist()) == S
        deg = np.diff(rowptr)
        cnt = eng.list_counts.cpu().numpy()
        for k, (want, lists) in enumerate(((S, eng.s_lists), (F1, eng.hop_lists))):
            nl = lists[0][:cnt[2 * k]].cpu().numpy()
            wl = lists[1][:cnt[2 * k + 1]].cpu().numpy()
            both = np.concatenate([nl, wl])
            assert len(both) == len(want) and set(both.tolist()) == want
            assert (deg[nl] <= eng.narrow_max).all() and (deg[wl] > eng.narrow_max).all()

    B = 700
    us = torch.from_numpy(rng.integers(0, n_users, B)).int().cuda()
    ps = torch.from_numpy(rng.integers(0, m_items, B)).int().cuda()
    ns_ = torch.from_numpy(rng.integers(0, m_items, B)).int().cuda()
    eng.compute_frontier(us, ps, ns_)
    S = np.concatenate([us.cpu().numpy(), n_users + ps.cpu().numpy(),
                        n_users + ns_.cpu().numpy()])
    check_sets(S)
    keys = np.concatenate([rng.integers(0, N, 3000), [N, N, -1]]).astype(np.int32)
    eng.compute_frontier(keys=torch.from_numpy(keys).cuda(), n_keys=len(keys))
    check_sets(keys[(keys >= 0) & (keys < N)])


def test_sampler_invariants():
    from furusato_recommend_amd import LightGCN, SyntheticBipartite
    ds = SyntheticBipartite(500, 300, 6000, seed=3, test_frac=0)
    m = LightGCN({"recdim": 16, "layer": 1, "lr": 1e-3, "decay": 1e-4, "device": "cuda:0",
                  "bpr_batch_size": 64}, ds)
    S = 200_000
    u, p, n = m.sample(S, seed=11)
    assert int(m._sample_err.item()) == 0
    u, p, n = u.cpu().numpy(), p.cpu().numpy(), n.cpu().numpy()
    pos_sets = [set(x.tolist()) for x in ds.allPos]
    assert all(pi in pos_sets[ui] for ui, pi in zip(u[:20000], p[:20000]))
    assert all(ni not in pos_sets[ui] for ui, ni in zip(u[:20000], n[:20000]))
    # users uniform (chi-square, 499 dof: mean 499, sd ~31.6)
    cnt = np.bincount(u, minlength=500)
    chi2 = float(((cnt - S / 500) ** 2 / (S / 500)).sum())
    assert chi2 < 499 + 6 * 31.6
    # reproducible, shape-independent counter RNG
    u2, p2, n2 = m.sample(S, seed=11)
    assert np.array_equal(u, u2.cpu().numpy()) and np.array_equal(n, n2.cpu().numpy())
    u3, _, _ = m.sample(1000, seed=11, offset=5000)
    assert np.array_equal(u3.cpu().numpy(), u[5000:6000])
    # sharded: users of shard r are u % G == r
    us, _, _ = m.sample(10000, seed=1, shard=1, n_shards=4)
    assert np.all(us.cpu().numpy() % 4 == 1)


def test_weighted_positive_sampler(golden):
    """sample_pow (negative_sample.py:53-56): the device sampler with the
    per-user probabilities of the reference-generated fixture
    (sampler_weighted.npz; the reference's own draws pin the oracle, test
    _oracle.py).  The RNG streams differ from numpy's, so the check is
    distributional: per (user, item) cell the positive counts against S x
    P(user) x P(item | user) (chi-square, cells with expectation >= 5),
    zero-probability positives never drawn; the users and negatives are the
    uniform sampler's bit for bit (one draw per positive either way); the
    capped epoch sampler draws its candidates' positives the same way."""
    from furusato_recommend_amd import LightGCN
    from furusato_recommend_amd.engine import sample_epoch_capped
    f = golden("sampler_weighted.npz")
    u, i, nu, mi = f["train_user"], f["train_item"], int(f["n_users"]), int(f["m_items"])
    all_pos = [i[u == k] for k in range(nu)]
    probs = np.split(np.asarray(f["probs_flat"], np.float64),
                     np.cumsum([len(p) for p in all_pos])[:-1])

    class DS:
        n_users, m_items, trainUser, trainItem = nu, mi, u, i
    cfg = {"recdim": 16, "layer": 1, "lr": 1e-3, "decay": 1e-4, "device": "cuda:0",
           "bpr_batch_size": 64}
    plain = LightGCN(cfg, DS)
    m = LightGCN({**cfg, "sample_probs": probs}, DS)
    S = 400_000
    uw, pw, nw = (t.cpu().numpy() for t in m.sample(S, seed=5))
    uu, pu, nn_ = (t.cpu().numpy() for t in plain.sample(S, seed=5))
    assert int(m._sample_err.item()) == 0
    assert np.array_equal(uw, uu) and np.array_equal(nw, nn_)
    assert not np.array_equal(pw, pu)
    # expected cell probabilities (multi-edges: an item's entries add up)
    exp = np.zeros((nu, mi))
    for k in range(nu):
        for it, pr in zip(all_pos[k], probs[k]):
            exp[k, it] += pr / nu
    cnt = np.zeros((nu, mi))
    np.add.at(cnt, (uw, pw), 1)
    assert cnt[exp == 0].sum() == 0  # never a zero-probability positive
    e = exp * S
    big = e >= 5
    chi2 = float(((cnt[big] - e[big]) ** 2 / e[big]).sum())
    dof = int(big.sum()) - 1
    assert chi2 < dof + 6 * np.sqrt(2 * dof), (chi2, dof)
    assert all(nw[k] not in all_pos[uw[k]] for k in range(0, S, 101))
    # the capped epoch sampler: candidate positives from the same CDFs
    _, _, _, cu, cp = sample_epoch_capped(m.graph, 200_000, 10**6, seed=3, return_candidates=True)
    cu, cp = cu.cpu().numpy(), cp.cpu().numpy()
    ok = cp >= 0
    c2 = np.zeros((nu, mi))
    np.add.at(c2, (cu[ok], cp[ok]), 1)
    assert c2[exp == 0].sum() == 0
    e2 = exp / exp[np.unique(cu[ok])].sum() * ok.sum()
    big2 = e2 >= 5
    chi2b = float(((c2[big2] - e2[big2]) ** 2 / e2[big2]).sum())
    dof2 = int(big2.sum()) - 1
    assert chi2b < dof2 + 6 * np.sqrt(2 * dof2), (chi2b, dof2)


@pytest.mark.parametrize("narrow_max", [0, 64])
def test_full_size_properties(narrow_max):
    """BASELINE C2 size (1M users x 100K items, 20M edges): size-independent
    checks — sqrt(deg) is a fixed point of Â, sampled rows vs float64 host
    sums, adjointness <x, Ây> = <Âx, y>."""
    from furusato_recommend_amd import Graph, SyntheticBipartite
    from furusato_recommend_amd.engine import PropagationEngine
    ds = SyntheticBipartite(1_000_000, 100_000, 20_000_000, seed=0, test_frac=0)
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    eng = PropagationEngine(g, 64, 3, 2048)
    eng.narrow_max = narrow_max
    N = g.n_nodes
    deg = torch.from_numpy(g.degree().astype(np.float32)).cuda()
    x = torch.randn(N, 64, device="cuda") * 0.1
    x[:, 0] = deg.sqrt()
    y = torch.empty_like(x)
    eng.propagate_once(x, y)
    assert rel(y[:, 0], x[:, 0]) < 1e-5
    rows = np.random.default_rng(0).choice(N, 512, replace=False)
    xh = x.cpu().double().numpy()
    dinv = g.dinv.cpu().double().numpy()
    rp, col = g.rowptr_host, g.col_host
    ref = np.stack([dinv[r] * (dinv[col[rp[r]:rp[r + 1]], None] * xh[col[rp[r]:rp[r + 1]]]).sum(0)
                    for r in rows])
    assert rel(y[torch.from_numpy(rows).cuda()], ref) < 1e-5
    z = torch.randn_like(x)
    az = torch.empty_like(z)
    eng.propagate_once(z, az)
    lhs = float((x.double() * az.double()).sum())
    rhs = float((y.double() * z.double()).sum())
    assert abs(lhs - rhs) < 1e-4 * max(abs(lhs), 1.0)


@pytest.mark.parametrize("d", [32, 64, 256])
def test_zipf_long_rows_match_unsplit(d):
    """Skewed items force the segment path at default split (segments +
    the one-workgroup-per-row finalize, whose lane-group count depends on
    d); results equal the unsplit kernel up to summation order."""
    from furusato_recommend_amd import Graph, SyntheticBipartite
    from furusato_recommend_amd.engine import PropagationEngine
    ds = SyntheticBipartite(50_000, 5_000, 1_000_000, seed=2, kind="zipf", test_frac=0)
    ga = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    gb = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0",
                                 split=1 << 30)
    assert ga.n_long > 0 and gb.n_long == 0
    # a fixed input: the default CUDA generator seeds itself anew in every
    # process, and the figure below moves with the draw
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(ga.n_nodes, d, device="cuda", generator=gen)
    outs = []
    for g in (ga, gb):
        e = PropagationEngine(g, d, 3, 64)
        outs.append(e.forward(x).clone())
    assert rel(outs[0], outs[1]) < 1e-5


@pytest.mark.parametrize("ways", [2, 3])
@pytest.mark.parametrize("name", LGCN)
def test_seed_exchange_two_ranks_in_one_process(golden, name, ways):
    """The DP sparse exchange (pack -> concatenate as an all-gather would ->
    merge) for 2 or 3 simulated ranks == the reference gradient of the union
    (3 ranks: the first 63 triples in equal parts, grad_scale = 1/3, against
    the CPU oracle's gradient of those 63)."""
    f = golden(name)
    m = lgcn_from(f)
    t = torch.from_numpy(f["triples"]).cuda().int()
    if ways == 2:
        parts, ref = (t[:32], t[32:]), f["grad"]
    else:
        from oracle.lightgcn_oracle import OracleLightGCN
        parts = (t[:21], t[21:42], t[42:63])
        o = OracleLightGCN(f["train_user"], f["train_item"], int(f["n_users"]),
                           int(f["m_items"]), int(f["dim"]), int(f["n_layers"]), float(f["lr"]),
                           float(f["decay"]), emb=torch.from_numpy(f["emb0"]))
        t63 = torch.from_numpy(f["triples"][:63])
        ref = o.grad(t63[:, 0], t63[:, 1], t63[:, 2])
    eng, w = m.engine, m.all_embedding.weight
    out = eng.forward(w)
    gathered = []
    for part in parts:
        eng.bpr(out, w, part[:, 0].contiguous(), part[:, 1].contiguous(),
                part[:, 2].contiguous(), float(f["decay"]), grad_scale=1.0 / ways)
        gathered.append([x.clone() for x in eng.export_seeds()])
    assert int((eng.slot != -1).sum()) == 0
    eng.import_seeds(*(torch.cat([g[i] for g in gathered]) for i in range(3)))
    g = torch.empty_like(w)
    eng.backward(w, grad_out=g)
    assert rel(g, ref) < TOL
    assert int((eng.slot != -1).sum()) == 0


@pytest.mark.parametrize("mode", ["sparse", "dense", "sharded"])
def test_data_parallel_rccl_world1(golden, mode):
    """dist.DataParallel through real RCCL collectives (world_size 1) ==
    the reference's stageOne."""
    import socket

    import torch.distributed as dist

    from furusato_recommend_amd.dist import DataParallel
    f = golden("lgcn_d64_L3.npz")
    m = lgcn_from(f)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0,
                            world_size=1, device_id=torch.device("cuda:0"))
    try:
        dp = DataParallel(m.engine, m.all_embedding.weight.data, m.optim, mode=mode)
        t = torch.from_numpy(f["triples"]).cuda().int()
        for k in (1, 2):
            dp.step(t[:, 0].contiguous(), t[:, 1].contiguous(), t[:, 2].contiguous(),
                    float(f["decay"]))
            assert rel(m.all_embedding.weight, f[f"emb_step{k}"]) < TOL
    finally:
        dist.destroy_process_group()


def _nccl_world1():
    import socket

    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0,
                            world_size=1, device_id=torch.device("cuda:0"))


def _pipelined_world1(backend):
    """3 steps of DenseGradDataParallel(GraphSAGE, fetch, 3 micro-batches)
    in a world of one process over ``backend``; the parameters after them."""
    import socket

    import torch.distributed as dist

    from furusato_recommend_amd.dist import DenseGradDataParallel
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    kw = {"device_id": torch.device("cuda:0")} if backend == "nccl" else {}
    dist.init_process_group(backend, init_method=f"tcp://127.0.0.1:{port}", rank=0,
                            world_size=1, **kw)
    try:
        m, ds = _union_model("sage")
        dp = DenseGradDataParallel(m, table_exchange="fetch", microbatches=3)
        assert dp.distributed and dp.world == 1
        for i, n in enumerate((256, 100, 2)):
            u, p, q = _union_batch(m, ds, "sage", i, 0, 1, n)
            dp.step(u, p, q)
        dp.gather_optimizer_state()
        torch.cuda.synchronize()
        return [x.detach().cpu().clone() for x in m.parameters()]
    finally:
        dist.destroy_process_group()


def test_pipelined_exchange_rccl_world1_equals_gloo():
    """The pipelined exchange's overlap machinery runs only under RCCL
    (asynchronous all-to-all work handles, the route on a side stream that
    waits for one micro-batch's export event, record_stream of the received
    blocks, the main stream waiting for the side stream): at world size 1
    through real RCCL it gives the gloo run's parameters bit for bit (the
    same sums in the same order; gloo runs the transfers synchronously)."""
    a = _pipelined_world1("nccl")
    b = _pipelined_world1("gloo")
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_data_parallel_auto_calibration_rccl_world1(golden):
    """mode="auto" through real RCCL (world 1, calibration forced): both
    exchanges run — the sharded one with its row-block async all-gathers,
    the barrier, the MAX all-reduce of the timings, the table all-gather
    timing — and the 1 + 1 + 1 + 1 calibration steps plus one more equal
    five steps of the reference's stageOne (the oracle)."""
    import torch.distributed as dist

    from furusato_recommend_amd.dist import DataParallel
    from oracle.lightgcn_oracle import OracleLightGCN
    f = golden("lgcn_d64_L3.npz")
    m = lgcn_from(f)
    _nccl_world1()
    try:
        dp = DataParallel(m.engine, m.all_embedding.weight.data, m.optim, mode="auto", chunks=3)
        t = torch.from_numpy(f["triples"]).cuda().int()

        def run_step():
            dp.step(t[:, 0].contiguous(), t[:, 1].contiguous(), t[:, 2].contiguous(),
                    float(f["decay"]))
        cal = dp.calibrate(run_step, steps=1, force=True)
        run_step()
        torch.cuda.synchronize()
        assert cal["choice"] in ("sparse", "sharded") and cal["table_allgather_ms"] > 0
        assert not m.optim.stale_rows  # world 1: nothing is stale
    finally:
        dist.destroy_process_group()
    o = OracleLightGCN(f["train_user"], f["train_item"], int(f["n_users"]), int(f["m_items"]),
                       64, 3, float(f["lr"]), float(f["decay"]), emb=torch.from_numpy(f["emb0"]))
    tt = f["triples"]
    for _ in range(5):
        o.stageOne(tt[:, 0], tt[:, 1], tt[:, 2])
    assert rel(m.all_embedding.weight, o.emb.detach()) < TOL


@pytest.mark.parametrize("kind,exchange", [("sage", "routed"), ("sage", "fetch"),
                                           ("sasrec", "routed")])
def test_routed_table_exchange_rccl_world1(kind, exchange):
    """The routed table exchange through real RCCL calls (world 1: the
    counts all-to-all, the uneven id / row all-to-alls, the in-place table
    all-gather; fetch: the norms' all-gather) == the single-GPU step with
    the fused sorted-gradient Adam:
    the first step's parameters bit for bit (S of the own rows = 0 + S;
    untouched rows form fma(c, w, 0) either way), later steps to 1e-6 (the
    next forward takes the table norm from a fresh pass instead of the fused
    Adam's block partials: fp32 order).  SASRec runs its split captured
    step."""
    import torch.distributed as dist

    from furusato_recommend_amd.dist import DenseGradDataParallel
    a, ds = _union_model(kind, graph=True)
    b, _ = _union_model(kind, graph=True)
    b.load_state_dict(a.state_dict())
    _nccl_world1()
    try:
        dp = DenseGradDataParallel(a, table_exchange=exchange)
        for i in range(3):
            u, p, n = _union_batch(a, ds, kind, i, 0, 1)
            if kind == "sasrec":  # the same dropout keys on both sides
                st = torch.get_rng_state()
                dp.step(u, p, n)
                torch.set_rng_state(st)
            else:
                dp.step(u, p, n)
            b.stageOne(u, p, n)
            torch.cuda.synchronize()
            for x, y in zip(a.parameters(), b.parameters()):
                assert torch.equal(x, y) if i == 0 else rel(x, y) < 1e-6
        assert dp.last_exchange_bytes == 0  # world 1: nothing from other ranks
    finally:
        dist.destroy_process_group()


def test_dense_grad_sharded_adam_rccl_world1():
    """DenseGradDataParallel's sharded table Adam through real RCCL calls
    (reduce_scatter_tensor, in-place all_gather_into_tensor; world_size 1,
    sharding forced) == the GraphSAGE step with the same materialised table
    gradient and the full-table Adam, parameters bit for bit."""
    import socket

    import torch.distributed as dist

    from furusato_recommend_amd import GraphSAGE, SyntheticBipartite
    from furusato_recommend_amd.dist import DenseGradDataParallel
    ds = SyntheticBipartite(20_000, 2_000, 200_000, seed=2)  # table above BUCKET_MIN
    cfg = {"recdim": 64, "layer": 2, "lr": 1e-3, "decay": 1e-4, "device": "cuda:0",
           "bpr_batch_size": 256, "fanouts": [10, 5]}
    torch.manual_seed(3)
    a = GraphSAGE(cfg, ds)
    b = GraphSAGE(cfg, ds)
    b.load_state_dict(a.state_dict())
    a._tg.dense = b._tg.dense = True  # the materialised table gradient, as under DP
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0,
                            world_size=1, device_id=torch.device("cuda:0"))
    try:
        dp = DenseGradDataParallel(a, shard_optimizer=True, table_exchange="dense")
        for i in range(3):
            u, p, n = a.sample(256, seed=9, offset=256 * i)
            dp.step(u, p, n)
            b.stageOne(u, p, n)
        torch.cuda.synchronize()
        assert id(a._table) in dp._sharded
        for x, y in zip(a.parameters(), b.parameters()):
            assert torch.equal(x, y)
    finally:
        dist.destroy_process_group()


def test_pruned_step_equals_dense_step_full_size():
    """C2 size: the frontier-pruned training step (only the rows the loss
    depends on) updates E exactly like the full-graph step (fp32 summation
    order aside), for several steps with different batches."""
    from furusato_recommend_amd import SyntheticBipartite
    from furusato_recommend_amd.engine import AdamState, PropagationEngine, sample_triples
    from furusato_recommend_amd.graph import Graph
    ds = SyntheticBipartite(1_000_000, 100_000, 20_000_000, seed=0, test_frac=0)
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    torch.manual_seed(0)
    e0 = torch.randn(g.n_nodes, 64, device="cuda") * 0.1
    res = []
    for prune in (True, False):
        eng = PropagationEngine(g, 64, 3, 2048, prune=prune)
        e = e0.clone()
        adam = AdamState(e, 1e-3)
        u = torch.empty(2048, dtype=torch.int32, device="cuda")
        p, n = torch.empty_like(u), torch.empty_like(u)
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        losses = []
        for step in range(3):
            sample_triples(g, 2048, 7, step * 2048, u, p, n, err)
            losses.append(float(eng.train_step(e, adam, u, p, n, 1e-4)))
        res.append((e, losses))
    assert rel(res[0][0], res[1][0]) < 1e-5
    assert np.allclose(res[0][1], res[1][1], rtol=1e-5)
    assert not torch.equal(res[0][0], e0)


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5])
def test_pruned_equals_dense_any_depth(L):
    """Frontier pruning's layer/row bookkeeping for every depth: pruned and
    dense steps give the same parameters, loss and layer-mean embeddings."""
    from furusato_recommend_amd import SyntheticBipartite
    from furusato_recommend_amd.engine import AdamState, PropagationEngine, sample_triples
    from furusato_recommend_amd.graph import Graph
    ds = SyntheticBipartite(5000, 800, 60_000, seed=4, test_frac=0)
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    torch.manual_seed(1)
    e0 = torch.randn(g.n_nodes, 32, device="cuda") * 0.1
    res = []
    for prune in (True, False):
        eng = PropagationEngine(g, 32, L, 256, prune=prune)
        e = e0.clone()
        adam = AdamState(e, 1e-2)
        u = torch.empty(256, dtype=torch.int32, device="cuda")
        p, n = torch.empty_like(u), torch.empty_like(u)
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        losses = []
        for step in range(3):
            sample_triples(g, 256, 3, step * 256, u, p, n, err)
            losses.append(float(eng.train_step(e, adam, u, p, n, 1e-4)))
        res.append((e, losses))
    assert rel(res[0][0], res[1][0]) < 1e-5
    assert np.allclose(res[0][1], res[1][1], rtol=1e-5)


def test_topk_masked_matches_torch():
    """mirec_topk_masked == rating[train positives] = -1024; torch.topk
    (trainer.py:132-138) on random scores (no ties)."""
    from furusato_recommend_amd import SyntheticBipartite
    from furusato_recommend_amd.evaluate import topk_masked
    from furusato_recommend_amd.graph import Graph
    ds = SyntheticBipartite(3000, 1500, 40_000, seed=5, test_frac=0)
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    users = torch.arange(0, 3000, 7, device="cuda")
    # seeded (an unseeded draw once held an exact tie in a top-64, which
    # torch.topk may order either way)
    gen = torch.Generator(device="cuda").manual_seed(0)
    rating = torch.randn(len(users), ds.m_items, device="cuda", generator=gen)
    ref = rating.clone()
    for r, u in enumerate(users.tolist()):
        ref[r, torch.from_numpy(ds.allPos[u]).cuda()] = -(1 << 10)
    top = torch.topk(ref, k=65).values
    assert bool((top[:, 1:] != top[:, :-1]).all())  # no ties: the order is unique
    for k in (1, 20, 50, 64):
        rv, ri = torch.topk(ref, k=k)
        val, idx = topk_masked(rating.clone(), users, g, k)
        assert torch.equal(idx.long(), ri)
        assert torch.equal(val, rv)


@pytest.mark.parametrize("d", [16, 32, 64, 128, 256])
def test_score_topk_streaming_matches_exact_topk(d):
    """mirec_score_topk (scores streamed through MFMA tiles into per-user
    candidate lists, never materialised) == the exact masked top-k: integer
    embeddings make every score exact in f32, so the order — score
    descending, ties to the lower item id, train positives at -1024 — is
    compared exactly, ties included, for k = 1, 20, 32, with ragged user and
    item counts."""
    from furusato_recommend_amd import SyntheticBipartite
    from furusato_recommend_amd.evaluate import score_topk
    from furusato_recommend_amd.graph import Graph
    ds = SyntheticBipartite(2000, 1337, 30_000, seed=7, test_frac=0)
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    gen = torch.Generator().manual_seed(d)
    users = torch.arange(3, 2000, 11)
    U = torch.randint(-3, 4, (len(users), d), generator=gen).float()
    I = torch.randint(-3, 4, (ds.m_items, d), generator=gen).float()
    ref = (U.double() @ I.double().t()).numpy()
    for r, u in enumerate(users.tolist()):
        ref[r, ds.allPos[u]] = -1024.0
    for k in (1, 20, 32):
        val, idx = score_topk(U.cuda(), I.cuda(), users.cuda(), g, k)
        val, idx = val.cpu().numpy(), idx.cpu().numpy()
        items = np.arange(ds.m_items)
        for r in range(len(users)):
            order = np.lexsort((items, -ref[r]))[:k]
            assert np.array_equal(idx[r], order), (k, r)
            assert np.array_equal(val[r], ref[r, order].astype(np.float32)), (k, r)


@pytest.mark.parametrize("d", [16, 64])
def test_score_topk_streaming_exact_past_65536_items(d):
    """mirec_score_topk past 65 536 items (several chunks of <= 65 536: the
    candidates' 16-bit ids, both slot counts) == the exact masked top-k
    (integer embeddings: exact scores, many ties, train positives at -1024)
    for k = 1, 20, 32, with a ragged item count."""
    from furusato_recommend_amd import SyntheticBipartite
    from furusato_recommend_amd.evaluate import score_topk
    from furusato_recommend_amd.graph import Graph
    ds = SyntheticBipartite(1500, 70_003, 120_000, seed=9, test_frac=0)
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    gen = torch.Generator().manual_seed(d + 1)
    users = torch.arange(5, 1500, 13)
    U = torch.randint(-2, 3, (len(users), d), generator=gen).float()
    I = torch.randint(-2, 3, (ds.m_items, d), generator=gen).float()
    ref = (U.double() @ I.double().t()).numpy()
    for r, u in enumerate(users.tolist()):
        ref[r, ds.allPos[u]] = -1024.0
    items = np.arange(ds.m_items)
    for k in (1, 20, 32):
        val, idx = score_topk(U.cuda(), I.cuda(), users.cuda(), g, k)
        val, idx = val.cpu().numpy(), idx.cpu().numpy()
        for r in range(len(users)):
            order = np.lexsort((items, -ref[r]))[:k]
            assert np.array_equal(idx[r], order), (k, r)
            assert np.array_equal(val[r], ref[r, order].astype(np.float32)), (k, r)


def test_evaluate_matches_oracle():
    """Recall/Precision/NDCG/HR@{10,20} of evaluate() == the oracle's
    restatement of Trainer.test on the same propagated embeddings."""
    from furusato_recommend_amd import LightGCN, SyntheticBipartite
    from furusato_recommend_amd.evaluate import evaluate
    from oracle.lightgcn_oracle import OracleLightGCN
    from oracle.lightgcn_oracle import evaluate as oracle_evaluate
    ds = SyntheticBipartite(4000, 900, 50_000, seed=6, test_frac=0.3)
    m = LightGCN({"recdim": 32, "layer": 2, "lr": 1e-3, "decay": 1e-4, "device": "cuda:0",
                  "bpr_batch_size": 512}, ds)
    for _ in range(3):
        m.OneEpoch(*m.sample(2048, seed=1))
    res, top = evaluate(m, ds.testDict, (10, 20), batch=1000, return_topk=True)
    o = OracleLightGCN(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, 32, 2, 1e-3, 1e-4,
                       emb=m.all_embedding.weight.detach().cpu())
    out = o.propagated()
    assert rel(m.propagated(), out) < TOL
    ref = oracle_evaluate(out[:ds.n_users], out[ds.n_users:], ds.testDict, ds.allPos, (10, 20))
    # Every GPU top-20 item against the float64 scores of the oracle's
    # embeddings (train positives excluded): it is in the exact top-20, or its
    # score is within fp32 rounding of the exact 20th score (a near-tie).
    users = np.array(sorted(ds.testDict.keys()), dtype=np.int64)
    o64 = out.double()
    s = (o64[users] @ o64[ds.n_users:].T).numpy()
    for j, u in enumerate(users):
        s[j, np.asarray(ds.allPos[u], dtype=np.int64)] = -np.inf
    kth = -np.sort(-s, axis=1)[:, 19]
    eps = 1e-5 * np.abs(s[np.isfinite(s)]).max()
    picked = np.take_along_axis(s, top[:, :20].astype(np.int64), axis=1)
    exact = picked >= kth[:, None]
    assert np.all(picked >= kth[:, None] - eps)
    n = len(ds.testDict)
    n_tie_users = int((~exact.all(axis=1)).sum())
    assert n_tie_users <= max(2, n // 1000), n_tie_users
    # so a swap can move a user's metrics by at most one hit: the batch sums
    # agree within the near-tie users' share
    for k in res:
        assert np.all(np.abs(res[k] - ref[k]) <= (n_tie_users + 0.5) / n + 1e-9), (k, res[k],
                                                                                 ref[k])


def _near_tie_check(s, top, k, n_users_total):
    """Every picked item of every row of ``top`` [n, >= k] is in the exact
    top-k of the float64 scores ``s`` (train positives at -inf) or within
    fp32 rounding of the exact k-th score; returns the number of rows with
    such a near-tie pick (bounded by the caller)."""
    kth = -np.sort(-s, axis=1)[:, k - 1]
    eps = 1e-5 * np.abs(s[np.isfinite(s)]).max()
    picked = np.take_along_axis(s, top[:, :k].astype(np.int64), axis=1)
    assert np.all(picked >= kth[:, None] - eps)
    return int((~(picked >= kth[:, None]).all(axis=1)).sum())


def test_mf_c1_size_epoch_and_streamed_evaluation():
    """BASELINE config C1 at its stated size (model/MF.py:35-112, README.md
    5-core): 10 000 users x 1 000 items, 4 train + 1 test item per user,
    d = 32, N(0, 1) init.  One OneEpoch over the reference sampler's triples
    (negative_sample.py:98-134, numpy seed 2020) == OracleMF (loss, both
    tables at 1e-4), then evaluate() — the streamed top-k of the raw scores,
    no rating matrix — against the oracle's Trainer.test (trainer.py:115-170)
    on its tables, and checked to be a valid top-20 of the reference's fp32
    sigmoid(U Iᵀ) ratings with train positives at -1024 (model/MF.py:56-60)."""
    from furusato_recommend_amd import MF, FiveCore
    from furusato_recommend_amd.evaluate import evaluate
    from oracle.lightgcn_oracle import OracleMF, uniform_sample
    from oracle.lightgcn_oracle import evaluate as oracle_evaluate
    ds = FiveCore(10_000, 1_000, 5, seed=0)
    cfg = {"latent_dim_rec": 32, "lr": 1e-3, "decay": 1e-4, "device": "cuda:0",
           "bpr_batch_size": 2048}
    torch.manual_seed(2020)
    m = MF(cfg, ds)
    o = OracleMF(m.embedding_user.weight.cpu(), m.embedding_item.weight.cpu(), 1e-3, 1e-4)
    np.random.seed(2020)
    S = uniform_sample(ds.n_users, ds.m_items, ds.allPos, ds.trainDataSize)
    assert len(S) == 40_000
    lg = float(m.OneEpoch(torch.from_numpy(S[:, 0]), torch.from_numpy(S[:, 1]),
                          torch.from_numpy(S[:, 2])))
    acc = 0.0
    for i in range(0, len(S), 2048):
        acc += o.stageOne(S[i:i + 2048, 0], S[i:i + 2048, 1], S[i:i + 2048, 2])
    lo = acc / (len(S) // 2048 + 1)
    assert abs(lg - lo) < TOL * abs(lo)
    assert rel(m.embedding_user.weight, o.user.detach()) < TOL
    assert rel(m.embedding_item.weight, o.item.detach()) < TOL
    res, top = evaluate(m, ds.testDict, (10, 20), return_topk=True)
    users = np.array(sorted(ds.testDict.keys()))
    uo, io = o.user.detach(), o.item.detach()
    raw = (uo.double()[users] @ io.double().T).numpy()
    for j, u in enumerate(users):
        raw[j, ds.allPos[u]] = -np.inf
    n_tie = _near_tie_check(raw, top, 20, len(users))
    assert n_tie <= max(2, len(users) // 1000), n_tie
    # a valid top-20 of the reference's fp32 sigmoid ratings: with N(0, 1)
    # weights the fp32 sigmoid rounds many top scores together (0.30 of the
    # users have a tie across rank 10 or 20 here) and torch.topk breaks such
    # ties arbitrarily, so the set is compared, not the reference's pick
    rating = torch.sigmoid(uo[users] @ io.T)
    for j, u in enumerate(users):
        rating[j, ds.allPos[u]] = -(1 << 10)
    kth = torch.topk(rating, k=20).values[:, -1:]
    picked = torch.gather(rating, 1, torch.from_numpy(top[:, :20]).long())
    assert bool((picked >= kth - 2e-7).all())
    # the metrics against the oracle's Trainer.test on its raw scores
    # (oracle.evaluate: the same ranking without the saturation)
    ref = oracle_evaluate(uo, io, ds.testDict, ds.allPos, (10, 20))
    for k in res:
        assert np.all(np.abs(res[k] - ref[k]) <= (n_tie + 0.5) / len(users) + 1e-9), (k, res[k],
                                                                                     ref[k])


def test_users_rating_propagates_once_per_table_version():
    """getUsersRating (model/lgcn.py:120-125) is called once per 10 000-user
    batch by the reference Trainer.test (trainer.py:130): the propagation is
    reused while the table is unchanged, recomputed after a training step
    and after an in-place write, and always equals a fresh propagation."""
    from furusato_recommend_amd import LightGCN, SyntheticBipartite
    ds = SyntheticBipartite(3000, 500, 30_000, seed=3, test_frac=0)
    m = LightGCN({"recdim": 32, "layer": 3, "lr": 1e-3, "decay": 1e-4, "device": "cuda:0",
                  "bpr_batch_size": 256}, ds)
    calls = []
    fwd = m.engine.forward
    m.engine.forward = lambda *a, **k: (calls.append(1), fwd(*a, **k))[1]
    users = torch.arange(0, 3000, 3, device="cuda")
    r1 = m.getUsersRating(users[:500]).clone()
    m.getUsersRating(users[500:])
    assert len(calls) == 1
    m.stageOne(*m.sample(256, seed=1))
    r2 = m.getUsersRating(users[:500]).clone()
    assert len(calls) == 3  # the step's own (pruned) forward + one full propagation
    assert not torch.equal(r1, r2)
    with torch.no_grad():
        m.all_embedding.weight.mul_(0.5)
    r3 = m.getUsersRating(users[:500])
    assert len(calls) == 4
    m.engine.forward = fwd
    fresh = m.engine.forward(m.all_embedding.weight)
    assert torch.equal(r3, fresh[users[:500]] @ fresh[ds.n_users:].t())


def test_training_trajectory_and_recall_match_oracle():
    """End to end on a graph with structure (communities): 3 epochs of the
    reference's UniformSample triples (same numpy seeds) through OneEpoch on
    the HIP engine and through the CPU oracle; the trained tables agree and
    so does Recall@20, which is far above chance."""
    from furusato_recommend_amd import LightGCN, SyntheticBipartite
    from furusato_recommend_amd.evaluate import evaluate
    from oracle.lightgcn_oracle import OracleLightGCN, uniform_sample
    from oracle.lightgcn_oracle import evaluate as oracle_evaluate
    ds = SyntheticBipartite(2000, 400, 30_000, seed=3, kind="cluster", test_frac=0.2)
    cfg = {"recdim": 32, "layer": 3, "lr": 5e-3, "decay": 1e-4, "device": "cuda:0",
           "bpr_batch_size": 1024}
    torch.manual_seed(0)
    m = LightGCN(cfg, ds)
    o = OracleLightGCN(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, 32, 3, 5e-3, 1e-4,
                       emb=m.all_embedding.weight.detach().cpu().clone())
    for e in range(3):
        np.random.seed(100 + e)
        S = uniform_sample(ds.n_users, ds.m_items, ds.allPos, ds.trainDataSize)
        lg = float(m.OneEpoch(S[:, 0], S[:, 1], S[:, 2]))
        lo = o.OneEpoch(S[:, 0], S[:, 1], S[:, 2], 1024)
        assert abs(lg - lo) < 1e-4 * abs(lo)
    # the north star's 1e-4 rel on the trained tables (measured 1.7e-6)
    assert rel(m.all_embedding.weight, o.emb.detach()) < 1e-4
    res = evaluate(m, ds.testDict, (20,), batch=1000)
    out = o.propagated()
    ref = oracle_evaluate(out[:ds.n_users], out[ds.n_users:], ds.testDict, ds.allPos, (20,))
    n = len(ds.testDict)
    assert abs(res["recall"][0] - ref["recall"][0]) <= 2.0 / n
    assert res["recall"][0] > 3 * 20 / ds.m_items  # far above chance


def test_trainer_epochs_and_checkpoint(tmp_path):
    """Trainer surface: train / test / train_epoch; a reference-style
    state_dict round-trips (key all_embedding.weight)."""
    from furusato_recommend_amd import LightGCN, SyntheticBipartite
    from furusato_recommend_amd.trainer import Trainer
    ds = SyntheticBipartite(3000, 500, 30_000, seed=7, test_frac=0.2)
    cfg = {"recdim": 64, "layer": 3, "lr": 1e-2, "decay": 1e-4, "device": "cuda:0",
           "bpr_batch_size": 1024, "test_span": 1, "checkpoint_path": str(tmp_path / "m.pth")}
    m = LightGCN(cfg, ds)
    t = Trainer(cfg, ds, m)
    hist = t.train_epoch(epochs=3)
    losses = [h["loss"] for h in hist if "loss" in h]
    assert len(losses) == 3 and losses[-1] < losses[0]
    sd = torch.load(tmp_path / "m.pth", weights_only=True)
    assert list(sd.keys()) == ["all_embedding.weight"]
    assert sd["all_embedding.weight"].shape == (3500, 64)
    m2 = LightGCN(cfg, ds)
    m2.load_state_dict(sd)
    assert torch.equal(m2.all_embedding.weight.cpu(), sd["all_embedding.weight"].cpu())


def sage_from(f, dropout=0.0):
    from furusato_recommend_amd import GraphSAGE
    ds = DS(f["train_user"], f["train_item"], f["n_users"], f["m_items"])
    L = int(f["n_layers"])
    cfg = {"recdim": int(f["dim"]), "layer": L, "fanouts": [int(x) for x in f["sizes"]],
           "lr": float(f["lr"]), "decay": float(f["decay"]), "device": "cuda:0",
           "bpr_batch_size": int(f["batch"]), "dropout_p": dropout}
    m = GraphSAGE(cfg, ds)
    with torch.no_grad():
        m._table.copy_(torch.from_numpy(f["table0"]))
        for k, li in enumerate(m.w_linears):
            li.weight.copy_(torch.from_numpy(f[f"w{k}"]))
            li.bias.copy_(torch.from_numpy(f[f"b{k}"]))
    return m


@pytest.mark.parametrize("name", SAGE)
def test_sage_step_matches_reference(golden, name):
    """GraphSAGE forward on the reference's sampled tree, its loss, gradients
    (HIP gather/scatter + fanout mean) and one Adam step == the reference's
    own GraphSAGE.forward / loss + torch Adam (dropout off).  The stepped
    tensors vs the fixture are a MASKED comparison (elements with |g_ref| >=
    1e-6, at least 90 % of them; reason below); on every element the step
    equals torch.optim.Adam applied to this path's gradient, and the
    gradients match the fixture everywhere (the next test)."""
    from furusato_recommend_amd.graphsage import SampleTree
    f = golden(name)
    m = sage_from(f)
    L, B = int(f["n_layers"]), int(f["batch"])
    groups = [torch.from_numpy(g.astype(np.int32)).cuda()
              for g in np.split(f["groups"], np.cumsum(f["group_len"])[:-1])]
    tree = SampleTree.from_groups(groups, L)
    out = m.forward(tree)
    assert rel(out, f["emb_out"][:3 * B]) < TOL
    # stageOne's pieces (graphsage.py:366-397), keeping the gradients the
    # step consumed
    for q in m.parameters():
        q.grad = None
    out = m.forward(tree)
    loss_t = m.loss_fused(out)  # stageOne's loss node
    loss_t.backward()
    grads = {id(m._table): m.table_grad_dense().clone()}
    for li in m.w_linears:
        grads[id(li.weight)] = li.weight.grad.clone()
        grads[id(li.bias)] = li.bias.grad.clone()
    m.optimizer_step()
    loss = float(loss_t)
    # Adam's first step is lr * g / (|g| + eps): for |g| near eps it maps
    # fp32 summation-order noise in g onto the update with a gain of up to
    # lr * eps / (|g| + eps)^2 (~5e4 at |g| = 4e-9), so the reference's own
    # CPU arithmetic under another order moves such elements by ~1e-5.
    # The stepped tensors are compared where the step is well conditioned
    # (|g_ref| >= 1e-6, gain <= 10); the gradients themselves are compared
    # everywhere in test_sage_gradients_match_reference, and the Adam kernel
    # against torch.optim.Adam on this path's own gradient below.
    pairs = [(m._table, "table_step1", "g_table", "table0")]
    pairs += [(li.weight, f"w{k}_step1", f"g_w{k}", f"w{k}") for k, li in enumerate(m.w_linears)]
    pairs += [(li.bias, f"b{k}_step1", f"g_b{k}", f"b{k}") for k, li in enumerate(m.w_linears)]
    for prm, after, gname, before in pairs:
        ok = np.abs(f[gname]) >= 1e-6
        assert ok.mean() > 0.9
        got = prm.detach().cpu().numpy()
        assert rel(got[ok], f[after][ok]) < TOL, after
        ref = torch.nn.Parameter(torch.from_numpy(f[before]).clone())
        ref.grad = grads[id(prm)].detach().cpu().clone()
        torch.optim.Adam([ref], lr=float(f["lr"])).step()
        assert rel(prm, ref) < 1e-6, after


@pytest.mark.parametrize("loss_path", ["torch", "fused"])
@pytest.mark.parametrize("name", SAGE)
def test_sage_gradients_match_reference(golden, name, loss_path):
    """Gradients of every parameter vs the reference's autograd, through the
    torch-op loss (graphsage.py:326-337 written out) and through the fused
    loss node stageOne uses."""
    from furusato_recommend_amd.graphsage import SampleTree
    f = golden(name)
    m = sage_from(f)
    L, B = int(f["n_layers"]), int(f["batch"])
    groups = [torch.from_numpy(g.astype(np.int32)).cuda()
              for g in np.split(f["groups"], np.cumsum(f["group_len"])[:-1])]
    out = m.forward(SampleTree.from_groups(groups, L))
    if loss_path == "torch":
        loss = m.loss(out[:B], out[B:2 * B], out[2 * B:])
    else:
        loss = m.loss_fused(out)
    assert abs(float(loss.detach()) - float(f["loss"])) < TOL * abs(float(f["loss"]))
    loss.backward()
    assert rel(m.table_grad_dense(), f["g_table"]) < TOL
    for k, li in enumerate(m.w_linears):
        assert rel(li.weight.grad, f[f"g_w{k}"]) < TOL
        assert rel(li.bias.grad, f[f"g_b{k}"]) < TOL


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("n", [1, 300, 20_000])
def test_sage_linear_matches_cat_linear(n, relu):
    """The fused hop Linear (two A blocks, bias + ReLU epilogue; masked dY,
    split dX, dW / db in one pass) == cat + Linear + ReLU in float64."""
    from furusato_recommend_amd.linear import sage_linear
    torch.manual_seed(n)
    d, no = 128, 128
    xs = torch.randn(n, d, device="cuda", requires_grad=True)
    xn = torch.randn(n, d, device="cuda", requires_grad=True)
    w = (torch.randn(no, 2 * d, device="cuda") * 0.05).requires_grad_(True)
    b = (torch.randn(no, device="cuda") * 0.1).requires_grad_(True)
    y = sage_linear(xs, xn, w, b, relu)
    gy = torch.randn_like(y)
    y.backward(gy)
    ref_in = [t.detach().double().requires_grad_(True) for t in (xs, xn, w, b)]
    yr = torch.nn.functional.linear(torch.cat(ref_in[:2], 1), ref_in[2], ref_in[3])
    if relu:
        yr = yr.relu()
    yr.backward(gy.double())
    assert rel(y, yr) < 1e-5
    for t, r in zip((xs, xn, w, b), ref_in):
        assert rel(t.grad, r.grad) < 1e-5


def test_fanout_sampler_and_dropout_mean():
    """Fixed-fanout sampling with replacement (neighbor_sampling.py:14-30):
    children come from the CSR row, uniformly; isolated nodes give -1.
    Dropout mean: E[mean] == plain mean, backward consistent with forward."""
    import ctypes

    from furusato_recommend_amd import SyntheticBipartite, _lib
    from furusato_recommend_amd.graph import Graph
    ds = SyntheticBipartite(300, 60, 3000, seed=9, test_frac=0)
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    nodes = torch.arange(g.n_nodes, dtype=torch.int32, device="cuda")
    k = 400
    ch = torch.empty(g.n_nodes * k, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib.mirec_sample_fanout(g.csr_ptr(), nodes.data_ptr(), g.n_nodes, k,
                                            ctypes.c_uint64(3), ctypes.c_uint64(0), ch.data_ptr(),
                                            _lib.stream_handle()), "sample")
    ch = ch.view(g.n_nodes, k).cpu().numpy()
    deg = g.degree()
    for v in range(0, g.n_nodes, 7):
        row = g.col_host[g.rowptr_host[v]:g.rowptr_host[v + 1]]
        if deg[v] == 0:
            assert np.all(ch[v] == -1)
            continue
        assert np.all(np.isin(ch[v], row))
        # multiplicity-aware uniformity over the row's entries (chi-square)
        vals, cnt = np.unique(row, return_counts=True)
        obs = np.array([(ch[v] == x).sum() for x in vals])
        exp = cnt / cnt.sum() * k
        chi2 = float(((obs - exp) ** 2 / exp).sum())
        assert chi2 < len(vals) - 1 + 8 * np.sqrt(2 * max(len(vals) - 1, 1)) + 10
    x = torch.randn(4000 * 8, 64, device="cuda")
    valid = torch.zeros(4000 * 8, dtype=torch.int32, device="cuda")
    plain = torch.empty(4000, 64, device="cuda")
    drop = torch.empty_like(plain)
    for p, out in ((0.0, plain), (0.2, drop)):
        _lib.check(_lib.lib.mirec_fanout_mean(x.data_ptr(), valid.data_ptr(), 4000, 8, 64, p,
                                              ctypes.c_uint64(5), out.data_ptr(),
                                              _lib.stream_handle()), "mean")
    assert rel(plain, x.view(4000, 8, 64).mean(1)) < 1e-6
    assert abs(float((drop - plain).mean())) < 0.01
    gx = torch.empty_like(x)
    go = torch.randn(4000, 64, device="cuda")
    _lib.check(_lib.lib.mirec_fanout_mean_bwd(go.data_ptr(), valid.data_ptr(), 4000, 8, 64, 0.2,
                                              ctypes.c_uint64(5), gx.data_ptr(),
                                              _lib.stream_handle()), "bwd")
    # <go, mean(x)> == <gx, x> (the backward is the forward's adjoint)
    assert abs(float((go * drop).sum()) - float((gx * x).sum())) < 1e-3 * float((go * drop).abs().sum())


def test_sage_full_graph_inference_and_training():
    """getUsersRating('all') == layer-wise full-neighbourhood means on the CPU;
    a few OneEpoch steps with dropout reduce the loss."""
    from furusato_recommend_amd import GraphSAGE, SyntheticBipartite
    ds = SyntheticBipartite(2000, 400, 20_000, seed=10, test_frac=0.1)
    m = GraphSAGE({"recdim": 32, "layer": 2, "fanouts": [8, 4], "lr": 5e-3, "decay": 1e-5,
                   "device": "cuda:0", "bpr_batch_size": 256}, ds)
    out = m.propagated()
    # CPU reference of graphsage.py:401-424 (scatter mean over train edges)
    x = m._table.detach().cpu()
    tu = torch.from_numpy(ds.trainUser)
    ti = torch.from_numpy(ds.trainItem) + ds.n_users
    src = torch.cat([ti, tu])
    dst = torch.cat([tu, ti])
    for i, li in enumerate(m.w_linears):
        agg = torch.zeros_like(x).index_add_(0, dst, x[src])
        cnt = torch.zeros(x.shape[0]).index_add_(0, dst, torch.ones(len(dst))).clamp(min=1)
        x = torch.nn.functional.linear(torch.cat([x, agg / cnt[:, None]], 1),
                                       li.weight.detach().cpu(), li.bias.detach().cpu())
        if i == 0:
            x = x.relu()
    assert rel(out, x) < TOL
    losses = [float(m.OneEpoch(*m.sample(2048, seed=s))) for s in range(6)]
    assert losses[-1] < losses[0]


def sasrec_from(f):
    from furusato_recommend_amd import SASRec
    from furusato_recommend_amd.sasrec import SequenceData

    class Tiny:
        n_users, m_items = 6, 10

    d, heads, L = int(f["d"]), int(f["heads"]), int(f["L"])
    m = SASRec({"recdim": d, "layer": L, "heads": heads, "lr": 1e-3, "decay": 1e-4,
                "device": "cuda:0", "bpr_batch_size": 6, "dropout_p": 0.0}, Tiny,
               sequences=SequenceData.synthetic(6, 10, "cuda:0", max_len=50))
    with torch.no_grad():
        for i in range(L):
            a = m.attn_layers[i]
            a.in_proj_weight.copy_(torch.from_numpy(f[f"in_w{i}"]))
            a.in_proj_bias.copy_(torch.from_numpy(f[f"in_b{i}"]))
            a.out_proj.weight.copy_(torch.from_numpy(f[f"out_w{i}"]))
            a.out_proj.bias.copy_(torch.from_numpy(f[f"out_b{i}"]))
            m.attn_norm_layers[i].weight.copy_(torch.from_numpy(f[f"ln1_w{i}"]))
            m.attn_norm_layers[i].bias.copy_(torch.from_numpy(f[f"ln1_b{i}"]))
            m.ffn_norm_layers[i].weight.copy_(torch.from_numpy(f[f"ln2_w{i}"]))
            m.ffn_norm_layers[i].bias.copy_(torch.from_numpy(f[f"ln2_b{i}"]))
            m.ffn_layers[i].weight.copy_(torch.from_numpy(f[f"ffn_w{i}"]))
            m.ffn_layers[i].bias.copy_(torch.from_numpy(f[f"ffn_b{i}"]))
    return m


@pytest.fixture(params=["hybrid", "wave", "block"])
def attn_impl(request, monkeypatch):
    """Every attention core: one wave per (sequence, head), one workgroup per
    (sequence, head), and the wave forward + ordered workgroup backward
    (sasrec.ATTN_IMPL)."""
    from furusato_recommend_amd import sasrec as S
    monkeypatch.setattr(S, "ATTN_IMPL", request.param)
    return request.param


@pytest.mark.parametrize("name", ["sasrec_d64_h8.npz", "sasrec_d128_h2.npz"])
def test_sasrec_attention_block_matches_reference(golden, name, attn_impl):
    """The SASRec block with the MFMA attention core (fwd + bwd) == the
    reference's forward_user over torch.nn.MultiheadAttention: outputs and
    the gradients of the input and of every block parameter."""
    f = golden(name)
    m = sasrec_from(f)
    L = int(f["L"])
    x = torch.from_numpy(f["x"]).cuda().requires_grad_(True)
    length = torch.from_numpy(f["lengths"]).cuda()
    out = m.forward_user(x, length)
    assert rel(out, f["out"]) < TOL
    (out * torch.from_numpy(f["wts"]).cuda()).sum().backward()
    assert rel(x.grad, f["g_x"]) < TOL
    for i in range(L):
        a = m.attn_layers[i]
        pairs = [(a.in_proj_weight, "in_w"), (a.in_proj_bias, "in_b"),
                 (a.out_proj.weight, "out_w"), (a.out_proj.bias, "out_b"),
                 (m.attn_norm_layers[i].weight, "ln1_w"), (m.ffn_layers[i].weight, "ffn_w")]
        for prm, key in pairs:
            assert rel(prm.grad, f[f"g_{key}{i}"]) < TOL, (key, i)


def test_sasrec_attention_kernel_vs_torch_sdpa(attn_impl):
    """Raw kernel vs torch's causal SDPA (fp32) over every supported head dim
    and T up to 64, fwd and bwd."""
    import torch.nn.functional as F

    from furusato_recommend_amd.sasrec import _CausalAttention
    torch.manual_seed(0)
    for heads, dh, T in ((8, 16, 50), (2, 64, 64), (4, 32, 7), (1, 64, 1), (8, 8, 33), (3, 48, 20)):
        d = heads * dh
        qkv = torch.randn(5, T, 3 * d, device="cuda", requires_grad=True)
        out = _CausalAttention.apply(qkv, heads)
        q, k, v = qkv.split(d, dim=2)
        sh = lambda t: t.reshape(5, T, heads, dh).transpose(1, 2)  # noqa: E731
        ref = F.scaled_dot_product_attention(sh(q), sh(k), sh(v), is_causal=True)
        ref = ref.transpose(1, 2).reshape(5, T, d)
        assert rel(out, ref) < TOL
        go = torch.randn_like(out)
        g1, = torch.autograd.grad(out, qkv, go)
        g2, = torch.autograd.grad(ref, qkv, go)
        assert rel(g1, g2) < TOL


def test_sasrec_varlen_attention_matches_padded(attn_impl):
    """Packed (varlen) kernels == padded kernels on every real row, fwd and
    bwd (padding rows carry zero output gradient, as under the pooled loss),
    incl. lengths 1 and 64 and a zero-length sequence."""
    from furusato_recommend_amd.sasrec import _CausalAttention, _CausalAttentionVarlen
    torch.manual_seed(1)
    for heads, dh in ((2, 64), (8, 16), (3, 20)):
        d, T = heads * dh, 64
        lens = torch.tensor([1, 64, 17, 0, 50, 33])
        B = lens.numel()
        qkv = torch.randn(B, T, 3 * d, device="cuda")
        mask = (torch.arange(T)[None, :] < lens[:, None]).cuda()
        go = torch.randn(B, T, d, device="cuda") * mask.unsqueeze(2)
        qp = qkv.clone().requires_grad_(True)
        out_p = _CausalAttention.apply(qp, heads)
        gp, = torch.autograd.grad(out_p, qp, go)
        offsets = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
        offsets[1:] = torch.cumsum(lens.cuda(), 0).int()
        qv = qkv[mask].clone().requires_grad_(True)
        out_v = _CausalAttentionVarlen.apply(qv, offsets, heads)
        gv, = torch.autograd.grad(out_v, qv, go[mask])
        assert rel(out_v, out_p[mask]) < TOL
        assert rel(gv, gp[mask]) < TOL


def test_sasrec_bucketed_attention_matches_varlen():
    """Length-bucketed launches (workgroups of 16*NB rows) == the one-bucket
    packed kernels, fwd and bwd, at every bucket edge (0, 1, 16, 17, 32, 33,
    48, 49, 64), with empty buckets, odd head dims and dh = 64; malformed
    bucket counts are rejected."""
    from furusato_recommend_amd import sasrec as S
    from furusato_recommend_amd.sasrec import _CausalAttentionVarlen, length_buckets
    prev, S.ATTN_IMPL = S.ATTN_IMPL, "block"
    try:
        _bucketed_vs_varlen()
    finally:
        S.ATTN_IMPL = prev


def _bucketed_vs_varlen():
    from furusato_recommend_amd.sasrec import _CausalAttentionVarlen, length_buckets
    torch.manual_seed(2)
    edge = [0, 1, 16, 17, 32, 33, 48, 49, 64, 5, 50, 40, 23, 9]
    for heads, dh, lens in (((2, 64, edge)), ((8, 16, edge)), ((3, 20, edge)),
                            ((2, 64, [3, 7, 12, 16])), ((1, 32, [60, 64, 49])),
                            ((2, 8, [20, 33, 1]))):
        order, be = length_buckets(lens)
        lens_o = torch.tensor(lens)[torch.from_numpy(order)]
        d, B = heads * dh, len(lens)
        offsets = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
        offsets[1:] = torch.cumsum(lens_o.cuda(), 0).int()
        n = int(lens_o.sum())
        qkv = torch.randn(n, 3 * d, device="cuda")
        go = torch.randn(n, d, device="cuda")
        q1 = qkv.clone().requires_grad_(True)
        o1 = _CausalAttentionVarlen.apply(q1, offsets, heads)
        g1, = torch.autograd.grad(o1, q1, go)
        q2 = qkv.clone().requires_grad_(True)
        o2 = _CausalAttentionVarlen.apply(q2, offsets, heads, be)
        g2, = torch.autograd.grad(o2, q2, go)
        assert rel(o2, o1) < TOL and rel(g2, g1) < TOL
    with pytest.raises(ValueError):
        _CausalAttentionVarlen.apply(qkv, offsets, heads, (0, 2, 1, B))


def test_attention_wave_matches_block_and_repeats(monkeypatch):
    """The wave-per-(sequence, head) core == the workgroup core on packed
    sequences at every block edge (0, 1, 16, 17, ..., 64 positions), fwd and
    bwd, for head dims 16 / 32 / 64; reruns are bitwise equal; head dims it
    does not take (20) fall back to the workgroup core."""
    from furusato_recommend_amd import _lib
    from furusato_recommend_amd import sasrec as S
    from furusato_recommend_amd.sasrec import _CausalAttentionVarlen
    assert [int(_lib.lib.mirec_attention_wave_supported(x)) for x in (8, 16, 20, 32, 64)] == \
        [0, 1, 0, 1, 1]
    monkeypatch.setattr(S, "ATTN_IMPL", "hybrid")  # restored after the test
    torch.manual_seed(3)
    lens = [0, 1, 16, 17, 32, 33, 48, 49, 64, 5, 50, 40, 23, 9]
    offsets = torch.zeros(len(lens) + 1, dtype=torch.int32, device="cuda")
    offsets[1:] = torch.cumsum(torch.tensor(lens), 0).int().cuda()
    n = sum(lens)
    for heads, dh in ((2, 64), (8, 16), (4, 32), (3, 20)):
        d = heads * dh
        qkv = torch.randn(n, 3 * d, device="cuda")
        go = torch.randn(n, d, device="cuda")
        res = {}
        for impl in ("block", "wave", "wave", "hybrid"):
            S.ATTN_IMPL = impl
            q = qkv.clone().requires_grad_(True)
            o = _CausalAttentionVarlen.apply(q, offsets, heads)
            g, = torch.autograd.grad(o, q, go)
            if impl in res:
                assert torch.equal(o, res[impl][0]) and torch.equal(g, res[impl][1])
            res[impl] = (o, g)
        S.ATTN_IMPL = "wave"
        for impl in ("wave", "hybrid"):
            assert rel(res[impl][0], res["block"][0]) < TOL, (impl, heads, dh)
            assert rel(res[impl][1], res["block"][1]) < TOL, (impl, heads, dh)


@pytest.mark.parametrize("heads,dh", [(2, 64), (4, 32), (8, 16)])
def test_packed_bwd_from_forward_lse_equals_recomputed(heads, dh):
    """mirec_attention_packed_bwd_lse (phase A's P from the wave forward's
    base-2 lse: no max / sum reductions) ==
    mirec_attention_packed_bwd (softmax statistics recomputed in the kernel)
    on packed sequences at every block edge, capacity padding rows zero in
    both; reruns bitwise equal."""
    from furusato_recommend_amd import _lib
    from furusato_recommend_amd.sasrec import _length_order
    lib, st = _lib.lib, _lib.stream_handle()
    torch.manual_seed(11)
    lens = torch.tensor([0, 1, 16, 17, 32, 33, 48, 49, 64, 5, 50, 40, 23, 9, 2, 3, 4, 31])
    B, n = len(lens), int(lens.sum())
    cap = n + 300
    d = heads * dh
    offs = torch.zeros(B + 1, dtype=torch.int32)
    offs[1:] = torch.cumsum(lens, 0)
    offs = offs.cuda()
    qkv = torch.randn(cap, 3 * d, device="cuda")
    dout = torch.randn(cap, d, device="cuda")
    out = torch.empty(cap, d, device="cuda")
    lse = torch.empty(cap, heads, device="cuda")
    order = _length_order(offs, B)
    packs = order[-(-B // 4) * 4:]
    _lib.check(lib.mirec_attention_wave_fwd(qkv.data_ptr(), offs.data_ptr(), order.data_ptr(), B,
                                            0, heads, dh, out.data_ptr(), lse.data_ptr(), cap,
                                            st), "wave_fwd")
    res = []
    for stats in (False, True, True):
        g = torch.full_like(qkv, float("nan"))
        if stats:
            rc = lib.mirec_attention_packed_bwd_lse(
                qkv.data_ptr(), lse.data_ptr(), dout.data_ptr(), offs.data_ptr(),
                packs.data_ptr(), B, heads, dh, g.data_ptr(), cap, st)
        else:
            rc = lib.mirec_attention_packed_bwd(qkv.data_ptr(), dout.data_ptr(), offs.data_ptr(),
                                                packs.data_ptr(), B, heads, dh, g.data_ptr(), cap,
                                                st)
        _lib.check(rc, "packed_bwd")
        assert torch.isfinite(g).all() and float(g[n:].abs().max()) == 0.0
        res.append(g)
    assert torch.equal(res[1], res[2])
    assert rel(res[1][:n], res[0][:n]) < 1e-5


def test_attention_capacity_padding_rows_zero(attn_impl):
    """A capacity-padded packed batch (the captured step's form): the rows
    past the last sequence come out zero in the output and in dqkv, even when
    the buffers held NaN before (the zeroing is folded into the ordering
    pass and the packed backward's spare workgroups)."""
    from furusato_recommend_amd.sasrec import _CausalAttentionVarlen
    torch.manual_seed(4)
    heads, dh = 2, 64
    d = heads * dh
    lens = torch.tensor([5, 50, 17, 33, 1, 64, 16, 0, 40])
    n_tok, cap = int(lens.sum()), int(lens.sum()) + 1500
    offsets = torch.zeros(len(lens) + 1, dtype=torch.int32, device="cuda")
    offsets[1:] = torch.cumsum(lens, 0).int().cuda()
    qkv = torch.randn(cap, 3 * d, device="cuda")
    for _ in range(2):
        junk = torch.full((cap, 3 * d), float("nan"), device="cuda")  # freed: reused below
        del junk
        q = qkv.clone().requires_grad_(True)
        out = _CausalAttentionVarlen.apply(q, offsets, heads, None, True)
        go = torch.randn_like(out)
        go[n_tok:] = 0
        g, = torch.autograd.grad(out, q, go)
        assert torch.isfinite(out).all() and float(out[n_tok:].abs().max()) == 0.0
        assert torch.isfinite(g).all() and float(g[n_tok:].abs().max()) == 0.0


def test_sasrec_packed_path_equals_padded():
    """The training path (packed sequences) gives the padded path's user
    embeddings and parameter gradients (dropout off)."""
    from furusato_recommend_amd import SASRec, SyntheticBipartite
    ds = SyntheticBipartite(600, 300, 12_000, seed=5)
    torch.manual_seed(0)
    m = SASRec({"recdim": 64, "layer": 2, "heads": 2, "lr": 1e-3, "decay": 1e-4,
                "device": "cuda:0", "bpr_batch_size": 128, "dropout_p": 0.0}, ds)
    u_h = np.random.default_rng(0).integers(0, 600, 128)
    for buckets in (False, True):  # caller order / length-bucket order
        m.config["attn_buckets"] = buckets
        x, offs, seg, length = m.packed_input(u_h)
        assert (offs.order is not None) == buckets
        up = m.forward_user_packed(x, offs, seg, length)
        xp, lp = m.sequence_input(torch.as_tensor(u_h, device="cuda"))
        ud = m.forward_user(xp, lp)
        assert rel(up, ud) < TOL
        w = torch.randn_like(up)
        params = [p for p in m.parameters() if p.requires_grad]
        g1 = torch.autograd.grad((up * w).sum(), params, allow_unused=True)
        g2 = torch.autograd.grad((ud * w).sum(), params, allow_unused=True)
        for a, b in zip(g1, g2):
            if b is None:
                assert a is None or float(a.abs().max()) == 0.0
            else:
                assert rel(a, b) < TOL


@pytest.mark.parametrize("d", [4, 12, 36, 64, 128, 256, 1024])
def test_resnorm_rows_match_torch(d):
    """mirec_resnorm_* (the fused dropout / residual / ReLU / LayerNorm row
    pass) == the torch composition, fwd and every gradient incl. the column
    sums, for the padded shapes of the dispatch (d/4 not a power of two,
    several float4 per lane) and row counts 0, 1 and many."""
    import torch.nn.functional as F

    from furusato_recommend_amd.sasrec import resnorm
    torch.manual_seed(d)
    for n in (0, 1, 3001):
        for relu, with_res in ((True, True), (False, True), (False, False)):
            res = torch.randn(n, d, device="cuda", requires_grad=True) if with_res else None
            z = torch.randn(n, d, device="cuda", requires_grad=True)
            bias = (torch.randn(d, device="cuda") * 0.1).requires_grad_(True) if with_res else None
            ln = torch.nn.LayerNorm(d, device="cuda")
            with torch.no_grad():
                ln.weight.uniform_(0.5, 1.5)
                ln.bias.uniform_(-0.2, 0.2)
            out, y = resnorm(res, z, bias, ln, relu=relu)
            pre = z if not with_res else res + (z + bias)
            o_ref = pre.relu() if relu else pre
            y_ref = F.layer_norm(o_ref, (d,), ln.weight, ln.bias, ln.eps)
            if n:
                assert out is None or rel(out, o_ref) < TOL
                assert rel(y, y_ref) < TOL
            go = torch.randn(n, d, device="cuda")
            gy = torch.randn(n, d, device="cuda")
            leaves = [t for t in (res, z, bias, ln.weight, ln.bias) if t is not None]
            outs = [y] + ([out] if out is not None else [])
            grads_in = [gy] + ([go] if out is not None else [])
            g1 = torch.autograd.grad(outs, leaves, grads_in)
            outs_r = [y_ref] + ([o_ref] if out is not None else [])
            g2 = torch.autograd.grad(outs_r, leaves, grads_in)
            for a, b in zip(g1, g2):
                if n:
                    assert rel(a, b) < TOL
                else:
                    assert float(a.abs().sum()) == 0.0


@pytest.mark.parametrize("layers", [1, 2, 3])
def test_blocks_with_fused_qkv_equal_separate_projections(layers):
    """SASRec.blocks with every LayerNorm -> QKV projection pair inside one
    node (_LnQkvHead, _BlockTail with the next layer's projection: the
    projection's input gradient meets the LayerNorm backward in one kernel)
    == the same blocks with the projections as their own nodes: forward bit
    for bit, every parameter and input gradient to fp32 rounding."""
    from furusato_recommend_amd import SASRec
    from furusato_recommend_amd import sasrec as S

    class DS:
        n_users, m_items, allPos = 50, 300, [[1, 2]] * 50

    m = SASRec({"recdim": 128, "layer": layers, "heads": 2, "lr": 1e-3, "decay": 1e-4,
                "device": "cuda:0", "dropout_p": 0.2}, DS)
    lens = torch.randint(1, 51, (300,), generator=torch.Generator().manual_seed(layers))
    offsets = torch.zeros(301, dtype=torch.int32)
    offsets[1:] = torch.cumsum(lens, 0)
    offsets = offsets.cuda()
    n = int(lens.sum())
    x = torch.randn(n, 128, device="cuda", requires_grad=True)
    runs = []
    for fuse in (True, False):
        S.FUSE_QKV = fuse
        try:
            torch.manual_seed(5)  # dropout seeds
            out = m.blocks(x, offsets)
        finally:
            S.FUSE_QKV = True
        g = torch.randn(out.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        grads = torch.autograd.grad(out, [x] + list(m.parameters()), g, allow_unused=True)
        runs.append((out.detach(), grads))
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        if a is None or b is None:
            assert a is None and b is None
            continue
        assert rel(a, b) < 1e-6


@pytest.mark.parametrize("has_next", [True, False])
def test_block_tail_equals_two_linear_resnorm_nodes(has_next):
    """The fused layer tail (one node: two mirec_gemm_resnorm forwards, the
    FFN's input gradient handed to the first row tail's backward inside
    mirec_gemm_nn_resnorm_bwd) == the two linear_resnorm nodes: forward bit
    for bit; gradients to fp32 rounding (the second stage's bit for bit; the
    first stage's row arithmetic is the same expression compiled in another
    kernel — ~1 ulp — and its column sums run per 64-row tile)."""
    from furusato_recommend_amd import sasrec as S
    d = 128
    for n in (1, 777, 56321):
        torch.manual_seed(n)
        o = torch.randn(n, d, device="cuda", requires_grad=True)
        res = torch.randn(n, d, device="cuda", requires_grad=True)
        w_o = (torch.randn(d, d, device="cuda") * d ** -0.5).requires_grad_(True)
        w_f = (torch.randn(d, d, device="cuda") * d ** -0.5).requires_grad_(True)
        b_o = (torch.randn(d, device="cuda") * 0.1).requires_grad_(True)
        b_f = (torch.randn(d, device="cuda") * 0.1).requires_grad_(True)
        ln_f = torch.nn.LayerNorm(d, device="cuda")
        ln_n = torch.nn.LayerNorm(d, device="cuda") if has_next else None
        with torch.no_grad():
            for ln in (ln_f, ln_n):
                if ln is not None:
                    ln.weight.uniform_(0.5, 1.5)
                    ln.bias.uniform_(-0.2, 0.2)
        outs = []
        for fuse in (True, False):
            S.FUSE_BLOCK_TAIL = fuse
            try:
                torch.manual_seed(11)  # the dropout seeds come from torch's CPU generator
                r2, y2 = S.block_tail(o, res, w_o, b_o, ln_f, w_f, b_f, ln_n, p=0.2)
            finally:
                S.FUSE_BLOCK_TAIL = True
            outs.append((r2, y2))
        (r_a, y_a), (r_b, y_b) = outs
        assert torch.equal(r_a, r_b)
        assert (y_a is None) == (y_b is None) and (y_a is None or torch.equal(y_a, y_b))
        g_r = torch.randn(n, d, device="cuda")
        g_y = torch.randn(n, d, device="cuda") if has_next else None
        leaves_row = [o, res, w_o, w_f]
        leaves_col = [b_o, b_f, ln_f.weight, ln_f.bias] + (
            [ln_n.weight, ln_n.bias] if has_next else [])
        grads = []
        for r2, y2 in outs:
            ys, gs = [r2], [g_r]
            if has_next:
                ys.append(y2)
                gs.append(g_y)
            grads.append(torch.autograd.grad(ys, leaves_row + leaves_col, gs))
        for a, b in zip(grads[0], grads[1]):
            assert rel(a, b) < 1e-6


def test_gemm_nn_resnorm_bwd_repeatable():
    """mirec_gemm_nn_resnorm_bwd (g_y = A W and the row tail's backward in one
    kernel) == gemm_nn_ex + mirec_resnorm_bwd to fp32 rounding, and bit for
    bit repeatable over 12 launches, at ragged and aligned row counts: with
    exec-masked loads of its row data and the bf16x6 k loop, up to one
    launch in two at n = 56321 gave one row with wrong statistics
    (gemm.hip, tools/dbg_rnbwd.py)."""
    from furusato_recommend_amd import _lib
    from furusato_recommend_amd.linear import gemm_nn
    lib, st = _lib.lib, _lib.stream_handle()
    d = 128
    for n in (56321, 56320, 777):
        torch.manual_seed(n)
        A = torch.randn(n, d, device="cuda")
        W = torch.randn(d, d, device="cuda") * d ** -0.5
        out = torch.randn(n, d, device="cuda")
        mean = out.mean(1)
        rstd = (out.var(1, unbiased=False) + 1e-5).rsqrt()
        g_out = torch.randn(n, d, device="cuda")
        gamma = torch.rand(d, device="cuda") + 0.5
        ref = [torch.empty(n, d, device="cuda"), torch.empty(n, d, device="cuda")] + [
            torch.empty(d, device="cuda") for _ in range(3)]
        work = torch.empty(int(lib.mirec_resnorm_work_floats(n, d)), device="cuda")
        _lib.check(lib.mirec_resnorm_bwd(gemm_nn(A, W).data_ptr(), g_out.data_ptr(),
                                         out.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                         gamma.data_ptr(), n, d, 1, 0.0, 0, None,
                                         *[t.data_ptr() for t in ref[:2]], work.data_ptr(),
                                         *[t.data_ptr() for t in ref[2:]], st), "resnorm_bwd")
        first = None
        for _ in range(12):
            got = [torch.empty(n, d, device="cuda"), torch.empty(n, d, device="cuda")] + [
                torch.empty(d, device="cuda") for _ in range(3)]
            work1 = torch.empty(int(lib.mirec_gemm_nn_resnorm_bwd_work_floats(n, d)),
                                device="cuda")
            _lib.check(lib.mirec_gemm_nn_resnorm_bwd(
                A.data_ptr(), W.data_ptr(), n, d, d, g_out.data_ptr(), out.data_ptr(),
                mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), 1, 0.0, 0, None,
                *[t.data_ptr() for t in got[:2]], work1.data_ptr(),
                *[t.data_ptr() for t in got[2:]], st), "gemm_nn_resnorm_bwd")
            for a, b in zip(got, ref):
                assert rel(a, b) < 1e-6
            if first is None:
                first = got
            assert all(torch.equal(a, b) for a, b in zip(got, first))


def test_gemm_resnorm_repeatable():
    """mirec_gemm_resnorm (bf16x6 k loop + row tail) bit for bit repeatable
    over 12 launches (out, y, mean, rstd) at ragged and aligned row counts —
    the companion of test_gemm_nn_resnorm_bwd_repeatable."""
    from furusato_recommend_amd import _lib
    lib, st = _lib.lib, _lib.stream_handle()
    d = 128
    for n, k in ((56321, 128), (56320, 256), (777, 128)):
        torch.manual_seed(n + k)
        x = torch.randn(n, k, device="cuda")
        w = torch.randn(d, k, device="cuda") * k ** -0.5
        res = torch.randn(n, d, device="cuda")
        bias = torch.randn(d, device="cuda") * 0.1
        gam = torch.rand(d, device="cuda") + 0.5
        bet = torch.randn(d, device="cuda") * 0.1
        first = None
        for _ in range(12):
            out = torch.empty(n, d, device="cuda")
            y = torch.empty_like(out)
            mean = torch.empty(n, device="cuda")
            rstd = torch.empty_like(mean)
            _lib.check(lib.mirec_gemm_resnorm(x.data_ptr(), w.data_ptr(), n, k, d, res.data_ptr(),
                                              bias.data_ptr(), gam.data_ptr(), bet.data_ptr(), 1,
                                              0.0, 0, None, 1e-5, out.data_ptr(), y.data_ptr(),
                                              mean.data_ptr(), rstd.data_ptr(), st), "gemm_resnorm")
            got = (out, y, mean, rstd)
            if first is None:
                first = got
                pre = res + (x.double() @ w.double().t() + bias.double()).float()
                assert rel(out, torch.relu(pre)) < 1e-6
            assert all(torch.equal(a, b) for a, b in zip(got, first))


@pytest.mark.parametrize("k", [128, 256])
def test_gemm_resnorm_equals_two_kernel_path(k):
    """mirec_gemm_resnorm (the Linear and the row tail in one kernel) ==
    linear() then resnorm() bit for bit in the forward (same MFMA k loop,
    same per-row arithmetic), dropout masks included; gradients of x, W,
    res, bias, gamma, beta equal the two-node chain.  Row counts around the
    64 / 128-row tiles, with and without ReLU / LayerNorm / dropout."""
    from furusato_recommend_amd import sasrec as S
    from furusato_recommend_amd.linear import linear
    d = 128
    for n, relu, norm, p in ((1, True, True, 0.0), (1000, True, True, 0.2),
                             (56321, False, True, 0.2), (3000, False, False, 0.0),
                             (70000, True, False, 0.1)):
        torch.manual_seed(n + k)
        x = torch.randn(n, k, device="cuda", requires_grad=True)
        w = (torch.randn(d, k, device="cuda") * k ** -0.5).requires_grad_(True)
        res = torch.randn(n, d, device="cuda", requires_grad=True)
        bias = (torch.randn(d, device="cuda") * 0.1).requires_grad_(True)
        ln = torch.nn.LayerNorm(d, device="cuda") if norm else None
        if ln is not None:
            with torch.no_grad():
                ln.weight.uniform_(0.5, 1.5)
                ln.bias.uniform_(-0.2, 0.2)
        torch.manual_seed(7)  # the dropout seed is drawn from torch's CPU generator
        out1, y1 = S.linear_resnorm(x, w, res, bias, ln, relu=relu, p=p)
        torch.manual_seed(7)
        out2, y2 = S.resnorm(res, linear(x, w), bias, ln, relu=relu, p=p)
        assert torch.equal(out1, out2)
        assert (y1 is None) == (y2 is None) and (y1 is None or torch.equal(y1, y2))
        go = torch.randn(n, d, device="cuda")
        outs1, outs2, gin = [out1], [out2], [go]
        if norm:
            gy = torch.randn(n, d, device="cuda")
            outs1.append(y1)
            outs2.append(y2)
            gin.append(gy)
        leaves = [x, w, res, bias] + ([ln.weight, ln.bias] if norm else [])
        g1 = torch.autograd.grad(outs1, leaves, gin)
        g2 = torch.autograd.grad(outs2, leaves, gin)
        for a, b in zip(g1, g2):
            assert torch.equal(a, b)


def test_resnorm_dropout_mask_is_recomputed():
    """With p > 0: kept entries are scaled by 1/(1-p), the kept fraction is
    1-p, and the backward applies the same mask (d_z = keep * g / (1-p))."""
    from furusato_recommend_amd.sasrec import resnorm
    torch.manual_seed(3)
    n, d, p = 20000, 128, 0.3
    z = (torch.rand(n, d, device="cuda") + 0.5).requires_grad_(True)
    res = torch.zeros(n, d, device="cuda", requires_grad=True)
    out, _ = resnorm(res, z, p=p)
    kept = out != 0
    frac = float(kept.float().mean())
    assert abs(frac - (1 - p)) < 0.005
    assert rel(out[kept], z.detach()[kept] / (1 - p)) < 1e-6
    g = torch.randn(n, d, device="cuda")
    gr, gz = torch.autograd.grad(out, [res, z], g)
    assert torch.equal(gr, g)
    assert rel(gz, g * kept / (1 - p)) < 1e-6
    out2, _ = resnorm(res, z, p=p)   # a fresh draw
    assert not torch.equal(out2 != 0, kept)


@pytest.mark.parametrize("d,heads", [(64, 2), (128, 2), (48, 3)])
def test_sasrec_fused_blocks_equal_oneblock_chain(d, heads):
    """SASRec.blocks (fused row passes) == the reference-shaped oneblock
    chain (nn.LayerNorm, nn.Dropout, separate residual / ReLU), dropout
    off, packed and padded: outputs and every parameter / input gradient."""
    from furusato_recommend_amd import SASRec, SyntheticBipartite
    ds = SyntheticBipartite(400, 200, 8_000, seed=2)
    torch.manual_seed(1)
    m = SASRec({"recdim": d, "layer": 3, "heads": heads, "lr": 1e-3, "decay": 1e-4,
                "device": "cuda:0", "bpr_batch_size": 64, "dropout_p": 0.0}, ds)
    with torch.no_grad():
        for ln in list(m.attn_norm_layers) + list(m.ffn_norm_layers):
            ln.weight.uniform_(0.5, 1.5)
            ln.bias.uniform_(-0.2, 0.2)
    params = [p for mod in (m.attn_layers, m.attn_norm_layers, m.ffn_norm_layers, m.ffn_layers)
              for p in mod.parameters()]
    x, offs, _, _ = m.packed_input(np.random.default_rng(0).integers(0, 400, 64))
    xp = torch.randn(7, 50, d, device="cuda")
    for inp, o in ((x.detach(), offs), (xp, None)):
        inp = inp.clone().requires_grad_(True)
        fused = m.blocks(inp, o)
        ref = inp
        for i in range(m.num_layers):
            ref = m.oneblock(ref, i, o)
        assert rel(fused, ref) < TOL
        w = torch.randn_like(ref)
        g1 = torch.autograd.grad((fused * w).sum(), [inp] + params)
        g2 = torch.autograd.grad((ref * w).sum(), [inp] + params)
        for a, b in zip(g1, g2):
            assert rel(a, b) < TOL


def test_sasrec_stage_one_equals_unfused_composition():
    """stageOne (one lookup for sequences / positives / negatives, one item
    tower pass, fused block rows) == the reference-shaped step (separate
    lookups, the tower once per side, oneblock chain): loss, every gradient
    and every parameter after the Adam step, dropout off."""
    from furusato_recommend_amd import SASRec, SyntheticBipartite
    from furusato_recommend_amd.rows import gather_rows
    ds = SyntheticBipartite(500, 300, 10_000, seed=4)
    cfg = {"recdim": 64, "layer": 2, "heads": 2, "lr": 1e-3, "decay": 1e-4,
           "device": "cuda:0", "bpr_batch_size": 128, "dropout_p": 0.0}
    torch.manual_seed(9)
    a = SASRec(cfg, ds)
    torch.manual_seed(9)
    b = SASRec(dict(cfg, fused_rows=False), ds)
    rng = np.random.default_rng(1)
    users = rng.integers(0, 500, 128)
    pos = torch.as_tensor(rng.integers(0, 300, 128), device="cuda")
    neg = torch.as_tensor(rng.integers(0, 300, 128), device="cuda")
    grads = {}

    def grab():  # between backward and Adam
        grads.update((n, q.grad.clone()) for n, q in a.named_parameters())
    la = float(a.stageOne(users, pos, neg, grad_hook=grab))
    x, offs, seg, length = b.packed_input(users)
    u = b.forward_user_packed(x, offs, seg, length)
    w = b.item_id_embedding.weight
    loss = b.loss(u, b.forward_item(gather_rows(w, pos)), b.forward_item(gather_rows(w, neg)))
    loss.backward()
    lb = float(loss.detach())
    assert abs(la - lb) <= TOL * abs(lb)
    live = {}
    for (name, pa), pb in zip(a.named_parameters(), b.parameters()):
        scale = float(pb.grad.abs().max())
        # item_last_proj.bias and the key part of in_proj_bias have exactly
        # zero gradient (the bias cancels in pos - neg / in the softmax): the
        # fused tower sums pos and neg rows in one fixed-order column sum, so
        # that zero arrives as rounding noise (~1e-8) — floor 1e-3 x TOL
        assert float((grads[name] - pb.grad).abs().max()) <= TOL * max(scale, 1e-3), name
        live[name] = pb.grad.abs() > 1e-5 * scale
    b.optims.step()
    for (name, pa), pb in zip(a.named_parameters(), b.parameters()):
        # Adam divides by sqrt(v): compare the update in units of lr; a zero
        # gradient's rounding noise becomes a full lr step, so only elements
        # above the noise floor are compared
        diff = (pa - pb).abs()[live[name]]
        assert diff.numel() == 0 or float(diff.max()) < 1e-2 * cfg["lr"], name


@pytest.mark.parametrize("graph,mode", [(False, "sorted"), (True, "sorted"), (True, "atomic")])
def test_sasrec_sorted_table_step_matches_dense(graph, mode):
    """The item table's sorted gradient + fused table Adam (TableGrad, the
    default) == the materialised gradient + dense Adam, over three steps,
    eager and captured: every parameter within 1e-2 lr of the dense run (the
    only difference is the summation order of repeated ids)."""
    from furusato_recommend_amd import SASRec, SyntheticBipartite
    ds = SyntheticBipartite(500, 300, 10_000, seed=4)
    cfg = {"recdim": 64, "layer": 2, "heads": 2, "lr": 1e-3, "decay": 1e-4,
           "device": "cuda:0", "bpr_batch_size": 128, "dropout_p": 0.0, "graph": graph}
    torch.manual_seed(9)
    a = SASRec(dict(cfg, table_grad=mode), ds)
    torch.manual_seed(9)
    b = SASRec(dict(cfg, table_grad="dense"), ds)
    assert a._tg is not None and b._tg is None and a._tg.atomic == (mode == "atomic")
    rng = np.random.default_rng(2)
    live = {n: True for n, _ in b.named_parameters()}

    def mark():  # elements whose dense gradient is above the rounding floor
        top = max(float(q.grad.abs().max()) for q in b.parameters())
        for n, q in b.named_parameters():
            floor = max(1e-5 * float(q.grad.abs().max()), 1e-6 * top)
            live[n] = live[n] & (q.grad.abs() > floor)
    for _ in range(3):
        users = rng.integers(0, 500, 128)
        pos = torch.as_tensor(rng.integers(0, 300, 128), device="cuda")
        neg = torch.as_tensor(rng.integers(0, 300, 128), device="cuda")
        la = float(a.stageOne(users, pos, neg))
        b.config["graph"] = False  # the hook runs in the eager step
        lb = float(b.stageOne(users, pos, neg, grad_hook=mark))
        assert abs(la - lb) <= 1e-5 * abs(lb)
    for (name, pa), pb in zip(a.named_parameters(), b.parameters()):
        # a zero gradient's rounding noise becomes a full lr step under Adam
        # (the key bias, item_last_proj.bias): compare the live elements
        diff = (pa - pb).abs()[live[name]]
        assert diff.numel() == 0 or float(diff.max()) < 1e-2 * cfg["lr"], name
    for sa, sb in zip(a.optims, b.optims):
        assert sa.n_steps == sb.n_steps == 3


def test_sasrec_sample_pairs():
    """sample_pairs: every positive is an element of its user's sequence,
    positions uniform (chi-square over one long user's positions), negatives
    in range and uniform; same (seed, offset) -> same draws."""
    from furusato_recommend_amd import SASRec, SyntheticBipartite
    from furusato_recommend_amd.sasrec import SequenceData
    ds = SyntheticBipartite(400, 300, 6000, seed=3)
    seq = SequenceData.synthetic(400, 300, "cuda", max_len=50, min_len=5, seed=1)
    m = SASRec({"recdim": 64, "layer": 1, "heads": 2, "lr": 1e-3, "decay": 1e-4,
                "device": "cuda:0", "bpr_batch_size": 64}, ds, sequences=seq)
    users = torch.randint(0, 400, (5000,), device="cuda")
    pn = m.sample_pairs(users, 11, 0)
    assert torch.equal(pn, m.sample_pairs(users, 11, 0))
    assert not torch.equal(pn, m.sample_pairs(users, 11, 5000))
    items, length = seq.items.long(), seq.length
    rows = items[users]
    hit = (rows == pn[0][:, None]) & (torch.arange(50, device="cuda")[None, :] < length[users][:, None])
    assert bool(hit.any(1).all())
    assert int(pn[1].min()) >= 0 and int(pn[1].max()) < 300
    u0 = int(torch.argmax(length))
    L = int(length[u0])
    N = L * 400
    many = m.sample_pairs(torch.full((N,), u0, device="cuda"), 5, 0)[0].cpu().numpy()
    vals, mult = np.unique(items[u0][:L].cpu().numpy(), return_counts=True)
    got = np.array([(many == v).sum() for v in vals], dtype=np.float64)
    exp = N * mult / L  # an item repeated in the sequence is drawn that much more often
    assert got.sum() == N
    chi2 = float(((got - exp) ** 2 / exp).sum())
    dof = len(vals) - 1
    assert chi2 < dof + 6 * (2 * dof) ** 0.5


def test_sasrec_trains():
    from furusato_recommend_amd import SASRec, SyntheticBipartite
    ds = SyntheticBipartite(3000, 500, 40_000, seed=11, test_frac=0.1)
    m = SASRec({"recdim": 128, "layer": 2, "heads": 2, "lr": 1e-3, "decay": 1e-6,
                "device": "cuda:0", "bpr_batch_size": 512}, ds)
    from furusato_recommend_amd.engine import sample_triples  # noqa: F401
    from furusato_recommend_amd.graph import Graph
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    losses = []
    for s in range(8):
        u = torch.empty(2048, dtype=torch.int32, device="cuda")
        p, n = torch.empty_like(u), torch.empty_like(u)
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        sample_triples(g, 2048, s, 0, u, p, n, err)
        losses.append(float(m.OneEpoch(u, p, n)))
    assert losses[-1] < losses[0]


@pytest.mark.parametrize("split", [None, 32])
@pytest.mark.parametrize("name,d", [("sym", 16), ("sym", 48), ("dir", 64), ("dir", 256)])
def test_lgconv_operator_matches_fixture(golden, name, d, split):
    """LGConv()(x, edge_index) on non-bipartite (skewed, duplicate edges,
    isolated nodes) and directed graphs: forward, input gradient (Âᵀ on the
    transposed CSR), normalize=False; odd widths are padded."""
    from furusato_recommend_amd import LGConv
    from tests.test_oracle import lgconv_case
    f = golden("lgconv_graphs.npz")
    ei, x, y, ybar, xbar, ysum = lgconv_case(f, name, d)
    conv = LGConv(split=split)
    eic = ei.cuda()
    xg = x.cuda().requires_grad_(True)
    yg = conv(xg, eic)
    if split is not None:
        assert conv._graph.n_long > 0
    assert conv._graph.symmetric == (name == "sym")
    assert rel(yg, y) < TOL
    (yg * ybar.cuda()).sum().backward()
    assert rel(xg.grad, xbar) < TOL
    g0 = conv._graph
    conv(xg.detach(), eic)
    assert conv._graph is g0          # CSR cached per edge_index
    if ysum is not None:
        assert rel(LGConv(normalize=False)(x.cuda(), eic), ysum) < TOL


def test_fused_leaf_gather_mean_equals_unfused():
    """mirec_fanout_mean_gather(_bwd) == row gather + mirec_fanout_mean (and
    its backward scattered into the table), dropout on, isolated children."""
    import ctypes

    from furusato_recommend_amd import _lib
    from furusato_recommend_amd._lib import check, lib
    from furusato_recommend_amd.graphsage import _FanoutMean
    from furusato_recommend_amd.rows import gather_rows
    torch.manual_seed(4)
    N, d, n_t, k, p, seed = 500, 32, 300, 5, 0.3, 123
    table = torch.randn(N, d, device="cuda", requires_grad=True)
    ids = torch.randint(0, N, (n_t * k,), device="cuda", dtype=torch.int32)
    ids[::7] = -1
    ids[:k] = -1  # a target with no valid child
    go = torch.randn(n_t, d, device="cuda")
    rows = gather_rows(table, ids)
    ref = _FanoutMean.apply(rows, ids, k, p, seed)
    gref, = torch.autograd.grad(ref, table, go)
    out = torch.empty(n_t, d, device="cuda")
    st = _lib.stream_handle()
    check(lib.mirec_fanout_mean_gather(table.data_ptr(), ids.data_ptr(), n_t, k, d, p,
                                       ctypes.c_uint64(seed), out.data_ptr(), st), "fmg")
    g = torch.zeros(N, d, device="cuda")
    check(lib.mirec_fanout_mean_gather_bwd(go.data_ptr(), ids.data_ptr(), n_t, k, d, p,
                                           ctypes.c_uint64(seed), g.data_ptr(), st), "fmg_bwd")
    assert torch.equal(out, ref.detach())
    assert rel(g, gref) < TOL


@pytest.mark.parametrize("filt", ["slot", "bytemap", "dense"])
def test_first_backward_layer_filters_agree(golden, filt):
    """The three ways of feeding the first backward layer (slot-filtered
    seeds, byte-map then slot, dense pre-scaled seed table) give the
    reference's two training steps."""
    f = golden("lgcn_d64_L3.npz")
    m = lgcn_from(f)
    m.engine.sparse_filter = filt
    t = torch.from_numpy(f["triples"])
    m.stageOne(t[:, 0], t[:, 1], t[:, 2])
    m.stageOne(t[:, 0], t[:, 1], t[:, 2])
    assert rel(m.all_embedding.weight, f["emb_step2"]) < TOL
    if filt == "dense":
        assert float(m.engine.seed_dense.abs().max()) == 0.0  # table restored


def test_adam_group_equals_per_tensor_adam():
    """AdamGroup (one multi-tensor launch per 32 small tensors, the dense
    kernel for large ones) == per-tensor mirec_adam_dense == torch Adam
    (same update; the compiler may contract FMAs differently per kernel)."""
    from furusato_recommend_amd.engine import AdamGroup, AdamState
    torch.manual_seed(2)
    shapes = [(7,), (128,), (3, 5), (1 << 20, 2)] + [(33,)] * 35
    a = [torch.randn(s, device="cuda") for s in shapes]
    b = [t.clone() for t in a]
    c = [t.clone().requires_grad_(True) for t in a]
    ga = AdamGroup(AdamState(t, lr=1e-2) for t in a)
    gb = [AdamState(t, lr=1e-2) for t in b]
    tor = torch.optim.Adam(c, lr=1e-2)
    for _ in range(3):
        gr = [torch.randn_like(t) for t in a]
        for t, g in zip(a, gr):
            t.grad = g
        for t, g in zip(b, gr):
            t.grad = g.clone()
        for t, g in zip(c, gr):
            t.grad = g.clone()
        ga.step()
        for s in gb:
            s.step()
        tor.step()
    for x, y, z in zip(a, b, c):
        assert rel(x, y) < 1e-6  # fma contraction may differ between the kernels
        assert rel(x, z.detach()) < TOL


def test_zipf_long_rows_not_walked_by_row_phase():
    """Performance regression guard: rows longer than the split are covered
    by their segments only (a wave's narrow gather once walked them serially:
    200x slower at C2 scale).  Loose bound: the Zipf graph's launch stays
    within 5x of a uniform graph with the same edge count."""
    from furusato_recommend_amd import Graph, SyntheticBipartite
    from furusato_recommend_amd.engine import propagate
    times = []
    for kind in ("zipf", "uniform"):
        ds = SyntheticBipartite(200_000, 20_000, 4_000_000, seed=1, kind=kind)
        g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items,
                                    "cuda:0")
        x = torch.randn(g.n_nodes, 64, device="cuda")
        y = torch.empty_like(x)
        for _ in range(2):
            propagate(g, x, y)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        propagate(g, x, y)
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
        if kind == "zipf":
            assert g.n_long > 0
    assert times[0] < 5 * times[1] + 0.5, times


@pytest.mark.parametrize("dim", [4, 8])
def test_small_dims_train_like_oracle(dim):
    """The smallest supported widths (one 16-B row per 1-2 lanes): two
    training steps vs the CPU oracle."""
    from furusato_recommend_amd import LightGCN, SyntheticBipartite
    from oracle.lightgcn_oracle import OracleLightGCN
    ds = SyntheticBipartite(500, 120, 6000, seed=dim, test_frac=0.0)
    torch.manual_seed(dim)
    m = LightGCN({"recdim": dim, "layer": 3, "lr": 1e-3, "decay": 1e-4, "device": "cuda:0",
                  "bpr_batch_size": 256}, ds)
    o = OracleLightGCN(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, dim, 3, 1e-3, 1e-4,
                       emb=m.all_embedding.weight.detach().cpu().clone())
    rng = np.random.default_rng(dim)
    for _ in range(2):
        u = rng.integers(0, ds.n_users, 256)
        p = rng.integers(0, ds.m_items, 256)
        n = rng.integers(0, ds.m_items, 256)
        lg = float(m.stageOne(torch.from_numpy(u), torch.from_numpy(p), torch.from_numpy(n)))
        lo = o.stageOne(u, p, n)
        assert abs(lg - lo) < TOL * abs(lo)
    assert rel(m.all_embedding.weight, o.emb.detach()) < TOL


def test_soak_many_steps_stay_finite_and_learn():
    """300 on-device-sampled training steps on a community graph: every loss
    finite, the table finite, the loss falls, the slot map ends clean."""
    from furusato_recommend_amd import LightGCN, SyntheticBipartite
    ds = SyntheticBipartite(100_000, 10_000, 2_000_000, seed=9, kind="cluster", test_frac=0.0)
    torch.manual_seed(0)
    m = LightGCN({"recdim": 64, "layer": 3, "lr": 1e-3, "decay": 1e-4, "device": "cuda:0",
                  "bpr_batch_size": 2048}, ds)
    acc = torch.zeros(1, device="cuda")
    first = last = None
    for i in range(300):
        u, p, n = m.sample(2048, seed=3, offset=i * 2048)
        loss = m.engine.train_step(m.all_embedding.weight.data, m.optim, u, p, n, 1e-4)
        if i == 0:
            first = float(loss)
        if i >= 290:
            acc += loss
    last = float(acc) / 10
    assert int(m._sample_err.item()) == 0
    assert np.isfinite(first) and np.isfinite(last) and last < 0.8 * first
    assert bool(torch.isfinite(m.all_embedding.weight).all())
    assert int((m.engine.slot != -1).sum()) == 0


def test_adam_device_hparams_equal_host_hparams():
    """mirec_adam_dense_dev / mirec_adam_multi_dev (scalars read from device
    memory, the graph-captured path) == the host-scalar kernels, bitwise."""
    import ctypes

    from furusato_recommend_amd import _lib
    from furusato_recommend_amd.engine import AdamGroup, AdamState
    torch.manual_seed(4)
    shapes = [(3000, 128), (7,), (129, 3), (1 << 20,)]
    ps = [torch.randn(*s, device="cuda") for s in shapes]
    qs = [p.clone() for p in ps]
    ga, gb = AdamGroup(AdamState(p, lr=1e-3) for p in ps), AdamGroup(AdamState(q, lr=1e-3) for q in qs)
    for it in range(3):
        for p, q in zip(ps, qs):
            p.grad = torch.randn_like(p)
            q.grad = p.grad.clone()
        ga.step()
        hp = gb.next_shared_hparams()
        h_dev = torch.frombuffer(bytearray(bytes(hp)), dtype=torch.float32).cuda()
        gb.step_device(h_dev)
        for p, q in zip(ps, qs):
            assert torch.equal(p, q)
    assert ctypes.sizeof(_lib.AdamH) == 24


def test_resnorm_seed_base_draws_fresh_masks():
    """With a device seed base (graph replays), the dropout mask changes with
    the base value and the backward recomputes the forward's mask."""
    from furusato_recommend_amd import sasrec as S
    torch.manual_seed(5)
    n, d, p = 4096, 128, 0.25
    z = (torch.rand(n, d, device="cuda") + 0.5).requires_grad_(True)
    res = torch.zeros(n, d, device="cuda", requires_grad=True)
    base = torch.zeros(1, dtype=torch.int64, device="cuda")
    masks = []
    try:
        S._SEED_BASE = base
        torch.manual_seed(11)
        out, _ = S.resnorm(res, z, p=p)
        g = torch.randn(n, d, device="cuda")
        base.fill_(12345)  # the backward must read the base its forward used
        base.fill_(0)
        gz, = torch.autograd.grad(out, [z], g)
        kept = out != 0
        assert rel(gz, g * kept / (1 - p)) < 1e-6
        masks.append(kept)
        for b in (1, 2):
            base.fill_(b)
            torch.manual_seed(11)  # same host seed: only the device base differs
            o2, _ = S.resnorm(res, z, p=p)
            masks.append(o2 != 0)
    finally:
        S._SEED_BASE = None
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[1], masks[2])
    for mk in masks:
        assert abs(float(mk.float().mean()) - (1 - p)) < 0.01


def test_sasrec_graph_step_equals_eager():
    """stageOne replaying a captured HIP graph (capacity-padded packing,
    device Adam scalars) == the eager step: losses of consecutive steps and
    every gradient of the first step (dropout off); the captured model keeps
    learning with dropout on and draws a fresh mask each replay."""
    from furusato_recommend_amd import SASRec, SyntheticBipartite
    ds = SyntheticBipartite(700, 300, 14_000, seed=6)
    # the table's gradient materialised (.grad) to compare it; the sorted
    # form in the captured step: test_sasrec_sorted_table_step_matches_dense
    cfg = {"recdim": 64, "layer": 2, "heads": 2, "lr": 1e-3, "decay": 1e-4,
           "device": "cuda:0", "bpr_batch_size": 128, "dropout_p": 0.0, "table_grad": "dense"}
    torch.manual_seed(3)
    a = SASRec(dict(cfg, graph=True), ds)
    torch.manual_seed(3)
    b = SASRec(dict(cfg, graph=False), ds)
    rng = np.random.default_rng(2)
    for it in range(3):
        users = rng.integers(0, 700, 128)
        pos = torch.as_tensor(rng.integers(0, 300, 128), device="cuda")
        neg = rng.integers(0, 300, 128)  # host array: goes through the staging copy
        la, lb = float(a.stageOne(users, pos, neg)), float(b.stageOne(users, pos, neg))
        assert abs(la - lb) <= 1e-5 * abs(lb), (it, la, lb)
        if it == 0:
            for (name, pa), pb in zip(a.named_parameters(), b.parameters()):
                # (item_last_proj.bias has an exactly-zero gradient: the bias
                # cancels in pos - neg; both sides hold ~1e-9 rounding noise)
                scale = float(pb.grad.abs().max())
                assert float((pa.grad - pb.grad).abs().max()) <= TOL * max(scale, 1e-3), name
    assert len(a._graphs) >= 1 and not getattr(b, "_graphs", None)
    # dropout on: same batch twice -> different losses (fresh masks), and
    # repeated steps on one batch lower its loss
    torch.manual_seed(3)
    c = SASRec(dict(cfg, dropout_p=0.3, lr=1e-2, table_grad="sorted"), ds)
    users = rng.integers(0, 700, 128)
    pos, neg = rng.integers(0, 300, 128), rng.integers(0, 300, 128)
    losses = [float(c.stageOne(users, pos, neg)) for _ in range(30)]
    assert len(set(losses[:5])) == 5
    assert np.mean(losses[-5:]) < np.mean(losses[:5])


def _sasrec_oracle_step(m, u, pos, neg, heads, dtype=torch.float64):
    """The reference's SASRec step (model/sasrec.py:385-435, 437-469) on the
    host (oracle.sasrec_forward_user) from m's parameters, in float64 (the
    exact step) or float32 (the reference's own arithmetic): (pooled user
    rows [B, d], loss, {parameter name: gradient})."""
    from oracle import lightgcn_oracle as O
    F = torch.nn.functional
    P = {n: p.detach().to(dtype).cpu().requires_grad_(True) for n, p in m.named_parameters()}
    W = P["item_id_embedding.weight"]
    L = m.num_layers
    items = m.seq.items[u].long().cpu()
    length = m.seq.length[u].cpu()
    T = int(length.max())
    mask = (torch.arange(T)[None, :] < length[:, None]).to(dtype)
    x = W[items[:, :T].clamp(min=0)] * mask[..., None]  # pad_sequence(padding_value=0)
    p = {}
    for i in range(L):
        a = f"attn_layers.{i}."
        p.update({f"in_w{i}": P[a + "in_proj_weight"], f"in_b{i}": P[a + "in_proj_bias"],
                  f"out_w{i}": P[a + "out_proj.weight"], f"out_b{i}": P[a + "out_proj.bias"],
                  f"ln1_w{i}": P[f"attn_norm_layers.{i}.weight"],
                  f"ln1_b{i}": P[f"attn_norm_layers.{i}.bias"],
                  f"ln2_w{i}": P[f"ffn_norm_layers.{i}.weight"],
                  f"ln2_b{i}": P[f"ffn_norm_layers.{i}.bias"],
                  f"ffn_w{i}": P[f"ffn_layers.{i}.weight"], f"ffn_b{i}": P[f"ffn_layers.{i}.bias"]})
    user = O.sasrec_forward_user(x, length, p, heads, L)

    def tower(z):  # sasrec.py:415-421
        for i in range(L - 1):
            z = F.linear(z, P[f"item_linears.{i}.weight"], P[f"item_linears.{i}.bias"]).relu()
        return F.linear(z, P["item_last_proj.weight"], P["item_last_proj.bias"])
    pe, ne = tower(W[pos.long().cpu()]), tower(W[neg.long().cpu()])
    all_param = 0
    for n_, v in P.items():  # sasrec.py:429-431 ('emb' parameters, doubling)
        if "emb" in n_:
            all_param = all_param + all_param + v.norm(2)
    loss = torch.mean(F.softplus((user * ne).sum(1) - (user * pe).sum(1))) \
        + all_param / user.shape[0] * m.config["decay"]
    loss.backward()
    return user.detach().double(), float(loss), {n_: v.grad.double() for n_, v in P.items()}


@pytest.mark.timeout(600)
def test_sasrec_c4_batch_step_matches_float64_oracle():
    """One C4 step (B = 2048 users, sequence lengths U[5, 50], d = 128, h = 2,
    L = 2, dropout off) through the packed, captured HIP-graph path — the
    length-ordered packs, the capacity padding, the sorted table gradient,
    the device pair sampling — against the reference's step restated in
    float64 on the host from the same parameters (model/sasrec.py:385-435):
    every pooled user row (the longest, the length-5 ones and every pack
    boundary among them), the loss, and the gradient of every parameter
    (the item table's formed from its sorted form, as the fused Adam forms
    it).  Rows and loss at 1e-4 relative to float64.  Every gradient at 1e-4
    relative to the reference's own float32 step on the host (the north
    star's criterion); the float64 errors of both are printed beside it.
    They are not the gate: a handful of the ~1.4e7 ReLU((x + attn))
    pre-activations lie within the float32 error of the attention output
    (|pre| ~ 1e-7 on operands ~1e-2..0.3), and both float32 paths take the
    other mask there than float64 does (DESIGN §9.5 names the elements).
    The item tower's last bias has an exactly zero gradient (it adds
    <u, b> to both scores); its rounding noise is bounded against its
    weight's gradient instead."""
    from furusato_recommend_amd import SASRec
    from furusato_recommend_amd.sasrec import SequenceData

    class DS:
        n_users, m_items = 50_000, 100_000
    seq = SequenceData.synthetic(DS.n_users, DS.m_items, "cuda:0", max_len=50, min_len=5, seed=0)
    torch.manual_seed(2020)
    m = SASRec({"recdim": 128, "layer": 2, "heads": 2, "lr": 1e-3, "decay": 1e-4,
                "device": "cuda:0", "bpr_batch_size": 2048, "dropout_p": 0.0, "graph": True},
               DS, sequences=seq)
    rng = np.random.default_rng(11)
    u_h = rng.integers(0, DS.n_users, 2048)
    lens = seq.length_host
    u_h[0] = int(np.argmax(lens))  # a length-50 and a length-5 sequence for sure
    u_h[1] = int(np.argmin(lens))
    u = torch.from_numpy(u_h).cuda()
    pn = m.sample_pairs(u, seed=3)
    pos, neg = pn[0], pn[1]
    user_ref, loss_ref, g_ref = _sasrec_oracle_step(m, u, pos, neg, heads=2)
    _, _, g32 = _sasrec_oracle_step(m, u, pos, neg, heads=2, dtype=torch.float32)
    names = [n for n, _ in m.named_parameters()]
    got = {}

    def grab():  # between graph A (forward / backward) and graph B (Adam)
        for n_, p_ in m.named_parameters():
            if p_.grad is not None:
                got[n_] = p_.grad.detach().clone()
        w = m.item_id_embedding.weight
        got["item_id_embedding.weight"] = m._tg.materialize(w.detach())
    loss = float(m.stageOne(u_h, pos, neg, grad_hook=grab, loss_scale=1.0, table_by_hook=False))
    torch.cuda.synchronize()
    (cap,) = m._graphs.values()
    assert cap.C >= int(lens[u_h].sum())  # packed into the captured capacity
    users = cap.user_rows.double().cpu()
    assert rel(users, user_ref) < TOL
    assert abs(loss - loss_ref) <= TOL * abs(loss_ref)
    assert set(got) == set(names)
    errs, bad = {}, []
    for n_ in names:
        b = g_ref[n_]
        if n_ == "item_last_proj.bias":
            scale = float(g_ref["item_last_proj.weight"].abs().max())
            err = lambda a, b: float((a - b).abs().max()) / scale  # noqa: E731
        else:
            err = rel
        a = got[n_].double().cpu()
        # hip vs the reference's own float32 step on the host is the gate
        # (north star: "match the reference CPU path within 1e-4 rel fp32");
        # float64 is printed as the sanity check beside it.
        errs[n_] = (err(a, b), err(g32[n_], b), err(a, g32[n_]))
        if errs[n_][2] >= TOL:
            bad.append(n_)
    print("gradient rel err (hip vs float64, host fp32 vs float64, hip vs host fp32):", errs)
    diag = None
    if "item_id_embedding.weight" in bad:  # where the table's rows differ
        a, b = got["item_id_embedding.weight"].double().cpu(), g32["item_id_embedding.weight"]
        e = (a - b).abs().max(1).values
        top = torch.topk(e, 5).indices.tolist()
        seq_ids = m.seq.items[u].cpu()
        seq_ids = seq_ids[torch.arange(seq_ids.shape[1])[None, :] < m.seq.length[u].cpu()[:, None]]
        diag = [(r, float(e[r]), float(b[r].abs().max()), int((seq_ids == r).sum()),
                 int((pos.cpu() == r).sum()), int((neg.cpu() == r).sum())) for r in top]
    assert not bad, (bad, errs, diag)


@pytest.mark.parametrize("n,kr,no", [(1, 32, 128), (100, 128, 128), (4096, 128, 384),
                                     (56_321, 128, 384), (3000, 384, 128), (777, 256, 256)])
def test_gemm_nt_matches_fp64(n, kr, no):
    """mirec_gemm_nt (the Linear forward / input-gradient GEMM) vs a float64
    reference, ragged row counts, with and without bias."""
    from furusato_recommend_amd import linear as LN
    from furusato_recommend_amd.linear import gemm_nt
    LN.FORCE_MIREC_GEMM = True
    torch.manual_seed(n)
    a = torch.randn(n, kr, device="cuda")
    b = torch.randn(no, kr, device="cuda")
    bias = torch.randn(no, device="cuda")
    for bb in (None, bias):
        c = gemm_nt(a, b, bb)
        ref = a.double() @ b.double().t() + (0 if bb is None else bb.double())
        assert c is not None and rel(c, ref) < 1e-6
    LN.FORCE_MIREC_GEMM = False


@pytest.mark.parametrize("n,no", [(56_321, 384), (200_003, 128), (70_001, 256)])
def test_gemm_nt_resident_b_equals_tiled(n, no):
    """At Kr = 128 mirec_gemm_nt runs the resident-B form (gemm_nt_res_kernel:
    B split once per workgroup, waves streaming 32-row units) when the call
    has at least 16 units of 32 rows x 128 columns per CU — every case here
    on MI355X's 256 CUs — and the tiled kernel below that (the row slices of
    at most 4 000 rows).  Rows are independent, so C of the slices must equal
    the same rows of the full product bit for bit: plain, with bias, and with
    bias + ReLU and the output split at column 128 (the GraphSAGE hop's
    epilogue forms)."""
    from furusato_recommend_amd import _lib
    torch.manual_seed(n + no)
    a = torch.randn(n, 128, device="cuda")
    b = torch.randn(no, 128, device="cuda")
    bias = torch.randn(no, device="cuda")
    st = _lib.stream_handle()

    def run(x, bb, relu, split):
        m = x.shape[0]
        c = torch.full((m, no), float("nan"), device="cuda")
        c1 = torch.full((m, 128), float("nan"), device="cuda")
        c2 = torch.full((m, no - 128), float("nan"), device="cuda")
        _lib.check(_lib.lib.mirec_gemm_nt_ex(
            x.data_ptr(), None, 0, None, b.data_ptr(), _lib.ptr(bb),
            c1.data_ptr() if split else c.data_ptr(), c2.data_ptr() if split else None,
            128 if split else 0, 1 if relu else 0, m, 128, no, st), "gemm_nt_ex")
        return torch.cat([c1, c2], 1) if split else c

    forms = [(None, False, False), (bias, False, False)]
    if no > 128:
        forms.append((bias, True, True))
    for bb, relu, split in forms:
        full = run(a, bb, relu, split)
        ref = a.double() @ b.double().t() + (0 if bb is None else bb.double())
        if relu:
            ref = ref.clamp_min(0)
        assert rel(full, ref) < 1e-6
        for lo, hi in ((0, 4000), (n // 2 - 1000, n // 2 + 777), (max(n - 3001, 0), n)):
            part = run(a[lo:hi].contiguous(), bb, relu, split)
            assert torch.equal(part, full[lo:hi]), (lo, hi, bb is None, relu, split)


@pytest.mark.parametrize("n,kr,no", [(1, 32, 128), (100, 384, 128), (56_321, 384, 128),
                                     (3000, 128, 256), (777, 256, 384)])
def test_gemm_nn_matches_fp64(n, kr, no):
    """mirec_gemm_nn_ex (dX = dY W with W as stored, [Kr, No]) vs float64,
    plain and with the ReLU mask on A and the output split at a 128-column
    boundary (the GraphSAGE hop's input gradient)."""
    from furusato_recommend_amd import _lib
    from furusato_recommend_amd.linear import gemm_nn
    torch.manual_seed(n + kr)
    a = torch.randn(n, kr, device="cuda")
    b = torch.randn(kr, no, device="cuda")
    c = gemm_nn(a, b)
    assert c is not None and rel(c, a.double() @ b.double()) < 1e-6
    mask = torch.randn(n, kr, device="cuda")
    am = torch.where(mask > 0, a, torch.zeros_like(a))
    ref = am.double() @ b.double()
    if no >= 256:
        c1 = torch.empty(n, 128, device="cuda")
        c2 = torch.empty(n, no - 128, device="cuda")
        _lib.check(_lib.lib.mirec_gemm_nn_ex(a.data_ptr(), mask.data_ptr(), b.data_ptr(),
                                             c1.data_ptr(), c2.data_ptr(), 128, n, kr, no,
                                             _lib.stream_handle()), "gemm_nn_ex")
        assert rel(torch.cat([c1, c2], 1), ref) < 1e-6


def test_gemm_split_bf16_is_f32_accurate():
    """The GEMMs multiply f32 operands as an exact three-term bf16 split
    (gemm.hip, MIREC_GEMM_X6).  Claim: f32-class accuracy.  Check: on
    operands spanning twelve decades (row / column scales 10^U(-6, 6)), the
    error of every output element relative to its own scale Σ_k |a_ik b_kj|
    (float64) is below 1e-6 and within 4x of torch's fp32 matmul on the same
    operands, for the nt, nn and tn forms."""
    from furusato_recommend_amd import linear as LN
    from furusato_recommend_amd.linear import gemm_nn, gemm_nt, gemm_tn
    LN.FORCE_MIREC_GEMM = True
    prev = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        torch.manual_seed(5)
        for n, k, m in ((4096, 128, 384), (20_000, 384, 128)):
            a = torch.randn(n, k, device="cuda") * 10 ** (12 * torch.rand(n, 1, device="cuda") - 6)
            b = torch.randn(m, k, device="cuda") * 10 ** (12 * torch.rand(m, 1, device="cuda") - 6)
            scale = a.double().abs() @ b.double().abs().t()
            ref = a.double() @ b.double().t()

            def err(c):
                return float(((c.double() - ref).abs() / scale).max())
            e_torch = err(a @ b.t())
            for name, c in (("nt", gemm_nt(a, b)), ("nn", gemm_nn(a, b.t().contiguous()))):
                e = err(c)
                assert e < 1e-6 and e < 4 * e_torch + 1e-8, (name, n, e, e_torch)
            # tn: C = Aᵀ B over the n rows
            bt = torch.randn(n, m, device="cuda") * 10 ** (12 * torch.rand(1, m, device="cuda") - 6)
            at = a
            scale = at.double().abs().t() @ bt.double().abs()
            ref = at.double().t() @ bt.double()
            e_torch = float(((at.t() @ bt).double() - ref).abs().div(scale).max())
            c, _ = gemm_tn(at, bt, False)
            e = float(((c.double() - ref).abs() / scale).max())
            assert e < 1e-6 and e < 4 * e_torch + 1e-8, ("tn", n, e, e_torch)
    finally:
        LN.FORCE_MIREC_GEMM = False
        torch.backends.cuda.matmul.allow_tf32 = prev


@pytest.mark.parametrize("n,m,no", [(0, 128, 128), (1, 128, 128), (100, 384, 128),
                                    (56_321, 384, 128), (9000, 128, 256), (33, 256, 384)])
def test_gemm_tn_matches_fp64(n, m, no):
    """mirec_gemm_tn (dW = dYᵀ X and db = Σ dY, sliced rows summed in a fixed
    order) vs float64, ragged and empty row counts; bitwise deterministic."""
    from furusato_recommend_amd.linear import gemm_tn
    torch.manual_seed(n + m)
    a = torch.randn(n, m, device="cuda")
    b = torch.randn(n, no, device="cuda")
    c, cs = gemm_tn(a, b, True)
    if n == 0:
        assert float(c.abs().max()) == 0.0 and float(cs.abs().max()) == 0.0
        return
    ref = a.double().t() @ b.double()
    assert rel(c, ref) < 1e-6
    assert rel(cs, a.double().sum(0)) < 1e-6
    c2, cs2 = gemm_tn(a, b, True)
    assert torch.equal(c, c2) and torch.equal(cs, cs2)



@pytest.mark.parametrize("n,m,pad", [(700, 384, 324), (4096, 128, 1000), (56_321, 384, 4_000),
                                     (56_321, 128, 9_215)])
def test_col_sums_invariant_to_zero_padding_rows(n, m, pad):
    """the captured SASRec step sums its row gradients over
    the token capacity (the real rows, then zero padding rows), the eager
    step over the real rows only.  mirec_col_sums gives the same bits for
    both (fixed 64-row slices at these sizes, partials added in slice order:
    appended zeros add exact zeros); torch's sum(0) picks its reduction tree
    from the row count, so its two results differ in the last bits — which
    Adam's first steps turn into ±lr updates wherever the gradient is
    rounding noise (the structurally zero key-bias slice of the QKV bias).
    Torch's behaviour is printed, not asserted."""
    from furusato_recommend_amd.linear import col_sums
    torch.manual_seed(n + m + pad)
    a = torch.randn(n, m, device="cuda")
    ap = torch.cat([a, torch.zeros(pad, m, device="cuda")])
    c, cp = col_sums(a), col_sums(ap)
    assert torch.equal(c, cp)
    assert rel(c, a.double().sum(0)) < 1e-6
    t, tp = a.sum(0), ap.sum(0)
    print(f"torch sum(0) n={n} m={m} +{pad} zero rows: "
          f"{int((t != tp).sum())} of {m} columns differ, max |diff| {float((t - tp).abs().max()):.3g}")

@pytest.mark.parametrize("n,m", [(0, 5), (1, 1), (3, 7), (63, 192), (64, 192), (7169, 192),
                                 (70_001, 64), (32, 12_288)])
def test_col_sums_matches_fp64_and_replays_equal(n, m):
    """mirec_col_sums (the bias gradient of Linear widths the GEMM tiles do
    not take, and the split weight gradient's slice sum) vs float64; bitwise
    repeatable, and a captured HIP graph's replays give the eager bits."""
    from furusato_recommend_amd.linear import col_sums
    torch.manual_seed(n + m)
    a = torch.randn(n, m, device="cuda")
    c = col_sums(a)
    assert c.shape == (m,)
    if n == 0:
        assert float(c.abs().max()) == 0.0
        return
    assert rel(c, a.double().sum(0)) < 1e-6
    assert torch.equal(c, col_sums(a))
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        col_sums(a)  # warm-up off the capture
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(g):
        out = col_sums(a)
    for _ in range(3):
        out.zero_()
        g.replay()
        assert torch.equal(out, c)


def test_linear_on_mirec_gemms_matches_torch():
    """Linear (mirec GEMMs) == F.linear: output, input / weight / bias
    gradients, token-row shapes of the SASRec block and odd widths that fall
    back to torch."""
    import torch.nn.functional as F

    from furusato_recommend_amd.linear import Linear
    torch.manual_seed(8)
    for n, k, nout in ((56_320, 128, 384), (4096, 128, 128), (5000, 256, 128), (300, 48, 20)):
        lin = Linear(k, nout, device="cuda")
        x = torch.randn(n, k, device="cuda", requires_grad=True)
        y = lin(x)
        yr = F.linear(x, lin.weight, lin.bias)
        assert rel(y, yr) < 1e-5
        g = torch.randn_like(y)
        g1 = torch.autograd.grad(y, [x, lin.weight, lin.bias], g)
        g2 = torch.autograd.grad(yr, [x, lin.weight, lin.bias], g)
        for a, b in zip(g1, g2):
            assert rel(a, b) < 1e-5


def test_segment_mean_pool_and_backward():
    """mirec_segment_mean (the packed masked-mean pool) == per-sequence means
    in float64, empty sequences give 0/0 like the reference's division, and
    the backward spreads grad / length over each sequence's rows with zero on
    padding rows (seg == B)."""
    from furusato_recommend_amd.sasrec import _SegmentMean
    torch.manual_seed(12)
    lens = torch.tensor([3, 1, 64, 0, 17, 50], device="cuda")
    B, d = lens.numel(), 128
    offsets = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
    offsets[1:] = torch.cumsum(lens, 0).int()
    n_tok = int(lens.sum())
    pad = 7
    x = torch.randn(n_tok + pad, d, device="cuda", requires_grad=True)
    seg = torch.cat([torch.repeat_interleave(torch.arange(B, device="cuda"), lens),
                     torch.full((pad,), B, device="cuda")])
    out = _SegmentMean.apply(x, offsets, seg, lens)
    xd = x.detach().double()
    for b in range(B):
        s, e = int(offsets[b]), int(offsets[b + 1])
        if e > s:
            assert rel(out[b], xd[s:e].mean(0)) < 1e-6
        else:
            assert torch.isnan(out[b]).all()
    g = torch.randn(B, d, device="cuda")
    g[3] = 0  # the empty sequence has no rows to receive its gradient
    gx, = torch.autograd.grad(out, x, g)
    ref = torch.zeros_like(gx)
    for b in range(B):
        s, e = int(offsets[b]), int(offsets[b + 1])
        ref[s:e] = g[b] / max(e - s, 1)
    assert rel(gx, ref) < 1e-6 and float(gx[n_tok:].abs().max()) == 0.0


def test_seq_pack_matches_host_packing():
    """mirec_seq_pack (the captured step's packing) == the packing computed
    on the host: offsets, lengths, token ids, seg, padding rows (-1 / B), the
    int32 positives / negatives after the tokens, and clamping when the batch
    exceeds the capacity (no row past it is ever addressed)."""
    from furusato_recommend_amd import SASRec, SyntheticBipartite
    ds = SyntheticBipartite(900, 200, 20_000, seed=8)
    m = SASRec({"recdim": 64, "layer": 1, "heads": 2, "lr": 1e-3, "decay": 1e-4,
                "device": "cuda:0", "bpr_batch_size": 1500, "dropout_p": 0.0}, ds)
    rng = np.random.default_rng(4)
    items = m.seq.items.cpu().numpy()
    lens_tab = m.seq.length_host
    for B in (1, 7, 1500):
        users = rng.integers(0, 900, B)
        pos, neg = rng.integers(0, 200, B), rng.integers(0, 200, B)
        lens = lens_tab[users]
        n_tok = int(lens.sum())
        for cap in (n_tok + 300, max(n_tok // 2, 1)):
            ud = torch.as_tensor(users, device="cuda")
            ids_all, pk, seg, length = m.packed_ids_static(
                ud, cap, torch.as_tensor(pos, device="cuda"), torch.as_tensor(neg, device="cuda"))
            off = np.minimum(np.concatenate([[0], np.cumsum(lens)]), cap)
            assert np.array_equal(pk.offsets.cpu().numpy(), off)
            assert np.array_equal(length.cpu().numpy(), lens)
            ids_ref = np.full(cap, -1)
            seg_ref = np.full(cap, B)
            for b in range(B):
                for t in range(off[b], off[b + 1]):
                    ids_ref[t] = items[users[b], t - off[b]]
                    seg_ref[t] = b
            got = ids_all.cpu().numpy()
            assert np.array_equal(got[:cap], ids_ref)
            assert np.array_equal(seg.cpu().numpy(), seg_ref)
            assert np.array_equal(got[cap:cap + B], pos) and np.array_equal(got[cap + B:], neg)


def test_slice_norms_match_fp64():
    """mirec_slice_norms (the id-table norm terms of the SAGE / SASRec loss)
    == float64 norms of both slices, empty slices give 0, bitwise repeatable."""
    from furusato_recommend_amd.rows import slice_norms
    torch.manual_seed(13)
    for rows, split in ((1000, 600), (1, 0), (1, 1), (70_001, 35_000), (4, 4)):
        t = torch.randn(rows, 128, device="cuda")
        a, b = slice_norms(t, split)
        td = t.double()
        assert abs(float(a) - float(td[:split].norm())) <= 1e-6 * max(1.0, float(td[:split].norm()))
        assert abs(float(b) - float(td[split:].norm())) <= 1e-6 * max(1.0, float(td[split:].norm()))
        a2, b2 = slice_norms(t, split)
        assert torch.equal(a, a2) and torch.equal(b, b2)


def test_sorted_leaf_backward_matches_atomic_and_is_deterministic():
    """mirec_fanout_mean_gather_bwd_sorted (radix sort by child id + ordered
    per-row sums) == the float-atomic scatter within fp32 rounding, with
    dropout, invalid (-1) children and hub ids repeated many times; two runs
    are bitwise equal."""
    import ctypes

    from furusato_recommend_amd import _lib
    lib = _lib.lib
    torch.manual_seed(14)
    n_rows, d, k, n_t = 5000, 128, 10, 30_000
    ids = torch.randint(0, n_rows, (n_t * k,), dtype=torch.int32, device="cuda")
    ids[torch.rand(n_t * k, device="cuda") < 0.1] = -1
    ids[::7] = 3  # a hub
    g = torch.randn(n_t, d, device="cuda")
    base = torch.randn(n_rows, d, device="cuda")
    st = _lib.stream_handle()
    for p in (0.0, 0.3):
        a = base.clone()
        _lib.check(lib.mirec_fanout_mean_gather_bwd(g.data_ptr(), ids.data_ptr(), n_t, k, d, p,
                                                    ctypes.c_uint64(5), a.data_ptr(), st), "atomic")
        outs = []
        for _ in range(2):
            b = base.clone()
            nb = ctypes.c_size_t()
            _lib.check(lib.mirec_fanout_mean_gather_bwd_sorted_workspace(n_t, k, n_rows,
                                                                         ctypes.byref(nb)), "ws")
            ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
            _lib.check(lib.mirec_fanout_mean_gather_bwd_sorted(
                g.data_ptr(), ids.data_ptr(), n_t, k, d, p, ctypes.c_uint64(5), n_rows,
                b.data_ptr(), ws.data_ptr(), nb.value, st), "sorted")
            outs.append(b)
        # two fp32 summation orders of a 43 K-entry hub row: ~sqrt(n) eps apart
        assert rel(outs[0], a) < 5e-5
        assert torch.equal(outs[0], outs[1])
        if p == 0.0:  # both against the exact sum
            idc = ids.view(n_t, k).long()
            cnt = (idc >= 0).sum(1).clamp(min=1).double()
            ref = base.double().clone()
            ok = idc >= 0
            rows = torch.arange(n_t, device="cuda").view(-1, 1).expand(n_t, k)[ok]
            ref.index_add_(0, idc[ok], (g.double() / cnt[:, None])[rows])
            assert rel(outs[0], ref) < 1e-5 and rel(a, ref) < 1e-5


# ------------------------------------------------------------------ C5 / C3 full size
@pytest.mark.timeout(900)
def test_c5_full_size_properties():
    """BASELINE C5 model configuration on one GPU: LightGCN-3 d=256 on the
    10M users x 1M items / 200M-edge graph (SURVEY §8d recipe).  Size-
    independent checks: sqrt(deg) is a fixed point of Â, 256 sampled rows vs
    float64 host sums, and two frontier-pruned training steps equal two
    full-graph steps (fp32 summation order aside)."""
    from furusato_recommend_amd import Graph, SyntheticBipartite
    from furusato_recommend_amd.engine import AdamState, PropagationEngine, sample_triples
    ds = SyntheticBipartite(10_000_000, 1_000_000, 200_000_000, seed=0, test_frac=0)
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    del ds
    N, D = g.n_nodes, 256
    assert N == 11_000_000 and g.nnz == 400_000_000
    eng = PropagationEngine(g, D, 3, 2048)
    x = torch.randn(N, D, device="cuda") * 0.1
    deg = torch.from_numpy(g.degree().astype(np.float32)).cuda()
    x[:, 0] = deg.sqrt()
    y = torch.empty_like(x)
    eng.propagate_once(x, y)
    assert rel(y[:, 0], x[:, 0]) < 1e-5
    rows = np.random.default_rng(1).choice(N, 256, replace=False)
    rows = np.concatenate([rows, [N - 1, g.n_users - 1, g.n_users]])  # ends of both halves
    xr = {}
    rp, col = g.rowptr_host, g.col_host
    need = np.unique(np.concatenate([col[rp[r]:rp[r + 1]] for r in rows]))
    xh = dict(zip(need.tolist(), x[torch.from_numpy(need).cuda()].cpu().double().numpy()))
    dinv = g.dinv.cpu().double().numpy()
    for r in rows:
        nb = col[rp[r]:rp[r + 1]]
        xr[r] = dinv[r] * sum(dinv[j] * xh[int(j)] for j in nb) if len(nb) else np.zeros(D)
    ref = np.stack([xr[r] for r in rows])
    assert rel(y[torch.from_numpy(rows).cuda()], ref) < 1e-5
    del x, y, eng
    torch.cuda.empty_cache()
    torch.manual_seed(0)
    e0 = torch.randn(N, D, device="cuda") * 0.1
    tables, losses = [], []
    for prune in (True, False):
        eng = PropagationEngine(g, D, 3, 2048, prune=prune)
        e = e0.clone()
        adam = AdamState(e, 1e-3)
        u = torch.empty(2048, dtype=torch.int32, device="cuda")
        p, n = torch.empty_like(u), torch.empty_like(u)
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        ls = []
        for step in range(2):
            sample_triples(g, 2048, 7, step * 2048, u, p, n, err)
            ls.append(float(eng.train_step(e, adam, u, p, n, 1e-4)))
        assert int(err.item()) == 0
        # compare on a fixed random subset of rows + every batch row
        pick = torch.cat([torch.randint(0, N, (200_000,), device="cuda",
                                        generator=torch.Generator("cuda").manual_seed(3)),
                          u.long(), p.long() + g.n_users, n.long() + g.n_users])
        tables.append(e[pick].cpu())
        losses.append(ls)
        del eng, e, adam
        torch.cuda.empty_cache()
    assert rel(tables[0], tables[1]) < 1e-5
    assert np.allclose(losses[0], losses[1], rtol=1e-5)
    assert not torch.equal(tables[0], e0[pick].cpu())


@pytest.mark.timeout(600)
def test_c3_full_size_sorted_vs_atomic_and_learns():
    """BASELINE C3 model configuration: GraphSAGE 2-hop fanout [25, 10],
    d=128 on the C2 graph (1M x 100K / 20M).  The deterministic sorted
    table-gradient path equals the float-atomic one (fp32 order aside) and
    is bitwise repeatable; the root outputs, the loss and the table gradient
    on ~260 sampled rows (touched and untouched by the tree, the hub item,
    both slice ends) match float64 host sums of the same tree (the oracle's
    restatement, no dropout); training from random init drives the BPR loss
    down and stays finite."""
    from furusato_recommend_amd import GraphSAGE, SyntheticBipartite
    from furusato_recommend_amd import graphsage as gs
    ds = SyntheticBipartite(1_000_000, 100_000, 20_000_000, seed=0, test_frac=0)
    cfg = {"recdim": 128, "layer": 2, "fanouts": [25, 10], "lr": 1e-3, "decay": 1e-7,
           "device": "cuda:0", "bpr_batch_size": 2048}
    torch.manual_seed(2020)
    m = GraphSAGE(cfg, ds)
    u, p, n = m.sample(2048, seed=7)
    seeds = torch.cat([u, p + m.n_user, n + m.n_user])
    tree = m.sample_tree(seeds, 1234)
    grads = []
    saved = gs.SORTED_LEAF_BACKWARD
    try:
        for mode in (True, True, False):
            gs.SORTED_LEAF_BACKWARD = mode
            for q in m.parameters():
                q.grad = None
            out = m.forward(tree, dropout_seed=99)
            B = 2048
            m.loss(out[:B], out[B:2 * B], out[2 * B:]).backward()
            grads.append(m.table_grad_dense().clone())
    finally:
        gs.SORTED_LEAF_BACKWARD = saved
    assert torch.equal(grads[0], grads[1])          # deterministic
    assert rel(grads[2], grads[0]) < 1e-5            # == float-atomic scatter
    assert float(grads[0].abs().sum()) > 0
    # float64 host reference of the same tree (no dropout): the oracle's
    # restatement of graphsage.py:311-337 over the whole 1.76 M-row tree
    from oracle import lightgcn_oracle as O
    B = 2048
    for q in m.parameters():
        q.grad = None
    out = m.forward(tree, dropout_seed=None)
    loss = m.loss(out[:B], out[B:2 * B], out[2 * B:])
    loss.backward()
    g32 = m.table_grad_dense()
    touched = torch.nonzero(m._tg.stamp == m._tg.gen).view(-1).cpu()
    t64 = m._table.detach().cpu().double().requires_grad_(True)
    lin = []
    for w in m.w_linears:
        a = torch.nn.Linear(256, 128).double()
        a.load_state_dict({k: v.detach().cpu().double() for k, v in w.state_dict().items()})
        lin.append(a)
    groups = [g.cpu().numpy() for g, _ in tree.groups]
    o64 = O.sage_forward(t64, lin, groups, 2, [25, 10])
    reg = [t64[:m.n_user], t64[m.n_user:]] + [q for a in lin for q in (a.weight, a.bias)]
    l64 = O.sage_loss(o64[:B], o64[B:2 * B], o64[2 * B:], reg, 1e-7)
    l64.backward()
    assert rel(out, o64) < 1e-5                       # every seed's hop-2 output
    assert abs(float(loss) - float(l64)) < 1e-5 * abs(float(l64))
    gen = torch.Generator().manual_seed(3)
    deg = torch.from_numpy(m.graph.degree())
    hub = int(torch.argmax(deg))
    untouched = torch.nonzero(m._tg.stamp.cpu() != m._tg.gen).view(-1)
    rows = torch.cat([touched[torch.randperm(len(touched), generator=gen)[:192]],
                      untouched[torch.randperm(len(untouched), generator=gen)[:60]],
                      torch.tensor([0, m.n_user - 1, m.n_user, hub, len(deg) - 1])]).unique()
    assert hub in touched.tolist()                    # the most repeated id is in the tree
    ref = t64.grad[rows]
    assert rel(g32.cpu()[rows], ref) < 1e-4
    # the sparse rows against their own scale (the norm term alone is ~1e-9)
    tr = rows[torch.isin(rows, touched)]
    assert rel(g32.cpu()[tr], t64.grad[tr]) < 1e-4
    del t64, o64, l64, lin
    losses = []
    for i in range(40):
        u, p, n = m.sample(2048, seed=11, offset=i * 2048)
        losses.append(float(m.stageOne(u, p, n)))
    assert np.all(np.isfinite(losses))
    assert np.mean(losses[-8:]) < np.mean(losses[:8])
    assert torch.isfinite(m._table).all()


def test_sage_training_steps_bitwise_repeatable():
    """Two GraphSAGE models from the same seed, fed the same batches: every
    parameter (the id table, its Adam moments, the Linear layers) is bitwise
    equal after three full steps — sampling, dropout, the sorted table
    gradient (inner rows and leaf means), the hop GEMMs' fixed-order weight
    gradients and the end-of-backward norm-gradient launch run in fixed
    orders (no float atomics on the step's path)."""
    from furusato_recommend_amd import GraphSAGE, SyntheticBipartite
    ds = SyntheticBipartite(20_000, 3_000, 300_000, seed=3, kind="zipf", test_frac=0)
    cfg = {"recdim": 128, "layer": 2, "fanouts": [25, 10], "lr": 1e-3, "decay": 1e-4,
           "device": "cuda:0", "bpr_batch_size": 512}
    models = []
    for _ in range(2):
        torch.manual_seed(77)
        m = GraphSAGE(cfg, ds)
        for i in range(3):
            u, p, n = m.sample(512, seed=5, offset=i * 512)
            m.stageOne(u, p, n)
        models.append(m)
    a, b = models
    for x, y in zip(a.parameters(), b.parameters()):
        assert torch.equal(x, y)
    assert torch.equal(a._table, b._table)
    assert torch.equal(a._table_state.exp_avg, b._table_state.exp_avg)
    assert torch.equal(a._table_state.exp_avg_sq, b._table_state.exp_avg_sq)


# ------------------------------------------------------------ multi-rank on one GPU
def _dp_rank_lgcn(rank, world, port, fpath, mode, q):
    """One rank of the LightGCN data-parallel step on cuda:0 (gloo
    collectives; RCCL needs a GPU per rank): the real PropagationEngine,
    disjoint halves of the fixture's triples."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist

    from furusato_recommend_amd.dist import DataParallel, init_distributed
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    init_distributed("gloo", rank=rank, world_size=world, timeout_s=120)
    try:
        f = dict(np.load(fpath))
        m = lgcn_from(f)
        if rank:  # a different init: the constructor broadcast must fix it
            with torch.no_grad():
                m.all_embedding.weight.add_(0.5)
        dp = DataParallel(m.engine, m.all_embedding.weight.data, m.optim, mode=mode)
        t = torch.from_numpy(f["triples"]).cuda().int()
        half = t.shape[0] // world
        mine = t[rank * half:(rank + 1) * half]
        tabs = []
        for _ in range(2):
            dp.step(mine[:, 0].contiguous(), mine[:, 1].contiguous(), mine[:, 2].contiguous(),
                    float(f["decay"]))
            tabs.append(m.all_embedding.weight.detach().cpu().numpy().copy())
        torch.cuda.synchronize()
        q.put((rank, tabs))
    finally:
        dist.destroy_process_group()


def _dp_rank_autograd(rank, world, port, kind, shard, q):
    """One rank of DenseGradDataParallel over the real GraphSAGE / SASRec on
    cuda:0: every rank steps on its own user shard; the gradient all-reduce
    (or the sharded table Adam) must keep the replicas identical."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist

    from furusato_recommend_amd import GraphSAGE, SASRec, SyntheticBipartite
    from furusato_recommend_amd.dist import DenseGradDataParallel, init_distributed
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    init_distributed("gloo", rank=rank, world_size=world, timeout_s=120)
    try:
        ds = SyntheticBipartite(20_000, 2_000, 200_000, seed=0)
        torch.manual_seed(100 + rank)
        cfg = {"recdim": 64, "layer": 2, "lr": 1e-3, "decay": 1e-4, "device": "cuda:0",
               "bpr_batch_size": 256, "heads": 2, "fanouts": [10, 5]}
        m = GraphSAGE(cfg, ds) if kind == "sage" else SASRec(cfg, ds)
        init = [x.detach().cpu().clone() for x in m.parameters()]
        dp = DenseGradDataParallel(m, shard_optimizer=shard, table_exchange="dense")
        assert dp.shard_optimizer == shard
        if rank == 0:
            init = [x.detach().cpu().clone() for x in m.parameters()]
        batches = []
        for i in range(3):
            if kind == "sage":
                u, p, n = m.sample(256, seed=5, offset=i * 256, shard=rank, n_shards=world)
            else:
                g = torch.Generator().manual_seed(1000 * i + rank)
                u = torch.randint(0, ds.n_users // world, (256,), generator=g) * world + rank
                p = torch.randint(0, ds.m_items, (256,), generator=g)
                n = torch.randint(0, ds.m_items, (256,), generator=g)
            # numpy: torch tensors travel through a file descriptor that dies
            # with this process
            batches.append([torch.as_tensor(x).cpu().numpy() for x in (u, p, n)])
            dp.step(u, p, n)
        torch.cuda.synchronize()
        if shard:
            dp.gather_optimizer_state()
        mom = [s.exp_avg.detach().cpu().numpy().copy() for s in m.optims][:1]
        q.put((rank, [x.detach().cpu().numpy().copy() for x in m.parameters()], batches,
               [x.numpy() for x in init], mom))
    finally:
        dist.destroy_process_group()


def _run_ranks(target, args, world=2, timeout=300):
    import multiprocessing as mpp
    import socket
    ctx = mpp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=target, args=(r, world, port, *args, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    try:
        res = dict((r, rest) for r, *rest in (q.get(timeout=timeout) for _ in range(world)))
    finally:
        for pr in procs:
            pr.join(timeout=60)
            if pr.is_alive():
                pr.kill()
    assert all(pr.exitcode == 0 for pr in procs)
    return res


@pytest.mark.timeout(600)
@pytest.mark.parametrize("mode", ["sparse", "dense", "sharded"])
def test_data_parallel_two_ranks_hip_engine(golden, mode):
    """2 ranks (processes) of dist.DataParallel with the real HIP engine on
    one GPU: replicas bit-identical after each step and equal to the
    reference's stageOne on the union batch (emb_step1 / emb_step2)."""
    from tests.conftest import GOLDEN
    f = golden("lgcn_d64_L3.npz")
    res = _run_ranks(_dp_rank_lgcn, (os.path.join(GOLDEN, "lgcn_d64_L3.npz"), mode))
    for k in range(2):
        assert np.array_equal(res[0][0][k], res[1][0][k])
        assert rel(res[0][0][k], f[f"emb_step{k + 1}"]) < TOL


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind", ["sage", "sasrec"])
def test_dense_grad_data_parallel_two_ranks(kind):
    """DenseGradDataParallel over the real GraphSAGE / SASRec, 2 ranks on one
    GPU: replicas stay bit-identical and move away from the broadcast init;
    the sharded table Adam (each rank steps its half of the table's rows,
    then an in-place all-gather) gives the same parameters bit for bit as
    the all-reduce + full Adam, and its gathered Adam moments equal theirs."""
    res = _run_ranks(_dp_rank_autograd, (kind, False))
    p0, p1 = res[0][0], res[1][0]
    assert len(p0) == len(p1)
    for a, b in zip(p0, p1):
        assert np.array_equal(a, b)
        assert np.all(np.isfinite(a))
    init0 = res[0][2]
    assert any(not np.array_equal(a, b) for a, b in zip(p0, init0))
    rs = _run_ranks(_dp_rank_autograd, (kind, True))
    for r in range(2):
        for a, b in zip(rs[r][0], p0):
            assert np.array_equal(a, b)
        assert np.array_equal(rs[r][3][0], res[0][3][0])


def _dp_rank_union(rank, world, port, kind, exchange, q, over=None, bucket_min=None, steps=3,
                   microbatches=1, sizes=None):
    """One rank of DenseGradDataParallel (GraphSAGE / SASRec) on cuda:0 with
    the table exchange ``exchange``; returns what the single-process
    reference step needs (the batches, the CPU generator states SASRec's
    dropout seeds come from) and the parameters after ``steps`` steps.
    ``bucket_min`` lowers the in-place / row-sharded threshold so a test-sized
    id table takes the large-table route (the row-sharded Adam)."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist

    from furusato_recommend_amd.dist import DenseGradDataParallel, init_distributed
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    init_distributed("gloo", rank=rank, world_size=world, timeout_s=120)
    try:
        m, ds = _union_model(kind, **(over or {}))
        if bucket_min is not None:
            DenseGradDataParallel.BUCKET_MIN = int(bucket_min)
        dp = DenseGradDataParallel(m, table_exchange=exchange, microbatches=microbatches)
        assert dp.table_exchange == exchange
        if bucket_min is not None and exchange == "dense":
            assert dp.table_stepped_by_hook()  # the row-sharded table Adam
        batches, states, losses = [], [], []
        for i in range(steps):
            u, p, n = _union_batch(m, ds, kind, i, rank, world, sizes[i] if sizes else 256)
            batches.append([torch.as_tensor(x).cpu().numpy() for x in (u, p, n)])
            states.append(torch.get_rng_state().numpy().copy())
            losses.append(float(dp.step(u, p, n)))
        torch.cuda.synchronize()
        dp.gather_optimizer_state()
        st = m._table_state
        q.put((rank, [x.detach().cpu().numpy().copy() for x in m.parameters()], batches, states,
               st.exp_avg.cpu().numpy().copy(), dp.last_exchange_bytes, losses))
    finally:
        dist.destroy_process_group()


def _union_model(kind, **over):
    from furusato_recommend_amd import GraphSAGE, SASRec, SyntheticBipartite
    ds = SyntheticBipartite(20_000, 2_000, 200_000, seed=0)
    torch.manual_seed(100)
    cfg = {"recdim": 64, "layer": 2, "lr": 1e-3, "decay": 1e-4, "device": "cuda:0",
           "bpr_batch_size": 256, "heads": 2, "fanouts": [10, 5], "graph": False}
    cfg.update(over)
    return (GraphSAGE(cfg, ds) if kind == "sage" else SASRec(cfg, ds)), ds


def _union_batch(m, ds, kind, i, rank, world, n=256):
    if kind == "sage":
        return m.sample(n, seed=5, offset=i * 256, shard=rank, n_shards=world)
    g = torch.Generator().manual_seed(1000 * i + rank)
    u = torch.randint(0, ds.n_users // world, (256,), generator=g) * world + rank
    return u, torch.randint(0, ds.m_items, (256,), generator=g), \
        torch.randint(0, ds.m_items, (256,), generator=g)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind,exchange", [("sage", "fetch"), ("sage", "routed"),
                                           ("sage", "dense"), ("sasrec", "routed"),
                                           ("sasrec", "dense")])
def test_dense_grad_data_parallel_equals_union_step(kind, exchange):
    """DenseGradDataParallel, 2 ranks on one GPU, against ONE process that
    takes, at the same parameters, the gradient of each rank's batch with the
    loss x 1/2 (same sampled trees / dropout seeds), sums them and steps Adam
    on the dense sum — DDP's averaged gradient (ddp_sage.py:754-878 meant
    this; its .module.OneEpoch never synchronised, :805).  3 steps.  Every
    parameter matches bit for bit under the dense reduce-scatter (the
    reference's own dense Adam on the same sum) and to 1e-6 under the routed
    exchange, which adds the ranks' sparse terms before the norm term
    (c·W + (S_0 + S_1) instead of (c_0·W + S_0) + (c_1·W + S_1): fp32
    rounding of the table, which the next steps' gradients then see) — on
    every element whose exact gradient is not zero (see the comparison);
    Adam moments (gathered from the row shards) likewise."""
    res = _run_ranks(_dp_rank_union, (kind, exchange))
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b)
    m, ds = _union_model(kind)
    m._tg.dense = True  # the reference materialises every rank's dense table gradient
    params = list(m.parameters())
    for i in range(3):
        grads = []
        for r in (0, 1):
            u, p, n = (torch.from_numpy(x).cuda() for x in res[r][1][i])
            for x in params:
                x.grad = None
            if kind == "sage":
                seed = m._step_seed * 7919 + i
                seeds = torch.cat([u.int(), p.int() + m.n_user, n.int() + m.n_user])
                emb = m.forward(m.sample_tree(seeds, seed), dropout_seed=seed)
                m.loss_fused(emb).backward(torch.tensor(0.5, device="cuda"))
            else:  # the eager step's BLAS backend and dropout keys
                from furusato_recommend_amd.sasrec import blas_backend
                torch.set_rng_state(torch.from_numpy(res[r][2][i]))
                with blas_backend(m.config.get("blas", "cublas")):
                    ids, packing, seg, length = m.packed_ids(u)
                    m._step_body(ids, packing, seg, length, p, n, 0.5)
            grads.append([x.grad.clone() for x in params])
        for x, g0, g1 in zip(params, *grads):
            x.grad = g0 + g1
        m.optimizer_step()
    torch.cuda.synchronize()
    names = [n for n, _ in m.named_parameters()]
    diffs = {nm: rel(torch.from_numpy(got), x.detach().cpu())
             for nm, x, got in zip(names, params, res[0][0])}
    for nm, x, got in zip(names, params, res[0][0]):
        ref = x.detach().cpu()
        got = torch.from_numpy(got)
        if exchange == "dense":
            assert torch.equal(got, ref), diffs
            continue
        # Adam's step is lr·m̂/(√v̂ + eps): where the exact gradient is zero
        # and the computed one rounding noise, any fp32 difference becomes
        # up to ±lr per step.  SASRec has two such slices: the attention key
        # bias (softmax is invariant to q·b_k, the same for every key of a
        # query) and the item tower's last bias (it adds <u, b> to the
        # positive and the negative score alike: the BPR difference cancels
        # it).  They are bounded by the step size; every other element is
        # compared at 1e-6 — 1e-5 for GraphSAGE, whose rank-split table
        # gradient is summed in another association (each rank's row sums,
        # then the owner's sum over ranks) than the union's one sequential
        # sum per row, and whose last-layer bias gradient (a sum over the
        # 3B seed rows with the pos / neg terms largely cancelling) carries
        # that difference through three Adam steps.
        tol = 1e-5 if kind == "sage" else 1e-6
        ok = torch.ones_like(got, dtype=torch.bool)
        if nm.endswith("in_proj_bias"):
            ok[got.numel() // 3: 2 * got.numel() // 3] = False
        if nm == "item_last_proj.bias":
            ok[:] = False
        assert float((got - ref).abs().max()) <= 3 * 1e-3 + 1e-7, (nm, diffs)
        if bool(ok.any()):
            assert rel(got[ok], ref[ok]) < tol, (nm, diffs)
    mom = m._table_state.exp_avg.cpu()
    assert rel(torch.from_numpy(res[0][3]), mom) <= (1e-6 if exchange != "dense" else 0.0)
    assert res[0][4] > 0  # bytes received in the last step's exchange


@pytest.mark.parametrize("B", [256, 100, 2])
def test_sage_microbatch_gradient_equals_batch_gradient(B):
    """GraphSAGE.stageOne(chunks=3) on one process (the pipelined exchange's
    micro-batching, hooks doing nothing): the gradients summed over the
    micro-batches equal the gradient of the UNCHUNKED batch loss
    (model/graphsage.py:326-337: mean over all B triples of softplus, plus
    decay x all_param / B once), written out here in plain torch over the
    same micro-batch trees, for B divisible by 3, not divisible, and B < 3
    (two micro-batches); the returned loss is that loss.  1e-5 relative
    (fp32 summation order)."""
    import torch.nn.functional as F
    m, _ = _union_model("sage")
    m._tg.dense = True  # the table gradient lands in .grad (sums over backwards)
    params = list(m.parameters())
    u, p, n = m.sample(B, seed=9, offset=0)
    u, p, n = u.long(), p.long(), n.long()
    seed = m._step_seed * 7919 + m._calls
    C = min(3, B)
    bnd = m.chunk_bounds(B, C)
    for x in params:
        x.grad = None
    ref_loss = 0.0
    for k in range(C):
        a, b = bnd[k], bnd[k + 1]
        sk = m.chunk_seed(seed, k)
        seeds = torch.cat([u[a:b], p[a:b] + m.n_user, n[a:b] + m.n_user]).int()
        emb = m.forward(m.sample_tree(seeds, sk), dropout_seed=sk)
        m._slice_norms2 = None
        bk = b - a
        ue, pe, ne = emb[:bk], emb[bk:2 * bk], emb[2 * bk:]
        part = F.softplus((ue * ne).sum(1) - (ue * pe).sum(1)).sum() / B
        part.backward()
        ref_loss += float(part)
    all_param = 0
    for prm in m.reg_parameters():  # graphsage.py:329-332 (doubling)
        all_param = all_param + all_param + prm.norm(2)
    norm_term = all_param / B * m.config["decay"]
    norm_term.backward()
    ref_loss += float(norm_term)
    ref = [x.grad.detach().clone() for x in params]
    got = {}

    def grab():
        got["g"] = [x.grad.detach().clone() for x in params]
    loss = m.stageOne(u, p, n, chunks=3, chunk_hook=lambda k, phase: None, grad_hook=grab)
    assert m._calls == 1
    for (nm, _), a, b in zip(m.named_parameters(), got["g"], ref):
        assert rel(a, b) < 1e-5, (nm, rel(a, b))
    assert abs(float(loss) - ref_loss) <= 1e-5 * abs(ref_loss)


CHUNK_SIZES = (256, 100, 2)  # 85/85/86, 33/33/34, and fewer triples than micro-batches


def _dp_rank_union_chunks(rank, world, port, q):
    _dp_rank_union(rank, world, port, "sage", "fetch", q, microbatches=3, sizes=CHUNK_SIZES)


@pytest.mark.timeout(900)
def test_pipelined_fetch_equals_union_microbatches():
    """The pipelined fetch exchange (DenseGradDataParallel(microbatches=3):
    every micro-batch's read set routed up front, micro-batch k + 1's rows
    and micro-batch k's table-gradient rows in flight while the other
    computes), 2 ranks on one GPU, against ONE process that takes, at the
    same parameters, each rank's micro-batch gradients (micro-batch k of B_k
    of the B triples seeded with 1/2 x B_k/B, its norm term x 1/C_eff:
    GraphSAGE.stageOne(chunks=3)'s weights), sums them and steps the dense
    Adam, over 3 steps of 256, 100 and 2 triples per rank (B % 3 != 0, and
    B < 3: two micro-batches, the same count on both ranks): every
    parameter at 1e-5 relative (the routed sums are added in another order:
    fp32 rounding).  test_sage_microbatch_gradient_equals_batch_gradient
    checks those weights against the unchunked batch loss."""
    res = _run_ranks(_dp_rank_union_chunks, ())
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b)
    m, ds = _union_model("sage")
    m._tg.dense = True
    params = list(m.parameters())
    for i in range(3):
        grads = []
        for r in (0, 1):
            u, p, n = (torch.from_numpy(x).cuda() for x in res[r][1][i])
            assert u.numel() == CHUNK_SIZES[i]
            for x in params:
                x.grad = None
            seed = m._step_seed * 7919 + i
            B = u.numel()
            C = min(3, B)
            bnd = m.chunk_bounds(B, C)
            for k in range(C):
                a, b = bnd[k], bnd[k + 1]
                sk = m.chunk_seed(seed, k)
                seeds = torch.cat([u[a:b].int(), p[a:b].int() + m.n_user, n[a:b].int() + m.n_user])
                emb = m.forward(m.sample_tree(seeds, sk), dropout_seed=sk)
                m.loss_fused(emb, decay_scale=1.0 / C).backward(
                    torch.tensor(0.5 * (b - a) / B, device="cuda"))
            grads.append([x.grad.clone() for x in params])
        for x, g0, g1 in zip(params, *grads):
            x.grad = g0 + g1
        m.optimizer_step()
    torch.cuda.synchronize()
    for (nm, _), x, got in zip(m.named_parameters(), params, res[0][0]):
        ref, got = x.detach().cpu(), torch.from_numpy(got)
        assert float((got - ref).abs().max()) <= 3 * 1e-3 + 1e-7, nm
        assert rel(got, ref) < 1e-5, (nm, rel(got, ref))
    assert res[0][4] > 0


def _dp_trainer_rank(rank, world, port, kind, ckpt, q):
    """One rank of train_dp.DPTrainer on cuda:0 (gloo): the model's own
    on-device sampler per rank shard, two epochs with an evaluation each,
    then a fresh model resumes from the checkpoint for a third epoch."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist

    from furusato_recommend_amd import GraphSAGE, LightGCN, SyntheticBipartite
    from furusato_recommend_amd.dist import init_distributed
    from furusato_recommend_amd.train_dp import DPTrainer, optimizer_states
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    init_distributed("gloo", rank=rank, world_size=world, timeout_s=120)
    try:
        ds = SyntheticBipartite(20_000, 2_000, 200_000, seed=0, kind="cluster", n_clusters=50)
        cfg = {"recdim": 64, "layer": 2 if kind == "sage" else 3, "lr": 1e-3, "decay": 1e-4,
               "device": "cuda:0", "bpr_batch_size": 4096, "fanouts": [10, 5],
               "train_iterative": 1, "test_span": 1, "checkpoint_path": ckpt,
               "test_u_batch_size": 1000, "dp_mode": "sparse" if kind == "lgn" else None}

        def make(seed):
            torch.manual_seed(seed)
            return LightGCN(cfg, ds) if kind == "lgn" else GraphSAGE(cfg, ds)
        m = make(100 + rank)  # rank 1's init is replaced by the broadcast
        tr = DPTrainer(cfg, ds, m)
        hist = tr.fit(2)
        torch.cuda.synchronize()
        params = [p.detach().cpu().numpy().copy() for p in m.parameters()]
        m2 = make(7)
        tr2 = DPTrainer(cfg, ds, m2)
        loaded = tr2.load_checkpoint()
        resumed_at = tr2.epoch
        same = all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(m.parameters(), m2.parameters()))
        same_opt = all(torch.equal(a.exp_avg.cpu(), b.exp_avg.cpu())
                       for a, b in zip(optimizer_states(m), optimizer_states(m2)))
        # GraphSAGE's step counter (tree / dropout seeds) resumes too
        same_calls = getattr(m, "_calls", 0) == getattr(m2, "_calls", 0)
        h2 = tr2.fit(1)
        q.put((rank, params, hist, (loaded, resumed_at, same, same_opt, same_calls), h2))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind", ["lgn", "sage"])
def test_dp_trainer_two_ranks(kind, tmp_path):
    """train_dp.DPTrainer (ddp_lgcn.py:625-746 / ddp_sage.py:754-878) with the
    HIP models, 2 ranks on one GPU: the capped epoch sampler per rank shard,
    the exchange of dist.DataParallel / DenseGradDataParallel (fetch) every
    step, a checkpoint and an evaluation (Recall / Precision / NDCG / HR /
    Coverage @10, @20) every epoch on rank 0; replicas stay identical, the
    loss falls and recall rises on a community graph, and the checkpoint
    (table, Adam state, next epoch) reloads into a fresh model."""
    ckpt = str(tmp_path / f"ddp_{kind}_all.pth")
    res = _run_ranks(_dp_trainer_rank, (kind, ckpt), timeout=600)
    (p0, h0, r0, g0), (p1, h1, r1, g1) = res[0], res[1]
    for a, b in zip(p0, p1):
        assert np.array_equal(a, b)
    assert [h["epoch"] for h in h0] == [0, 1] and [h["epoch"] for h in g0] == [2]
    assert h0[0]["triples_per_rank"] == h1[0]["triples_per_rank"] > 0
    assert h0[0]["loss"] == h1[0]["loss"]
    assert g0[0]["loss"] < h0[0]["loss"]
    met = h0[1]["metrics"]
    for k in ("recall", "precision", "ndcg", "hr", "coverage"):
        assert len(met[k]) == 2 and all(np.isfinite(met[k]))
    assert met["recall"][1] > 0.0 and 0 < met["coverage"][0] <= met["coverage"][1] <= 1
    assert h1[1]["metrics"] is None
    assert r0 == (True, 2, True, True, True) and r1 == (True, 2, True, True, True)


def _dp_rank_union_graph(rank, world, port, exchange, graph, bucket_min, q):
    _dp_rank_union(rank, world, port, "sasrec", exchange, q,
                   over={"graph": graph, "dropout_p": 0.0, "blas": "cublas"},
                   bucket_min=bucket_min, steps=4)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("exchange,bucket_min", [("routed", None), ("dense", None),
                                                 ("dense", 1 << 16)])
def test_sasrec_data_parallel_captured_step_equals_eager(exchange, bucket_min):
    """SASRec under DenseGradDataParallel keeps its captured HIP-graph step:
    graph A (packing, forward, loss x 1/W, backward), the exchange between
    the replays, graph B (Adam of what the exchange does not step).  2 ranks
    on one GPU, dropout off (the captured step draws its dropout keys from a
    device seed base): the captured run gives the eager run's losses at every
    step and its parameters up to fp32 order (the step's row-slice sums see
    the capacity padding rows), and the replicas stay bit-identical.
    ``bucket_min`` = 2^16 puts the 2000 x 64 item table on the large-table
    route, the row-sharded Adam that consumes its .grad: every replay after
    the first must still step the table (it did not before the captured
    gradients were re-attached per replay), over 4 steps."""
    cap = _run_ranks(_dp_rank_union_graph, (exchange, True, bucket_min))
    eag = _run_ranks(_dp_rank_union_graph, (exchange, False, bucket_min))
    for a, b in zip(cap[0][0], cap[1][0]):
        assert np.array_equal(a, b)
    for r in (0, 1):  # every step's loss (as test_sasrec_graph_step_equals_eager)
        for lc, le in zip(cap[r][5], eag[r][5]):
            assert abs(lc - le) <= 1e-5 * abs(le), (r, cap[r][5], eag[r][5])
    m, _ = _union_model("sasrec")
    for (nm, _), a, b in zip(m.named_parameters(), cap[0][0], eag[0][0]):
        a, b = torch.from_numpy(a), torch.from_numpy(b)
        # (one BLAS backend for both) the captured step's row slices see the
        # capacity padding rows: fp32 order.  Adam's first steps are
        # ±lr·sign(g) wherever |g| >> eps, so an element whose gradient is
        # rounding noise — the structurally zero slices (attention key bias,
        # the item tower's last bias) and the occasional near-cancelling
        # table element — may step either way: every element within the 4
        # steps' bound, all but 0.1 % of each parameter's within 1e-4
        assert float((a - b).abs().max()) <= 2 * 4 * 1e-3 + 1e-7, nm
        far = (a - b).abs() > 1e-4 * float(b.abs().max())
        if nm.endswith("in_proj_bias"):
            far[a.numel() // 3: 2 * a.numel() // 3] = False
        if nm == "item_last_proj.bias":
            far[:] = False
        assert float(far.float().mean()) <= 1e-3, (nm, int(far.sum()))


# ------------------------------------------------------------ sorted table gradient
def _tg_groups(n_rows, d, seed, hub_count=0):
    """Row groups like a GraphSAGE step: inner rows (k=1) and two leaf mean
    groups with dropout; optionally one hub id repeated hub_count times."""
    g = torch.Generator().manual_seed(seed)
    inner_ids = torch.randint(0, n_rows, (3000,), generator=g)
    inner_ids[::97] = -1
    leaf1 = torch.randint(0, n_rows, (800 * 25,), generator=g)
    leaf1[::13] = -1
    leaf2 = torch.randint(0, n_rows // 10, (400 * 10,), generator=g)
    if hub_count:
        hub = torch.full((hub_count,), 7, dtype=torch.int64)
        leaf2 = torch.cat([leaf2, hub])
    leaf2 = leaf2[: (leaf2.numel() // 10) * 10]
    out = []
    for ids, k, mean, p, sd in ((inner_ids, 1, 0, 0.0, 0), (leaf1, 25, 1, 0.2, 11),
                                (leaf2, 10, 1, 0.1, 12)):
        gr = torch.randn(ids.numel() // k, d, generator=g)
        out.append((ids.int().cuda(), gr.cuda(), k, mean, p, sd))
    return out


def _tg_reference(groups, n_rows, d):
    """float64 sums of the same contributions with the dropout mask made on
    the host (tests/dropout_common.py, the rule of include/mirec.h: no kernel
    that shares the mask code takes part) — dense float64 on the host."""
    from tests import dropout_common
    acc = torch.zeros(n_rows, d, dtype=torch.float64)
    for ids, gr, k, mean, p, sd in groups:
        if mean:
            # one contribution row per entry: keep * scale * grad_out[t] / cnt_t
            mask, scale = dropout_common.fanout_mask(p, sd, ids.numel(), d)
            per = torch.from_numpy(dropout_common.entry_contributions(
                gr.cpu().numpy(), ids.cpu().numpy(), k, mask, scale))
        else:
            per = gr.cpu().double()
        idc = ids.cpu().long()
        ok = idc >= 0
        acc.index_add_(0, idc[ok], per[ok])
    return acc


def test_table_grad_hub_not_serial():
    """Timing guard for hub rows in the sorted table gradient (the C3 leaf
    backward on a skewed graph): 1.5 M leaf entries (150 K targets x 10, d =
    128, dropout) all naming ONE row must cost within 4x of the same entries
    spread uniformly over 1.1 M rows — a run is cut into fixed chunks whose
    partials are combined in order, not walked by one wave (which is ~100x
    slower at this size)."""
    from furusato_recommend_amd.graphsage import TableGrad
    n_rows, d, n_t, k = 1_100_000, 128, 150_000, 10
    g = torch.Generator(device="cuda").manual_seed(5)
    gr = torch.randn(n_t, d, device="cuda", generator=g)
    times = {}
    for kind in ("uniform", "hub"):
        if kind == "uniform":
            ids = torch.randint(0, n_rows, (n_t * k,), device="cuda", generator=g).int()
        else:
            ids = torch.full((n_t * k,), 12_345, dtype=torch.int32, device="cuda")
        tg = TableGrad(n_rows, 1_000_000, d, "cuda")
        groups = [(ids, gr, k, 1, 0.1, 3)]
        tg.accumulate(groups)
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            tg.accumulate(groups)
            e.record()
            torch.cuda.synchronize()
            ts.append(s.elapsed_time(e))
        times[kind] = sorted(ts)[2]
    assert times["hub"] < 4.0 * times["uniform"] + 0.05, times


@pytest.mark.parametrize("d", [16, 128, 256])
def test_table_grad_runs_of_every_length_and_alignment(d):
    """Pass 1 owns the runs that start in its chunk and sums a run that
    leaves the chunk whole when it ends within the next chunk's span, else
    (long runs) through the partial slots and pass 2: runs of every length
    1..40 (then 100, 300, 1000) laid end to end, so every run length meets
    every alignment to the chunk grid (8 entries), invalid entries mixed in
    — each row against float64, only touched rows stamped, bitwise equal on
    a rerun.  Inner (k = 1) rows and a dropout-mean leaf group (k = 10)."""
    from furusato_recommend_amd.graphsage import TableGrad
    n_rows = 6000
    g = torch.Generator().manual_seed(d)
    lens = torch.randint(1, 41, (1500,), generator=g)
    lens = torch.cat([lens, torch.tensor([100, 300, 1000, 17, 9, 8, 7, 16, 15])])
    ids = torch.repeat_interleave(torch.randperm(n_rows, generator=g)[:lens.numel()], lens)
    ids = ids[torch.randperm(ids.numel(), generator=g)]  # the sort restores the runs
    ids[::53] = -1
    n_inner = (ids.numel() // 3) // 10 * 10
    inner, leaf = ids[:n_inner], ids[n_inner:]
    leaf = leaf[: leaf.numel() // 10 * 10]
    groups = []
    for q, k, mean, p, sd in ((inner, 1, 0, 0.0, 0), (leaf, 10, 1, 0.2, 21)):
        gr = torch.randn(q.numel() // k, d, generator=g)
        groups.append((q.int().cuda(), gr.cuda(), k, mean, p, sd))
    tg = TableGrad(n_rows, 2000, d, "cuda")
    tg.accumulate(groups)
    a1, st = tg.acc.clone(), tg.stamp.clone()
    tg.accumulate(groups)
    assert torch.equal(tg.acc[st == 1], a1[st == 1])
    ref = _tg_reference(groups, n_rows, d)
    touched = torch.zeros(n_rows, dtype=torch.bool)
    for q, *_ in groups:
        qc = q.cpu().long()
        touched[qc[qc >= 0]] = True
    assert torch.equal(st.cpu() == 1, touched)
    got = a1.cpu().double()
    assert rel(got[touched], ref[touched]) < 1e-5
    # per row (a lost or doubled contribution is an O(1) error on its row)
    err = (got - ref).abs().max(1).values / ref.abs().max(1).values.clamp(min=1e-30)
    assert float(err[touched].max()) < 1e-3
    # the packed form (mirec_table_grad_sorted_rows) over the same runs
    from furusato_recommend_amd.dist import export_stamped
    tg.rows_parts = 4
    tg.accumulate(groups)
    rows, vals, counts, _ = export_stamped(tg, 4)
    ref_rows = torch.nonzero(st == 1).view(-1).int()
    assert int(counts[0]) == ref_rows.numel() and int(counts[1:].sum()) == ref_rows.numel()
    assert torch.equal(rows[:ref_rows.numel()], ref_rows)
    assert torch.equal(vals[:ref_rows.numel()], a1[ref_rows.long()])


@pytest.mark.parametrize("d", [16, 128, 256])
@pytest.mark.parametrize("hub", [0, 200_000])
def test_table_grad_sorted_matches_fp64_and_repeats(d, hub):
    """mirec_table_grad_sorted: per-row sums of inner rows and dropout-mean
    leaf entries == float64 sums (1e-5), only touched rows stamped, bitwise
    equal on a rerun; a hub id in 2e5 entries (3K chunks) goes through the
    chunk partials."""
    from furusato_recommend_amd.graphsage import TableGrad
    n_rows = 5000
    groups = _tg_groups(n_rows, d, seed=d + hub, hub_count=hub)
    tg = TableGrad(n_rows, 2000, d, "cuda")
    tg.accumulate(groups)
    a1 = tg.acc.clone()
    st = tg.stamp.clone()
    tg.accumulate(groups)
    assert torch.equal(tg.acc[st == 1], a1[st == 1])
    ref = _tg_reference(groups, n_rows, d)
    touched = torch.zeros(n_rows, dtype=torch.bool)
    for ids, *_ in groups:
        idc = ids.cpu().long()
        touched[idc[idc >= 0]] = True
    assert torch.equal((st.cpu() == 1), touched)
    got = a1.cpu().double()[touched]
    assert rel(got, ref[touched]) < 1e-5
    if hub:
        assert float((got[torch.nonzero(touched).squeeze(1) == 7] - ref[7]).abs().max()) \
            < 1e-5 * float(ref[7].abs().max())


@pytest.mark.parametrize("d", [16, 128, 256])
@pytest.mark.parametrize("hub", [0, 200_000])
@pytest.mark.parametrize("parts", [1, 3, 8])
def test_table_grad_packed_rows_equal_dense_form(d, hub, parts):
    """mirec_table_grad_sorted_rows (the pipelined exchange's export): the
    touched rows ascending with their rows of S bitwise equal to the dense
    form's acc rows, counts[0] = the touched rows and counts[1 + p] = those
    of owner block p (ragged last block), acc / stamp untouched; also
    through runs of every length and a hub (chunk partials, fixup)."""
    from furusato_recommend_amd.dist import export_stamped
    from furusato_recommend_amd.graphsage import TableGrad
    n_rows = 5000
    groups = _tg_groups(n_rows, d, seed=d + hub + 1, hub_count=hub)
    tg = TableGrad(n_rows, 2000, d, "cuda")
    tg.accumulate(groups)
    rows_ref = torch.nonzero(tg.stamp == tg.gen).view(-1).int()
    vals_ref = tg.acc[rows_ref.long()].clone()
    acc0, st0 = tg.acc.clone(), tg.stamp.clone()
    tg.rows_parts = parts
    tg.accumulate(groups)
    assert torch.equal(tg.acc, acc0) and torch.equal(tg.stamp, st0)
    rows, vals, counts, _ = export_stamped(tg, parts)
    assert tg.export is None
    n = int(counts[0])
    assert n == rows_ref.numel()
    assert torch.equal(rows[:n], rows_ref)
    assert torch.equal(vals[:n], vals_ref)
    per = n_rows // parts
    lo = torch.arange(parts, device="cuda") * per
    hi = torch.cat([lo[1:], torch.tensor([n_rows], device="cuda")])
    ref_counts = ((rows_ref[None, :] >= lo[:, None]) & (rows_ref[None, :] < hi[:, None])).sum(1)
    assert torch.equal(counts[1:].long(), ref_counts)


def test_fused_table_adam_equals_dense_adam():
    """mirec_adam_table (gradient formed in the kernel) == mirec_table_grad_dense
    + mirec_adam_dense, bitwise; the norms it leaves == the updated table's."""
    from furusato_recommend_amd.engine import AdamState
    from furusato_recommend_amd.graphsage import TableGrad
    from furusato_recommend_amd.rows import slice_norms
    n_rows, d, nu = 5000, 128, 2000
    groups = _tg_groups(n_rows, d, seed=3)
    torch.manual_seed(0)
    w0 = torch.randn(n_rows, d, device="cuda") * 0.1
    tg = TableGrad(n_rows, nu, d, "cuda")
    tg.coef.copy_(torch.tensor([1e-3, -2e-3]))
    wa, wb = w0.clone(), w0.clone()
    sa, sb = AdamState(wa, 1e-3), AdamState(wb, 1e-3)
    for it in range(3):
        tg.accumulate(groups)
        g = tg.materialize(wb)
        wb.grad = g
        sb.step()
        wb.grad = None
        norms = torch.empty(2, device="cuda")
        tg.adam(sa, norms)
        diff = (wa != wb)
        # same gradient arithmetic (explicit fma), same adam1
        assert not bool(diff.any()), (it, int(diff.sum()), float((wa - wb).abs().max()),
                                      float((sa.exp_avg - sb.exp_avg).abs().max()),
                                      float((sa.exp_avg_sq - sb.exp_avg_sq).abs().max()))
        ref = torch.stack(slice_norms(wa, nu))
        assert rel(norms, ref) < 1e-6


# ------------------------------------------------------------------ samplers
def test_capped_epoch_sampler_matches_sequential_rule():
    """mirec_bpr_sample_capped == ddp_lgcn.py's loop (ddp_lgcn.py:541-582)
    applied to the same candidate stream: users without positives skipped,
    a candidate kept iff its positive was kept < cap times before it (draw
    order), kept triples in draw order; negatives never positives."""
    from furusato_recommend_amd import SyntheticBipartite
    from furusato_recommend_amd.engine import sample_epoch_capped
    from furusato_recommend_amd.graph import Graph
    ds = SyntheticBipartite(3000, 400, 30_000, seed=4, kind="zipf", test_frac=0)
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    cap = 40
    u, p, n, cu, cp = sample_epoch_capped(g, 3 * 30_000, cap, seed=9, return_candidates=True)
    cu, cp = cu.cpu().numpy(), cp.cpu().numpy()
    cnt, kept = {}, []
    for t in range(len(cp)):
        if cp[t] < 0:
            continue
        if cnt.get(int(cp[t]), 0) >= cap:
            continue
        cnt[int(cp[t])] = cnt.get(int(cp[t]), 0) + 1
        kept.append(t)
    kept = np.array(kept)
    assert len(kept) == u.numel() and len(kept) < len(cp)  # the cap bit
    assert np.array_equal(u.cpu().numpy(), cu[kept]) and np.array_equal(p.cpu().numpy(), cp[kept])
    assert max(np.bincount(p.cpu().numpy())) <= cap
    rp, col = g.rowptr_host, g.col_host
    uu, pp, nn = u.cpu().numpy(), p.cpu().numpy(), n.cpu().numpy()
    for k in range(0, len(uu), 97):
        row = col[rp[uu[k]]:rp[uu[k] + 1]] - g.n_users
        assert pp[k] in row and nn[k] not in row


def test_host_sampler_equals_device_sampler(golden):
    """mirec_cpu_bpr_sample (C1's host path) draws the device sampler's
    triples bit for bit: the same counter streams, uniform and weighted
    positives, sharded."""
    import ctypes

    from furusato_recommend_amd import SyntheticBipartite, _lib
    from furusato_recommend_amd.graph import Graph
    ds = SyntheticBipartite(5000, 300, 200_000, seed=6, kind="zipf", test_frac=0)
    gd = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    gh = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cpu")
    rng = np.random.default_rng(1)
    probs = [rng.random(int(d)) + 0.01 for d in np.diff(gh.rowptr_host[: ds.n_users + 1])]
    for weighted in (False, True):
        for g in (gd, gh):
            g.set_positive_probs(probs if weighted else None)
        for shard, n_shards in ((0, 1), (2, 3)):
            dev = [torch.empty(20_000, dtype=torch.int32, device="cuda") for _ in range(3)]
            host = [torch.empty(20_000, dtype=torch.int32) for _ in range(3)]
            err = torch.zeros(1, dtype=torch.int32, device="cuda")
            herr = torch.zeros(1, dtype=torch.int32)
            _lib.check(_lib.lib.mirec_bpr_sample_ex(
                gd.csr_ptr(), _lib.ptr(gd.pos_cdf), gd.n_users, gd.m_items, 20_000,
                ctypes.c_uint64(9), ctypes.c_uint64(77), shard, n_shards, dev[0].data_ptr(),
                dev[1].data_ptr(), dev[2].data_ptr(), err.data_ptr(), _lib.stream_handle()), "d")
            _lib.check(_lib.lib.mirec_cpu_bpr_sample(
                gh.rowptr_host.ctypes.data, gh.col_host.ctypes.data, _lib.ptr(gh.col_sorted),
                _lib.ptr(gh.pos_cdf), gh.n_users, gh.m_items, 20_000, ctypes.c_uint64(9),
                ctypes.c_uint64(77), shard, n_shards, host[0].data_ptr(), host[1].data_ptr(),
                host[2].data_ptr(), herr.data_ptr(), 8), "h")
            assert int(err.item()) == 0 and int(herr.item()) == 0
            for a, b in zip(dev, host):
                assert torch.equal(a.cpu(), b), (weighted, shard)


def test_host_capped_sampler_equals_device_sampler():
    """mirec_cpu_bpr_sample_capped (a CPU model's epoch sampler) draws the
    device capped sampler's kept triples, count and candidates bit for bit:
    uniform and weighted positives, sharded."""
    from furusato_recommend_amd import SyntheticBipartite
    from furusato_recommend_amd.engine import sample_epoch_capped
    from furusato_recommend_amd.graph import Graph
    ds = SyntheticBipartite(5000, 300, 200_000, seed=6, kind="zipf", test_frac=0)
    gd = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    gh = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cpu")
    rng = np.random.default_rng(1)
    probs = [rng.random(int(d)) + 0.01 for d in np.diff(gh.rowptr_host[: ds.n_users + 1])]
    for weighted in (False, True):
        for g in (gd, gh):
            g.set_positive_probs(probs if weighted else None)
        for shard, n_shards in ((0, 1), (2, 3)):
            kw = dict(seed=5, offset=123, shard=shard, n_shards=n_shards, return_candidates=True)
            dev = sample_epoch_capped(gd, 150_000, 200, **kw)
            host = sample_epoch_capped(gh, 150_000, 200, n_threads=8, **kw)
            for a, b in zip(dev, host):
                assert torch.equal(a.cpu(), b), (weighted, shard)


def test_sampler_binary_search_equals_scan():
    """With the sorted user rows (csr.col_sorted) the negative rejection is a
    binary search; the triples equal the row-scan ones draw for draw."""
    import ctypes

    from furusato_recommend_amd import SyntheticBipartite, _lib
    from furusato_recommend_amd.graph import Graph
    ds = SyntheticBipartite(5000, 300, 200_000, seed=6, kind="zipf", test_frac=0)
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    assert g.col_sorted is not None
    outs = []
    for sorted_rows in (True, False):
        csr = _lib.CSR.from_buffer_copy(g.csr)
        if not sorted_rows:
            csr.col_sorted, csr.n_sorted = None, 0
        t = [torch.empty(8192, dtype=torch.int32, device="cuda") for _ in range(3)]
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        _lib.check(_lib.lib.mirec_bpr_sample(ctypes.byref(csr), g.n_users, g.m_items, 8192,
                                             ctypes.c_uint64(3), ctypes.c_uint64(0), 0, 1,
                                             t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                             err.data_ptr(), _lib.stream_handle()), "sample")
        outs.append(torch.stack(t).cpu())
        assert int(err.item()) == 0
    assert torch.equal(outs[0], outs[1])


def test_fanout_sampler_without_replacement():
    """mirec_sample_fanout_norep (PyG NeighborSampler semantics): rows with
    deg <= k kept whole in row order (+ -1), longer rows give k distinct
    entries with inclusion probability k / deg each; isolated nodes -1."""
    import ctypes

    from furusato_recommend_amd import SyntheticBipartite, _lib
    from furusato_recommend_amd.graph import Graph
    ds = SyntheticBipartite(400, 40, 6000, seed=12, kind="zipf", test_frac=0)
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    k, reps = 12, 400
    nodes = torch.arange(g.n_nodes, dtype=torch.int32, device="cuda").repeat(reps)
    ch = torch.empty(nodes.numel() * k, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib.mirec_sample_fanout_norep(g.csr_ptr(), nodes.data_ptr(), nodes.numel(), k,
                                                  ctypes.c_uint64(5), ctypes.c_uint64(0),
                                                  ch.data_ptr(), _lib.stream_handle()), "norep")
    ch = ch.view(reps, g.n_nodes, k).cpu().numpy()
    rp, col = g.rowptr_host, g.col_host
    checked_long = 0
    for v in range(0, g.n_nodes, 3):
        row = col[rp[v]:rp[v + 1]]
        d = len(row)
        if d <= k:
            want = np.concatenate([row, -np.ones(k - d, np.int32)])
            assert np.all(ch[:, v] == want)
            continue
        # each draw: a sub-multiset of the row (distinct positions)
        vals, cnt = np.unique(row, return_counts=True)
        for r in range(0, reps, 50):
            dv, dc = np.unique(ch[r, v], return_counts=True)
            assert np.all(np.isin(dv, vals))
            assert np.all(dc <= cnt[np.searchsorted(vals, dv)])
        # inclusion frequency of each distinct value ~ k * mult / d
        obs = np.array([(ch[:, v] == x).sum() for x in vals], np.float64)
        exp = reps * k * cnt / d
        assert np.abs(obs - exp).max() < 6 * np.sqrt(exp.max()) + 3
        checked_long += 1
    assert checked_long > 5


def _mix64(x: int) -> int:
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


@pytest.mark.parametrize("k", [3, 10, 25, 40])
def test_fanout_sampler_without_replacement_exact_draws(k):
    """Every row of mirec_sample_fanout_norep equals Floyd's algorithm on the
    documented counter stream (draw m of target t: mix64(mix64(seed) ^
    (offset + t k + m)), mapped to [0, j] by the high product), restated
    here in Python — the register form (k <= 32) and the generic form
    (k = 40) give the same rows."""
    import ctypes

    from furusato_recommend_amd import SyntheticBipartite, _lib
    from furusato_recommend_amd.graph import Graph
    ds = SyntheticBipartite(300, 60, 9000, seed=4, kind="zipf", test_frac=0)
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    rng = np.random.default_rng(k)
    nodes_h = rng.integers(-1, g.n_nodes + 1, 700).astype(np.int32)  # out-of-range ids too
    nodes = torch.from_numpy(nodes_h).cuda()
    seed, offset = 77, 12345
    ch = torch.empty(nodes.numel() * k, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib.mirec_sample_fanout_norep(g.csr_ptr(), nodes.data_ptr(), nodes.numel(), k,
                                                  ctypes.c_uint64(seed), ctypes.c_uint64(offset),
                                                  ch.data_ptr(), _lib.stream_handle()), "norep")
    got = ch.view(-1, k).cpu().numpy()
    rp, col = g.rowptr_host, g.col_host
    key = _mix64(seed)
    n_long = 0
    for t, v in enumerate(nodes_h):
        ok = 0 <= v < g.n_nodes
        beg = int(rp[v]) if ok else 0
        deg = int(rp[v + 1]) - beg if ok else 0
        if deg <= k:
            want = [int(col[beg + c]) if c < deg else -1 for c in range(k)]
        else:
            n_long += 1
            pos = []
            for m in range(k):
                j = deg - k + m
                r = (_mix64(key ^ (offset + t * k + m)) * (j + 1)) >> 64
                pos.append(j if r in pos else r)
            want = [int(col[beg + p]) for p in pos]
        assert got[t].tolist() == want, (t, v, deg)
    assert n_long > 20


def test_torch_ops_lgcn_propagate_matches_module_and_autograd():
    """torch.ops.mirec.lgcn_propagate == the engine's propagation and its
    registered backward == Âᵀ ȳ (a non-symmetric edge list: the transposed
    CSR), against a dense float64 reference."""
    from furusato_recommend_amd import ops
    from furusato_recommend_amd.graph import Graph
    rng = np.random.default_rng(0)
    n, nnz = 300, 2000
    ei = rng.integers(0, n, (2, nnz))
    g = Graph.from_edge_index(ei, n, "cuda")
    x = torch.randn(n, 64, device="cuda", dtype=torch.float32, requires_grad=True)
    y = torch.ops.mirec.lgcn_propagate(x, ops.handle(g))
    deg = np.bincount(ei[1], minlength=n).astype(np.float64)
    dinv = np.where(deg > 0, deg ** -0.5, 0.0)
    A = np.zeros((n, n))
    np.add.at(A, (ei[1], ei[0]), dinv[ei[1]] * dinv[ei[0]])
    ref = A @ x.detach().double().cpu().numpy()
    assert rel(y, torch.from_numpy(ref)) < 1e-5
    gy = torch.randn_like(y)
    (gx,) = torch.autograd.grad(y, x, gy)
    assert rel(gx, torch.from_numpy(A.T @ gy.double().cpu().numpy())) < 1e-5


def test_lgconv_backward_outlives_module_and_cache():
    """The autograd node keeps its graph alive: backward through a temporary
    LGConv(), and through one module called on two different edge_index
    tensors before either backward, both give Âᵀ ȳ (the graph
    registry is weak and the module caches one graph only)."""
    import gc

    from furusato_recommend_amd import LGConv
    rng = np.random.default_rng(1)
    n = 200

    def dense_a(ei):
        deg = np.bincount(ei[1], minlength=n).astype(np.float64)
        dinv = np.where(deg > 0, deg ** -0.5, 0.0)
        A = np.zeros((n, n))
        np.add.at(A, (ei[1], ei[0]), dinv[ei[1]] * dinv[ei[0]])
        return A

    e1, e2 = rng.integers(0, n, (2, 1500)), rng.integers(0, n, (2, 900))
    x = torch.randn(n, 32, device="cuda", requires_grad=True)
    y = LGConv()(x, torch.from_numpy(e1).cuda())     # temporary module
    gc.collect()
    gy = torch.randn_like(y)
    (gx,) = torch.autograd.grad(y, x, gy)
    assert rel(gx, torch.from_numpy(dense_a(e1).T @ gy.double().cpu().numpy())) < 1e-5
    conv = LGConv()
    y1 = conv(x, torch.from_numpy(e1).cuda())
    y2 = conv(x, torch.from_numpy(e2).cuda())        # drops the cached first graph
    gc.collect()
    g1, g2 = torch.randn_like(y1), torch.randn_like(y2)
    (gx,) = torch.autograd.grad((y1 * g1).sum() + (y2 * g2).sum(), x)
    want = dense_a(e1).T @ g1.double().cpu().numpy() + dense_a(e2).T @ g2.double().cpu().numpy()
    assert rel(gx, torch.from_numpy(want)) < 1e-5


def test_shard_pack_unpack_ragged_world3():
    """mirec_shard_pack / _unpack (the sharded exchange's staging, row i
    owned by rank i mod W): W = 3 ranks simulated in one process over N = 11
    rows in blocks of 2 slots (a ragged last block); every rank ends with
    every owner's rows, and x0s = dinv ⊙ row for the rows another rank
    owned (its own rows untouched)."""
    from furusato_recommend_amd import _lib
    from furusato_recommend_amd._lib import check, lib
    N, D, W = 11, 8, 3
    S = -(-N // W)
    owned = [torch.randn(N, D, device="cuda") for _ in range(W)]  # rank r's view
    dinv = torch.rand(N, device="cuda") + 0.5
    want = torch.stack([owned[i % W][i] for i in range(N)])
    st = _lib.stream_handle()
    for s0 in range(0, S, 2):
        ns = min(2, S - s0)
        stage = torch.full((W, ns, D), float("nan"), device="cuda")
        for r in range(W):
            check(lib.mirec_shard_pack(owned[r].data_ptr(), N, D, W, r, s0, ns,
                                       stage[r].data_ptr(), st), "pack")
        for r in range(W):
            x0s = torch.full((N, D), -7.0, device="cuda")
            check(lib.mirec_shard_unpack(stage.data_ptr(), N, D, W, r, s0, ns, dinv.data_ptr(),
                                         owned[r].data_ptr(), x0s.data_ptr(), st), "unpack")
            rows = [i for i in range(s0 * W, min((s0 + ns) * W, N))]
            for i in rows:
                assert torch.equal(owned[r][i], want[i])
                if i % W != r:
                    assert torch.equal(x0s[i], dinv[i] * want[i])
                else:
                    assert bool((x0s[i] == -7.0).all())
    for r in range(W):
        assert torch.equal(owned[r], want)


@pytest.mark.parametrize("n_rows,n,lo,hi", [(1_100_000, 1_757_184, 137_500, 275_000),
                                            (4097, 10_000, 0, 0), (1, 5, 0, 1), (70_001, 0, 0, 0),
                                            (5000, 3, 4990, 5000)])
def test_distinct_rows_matches_unique(n_rows, n, lo, hi):
    """mirec_distinct_rows (the fetch exchange's read set) == torch.unique of
    the valid ids outside the own block, ascending; ids of -1 and ragged
    block tails included."""
    from furusato_recommend_amd.dist import distinct_rows
    g = torch.Generator(device="cuda").manual_seed(n_rows + n)
    ids = torch.randint(-1, n_rows, (n,), device="cuda", generator=g, dtype=torch.int32)
    got = distinct_rows(ids, n_rows, lo, hi)
    u = torch.unique(ids[ids >= 0].long())
    ref = u[(u < lo) | (u >= hi)].int()
    assert torch.equal(got, ref)


@pytest.mark.parametrize("n_own,n_blocks,per,d", [(137_500, 16, 60_000, 128), (5000, 70, 300, 8),
                                                  (1, 3, 1, 4), (4096, 0, 0, 16),
                                                  (10_000, 5, 0, 8), (3001, 6, 2000, 12),
                                                  (500, 5, 400, 520)])
def test_owner_sum_equals_index_add_sequence(n_own, n_blocks, per, d):
    """owner_sum (mirec_owner_sum: position maps + one ordered pass per 64
    blocks) == the index_add_ launches it replaces, bitwise: blocks of
    distinct ids in and outside the own block, overlapping across blocks,
    empty blocks, more than 64 blocks."""
    from furusato_recommend_amd.dist import owner_sum
    g = torch.Generator(device="cuda").manual_seed(n_own + n_blocks + per + d)
    lo = 3 * n_own
    ref = torch.zeros(n_own, d, device="cuda")
    sources = []
    for q in range(n_blocks):
        k = 0 if q % 7 == 3 else min(per, n_own + 50)
        ids = torch.randperm(n_own + 100, device="cuda", generator=g)[:k].int() + lo - 50
        rows = torch.randn(k, d, device="cuda", generator=g)
        sources.append((ids, rows))
        inside = (ids >= lo) & (ids < lo + n_own)
        ref.index_add_(0, (ids[inside] - lo).long(), rows[inside])
    got, _ = owner_sum(sources, lo, n_own, d, torch.device("cuda"))
    assert torch.equal(got, ref)


@pytest.mark.parametrize("n_own,n_blocks,per,d,n_user", [(137_500, 9, 60_000, 128, 50_000),
                                                         (5000, 64, 300, 8, 0),
                                                         (3001, 6, 2000, 12, 3001),
                                                         (1000, 0, 0, 16, 400)])
def test_owner_adam_equals_owner_sum_then_adam_table(n_own, n_blocks, per, d, n_user):
    """mirec_owner_adam (the owner sum folded into the table Adam, S never
    stored) == mirec_owner_sum then mirec_adam_table with every row
    stamped: parameters, moments and the updated slices' norms bitwise —
    overlapping blocks, ids outside the own block, empty blocks, 64 blocks,
    the user / item split inside the block, no blocks at all."""
    import ctypes

    from furusato_recommend_amd import _lib
    from furusato_recommend_amd._lib import check, lib
    from furusato_recommend_amd.dist import owner_adam, owner_sum
    from furusato_recommend_amd.engine import AdamState
    g = torch.Generator(device="cuda").manual_seed(n_own + n_blocks + d)
    lo = 2 * n_own
    sources = []
    for q in range(n_blocks):
        k = 0 if q % 5 == 2 else min(per, n_own + 50)
        ids = torch.randperm(n_own + 100, device="cuda", generator=g)[:k].int() + lo - 50
        sources.append((ids, torch.randn(k, d, device="cuda", generator=g)))
    w0 = torch.randn(n_own, d, device="cuda", generator=g)
    coef = torch.tensor([1e-3, -2e-3], device="cuda")
    sa, sb = AdamState(w0.clone(), 1e-3), AdamState(w0.clone(), 1e-3)
    for st in (sa, sb):  # non-zero moments
        st.exp_avg.copy_(torch.randn(n_own, d, device="cuda", generator=g) * 1e-3)
        st.exp_avg_sq.copy_(torch.rand(n_own, d, device="cuda", generator=g) * 1e-6)
    sb.exp_avg.copy_(sa.exp_avg)
    sb.exp_avg_sq.copy_(sa.exp_avg_sq)
    na, nb = torch.empty(2, device="cuda"), torch.empty(2, device="cuda")
    owner_adam(sources, lo, n_own, d, sa.param.view(-1), sa.exp_avg.view(-1),
               sa.exp_avg_sq.view(-1), coef, n_user, sa.next_hparams(), na)
    s_own, _ = owner_sum(sources, lo, n_own, d, torch.device("cuda"))
    ones = torch.ones(n_own, dtype=torch.int32, device="cuda")
    sumsq = torch.empty(int(lib.mirec_adam_table_sumsq_floats(n_own, d)), device="cuda")
    hp = sb.next_hparams()
    check(lib.mirec_adam_table(sb.param.data_ptr(), sb.exp_avg.data_ptr(),
                               sb.exp_avg_sq.data_ptr(), coef.data_ptr(), n_user,
                               s_own.data_ptr(), ones.data_ptr(), 1, n_own, d, ctypes.byref(hp),
                               sumsq.data_ptr(), nb.data_ptr(), _lib.stream_handle()), "adam")
    assert torch.equal(sa.param, sb.param)
    assert torch.equal(sa.exp_avg, sb.exp_avg) and torch.equal(sa.exp_avg_sq, sb.exp_avg_sq)
    assert torch.equal(na, nb)


@pytest.mark.parametrize("n_rows,n,d", [(1_100_000, 300_000, 128), (4097, 4097, 8), (10, 0, 4),
                                        (3000, 1001, 12), (100, 37, 520)])
def test_scatter_rows_equals_index_copy(n_rows, n, d):
    from furusato_recommend_amd.dist import scatter_rows
    g = torch.Generator(device="cuda").manual_seed(n_rows + n + d)
    dst = torch.randn(n_rows, d, device="cuda", generator=g)
    ids = torch.randperm(n_rows, device="cuda", generator=g)[:n].int()
    src = torch.randn(n, d, device="cuda", generator=g)
    ref = dst.clone().index_copy_(0, ids.long(), src)
    scatter_rows(dst, ids, src)
    assert torch.equal(dst, ref)


@pytest.mark.parametrize("n_rows,n,d", [(1_100_000, 300_000, 128), (5000, 4097, 12), (300, 7, 4),
                                        (1000, 513, 256), (64, 33, 520), (10, 0, 8)])
def test_row_movers_equal_indexing(n_rows, n, d):
    """The row movers (common.h shape: 1 << lg lanes per row, lanes past
    d / 4 idle, four rows per lane): mirec_gather_rows == table[ids] with
    zero rows for ids < 0, and mirec_gather_rows_counted == src[rows[:count]]
    with the rows past the device-side count untouched — ragged last block,
    d / 4 not a power of two (3, 130), d / 4 = 64, an empty list."""
    from furusato_recommend_amd._lib import check, lib
    from furusato_recommend_amd.dist import gather_rows
    g = torch.Generator(device="cuda").manual_seed(n_rows + n + d)
    table = torch.randn(n_rows, d, device="cuda", generator=g)
    ids = torch.randint(-1, n_rows, (n,), device="cuda", generator=g, dtype=torch.int32)
    ref = table[ids.clamp(min=0).long()] * (ids >= 0).float()[:, None]
    assert torch.equal(gather_rows(table, ids), ref)
    rows = torch.randint(0, n_rows, (n,), device="cuda", generator=g, dtype=torch.int32)
    cnt = torch.tensor([n // 2 + (n & 1)], dtype=torch.int32, device="cuda")
    out = torch.full((n, d), 7.0, device="cuda")
    check(lib.mirec_gather_rows_counted(table.data_ptr(), rows.data_ptr(), cnt.data_ptr(), n, d,
                                        out.data_ptr(), torch.cuda.current_stream().cuda_stream),
          "gather_rows_counted")
    k = int(cnt)
    assert torch.equal(out[:k], table[rows[:k].long()])
    assert bool((out[k:] == 7.0).all())


@pytest.mark.parametrize("n_rows,n", [(1_100_000, 880_000), (4097, 10_000), (1, 5), (70_001, 0)])
def test_distinct_rows_unseen_excludes_earlier_sets(n_rows, n):
    """distinct_rows(..., have=map) over three id lists (the pipelined
    exchange's micro-batch read sets): each call == the unique ids outside
    the own block not returned by an earlier call, and the map afterwards
    marks exactly the union."""
    from furusato_recommend_amd.dist import distinct_rows
    g = torch.Generator(device="cuda").manual_seed(n_rows + n + 1)
    lo, hi = n_rows // 8, n_rows // 4
    have = torch.zeros(n_rows, dtype=torch.bool, device="cuda")
    seen = torch.zeros(n_rows, dtype=torch.bool, device="cuda")
    for _ in range(3):
        ids = torch.randint(-1, n_rows, (n,), device="cuda", generator=g, dtype=torch.int32)
        got = distinct_rows(ids, n_rows, lo, hi, have=have)
        u = torch.unique(ids[ids >= 0].long())
        u = u[((u < lo) | (u >= hi)) & ~seen[u]]
        seen[u] = True
        assert torch.equal(got.long(), u)
        assert torch.equal(have, seen)


@pytest.mark.parametrize("n_rows,n,parts,cap", [(1_100_000, 880_000, 8, 137_500),
                                                (4097, 10_000, 2, 2049), (8, 3, 8, 1),
                                                (70_001, 0, 1, 5), (5000, 5000, 3, 700),
                                                (1000, 900, 4, 300)])
def test_route_pack_and_routed_gather(n_rows, n, parts, cap):
    """The pipelined planner's capacity-bounded routing: route_pack writes
    per owner block q (contiguous n_rows / parts rows, the last to n_rows)
    its count in-band and its ids (up to cap: (5000, 3, 700) and (1000, 4,
    300) overflow some blocks — the count stays the true one, the ids past
    cap are dropped), with no host read of the device count; gather_rows_
    routed over those blocks == the table rows of the kept ids in block
    order, past the total nothing written."""
    from furusato_recommend_amd.dist import distinct_rows, gather_rows_routed, route_pack
    g = torch.Generator(device="cuda").manual_seed(n_rows + n + parts)
    ids = torch.randint(0, n_rows, (n,), device="cuda", generator=g, dtype=torch.int32)
    buf, cnt = distinct_rows(ids, n_rows, sync=False)
    u = torch.unique(ids.long()).cpu().numpy()
    stride = cap + 3  # (blocks need not be packed)
    blocks = torch.full((parts * stride,), -7, dtype=torch.int32, device="cuda")
    route_pack(buf, cnt, n_rows, parts, cap, blocks, stride)
    b = blocks.cpu().numpy()
    per = n_rows // parts
    owner = np.minimum(u // per, parts - 1)
    kept = []
    for q in range(parts):
        mine = u[owner == q]
        assert b[q * stride] == mine.size, q
        k = min(mine.size, cap)
        assert np.array_equal(b[q * stride + 1: q * stride + 1 + k], mine[:k]), q
        assert (b[q * stride + 1 + k: (q + 1) * stride] == -7).all()
        kept.append(mine[:k])
    kept = np.concatenate(kept)
    table = torch.randn(n_rows, 16, device="cuda", generator=g)
    out = torch.full((parts * cap, 16), 5.0, device="cuda")
    gather_rows_routed(table, blocks, parts, cap, stride, out)
    got = out.cpu()
    assert torch.equal(got[:kept.size], table.cpu()[torch.from_numpy(kept).long()])
    assert bool((got[kept.size:] == 5.0).all())


@pytest.mark.parametrize("n_rows,n,parts", [(1_100_000, 880_000, 8), (4097, 10_000, 2),
                                            (8, 3, 8), (70_001, 0, 1), (5000, 5000, 3)])
def test_export_stamped_matches_nonzero(n_rows, n, parts):
    """export_stamped (the pipelined exchange's device-side export: mirec_
    stamped_rows + the counted gather) == torch.nonzero of stamp == gen, the
    gathered rows of S and the per-owner bincount of route_ids — with stale
    stamps of earlier generations in the map, ragged block tails and an
    empty generation."""
    from types import SimpleNamespace

    from furusato_recommend_amd.dist import export_stamped
    d = 8
    g = torch.Generator(device="cuda").manual_seed(n_rows + n + parts)
    stamp = torch.randint(0, 3, (n_rows,), device="cuda", generator=g, dtype=torch.int32)
    ids = torch.randint(0, n_rows, (n,), device="cuda", generator=g, dtype=torch.int32)
    stamp[ids.long()] = 5
    acc = torch.randn(n_rows, d, device="cuda", generator=g)
    tg = SimpleNamespace(n_rows=n_rows, dim=d, acc=acc, stamp=stamp, gen=5, entries=n)
    rows, vals, counts, _ = export_stamped(tg, parts)
    torch.cuda.synchronize()
    ref = torch.nonzero(stamp == 5).view(-1)
    c = counts.tolist()
    assert c[0] == ref.numel()
    assert torch.equal(rows[: c[0]].long(), ref)
    assert torch.equal(vals[: c[0]], acc[ref])
    owner = torch.div(ref, n_rows // parts, rounding_mode="floor").clamp_(max=parts - 1)
    assert c[1:] == torch.bincount(owner, minlength=parts).tolist()


@pytest.mark.parametrize("n,k,no", [(56_321, 384, 128), (56_321, 128, 128), (56_321, 128, 384)])
def test_plain_gemms_bitwise_repeatable(n, k, no):
    """gemm_nt / gemm_nn / gemm_tn on the split-bf16 loop at a ragged row
    count: 16 launches each give bit-identical results (their A loads are
    exec-masked by row, the form under which the fused row-tail kernel once
    returned wrong rows), and every launch agrees with float64 at 1e-6."""
    from furusato_recommend_amd.linear import gemm_nn, gemm_nt, gemm_tn
    torch.manual_seed(n + k + no)
    a = torch.randn(n, k, device="cuda")
    w_nt = torch.randn(no, k, device="cuda") * k ** -0.5
    w_nn = torch.randn(k, no, device="cuda") * k ** -0.5
    b = torch.randn(n, no, device="cuda")
    refs = {"nt": a.double() @ w_nt.double().t(), "nn": a.double() @ w_nn.double(),
            "tn": a.double().t() @ b.double()}
    runs = {"nt": lambda: gemm_nt(a, w_nt), "nn": lambda: gemm_nn(a, w_nn),
            "tn": lambda: gemm_tn(a, b, False)[0]}
    for name, fn in runs.items():
        first = fn().clone()
        assert rel(first, refs[name]) < 1e-6, name
        for _ in range(15):
            assert torch.equal(fn(), first), name
