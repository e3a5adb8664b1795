"""rAdjGCN on the HIP engine (model/radj.py): the reference's
fixtures, every launch form of the scaled kernels against a float64
restatement (tests/radj_common.py), the transpose, r = 0.5 compatibility,
evaluation and the two-rank data-parallel step.

Tolerances (max|a−b| / max|b|): 1e-4 against the reference's fp32 fixtures
(the project's north-star bar), 1e-5 against the float64 restatement
(summation order plus one rounding per scale), bitwise where stated."""
import numpy as np
import pytest
import torch

from tests.radj_common import CONFIGS, RADJ, DS, Radj64, load, model_from, rel

pytestmark = pytest.mark.gpu
TOL = 1e-4
TOL64 = 1e-5


def count_prescales(m):
    """Wrap the engine's prescale launch with a call counter."""
    calls = []
    inner = m.engine.prescale

    def counted(x, out):
        calls.append(1)
        return inner(x, out)
    m.engine.prescale = counted
    return calls


# ------------------------------------------------------------- fixture parity
@pytest.mark.parametrize("name", RADJ)
def test_fixture_forward_loss_gradient(name):
    from furusato_recommend_amd.engine import propagate
    f = load(name)
    L = int(f["n_layers"])
    m = model_from(f)
    assert (m.graph.scale_src is not None) == (float(f["r"]) != 0.5)
    users, items = m.forward()
    out = torch.cat([users, items])
    r_out = rel(out, f["out"])
    # per-layer outputs through single propagate calls on the r-graph
    x = torch.from_numpy(f["emb0"]).cuda()
    r_layers = []
    for k in range(1, L + 1):
        y = torch.empty_like(x)
        propagate(m.graph, x, y)
        r_layers.append(rel(y, f["layers"][k]))
        x = y
    t = torch.from_numpy(f["triples"]).cuda()
    m.optim.zero_grad()
    loss, reg = m.bpr_loss(t[:, 0], t[:, 1], t[:, 2])
    (loss + float(f["decay"]) * reg).backward()
    torch.cuda.synchronize()
    r_grad = rel(m.all_embedding.weight.grad, f["grad"])
    r_loss = abs(float(loss.detach()) - float(f["loss"])) / abs(float(f["loss"]))
    r_reg = abs(float(reg.detach()) - float(f["reg"])) / abs(float(f["reg"]))
    print(f"{name}: out {r_out:.2e} layers {max(r_layers):.2e} grad {r_grad:.2e} "
          f"loss {r_loss:.2e} reg {r_reg:.2e}")
    assert r_out < TOL and max(r_layers) < TOL and r_grad < TOL
    assert r_loss < TOL and r_reg < TOL


@pytest.mark.parametrize("name", RADJ)
def test_fixture_two_steps(name):
    """stageOne twice vs emb_step1 / emb_step2 / step_losses.  The second
    step gathers the x0s = a ⊙ E written by the first step's fused Adam
    epilogue: no prescale launch runs before it."""
    f = load(name)
    m = model_from(f)
    calls = count_prescales(m)
    t = torch.from_numpy(f["triples"])
    res = []
    for k in range(2):
        loss = float(m.stageOne(t[:, 0], t[:, 1], t[:, 2]))
        torch.cuda.synchronize()
        assert len(calls) == 1, (k, len(calls))  # the first forward's only
        res.append((rel(m.all_embedding.weight, f[f"emb_step{k + 1}"]),
                    abs(loss - f["step_losses"][k]) / abs(f["step_losses"][k])))
    print(f"{name}: steps {res}")
    for r_emb, r_loss in res:
        assert r_emb < TOL and r_loss < TOL
    assert list(m.state_dict().keys()) == ["all_embedding.weight"]


# ------------------------------------------------------- launch forms, r = 0.3
FORMS = {
    "pruned": dict(),
    "unpruned": dict(prune=False),
    "split16": dict(csr_split=16),
    "narrow0": dict(narrow_max=0),
    "slot": dict(sparse_filter="slot"),
    "bytemap": dict(sparse_filter="bytemap"),
    "dense": dict(sparse_filter="dense"),
}


@pytest.fixture(scope="module")
def tiny():
    return load("radj_r030_d64_L3.npz")


def run_form(f, E0, d, L, form, steps=2):
    kw = dict(FORMS[form])
    attrs = {k: kw.pop(k) for k in ("narrow_max", "sparse_filter") if k in kw}
    g = dict(f, dim=d, n_layers=L, emb0=E0)
    m = model_from(g, r=0.3, **kw)
    for k, v in attrs.items():
        setattr(m.engine, k, v)
    if form == "split16":
        assert m.graph.n_long > 0 and m.graph.n_seg > 0  # segments + finalize
    t = torch.from_numpy(f["triples"])
    first = m.propagated().clone()
    for _ in range(steps):
        m.stageOne(t[:, 0], t[:, 1], t[:, 2])
    table = m.all_embedding.weight.detach().clone()
    out = m.propagated().clone()
    torch.cuda.synchronize()
    return first, table, out


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("d", [16, 64, 256])
def test_launch_forms(tiny, d, L):
    """Forward, two train steps (at L = 1 the SPARSE first backward layer is
    also the Adam layer; step 2 reads the epilogue's x0s) and the forward of
    the trained table, per launch form, vs float64."""
    f = tiny
    E0 = (0.1 * torch.randn(250, d, generator=torch.Generator().manual_seed(100 * d + L))).numpy()
    o = Radj64(f["train_user"], f["train_item"], f["n_users"], f["m_items"], 0.3)
    ref_first = o.forward(E0, L)
    ref_table, _ = o.train(E0, L, [f["triples"]] * 2, float(f["lr"]), float(f["decay"]))
    ref_out = o.forward(ref_table, L)
    got = {}
    for form in FORMS:
        got[form] = run_form(f, E0, d, L, form)
        rs = [rel(a, b) for a, b in zip(got[form], (ref_first, ref_table, ref_out))]
        print(f"d={d} L={L} {form}: first {rs[0]:.2e} table {rs[1]:.2e} out {rs[2]:.2e}")
        assert max(rs) < TOL64, (form, rs)
    for a, b in zip(got["pruned"], got["unpruned"]):
        assert rel(a, b) < TOL64


# ------------------------------------------------------------ sweeps, d = 64
D, LS = 64, 3
GROUP = (200, 7, 256)
WAVE = dict(wave_items=(200, 256), wave_users=(100, 64), max_grid=8)


@pytest.fixture(scope="module")
def dataset():
    from furusato_recommend_amd import SyntheticBipartite
    return SyntheticBipartite(3000, 700, 40000, seed=1, test_frac=0)


def sweep_engine(ds, r=0.3):
    from furusato_recommend_amd.engine import PropagationEngine
    from furusato_recommend_amd.graph import Graph
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0", r=r)
    eng = PropagationEngine(g, D, LS, 64)
    eng.sweep_form = "wave"
    eng.sweep_users = True
    eng.set_sweep_sizes(*GROUP, **WAVE)
    assert eng.sweep is not None and eng.sweep_wave is not None
    assert eng.sweep_wave_users is not None
    return g, eng


def sweep_run(ds, form, users, use_sweep, batches):
    from furusato_recommend_amd.engine import AdamState
    g, eng = sweep_engine(ds)
    eng.use_sweep, eng.sweep_form, eng.sweep_users = use_sweep, form, users
    torch.manual_seed(0)
    emb = (0.1 * torch.randn(g.n_nodes, D)).cuda()
    first = eng.forward(emb).clone()
    adam = AdamState(emb, lr=1e-3)
    losses = []
    for b in batches:
        t = torch.from_numpy(b).cuda().int()
        losses.append(float(eng.train_step(emb, adam, t[:, 0].contiguous(), t[:, 1].contiguous(),
                                           t[:, 2].contiguous(), 1e-4)))
    out = eng.forward(emb).clone()
    torch.cuda.synchronize()
    return first, emb, out, losses


@pytest.fixture(scope="module")
def swept(dataset):
    ds = dataset
    rng = np.random.default_rng(4)
    batches = []
    for _ in range(3):
        u = rng.integers(0, ds.n_users, 64)
        p = np.array([ds.trainItem[ds.trainUser == k][0] for k in u])
        batches.append(np.stack([u, p, rng.integers(0, ds.m_items, 64)], 1))
    runs = {"rows": sweep_run(ds, "group", False, False, batches),
            "group": sweep_run(ds, "group", False, True, batches),
            "wave": sweep_run(ds, "wave", False, True, batches),
            "both": sweep_run(ds, "wave", True, True, batches)}
    o = Radj64(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, 0.3)
    torch.manual_seed(0)
    E0 = (0.1 * torch.randn(ds.n_users + ds.m_items, D)).numpy()
    table, losses = o.train(E0, LS, batches, 1e-3, 1e-4)
    ref = (o.forward(E0, LS), table, o.forward(table, LS), losses)
    return runs, ref


@pytest.mark.parametrize("form", ["rows", "group", "wave", "both"])
def test_sweep_forms_against_float64(swept, form):
    runs, ref = swept
    rs = [rel(a, b) for a, b in zip(runs[form][:3], ref[:3])]
    print(f"{form}: first {rs[0]:.2e} table {rs[1]:.2e} out {rs[2]:.2e}")
    assert max(rs) < TOL64
    assert np.allclose(runs[form][3], ref[3], rtol=1e-5, atol=0)


def test_sweep_ran_and_wave_equals_group(swept, dataset):
    runs, _ = swept
    nu = dataset.n_users
    for k in range(3):
        assert torch.equal(runs["wave"][k][nu:], runs["group"][k][nu:])
    # the sweep did run: ascending-column order, not the row kernel's
    assert not torch.equal(runs["wave"][0][nu:], runs["rows"][0][nu:])
    assert not torch.equal(runs["both"][0][:nu], runs["wave"][0][:nu])


# ---------------------------------------------------------------- transpose
def test_transpose_identity(tiny):
    """⟨x, Â_r y⟩ = ⟨Â_rᵀ x, y⟩ through the two directions of _prop, and the
    direction-swapped r-graph is the (1 − r)-graph's forward.  An inner
    product's rounding error scales with Σ|terms|, so that is the
    denominator."""
    from furusato_recommend_amd._lib import IN_RAW
    f = tiny
    m3, m7 = model_from(f, r=0.3), model_from(f, r=0.7)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(250, 64, generator=gen).cuda()
    y = torch.randn(250, 64, generator=gen).cuda()
    Ay, Atx, A7x = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    m3.engine._prop(in_mode=IN_RAW, x_in=y, out=Ay, direction="fwd")
    m3.engine._prop(in_mode=IN_RAW, x_in=x, out=Atx, direction="bwd")
    m7.engine._prop(in_mode=IN_RAW, x_in=x, out=A7x, direction="fwd")
    torch.cuda.synchronize()
    lhs, rhs = (x.double() * Ay.double()).sum(), (Atx.double() * y.double()).sum()
    scale = (x.double() * Ay.double()).abs().sum()
    r_t = float((lhs - rhs).abs() / scale)
    r_swap = rel(Atx, A7x)
    o = Radj64(f["train_user"], f["train_item"], f["n_users"], f["m_items"], 0.3)
    r_ref = rel(Atx, o.conv(x.cpu().double().numpy(), transposed=True))
    print(f"transpose: identity {r_t:.2e} swap {r_swap:.2e} float64 {r_ref:.2e}")
    assert r_t < TOL64 and r_swap < TOL64 and r_ref < TOL64
    assert rel(Atx, Ay) > 1e-2  # not symmetric: the direction matters


# ------------------------------------------------------- r = 0.5 compatibility
def three_steps(m, f):
    t = torch.from_numpy(f["triples"])
    losses = [float(m.stageOne(t[:, 0], t[:, 1], t[:, 2])) for _ in range(3)]
    rating = m.getUsersRating(torch.arange(0, 200, 7).cuda()).clone()
    torch.cuda.synchronize()
    return m.all_embedding.weight.detach().clone(), rating, losses


def test_r_half_is_lightgcn_bitwise(tiny):
    from furusato_recommend_amd import LightGCN
    ra = model_from(tiny, r=0.5)
    assert ra.graph.scale_src is None and ra.graph.scale_dst is None
    a, b = three_steps(ra, tiny), three_steps(model_from(tiny, cls=LightGCN, r=None), tiny)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]


def test_lightgcn_ignores_r(tiny):
    from furusato_recommend_amd import LightGCN
    with_r = model_from(tiny, cls=LightGCN, r=0.3)
    assert with_r.graph.scale_src is None
    a, b = three_steps(with_r, tiny), three_steps(model_from(tiny, cls=LightGCN, r=None), tiny)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]


def test_determinism(tiny):
    a, b = three_steps(model_from(tiny), tiny), three_steps(model_from(tiny), tiny)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert not torch.equal(a[0], three_steps(model_from(tiny, r=0.5), tiny)[0])  # r is read


# ----------------------------------------------------------------- evaluation
def test_streamed_evaluation():
    """evaluate() with the streamed top-k on the r = 0.3 model vs the host
    path on the same embeddings restated in float64: every streamed top-20
    item is in the exact top-20 or within fp32 rounding of the 20th score."""
    from furusato_recommend_amd import SyntheticBipartite, rAdjGCN
    from furusato_recommend_amd.evaluate import evaluate
    ds = SyntheticBipartite(4000, 900, 50_000, seed=6, test_frac=0.3)
    m = rAdjGCN({"recdim": 32, "layer": 2, "lr": 1e-3, "decay": 1e-4, "device": "cuda:0",
                 "bpr_batch_size": 512, "r": 0.3}, ds)
    for _ in range(2):
        m.OneEpoch(*m.sample(2048, seed=1))
    res, top = evaluate(m, ds.testDict, (10, 20), batch=1000, return_topk=True, stream=True)
    res_h, top_h = evaluate(m, ds.testDict, (10, 20), batch=1000, return_topk=True, stream=False)
    o = Radj64(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, 0.3)
    out = o.forward(m.all_embedding.weight.detach().cpu().numpy(), 2)
    assert rel(m.propagated(), out) < TOL64
    users = np.array(sorted(ds.testDict.keys()), dtype=np.int64)
    s = out[users] @ out[ds.n_users:].T
    for j, u in enumerate(users):
        s[j, np.asarray(ds.allPos[u], dtype=np.int64)] = -np.inf
    kth = -np.sort(-s, axis=1)[:, 19]
    eps = 1e-5 * np.abs(s[np.isfinite(s)]).max()
    n = len(users)
    ties = 0
    for t in (top, top_h):
        picked = np.take_along_axis(s, t[:, :20].astype(np.int64), axis=1)
        assert np.all(picked >= kth[:, None] - eps)
        ties = max(ties, int((~(picked >= kth[:, None]).all(axis=1)).sum()))
    assert ties <= max(2, n // 1000), ties
    # the two paths differ by near-tie picks only
    assert int((np.sort(top[:, :20], 1) != np.sort(top_h[:, :20], 1)).any(1).sum()) <= 2 * ties
    for k in res:
        assert np.all(np.abs(res[k] - res_h[k]) <= (2 * ties + 0.5) / n + 1e-9), (k, res[k])


# ------------------------------------------------------------ data parallelism
def run_ranks(target, args, world=2, timeout=240):
    """``world`` processes on cuda:0, each under its own time limit."""
    import multiprocessing as mp
    import socket
    ctx = mp.get_context("spawn")
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
def test_data_parallel_two_ranks(mode):
    """Two ranks of dist.DataParallel over the r = 0.3 engine on one GPU:
    replicas bit-identical, and equal to the reference's stageOne on the
    union batch (sharded: the unpack pre-scales the other rank's rows by a)."""
    from tests.radj_common import dp_rank
    name = "radj_r030_d64_L3.npz"
    f = load(name)
    res = run_ranks(dp_rank, (name, mode))
    for k in range(2):
        assert np.array_equal(res[0][0][k], res[1][0][k])
        r = rel(res[0][0][k], f[f"emb_step{k + 1}"])
        print(f"dp {mode} step {k + 1}: {r:.2e}")
        assert r < TOL


# --------------------------------------------------------------------- errors
@pytest.mark.parametrize("r", [-0.1, 1.5, float("nan")])
def test_r_out_of_range(tiny, r):
    with pytest.raises(ValueError):
        model_from(tiny, r=r, emb=False)


def test_operators_refuse_r_graph(tiny):
    from furusato_recommend_amd import ops
    with pytest.raises(ValueError):
        ops.handle(model_from(tiny, emb=False).graph)
    assert ops.handle(model_from(tiny, r=0.5, emb=False).graph) > 0


def test_r_with_edge_weight_is_rejected(tiny):
    from furusato_recommend_amd import Graph
    from furusato_recommend_amd._lib import IN_RAW, MirecError, Prop, check, lib, stream_handle
    import ctypes
    w = np.ones(len(tiny["train_user"]), np.float32)
    with pytest.raises(ValueError):
        model_from(tiny, r=0.3, emb=False, edge_weight=w)
    model_from(tiny, r=0.5, emb=False, edge_weight=w)  # r = 0.5 stays allowed
    # the library refuses scales on a CSR with values (before any launch)
    g = Graph.from_interactions(tiny["train_user"], tiny["train_item"], 200, 50, "cuda:0",
                                weight=w)
    x, y = torch.zeros(250, 16, device="cuda"), torch.zeros(250, 16, device="cuda")
    p = Prop()
    p.dim, p.in_mode, p.x_in, p.divisor, p.out = 16, IN_RAW, x.data_ptr(), 1.0, y.data_ptr()
    p.narrow_max = 64
    p.scale_src = g.dinv.data_ptr()
    with pytest.raises(MirecError):
        check(lib.mirec_propagate(g.csr_ptr(), ctypes.byref(p), stream_handle()), "propagate")


_ = (CONFIGS, DS)
