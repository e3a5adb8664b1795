"""Edge-weighted propagation on the GPU: LGConv(edge_weight) forward and both
gradients, the weighted engine step (frontier pruning, long-row segments,
fused Adam) and LightGCN with config["edge_weight"], each against a float64
reference written here (dense Â, torch autograd, torch.optim.Adam).

Tolerances are the project's own: 1e-4 relative error in the max norm
against float64 (tests/test_gpu_parity.py), 1e-5 where only the summation
order differs (tests/test_prop_sweep.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4
ORDER_TOL = 1e-5
WIDTHS = [4, 16, 64, 256, 20, 300]   # 20: padded to 32, 300: 256 + 44 (padded to 64)


def rel(a, b):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


# ------------------------------------------------------------ operator graph
N_OP = 60


def _operator_edges():
    """60 nodes, directed: rows of in-degree 0 (node 0, a source only), 1, 2,
    64, 65 and 130 (nodes 1..5; 65 and 130 are 2 and 3 chunks of 64 entries),
    small random rows, a self-loop (7 -> 7), a duplicated edge (8 -> 9, twice
    more; the long rows hold many more duplicates) and an isolated node (59)."""
    rng = np.random.default_rng(11)
    deg = {1: 1, 2: 2, 3: 64, 4: 65, 5: 130}
    for v in range(6, 59):
        deg[v] = int(rng.integers(0, 7))
    dst = np.concatenate([np.full(d, v) for v, d in deg.items()])
    src = rng.integers(0, 59, dst.shape[0])
    src = np.concatenate([src, [7, 8, 8, 8]])
    dst = np.concatenate([dst, [7, 9, 9, 9]])
    order = rng.permutation(src.shape[0])       # COO order unrelated to CSR order
    return np.stack([src[order], dst[order]]).astype(np.int64)


def _dense(ei, w, n, normalize):
    """float64 Â of PyG's LGConv with edge weights (gcn_norm, no self loops)."""
    a = np.zeros((n, n))
    np.add.at(a, (ei[1], ei[0]), np.asarray(w, np.float64))
    if normalize:
        deg = a.sum(1)
        dinv = np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)
        a = dinv[:, None] * a * dinv[None, :]
    return a


@pytest.fixture(scope="module")
def op_graph():
    ei = _operator_edges()
    rng = np.random.default_rng(12)
    w = rng.uniform(0.25, 4.0, ei.shape[1]).astype(np.float32)
    deg = np.bincount(ei[1], minlength=N_OP)
    assert {0, 1, 2, 64, 65, 130} <= set(deg.tolist()) and deg[59] == 0 and 59 not in ei[0]
    return ei, w


def _xy(d, n=N_OP, seed=0):
    g = torch.Generator().manual_seed(seed + d)
    x = torch.randn(n, d, generator=g)
    ybar = torch.randn(n, d, generator=g)
    return x, ybar


def _run(conv, x, ei, w, ybar, w_grad=False):
    xd = x.cuda().requires_grad_(True)
    wd = None
    if w is not None:
        wd = torch.as_tensor(w).cuda().requires_grad_(w_grad)
    y = conv(xd, torch.from_numpy(ei).cuda(), wd)
    y.backward(ybar.cuda())
    torch.cuda.synchronize()
    return y.detach(), xd.grad, (wd.grad if w_grad else None)


@pytest.mark.parametrize("split", [None, 32])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("d", WIDTHS)
def test_forward_and_x_grad_match_float64(op_graph, d, normalize, split):
    from furusato_recommend_amd import LGConv
    ei, w = op_graph
    conv = LGConv(normalize=normalize, split=split)
    x, ybar = _xy(d)
    y, gx, _ = _run(conv, x, ei, w, ybar)
    if split is not None:
        assert conv._graph.n_long == 3          # rows 3, 4, 5 run as segments + finalize
    a = _dense(ei, w, N_OP, normalize)
    e_y, e_g = rel(y, a @ x.double().numpy()), rel(gx, a.T @ ybar.double().numpy())
    print(f"d={d} normalize={normalize} split={split}: y {e_y:.2e} x.grad {e_g:.2e}")
    assert e_y < TOL and e_g < TOL
    assert torch.all(y[59] == 0) and torch.all(y[0] == 0)    # isolated / no in-edges


@pytest.mark.parametrize("normalize", [True, False])
def test_asymmetric_weights_on_symmetric_structure(normalize):
    from furusato_recommend_amd import LGConv
    rng = np.random.default_rng(5)
    half = rng.integers(0, N_OP, (2, 200))
    ei = np.concatenate([half, half[::-1]], 1).astype(np.int64)   # every edge both ways
    w = rng.uniform(0.25, 4.0, ei.shape[1]).astype(np.float32)    # w_ij != w_ji
    conv = LGConv(normalize=normalize)
    x, ybar = _xy(64, seed=3)
    y, gx, _ = _run(conv, x, ei, w, ybar)
    assert not conv._graph.symmetric
    a = _dense(ei, w, N_OP, normalize)
    assert np.abs(a - a.T).max() > 0.1
    assert rel(y, a @ x.double().numpy()) < TOL
    assert rel(gx, a.T @ ybar.double().numpy()) < TOL


@pytest.mark.parametrize("split", [None, 32])
def test_mixed_sign_weights_without_normalisation(op_graph, split):
    from furusato_recommend_amd import LGConv
    ei, w = op_graph
    sign = np.where(np.random.default_rng(6).random(w.shape[0]) < 0.5, -1.0, 1.0)
    w = (w * sign).astype(np.float32)
    x, ybar = _xy(64, seed=4)
    y, gx, _ = _run(LGConv(normalize=False, split=split), x, ei, w, ybar)
    a = _dense(ei, w, N_OP, False)
    assert rel(y, a @ x.double().numpy()) < TOL
    assert rel(gx, a.T @ ybar.double().numpy()) < TOL


@pytest.mark.parametrize("split", [None, 32])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("d", [16, 64, 20])
def test_all_ones_is_bitwise_the_unweighted_path(op_graph, d, normalize, split):
    """fma(1, v, acc) rounds as acc + v does: any difference means the order
    of the terms or the compaction changed."""
    from furusato_recommend_amd import LGConv
    ei, _ = op_graph
    x, ybar = _xy(d, seed=1)
    y0, g0, _ = _run(LGConv(normalize=normalize, split=split), x, ei, None, ybar)
    y1, g1, _ = _run(LGConv(normalize=normalize, split=split), x, ei,
                     np.ones(ei.shape[1], np.float32), ybar)
    assert torch.equal(y0, y1)
    assert torch.equal(g0, g1)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("d", [16, 64])
def test_integer_weights_equal_duplicated_edges(op_graph, d, normalize):
    from furusato_recommend_amd import LGConv
    ei, _ = op_graph
    k = np.random.default_rng(8).integers(1, 4, ei.shape[1])
    x, ybar = _xy(d, seed=2)
    yw, gw, _ = _run(LGConv(normalize=normalize), x, ei, k.astype(np.float32), ybar)
    yd, gd, _ = _run(LGConv(normalize=normalize), x, np.repeat(ei, k, axis=1), None, ybar)
    assert rel(yw, yd) < ORDER_TOL and rel(gw, gd) < ORDER_TOL


def _edge_dots(ei, x, ybar):
    xs, yb = x.double().numpy(), ybar.double().numpy()
    return np.einsum("ec,ec->e", yb[ei[1]], xs[ei[0]])


@pytest.mark.parametrize("split", [None, 32])
@pytest.mark.parametrize("d", WIDTHS)
def test_weight_grad_matches_per_edge_dots(op_graph, d, split):
    from furusato_recommend_amd import LGConv
    ei, w = op_graph
    x, ybar = _xy(d, seed=5)
    y, gx, gw = _run(LGConv(normalize=False, split=split), x, ei, w, ybar, w_grad=True)
    assert gw.shape == (ei.shape[1],)
    e_w = rel(gw, _edge_dots(ei, x, ybar))       # duplicates: each its own entry
    print(f"d={d} split={split}: w.grad {e_w:.2e}")
    assert e_w < TOL
    a = _dense(ei, w, N_OP, False)
    assert rel(y, a @ x.double().numpy()) < TOL and rel(gx, a.T @ ybar.double().numpy()) < TOL


def test_weight_grad_hub_row_between_empty_rows():
    """One row of 5 000 entries with empty rows on both sides: the per-entry
    dot kernel's chunks of entries start and end inside the hub and cross
    runs of empty rows."""
    from furusato_recommend_amd import LGConv
    rng = np.random.default_rng(9)
    n, hub = 300, 150
    dst = np.concatenate([rng.integers(0, 100, 333), np.full(5000, hub),
                          rng.integers(201, n, 333)])
    src = rng.integers(0, n, dst.shape[0])
    order = rng.permutation(dst.shape[0])
    ei = np.stack([src[order], dst[order]]).astype(np.int64)
    deg = np.bincount(ei[1], minlength=n)
    assert deg[hub] == 5000 and deg[100:hub].sum() == 0 and deg[hub + 1:201].sum() == 0
    w = rng.uniform(0.25, 4.0, ei.shape[1]).astype(np.float32)
    x, ybar = _xy(16, n=n, seed=6)
    y, gx, gw = _run(LGConv(normalize=False), x, ei, w, ybar, w_grad=True)
    assert rel(gw, _edge_dots(ei, x, ybar)) < TOL
    a = _dense(ei, w, n, False)
    assert rel(y, a @ x.double().numpy()) < TOL and rel(gx, a.T @ ybar.double().numpy()) < TOL


def test_each_backward_uses_the_weights_of_its_forward(op_graph):
    from furusato_recommend_amd import LGConv
    ei, w = op_graph
    rng = np.random.default_rng(10)
    w2 = rng.uniform(0.25, 4.0, w.shape[0]).astype(np.float32)
    conv = LGConv(normalize=False)
    eid = torch.from_numpy(ei).cuda()
    x, ybar = _xy(64, seed=7)
    xa, xb = x.cuda().requires_grad_(True), x.cuda().requires_grad_(True)
    wa = torch.from_numpy(w).cuda().requires_grad_(True)
    wb = torch.from_numpy(w2).cuda().requires_grad_(True)
    ya = conv(xa, eid, wa)
    yb = conv(xb, eid, wb)                       # the graph now holds w2
    g = conv._graph
    ya.backward(ybar.cuda())                     # ... and must put w back for this
    yb.backward(ybar.cuda())
    assert conv._graph is g                      # refreshed, not rebuilt
    aa, ab = _dense(ei, w, N_OP, False), _dense(ei, w2, N_OP, False)
    xs, ys = x.double().numpy(), ybar.double().numpy()
    assert rel(ya, aa @ xs) < TOL and rel(yb, ab @ xs) < TOL
    assert rel(xa.grad, aa.T @ ys) < TOL and rel(xb.grad, ab.T @ ys) < TOL
    assert rel(xa.grad, ab.T @ ys) > 1e-2        # the two really differ
    dots = _edge_dots(ei, x, ybar)
    assert rel(wa.grad, dots) < TOL and rel(wb.grad, dots) < TOL
    # an in-place update of the weights is seen by the next call
    with torch.no_grad():
        wa.mul_(2.0)
    y2 = conv(x.cuda(), eid, wa)
    assert rel(y2, 2.0 * (aa @ xs)) < TOL


def test_errors(op_graph):
    from furusato_recommend_amd import LGConv, ops
    from furusato_recommend_amd.graph import Graph
    ei, w = op_graph
    eid = torch.from_numpy(ei).cuda()
    x = torch.randn(N_OP, 16, device="cuda")
    wd = torch.from_numpy(w).cuda()
    with pytest.raises(NotImplementedError, match="normalize=True"):
        LGConv(normalize=True)(x, eid, wd.clone().requires_grad_(True))
    # the operator itself refuses too (a graph handed to it directly)
    g = Graph.from_edge_index(ei, N_OP, "cuda:0", edge_weight=w)
    with pytest.raises(NotImplementedError, match="normalize=True"):
        torch.ops.mirec.lgcn_propagate_w(x, wd.clone().requires_grad_(True), ops.handle(g))
    with pytest.raises(ValueError):
        LGConv()(x, eid, wd[:-1])
    with pytest.raises(ValueError):
        LGConv()(x, eid, -wd)                                   # negative, normalize=True
    bad = wd.clone()
    bad[3] = float("nan")
    with pytest.raises(ValueError):
        LGConv(normalize=False)(x, eid, bad)
    with pytest.raises(ValueError):
        LGConv()(x, eid, torch.ones(ei.shape[1], dtype=torch.int64, device="cuda"))
    plain = Graph.from_edge_index(ei, N_OP, "cuda:0")
    with pytest.raises(ValueError):
        torch.ops.mirec.lgcn_propagate_w(x, wd, ops.handle(plain))


# -------------------------------------------------------------- engine graph
NU, MI, NE, L, B = 300, 80, 3000, 3, 64
LR, DECAY = 1e-3, 1e-4


@pytest.fixture(scope="module")
def eng_data():
    rng = np.random.default_rng(21)
    u = rng.integers(0, NU, NE)
    i = np.minimum((rng.random(NE) ** 2 * MI).astype(np.int64), MI - 1)   # skewed items
    w = rng.uniform(0.25, 4.0, NE).astype(np.float32)
    batches = []
    for _ in range(3):
        e = rng.integers(0, NE, B)
        batches.append((u[e].astype(np.int32), i[e].astype(np.int32),
                        rng.integers(0, MI, B).astype(np.int32)))
    ei = np.stack([np.concatenate([u, NU + i]), np.concatenate([NU + i, u])])
    a = torch.from_numpy(_dense(ei, np.concatenate([w, w]), NU + MI, True))
    return u, i, w, batches, a


def _layer_mean(a, e):
    xs, x = [e], e
    for _ in range(L):
        x = a @ x
        xs.append(x)
    return torch.stack(xs).mean(0)


_ref_cache = {}


def _reference(eng_data, d):
    """Three Adam steps in float64 (computed once per width, shared)."""
    if d in _ref_cache:
        return _ref_cache[d]
    u, i, w, batches, a = eng_data
    e0 = torch.randn(NU + MI, d, generator=torch.Generator().manual_seed(d)) * 0.1
    e = e0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([e], lr=LR)
    losses = []
    for bu, bp, bn in batches:
        bu, bp, bn = (torch.from_numpy(t).long() for t in (bu, bp, bn))
        out = _layer_mean(a, e)
        ue, pe, ne = out[bu], out[NU + bp], out[NU + bn]
        reg = 0.5 * (e[bu].pow(2).sum() + e[NU + bp].pow(2).sum() + e[NU + bn].pow(2).sum()) / B
        loss = torch.nn.functional.softplus((ue * ne).sum(1) - (ue * pe).sum(1)).mean() \
            + DECAY * reg
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    st = opt.state[e]
    _ref_cache[d] = (e0, losses, e.detach(), st["exp_avg"], st["exp_avg_sq"])
    return _ref_cache[d]


def _engine_run(eng_data, d, prune, split, steps=3):
    from furusato_recommend_amd.engine import AdamState, PropagationEngine
    from furusato_recommend_amd.graph import DEFAULT_SPLIT, Graph
    u, i, w, batches, _ = eng_data
    g = Graph.from_interactions(u, i, NU, MI, "cuda:0", weight=w,
                                split=DEFAULT_SPLIT if split is None else split)
    if split is not None:
        assert g.n_seg > 0
    eng = PropagationEngine(g, d, L, B, prune=prune)
    eng.narrow_max = 4            # wide lists and the workgroup row path run
    assert eng.sweep is None
    e = _reference(eng_data, d)[0].cuda().clone()
    adam = AdamState(e, LR)
    losses = []
    for bu, bp, bn in batches[:steps]:
        t = [torch.from_numpy(x).cuda() for x in (bu, bp, bn)]
        losses.append(float(eng.train_step(e, adam, *t, DECAY)))
    torch.cuda.synchronize()
    return e, adam.exp_avg, adam.exp_avg_sq, losses


@pytest.mark.parametrize("split", [None, 16])
@pytest.mark.parametrize("d", [16, 64])
def test_engine_steps_match_float64_reference(eng_data, d, split):
    _, ref_losses, ref_e, ref_m, ref_v = _reference(eng_data, d)
    runs = {}
    for prune in (True, False):
        e, m, v, losses = runs[prune] = _engine_run(eng_data, d, prune, split)
        errs = (rel(e, ref_e), rel(m, ref_m), rel(v, ref_v),
                float(np.max(np.abs(np.array(losses) / np.array(ref_losses) - 1))))
        print(f"d={d} split={split} prune={prune}: table {errs[0]:.2e} m {errs[1]:.2e} "
              f"v {errs[2]:.2e} loss {errs[3]:.2e}")
        assert max(errs) < TOL
    p, f = runs[True], runs[False]
    assert rel(p[0], f[0]) < ORDER_TOL and rel(p[1], f[1]) < ORDER_TOL
    assert rel(p[2], f[2]) < ORDER_TOL
    assert np.allclose(p[3], f[3], rtol=ORDER_TOL)


@pytest.mark.parametrize("split", [None, 16])
def test_engine_step_is_deterministic(eng_data, split):
    r1 = _engine_run(eng_data, 64, True, split, steps=2)
    r2 = _engine_run(eng_data, 64, True, split, steps=2)
    assert all(torch.equal(x, y) for x, y in zip(r1[:3], r2[:3])) and r1[3] == r2[3]


class _DS:
    def __init__(self, u, i):
        self.trainUser, self.trainItem = np.asarray(u, np.int64), np.asarray(i, np.int64)
        self.n_users, self.m_items = NU, MI


def _model(eng_data, d, **cfg):
    from furusato_recommend_amd import LightGCN
    u, i, w, _, _ = eng_data
    config = {"recdim": d, "layer": L, "lr": LR, "decay": DECAY, "device": "cuda:0",
              "bpr_batch_size": B, "edge_weight": w}
    config.update(cfg)
    m = LightGCN(config, _DS(u, i))
    with torch.no_grad():
        m.all_embedding.weight.copy_(_reference(eng_data, d)[0])
    return m


def test_lightgcn_stage_one_is_the_engine_step(eng_data):
    from furusato_recommend_amd.engine import AdamState, PropagationEngine
    from furusato_recommend_amd.graph import Graph
    u, i, w, batches, _ = eng_data
    m = _model(eng_data, 64)
    assert m.graph.val is not None and m.engine.sweep is None
    g = Graph.from_interactions(u, i, NU, MI, "cuda:0", weight=w)
    eng = PropagationEngine(g, 64, L, B)
    e = _reference(eng_data, 64)[0].cuda().clone()
    adam = AdamState(e, LR)
    for bu, bp, bn in batches:
        t = [torch.from_numpy(x) for x in (bu, bp, bn)]
        l_model = m.stageOne(*t)
        l_eng = eng.train_step(e, adam, *(x.cuda() for x in t), DECAY)
        assert torch.equal(l_model, l_eng)
    assert torch.equal(m.all_embedding.weight.detach(), e)
    ref_e = _reference(eng_data, 64)[2]
    assert rel(e, ref_e) < TOL
    with pytest.raises(ValueError):
        _model(eng_data, 64, edge_weight=w[:-1])


def test_lightgcn_users_rating_matches_float64(eng_data):
    a = eng_data[4]
    m = _model(eng_data, 64)
    users = torch.arange(0, NU, 7, device="cuda")
    r = m.getUsersRating(users)
    out = _layer_mean(a, _reference(eng_data, 64)[0].double())
    ref = out[users.cpu()] @ out[NU:].T
    assert rel(r, ref) < TOL
    # and the differentiable forward
    au, ai = m.forward()
    assert rel(torch.cat([au, ai]), out) < TOL
