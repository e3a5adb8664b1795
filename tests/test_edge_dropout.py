"""Edge dropout on the GPU: single dropped launches (operator and engine),
the operator's autograd, engine training steps (frontier pruning, long-row
segments, fused Adam) and LightGCN with config["dropout"] / ["keep_prob"].

The float64 reference lives here: a dense matrix built from
mirec_edge_keep_mask's bytes over the graph's host CSR, divided by keep_prob,
with dinv of the UNDROPPED degrees (the reference drops entries of the
normalised matrix, model/MF.py:158-176); a training step is restated with
torch autograd and torch.optim.Adam in float64 on that matrix.

Tolerance: the project's 1e-4 relative error in the max norm against float64
(tests/test_gpu_parity.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4
NU, MI = 300, 40
N = NU + MI
SPLITS = [None, 32]
BASE_SEED = 2020


def rel(a, b):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def _interactions():
    """300 users, 40 items, about 3 000 interactions: item 0 is a hub (every
    user once, some twice: degree >= 300, five 64-entry chunks, beyond
    narrow_max), 200 users have degree <= 8, 100 users 13-30, item 39 is
    isolated, 80 interactions appear twice."""
    rng = np.random.default_rng(21)
    us, its = [np.arange(NU)], [np.zeros(NU, np.int64)]
    for u in range(NU):
        k = int(rng.integers(0, 7)) if u < 200 else int(rng.integers(12, 30))
        us.append(np.full(k, u))
        its.append(rng.integers(1, MI - 1, k))
    u, i = np.concatenate(us), np.concatenate(its)
    dup = rng.choice(len(u), 80, replace=False)
    u, i = np.concatenate([u, u[dup]]), np.concatenate([i, i[dup]])
    order = rng.permutation(len(u))
    return u[order].astype(np.int64), i[order].astype(np.int64)


class DS:
    def __init__(self):
        self.trainUser, self.trainItem = _interactions()
        self.n_users, self.m_items = NU, MI
        self.trainDataSize = len(self.trainUser)
        self.testDict = {}


class Ref:
    """The float64 side, shared by every test and never modified."""

    def __init__(self):
        from furusato_recommend_amd.graph import Graph
        self.ds = DS()
        g = Graph.from_interactions(self.ds.trainUser, self.ds.trainItem, NU, MI, "cpu")
        self.rowptr, self.col = g.rowptr_host.copy(), g.col_host.copy()
        self.deg = np.diff(self.rowptr).astype(np.float64)
        self.dinv = np.where(self.deg > 0, 1.0 / np.sqrt(np.maximum(self.deg, 1.0)), 0.0)
        self.rows = np.repeat(np.arange(N), np.diff(self.rowptr))
        self._dense = {}
        rng = np.random.default_rng(22)
        self.triples = [np.stack([rng.integers(0, NU, 64), rng.integers(0, MI, 64),
                                  rng.integers(0, MI, 64)], 1) for _ in range(2)]

    def keep(self, seed, p, transposed=False):
        from furusato_recommend_amd._lib import lib
        k = np.empty(len(self.col), np.uint8)
        assert lib.mirec_edge_keep_mask(self.rowptr.ctypes.data, self.col.ctypes.data, N, seed, p,
                                        int(transposed), k.ctypes.data) == 0
        return k

    def dense(self, seed=None, p=1.0):
        """Â (seed None) or Â_drop: entry (j -> i) counted when its byte is set,
        divided by keep_prob, dinv of the full graph on both sides."""
        key = (seed, p)
        if key not in self._dense:
            k = np.ones(len(self.col)) if seed is None else self.keep(seed, p).astype(np.float64)
            a = np.zeros((N, N))
            np.add.at(a, (self.rows, self.col), k / (1.0 if seed is None else float(np.float32(p))))
            self._dense[key] = self.dinv[:, None] * a * self.dinv[None, :]
        return self._dense[key]

    def emb(self, d, seed=0):
        return (0.1 * torch.randn(N, d, generator=torch.Generator().manual_seed(100 + d + seed)))

    def steps(self, E0, L, mats, lr, decay):
        """torch autograd + torch.optim.Adam in float64: step t on matrix
        mats[t] with triples[t]; returns (tables, losses)."""
        E = E0.double().clone().requires_grad_(True)
        opt = torch.optim.Adam([E], lr=lr)
        tabs, losses = [], []
        for M, t in zip(mats, self.triples):
            opt.zero_grad()
            loss = self.loss(E, L, torch.from_numpy(M), t, decay)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            tabs.append(E.detach().clone())
        return tabs, losses

    @staticmethod
    def loss(E, L, M, t, decay):
        x, acc = E, E
        for _ in range(L):
            x = M @ x
            acc = acc + x
        out = acc / (L + 1)
        u, p, n = (torch.from_numpy(t[:, k]) for k in range(3))
        p, n = p + NU, n + NU
        z = (out[u] * out[n]).sum(1) - (out[u] * out[p]).sum(1)
        reg = 0.5 * (E[u].pow(2).sum() + E[p].pow(2).sum() + E[n].pow(2).sum()) / len(u)
        return torch.nn.functional.softplus(z).mean() + decay * reg


@pytest.fixture(scope="module")
def ref():
    r = Ref()
    deg = r.deg
    assert deg[NU] >= 300 and deg[N - 1] == 0              # the hub, the isolated item
    assert (deg[:NU] <= 8).sum() >= 150 and 2800 <= len(r.ds.trainUser) <= 3400
    cell = r.rows * N + r.col
    assert len(np.unique(cell)) < len(cell)                # multi-edges
    return r


@pytest.fixture(scope="module", params=SPLITS, ids=lambda s: f"split{s}")
def graph(request, ref):
    from furusato_recommend_amd.graph import DEFAULT_SPLIT, Graph
    split = request.param
    g = Graph.from_interactions(ref.ds.trainUser, ref.ds.trainItem, NU, MI, "cuda:0",
                                split=DEFAULT_SPLIT if split is None else split)
    assert np.array_equal(g.col_host, ref.col)
    if split is not None:
        assert g.n_long >= 1 and g.n_seg >= 10             # the hub runs as segments + finalize
    else:
        assert g.n_seg == 0
    return g


def _engine(graph, d, L=1, prune=True):
    from furusato_recommend_amd.engine import PropagationEngine
    return PropagationEngine(graph, d, L, 64, prune=prune)


def _tri(t):
    return tuple(torch.from_numpy(t[:, k]).cuda().int().contiguous() for k in range(3))


# ------------------------------------------------------------ single launches
@pytest.mark.parametrize("p", [0.6, 0.25])
@pytest.mark.parametrize("d", [4, 16, 64, 256])
def test_single_launch_matches_float64(ref, graph, d, p):
    """RAW input through the operator and through engine._prop, PRESCALED
    input through engine._prop; the plain and the transposed mask."""
    from furusato_recommend_amd import ops
    from furusato_recommend_amd._lib import IN_PRESCALED, IN_RAW
    seed = 77 + d
    M = ref.dense(seed, p)
    x = torch.randn(N, d, generator=torch.Generator().manual_seed(d))
    xd = x.cuda()
    xs = (graph.dinv[:, None] * xd).contiguous()
    want = {False: M @ x.double().numpy(), True: M.T @ x.double().numpy()}
    # the two masks differ by far more than the tolerance: a kernel that
    # ignored the drop's `transposed` (or the mask) could not pass
    assert rel(want[True], want[False]) > 1000 * TOL
    assert rel(ref.dense() @ x.double().numpy(), want[False]) > 1000 * TOL
    h = ops.handle(graph)
    eng = _engine(graph, d)
    for tr in (False, True):
        op = torch.ops.mirec.lgcn_propagate_drop_t if tr else torch.ops.mirec.lgcn_propagate_drop
        y_op = op(xd, h, p, seed)
        eng.set_dropout(p, seed)
        y_raw, y_pre = torch.empty_like(xd), torch.empty_like(xd)
        eng._prop(in_mode=IN_RAW, x_in=xd, out=y_raw, direction="bwd" if tr else "fwd")
        eng._prop(in_mode=IN_PRESCALED, x_in=xs, out=y_pre, direction="bwd" if tr else "fwd")
        eng.set_dropout(None)
        torch.cuda.synchronize()
        errs = [rel(y, want[tr]) for y in (y_op, y_raw, y_pre)]
        print(f"d={d} p={p} transposed={tr}: operator {errs[0]:.2e} raw {errs[1]:.2e} "
              f"prescaled {errs[2]:.2e}")
        assert max(errs) < TOL
        assert min(rel(y, want[not tr]) for y in (y_op, y_raw, y_pre)) > 1000 * TOL
        assert torch.equal(y_op, y_raw)                    # one kernel, one order of terms
        assert torch.all(y_op[N - 1] == 0)                 # the isolated item


def test_mask_bytes_of_the_transposed_launch(ref):
    """The dense reference's transpose is what mirec_edge_keep_mask's
    transposed bytes describe (the graph is symmetric: one CSR)."""
    counts = []
    for tr in (False, True):
        a = np.zeros((N, N))
        np.add.at(a, (ref.rows, ref.col), ref.keep(5, 0.6, transposed=tr).astype(np.float64))
        counts.append(a)
    assert np.array_equal(counts[1], counts[0].T) and not np.array_equal(counts[1], counts[0])
    scaled = ref.dinv[:, None] * counts[1] * ref.dinv[None, :] / float(np.float32(0.6))
    assert np.allclose(scaled, ref.dense(5, 0.6).T, rtol=1e-14, atol=0)


@pytest.mark.parametrize("d", [16, 64])
def test_keep_all_and_fields_zero(ref, graph, d):
    from furusato_recommend_amd._lib import IN_PRESCALED, IN_RAW
    x = torch.randn(N, d, generator=torch.Generator().manual_seed(3 * d)).cuda()
    xs = (graph.dinv[:, None] * x).contiguous()
    fresh, eng = _engine(graph, d), _engine(graph, d)
    for mode, xin in ((IN_RAW, x), (IN_PRESCALED, xs)):
        base, one, off = (torch.empty_like(x) for _ in range(3))
        fresh._prop(in_mode=mode, x_in=xin, out=base)
        eng.set_dropout(1.0, 9)                            # the dropout instantiation, all kept
        eng._prop(in_mode=mode, x_in=xin, out=one)
        eng.set_dropout(None)                              # no dropout again
        eng._prop(in_mode=mode, x_in=xin, out=off)
        torch.cuda.synchronize()
        e = rel(one, base)
        print(f"d={d} mode={mode}: keep_prob=1 vs plain {e:.2e} (bitwise {torch.equal(one, base)})")
        assert e <= 1e-6
        assert torch.equal(off, base)
        assert rel(base, ref.dense() @ x.double().cpu().numpy()) < TOL


@pytest.mark.parametrize("d", [16, 64, 20])
def test_operator_autograd(ref, graph, d):
    """x.grad of lgcn_propagate_drop is Â_dropᵀ ȳ (d = 20: padded to 32)."""
    from furusato_recommend_amd import ops
    p, seed = 0.6, 31
    M = ref.dense(seed, p)
    g = torch.Generator().manual_seed(7 + d)
    x, ybar = torch.randn(N, d, generator=g), torch.randn(N, d, generator=g)
    xd = x.cuda().requires_grad_(True)
    y = torch.ops.mirec.lgcn_propagate_drop(xd, ops.handle(graph), p, seed)
    y.backward(ybar.cuda())
    torch.cuda.synchronize()
    e_y, e_g = rel(y, M @ x.double().numpy()), rel(xd.grad, M.T @ ybar.double().numpy())
    print(f"d={d}: y {e_y:.2e} x.grad {e_g:.2e}")
    assert e_y < TOL and e_g < TOL
    assert rel(xd.grad, M @ ybar.double().numpy()) > 1000 * TOL


def test_operator_traces_with_fake_tensors(graph):
    from torch._subclasses.fake_tensor import FakeTensorMode

    from furusato_recommend_amd import ops
    h = ops.handle(graph)
    with FakeTensorMode():
        x = torch.empty(N, 64, device="cuda")
        y = torch.ops.mirec.lgcn_propagate_drop(x, h, 0.6, 1)
        assert y.shape == x.shape and y.dtype == x.dtype


# -------------------------------------------------------------- engine steps
@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("prune", [True, False])
def test_engine_steps_match_float64_autograd(ref, graph, prune, L, d):
    from furusato_recommend_amd.engine import AdamState, PropagationEngine
    p, lr, decay = 0.6, 1e-2, 1e-3
    seeds = [PropagationEngine.dropout_seed(BASE_SEED, t) for t in range(2)]
    assert seeds[0] != seeds[1]
    E0 = ref.emb(d)
    want_tabs, want_loss = ref.steps(E0, L, [ref.dense(s, p) for s in seeds], lr, decay)
    runs = []
    for _ in range(2):                                     # two engines, the same seeds
        eng = _engine(graph, d, L, prune)
        E = E0.clone().cuda()
        adam = AdamState(E, lr=lr)
        tabs, losses = [], []
        for t in range(2):
            u, pp, n = _tri(ref.triples[t])
            loss = eng.train_step(E, adam, u, pp, n, decay, dropout=(p, seeds[t]))
            losses.append(float(loss))
            tabs.append(E.clone())
            assert eng._drop is None and eng._acc_full is None
        torch.cuda.synchronize()
        runs.append((tabs, losses))
    (tabs, losses), (tabs2, losses2) = runs
    assert losses == losses2 and all(torch.equal(a, b) for a, b in zip(tabs, tabs2))
    for t in range(2):
        e_l = abs(losses[t] - want_loss[t]) / abs(want_loss[t])
        # (the update alone, relative to its own size, is printed for the record:
        # Adam's normalised step magnifies the error of the smallest gradients)
        upd = tabs[t] - (E0.cuda() if t == 0 else tabs[t - 1])
        want_upd = want_tabs[t] - (E0.double() if t == 0 else want_tabs[t - 1])
        e_t, e_u = rel(tabs[t], want_tabs[t]), rel(upd, want_upd)
        print(f"prune={prune} L={L} d={d} step {t}: loss {e_l:.2e} table {e_t:.2e} "
              f"update {e_u:.2e}")
        assert e_l < TOL and e_t < TOL
    # the steps are dropped ones: the full graph's step differs visibly
    # (its loss does not: log 2 plus second-order terms at this table's scale)
    full_tabs, _ = ref.steps(E0, L, [ref.dense()] * 2, lr, decay)
    assert rel(full_tabs[1], want_tabs[1]) > 100 * TOL


@pytest.mark.parametrize("variant", ["row_mask", "bytemap", "dense", "wave_only"])
def test_engine_step_variants_match_float64(ref, graph, variant):
    """The pruned L = 3 step through the launch forms the defaults do not
    take: rows by byte map without row lists, the first backward layer's two
    other neighbour filters, and narrow_max = 0 (every row by a whole wave)."""
    from furusato_recommend_amd.engine import AdamState, PropagationEngine
    p, lr, decay, d, L = 0.25, 1e-2, 1e-3, 64, 3
    seeds = [PropagationEngine.dropout_seed(BASE_SEED + 1, t) for t in range(2)]
    E0 = ref.emb(d, seed=1)
    want_tabs, want_loss = ref.steps(E0, L, [ref.dense(s, p) for s in seeds], lr, decay)
    eng = _engine(graph, d, L, True)
    if variant == "row_mask":
        eng.use_hop_list = False
    elif variant == "wave_only":
        eng.narrow_max = 0
    else:
        eng.sparse_filter = variant
    E = E0.clone().cuda()
    adam = AdamState(E, lr=lr)
    for t in range(2):
        u, pp, n = _tri(ref.triples[t])
        loss = float(eng.train_step(E, adam, u, pp, n, decay, dropout=(p, seeds[t])))
        e_l, e_t = abs(loss - want_loss[t]) / abs(want_loss[t]), rel(E, want_tabs[t])
        print(f"{variant} step {t}: loss {e_l:.2e} table {e_t:.2e}")
        assert e_l < TOL and e_t < TOL


# --------------------------------------------------------------------- model
def _model(ref, split, cls=None, **over):
    from furusato_recommend_amd import LightGCN
    cfg = {"recdim": 64, "layer": 3, "lr": 1e-2, "decay": 1e-3, "device": "cuda:0",
           "bpr_batch_size": 64, "seed": BASE_SEED}
    if split is not None:
        cfg["csr_split"] = split
    cfg.update(over)
    m = (cls or LightGCN)(cfg, ref.ds)
    with torch.no_grad():
        m.all_embedding.weight.copy_(ref.emb(64))
    return m


@pytest.mark.parametrize("split", SPLITS)
def test_model_stage_one_is_the_engine_step(ref, split):
    from furusato_recommend_amd.engine import PropagationEngine
    m = _model(ref, split, dropout=1, keep_prob=0.6)
    plain = _model(ref, split)                             # no keys: drives its engine by hand
    assert m.dropout and m.training and not plain.dropout
    assert m.dropout_seed(3) == PropagationEngine.dropout_seed(BASE_SEED, 3)
    for t in range(2):
        u, p, n = _tri(ref.triples[t])
        la = m.stageOne(u, p, n)
        lb = plain.engine.train_step(plain.all_embedding.weight, plain.optim, u, p, n, 1e-3,
                                     dropout=(0.6, m.dropout_seed(t)))
        assert torch.equal(la, lb)
        assert torch.equal(m.all_embedding.weight, plain.all_embedding.weight)
    want_tabs, _ = ref.steps(ref.emb(64), 3, [ref.dense(m.dropout_seed(t), 0.6) for t in range(2)],
                             1e-2, 1e-3)
    assert rel(m.all_embedding.weight, want_tabs[1]) < TOL
    # the counter travels with the optimizer state
    sd = m.optimizer_state_dict()
    assert sd["edge_dropout_step"] == 2
    m2 = _model(ref, split, dropout=1, keep_prob=0.6)
    m2.load_state_dict(m.state_dict())
    m2.load_optimizer_state_dict(sd)
    u, p, n = _tri(ref.triples[0])
    assert torch.equal(m.stageOne(u, p, n), m2.stageOne(u, p, n))
    assert torch.equal(m.all_embedding.weight, m2.all_embedding.weight)
    assert "edge_dropout_step" not in plain.optimizer_state_dict()


def test_model_keepprob_alias_and_one_epoch(ref):
    a = _model(ref, None, dropout=1, keepprob=0.25)
    b = _model(ref, None, dropout=1, keep_prob=0.25)
    assert a.keep_prob == b.keep_prob == 0.25
    t = np.concatenate(ref.triples)
    u, p, n = _tri(t)
    la, lb = a.OneEpoch(u, p, n), b.OneEpoch(u, p, n)      # two batches of 64: two masks
    assert torch.equal(la, lb) and a._drop_step == b._drop_step == 2
    assert torch.equal(a.all_embedding.weight, b.all_embedding.weight)
    want_tabs, _ = ref.steps(ref.emb(64), 3, [ref.dense(a.dropout_seed(k), 0.25) for k in range(2)],
                             1e-2, 1e-3)
    assert rel(a.all_embedding.weight, want_tabs[1]) < TOL


@pytest.mark.parametrize("split", SPLITS)
def test_model_bpr_loss_backward_matches_float64(ref, split):
    m = _model(ref, split, dropout=1, keep_prob=0.6)
    decay = 1e-3
    for k in range(2):                                     # the second call draws the next mask
        t = ref.triples[k]
        u, p, n = _tri(t)
        m.all_embedding.weight.grad = None
        loss, reg = m.bpr_loss(u, p, n)
        other = m.forward()                                # a later forward (another mask) ...
        (loss + decay * reg).backward()                    # ... must not leak into this backward
        del other
        E = ref.emb(64).double().requires_grad_(True)
        M = ref.dense(m.dropout_seed(2 * k), 0.6)
        want = Ref.loss(E, 3, torch.from_numpy(M), t, decay)
        want.backward()
        got, want = float((loss + decay * reg).detach()), float(want.detach())
        e_l = abs(got - want) / abs(want)
        e_g = rel(m.all_embedding.weight.grad, E.grad)
        print(f"split={split} call {k}: loss {e_l:.2e} grad {e_g:.2e}")
        assert e_l < TOL and e_g < TOL
    assert m._drop_step == 4


def test_model_eval_uses_the_full_graph_and_the_cache_rule(ref):
    m = _model(ref, None, dropout=1, keep_prob=0.6)
    users = torch.arange(0, NU, 7).cuda()

    def full_ratings(E):
        out = Ref_out(ref, E)
        return out[users.cpu().numpy()] @ out[NU:].T

    m.eval()
    assert rel(m.getUsersRating(users), full_ratings(ref.emb(64))) < TOL
    assert m._drop_step == 0                               # evaluation draws no mask
    m.train()
    u, p, n = _tri(ref.triples[0])
    m.stageOne(u, p, n)
    assert m.engine._acc_full is None
    with torch.no_grad():
        m.forward()                                        # a dropped full forward ...
    assert m.engine._acc_full is None                      # ... leaves no evaluation cache
    m.eval()
    E1 = m.all_embedding.weight.detach().cpu()
    r1 = m.getUsersRating(users)
    assert rel(r1, full_ratings(E1)) < TOL
    assert m.engine._acc_full is not None
    assert torch.equal(m.getUsersRating(users), r1)        # served from the cache, full graph
    ue, ie = m.eval_embeddings()
    out = Ref_out(ref, E1)
    assert rel(ue, out[:NU]) < TOL and rel(ie, out[NU:]) < TOL
    assert rel(m.propagated(), out) < TOL
    assert rel(m.eval_ratings()(users), full_ratings(E1)) < TOL
    # the dropped ratings would have been far away
    Md = ref.dense(m.dropout_seed(0), 0.6)
    x = acc = E1.double().numpy()
    for _ in range(3):
        x = Md @ x
        acc = acc + x
    outd = acc / 4
    assert rel(outd[users.cpu().numpy()] @ outd[NU:].T, full_ratings(E1)) > 100 * TOL


def Ref_out(ref, E):
    A = ref.dense()
    x = acc = E.double().numpy()
    for _ in range(3):
        x = A @ x
        acc = acc + x
    return acc / 4


def test_dropout_zero_is_bitwise_the_model_without_the_keys(ref):
    a, b = _model(ref, None, dropout=0, keep_prob=0.6), _model(ref, None)
    for t in range(2):
        u, p, n = _tri(ref.triples[t])
        assert torch.equal(a.stageOne(u, p, n), b.stageOne(u, p, n))
    assert torch.equal(a.all_embedding.weight, b.all_embedding.weight)
    assert a._drop_step == 0 and a.engine.edge_dropout is None


# ------------------------------------------------------------------ refusals
def test_model_refusals(ref):
    from furusato_recommend_amd import rAdjGCN
    from furusato_recommend_amd.dist import DataParallel
    from furusato_recommend_amd.train_dp import wrap
    for r in (0.3, 0.5):
        with pytest.raises(ValueError, match="dropout"):
            _model(ref, None, cls=rAdjGCN, dropout=1, keep_prob=0.6, r=r)
    _model(ref, None, cls=rAdjGCN, dropout=0, r=0.3)       # off: still fine
    w = np.ones(len(ref.ds.trainUser), np.float32)
    with pytest.raises(ValueError, match="edge_weight"):
        _model(ref, None, dropout=1, keep_prob=0.6, edge_weight=w)
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="keep_prob"):
            _model(ref, None, dropout=1, keep_prob=bad)
    m = _model(ref, None, dropout=1, keep_prob=0.6)
    with pytest.raises(NotImplementedError, match="dropout"):
        wrap(m)
    with pytest.raises(NotImplementedError, match="dropout"):
        DataParallel(m.engine, m.all_embedding.weight.data, m.optim)
    with pytest.raises(ValueError):
        m.engine.set_dropout(1.5, 0)


def _launch_rc(graph, x, **fields):
    import ctypes

    from furusato_recommend_amd import _lib
    p = _lib.Prop()
    p.dim, p.in_mode, p.divisor, p.narrow_max = x.shape[1], _lib.IN_RAW, 1.0, 64
    out = torch.empty_like(x)
    p.x_in, p.out = x.data_ptr(), out.data_ptr()
    p.partial = _lib.ptr(graph.partial_buffer(x.shape[1]))
    drop = _lib.Drop()
    for k, v in fields.items():
        setattr(drop if k in ("keep_prob", "transposed", "seed") else p, k, v)
    rc = _lib.lib.mirec_propagate_drop(graph.csr_ptr(), ctypes.byref(p), ctypes.byref(drop),
                                       _lib.stream_handle())
    torch.cuda.synchronize()
    return rc, out


def test_launch_without_dropout_is_mirec_propagate(graph):
    """mirec_propagate_drop with an all-zero struct, or none, is bitwise
    mirec_propagate."""
    import ctypes

    from furusato_recommend_amd import _lib
    from furusato_recommend_amd.engine import propagate
    x = torch.randn(N, 16, generator=torch.Generator().manual_seed(1)).cuda()
    base = torch.empty_like(x)
    propagate(graph, x, base)
    rc, zero = _launch_rc(graph, x)
    assert rc == 0 and torch.equal(zero, base)
    p = _lib.Prop()
    p.dim, p.in_mode, p.divisor, p.narrow_max = 16, _lib.IN_RAW, 1.0, 64
    none = torch.empty_like(x)
    p.x_in, p.out = x.data_ptr(), none.data_ptr()
    p.partial = _lib.ptr(graph.partial_buffer(16))
    assert _lib.lib.mirec_propagate_drop(graph.csr_ptr(), ctypes.byref(p), None,
                                         _lib.stream_handle()) == 0
    torch.cuda.synchronize()
    assert torch.equal(none, base)


def test_launch_rejects_values_with_dropout(ref, graph):
    from furusato_recommend_amd.graph import Graph
    x = torch.randn(N, 16).cuda()
    assert _launch_rc(graph, x, keep_prob=0.6, seed=1)[0] == 0
    w = np.ones(len(ref.ds.trainUser), np.float32)
    gw = Graph.from_interactions(ref.ds.trainUser, ref.ds.trainItem, NU, MI, "cuda:0", weight=w)
    assert _launch_rc(gw, x)[0] == 0
    assert _launch_rc(gw, x, keep_prob=0.6, seed=1)[0] == 1             # MIREC_ERR_ARG


@pytest.mark.parametrize("which", ["scale_src", "scale_dst", "scale_next"])
def test_launch_rejects_a_scale_vector_with_dropout(graph, which):
    x = torch.randn(N, 16).cuda()
    s = graph.dinv.data_ptr()
    assert _launch_rc(graph, x, **{which: s})[0] == 0
    assert _launch_rc(graph, x, keep_prob=0.6, **{which: s})[0] == 1


@pytest.mark.parametrize("bad", [-0.5, 1.5, float("nan"), float("inf")])
def test_launch_rejects_keep_prob_outside_the_interval(graph, bad):
    x = torch.randn(N, 16).cuda()
    assert _launch_rc(graph, x, keep_prob=bad)[0] == 1
