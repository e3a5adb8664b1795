"""The first backward layer through the LDS-prefiltered list kernel
(prop_seeded_kernel, csrc/prop.hip; mirec_propagate_seeded, mirec_frontier_bits;
engine switch ``seeded_first``).

The kernel removes loads, not terms: the exact filter stays slot >= 0 and the
compaction, the fma order and the epilogue are prop_kernel's.  So every
comparison here is ``torch.equal`` between ``seeded_first`` on and off on the
same inputs, no tolerance.

The graph (300 users x 70 items, neither a multiple of 32: bit-word tails) has
rows of degree 0, 1, 15, 16, 17, 32, 33, 63, 64, 65 (chunk boundaries and the
narrow / wide switch at narrow_max = 64) and one of 205 (several 64-entry
chunks), and duplicate edges."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NU, MI = 300, 70
N = NU + MI
DEGREES = (0, 1, 15, 16, 17, 32, 33, 63, 64, 65)
SENTINEL = 12345.678


def edges():
    """(user, item) interactions.  Users 0..9 take DEGREES items out of items
    10..68 (cycling: duplicates past 59); items 0..9 take 205 (200 users and
    5 of them twice) and DEGREES[1:] users out of users 10..299; the other
    users get 0..3 random items of 10..68.  User 0 and item 69 (= node N - 1)
    stay isolated."""
    rng = np.random.default_rng(7)
    u, i = [], []
    for k, d in enumerate(DEGREES):
        u += [k] * d
        i += [10 + (3 * k + j) % 59 for j in range(d)]
    wide = list(range(10, 210)) + [10, 11, 12, 13, 14]
    u += wide
    i += [0] * len(wide)
    for k, d in enumerate(DEGREES[1:], start=1):
        u += list(10 + (rng.permutation(290)[:d]))
        i += [k] * d
    for usr in range(10, NU):
        for it in rng.integers(10, 69, rng.integers(0, 4)):
            u.append(usr)
            i.append(int(it))
    return np.asarray(u, np.int64), np.asarray(i, np.int64)


@pytest.fixture(scope="module")
def inter():
    u, i = edges()
    deg = np.concatenate([np.bincount(u, minlength=NU), np.bincount(i, minlength=MI)])
    assert set(DEGREES) | {205} <= set(deg.tolist())
    assert deg[0] == 0 and deg[N - 1] == 0
    pairs = u * MI + i
    assert len(np.unique(pairs)) < len(pairs)  # duplicate edges
    return u, i


def make_graph(inter, **kw):
    from furusato_recommend_amd.graph import Graph
    return Graph.from_interactions(inter[0], inter[1], NU, MI, "cuda:0", **kw)


# (users, pos items, neg items)
BATCHES = {
    "single": ([5], [20], [33]),
    "repeated": ([7, 7, 7, 12, 12, 40], [15, 15, 0, 0, 22, 22], [0, 15, 15, 31, 31, 31]),
    # nodes 0, n_users - 1, n_users and N - 1; user 0 and item 69 are the
    # isolated rows, so F1 holds degree-0 rows of both sides
    "ends": ([0, NU - 1, 0, 150], [0, MI - 1, 5, 0], [MI - 1, 0, 0, 9]),
    # the neighbours of the isolated rows' sides: low users and high items
    "near_isolated": ([1, 2, 3, 9], [68, 67, 10, 11], [66, 12, 68, 69 - 1]),
}


def batch(name):
    return tuple(torch.tensor(x, dtype=torch.int32, device="cuda") for x in BATCHES[name])


def all_nodes_batch():
    """Every node in S: all bits set, the prefilter passes everything."""
    u = torch.arange(NU, dtype=torch.int32, device="cuda")
    return u, (u % MI).contiguous(), ((u + 35) % MI).contiguous()


@contextlib.contextmanager
def counting():
    """Counts the calls of mirec_propagate_seeded."""
    from furusato_recommend_amd import _lib
    real, n = _lib.lib.mirec_propagate_seeded, [0]

    def wrapped(*a):
        n[0] += 1
        return real(*a)
    _lib.lib.mirec_propagate_seeded = wrapped
    try:
        yield n
    finally:
        _lib.lib.mirec_propagate_seeded = real


def engine(g, dim, L, seeded, max_batch=NU, lds=None, **kw):
    from furusato_recommend_amd.engine import PropagationEngine
    eng = PropagationEngine(g, dim, L, max_batch, **kw)
    eng.seeded_first = seeded
    if lds is not None:
        eng.seeded_lds_bytes = lds
    return eng


def table(g, dim):
    torch.manual_seed(0)
    return (0.1 * torch.randn(g.n_nodes, dim)).cuda()


def first_layer(g, dim, L, seeded, t, lds=None):
    """One step issued by hand with ``xs[0]`` (the first backward layer's
    output) preset to a sentinel: (xs[0], F1 byte map, seeded launches)."""
    from furusato_recommend_amd.engine import AdamState
    eng = engine(g, dim, L, seeded, lds=lds)
    emb = table(g, dim)
    adam = AdamState(emb, lr=1e-2)
    with counting() as n:
        eng.compute_frontier(*t)
        out = eng.forward(emb, pruned=True)
        eng.bpr(out, emb, *t, 1e-4)
        f1 = eng.bm_hop.view(torch.uint8)[:g.n_nodes].clone() != 0
        eng.xs[0].fill_(SENTINEL)
        eng.backward(emb, adam=adam)
        torch.cuda.synchronize()
    return eng.xs[0].clone(), f1, n[0]


def two_steps(g, dim, L, seeded, ts, lds=None, step=None, **kw):
    """Two training steps: (table, exp_avg, exp_avg_sq, seeded launches)."""
    from furusato_recommend_amd.engine import AdamState
    eng = engine(g, dim, L, seeded, lds=lds, **kw)
    emb = table(g, dim)
    adam = AdamState(emb, lr=1e-2)
    with counting() as n:
        for t in ts:
            if step is None:
                eng.train_step(emb, adam, *t, 1e-4)
            else:
                step(eng, emb, adam, t)
        torch.cuda.synchronize()
    return emb, adam.exp_avg, adam.exp_avg_sq, n[0]


def assert_same(a, b):
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)


@pytest.fixture(scope="module")
def graph(inter):
    return make_graph(inter)


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("dim", [16, 64, 256])
def test_first_backward_layer_and_steps(graph, dim, L):
    sent = torch.full((1,), SENTINEL).view(torch.int32).item()
    for name in BATCHES:
        t = batch(name)
        on, f1, n_on = first_layer(graph, dim, L, True, t)
        off, f1_off, n_off = first_layer(graph, dim, L, False, t)
        assert (n_on, n_off) == (1, 0), name
        assert torch.equal(f1, f1_off) and 0 < int(f1.sum()) < N, name
        assert torch.equal(on[f1], off[f1]), name
        # rows outside F1 are not written, bytewise
        assert bool((on[~f1].view(torch.int32) == sent).all()), name
        assert torch.equal(on.view(torch.int32), off.view(torch.int32)), name
    ts = [batch("repeated"), batch("ends")]
    a, b = two_steps(graph, dim, L, True, ts), two_steps(graph, dim, L, False, ts)
    assert (a[3], b[3]) == (2, 0)
    assert_same(a, b)


def test_one_layer_runs_the_old_path(graph):
    a = two_steps(graph, 64, 1, True, [batch("repeated")])
    b = two_steps(graph, 64, 1, False, [batch("repeated")])
    assert a[3] == 0
    assert_same(a, b)


def test_bits_are_the_seed_set(graph):
    """The two bit arrays after a frontier: exactly S at shift 0, its image
    under >> shift when coarse; words past the arrays stay clear."""
    for lds, want in ((8, None), (1 << 14, (0, 0))):
        eng = engine(graph, 64, 3, True, lds=lds)
        shifts = eng.seed_bit_shifts()
        if want is None:
            assert min(shifts) >= 2
        else:
            assert shifts == want
        t = batch("ends")
        eng.compute_frontier(*t)
        sb = eng._seed_bits_struct()
        words = eng._seed_bits_mem.cpu().numpy().view(np.uint32)
        got = np.unpackbits(words.view(np.uint8), bitorder="little")
        s = np.unique(np.concatenate([t[0].cpu().numpy(), NU + t[1].cpu().numpy(),
                                      NU + t[2].cpu().numpy()]))
        ref = np.zeros_like(got)
        for v in s:
            if v < NU:
                ref[v >> shifts[0]] = 1
            else:
                ref[32 * sb.words[0] + ((v - NU) >> shifts[1])] = 1
        assert np.array_equal(got, ref)


@pytest.mark.parametrize("dim", [16, 64, 256])
def test_prefilter_stress(graph, dim):
    """Coarse bits (both shifts >= 2), exact bits, and every node in S."""
    ts = [batch("repeated"), batch("near_isolated")]
    off = two_steps(graph, dim, 3, False, ts)
    for lds in (8, 1 << 14):
        on = two_steps(graph, dim, 3, True, ts, lds=lds)
        assert on[3] == 2
        assert_same(on, off)
        x_on, f1, n = first_layer(graph, dim, 3, True, ts[0], lds=lds)
        x_off, _, _ = first_layer(graph, dim, 3, False, ts[0])
        assert n == 1 and torch.equal(x_on.view(torch.int32), x_off.view(torch.int32))
    t = all_nodes_batch()
    for lds in (8, 1 << 14):
        x_on, f1, n = first_layer(graph, dim, 3, True, t, lds=lds)
        x_off, _, _ = first_layer(graph, dim, 3, False, t)
        assert n == 1 and int(f1.sum()) >= N - 2
        assert torch.equal(x_on.view(torch.int32), x_off.view(torch.int32))


def test_sampled_softmax_step(graph):
    """train_step_ssm, K = 4: the frontier comes from a key list."""
    torch.manual_seed(3)
    ts = []
    for name in ("repeated", "ends"):
        u, p, _ = batch(name)
        neg = torch.randint(0, MI, (u.shape[0], 4), dtype=torch.int32, device="cuda")
        ts.append((u, p, neg))

    def step(eng, emb, adam, t):
        eng.train_step_ssm(emb, adam, *t, 1e-4, 0.2)
    a = two_steps(graph, 64, 3, True, ts, step=step, n_neg=4)
    b = two_steps(graph, 64, 3, False, ts, step=step, n_neg=4)
    assert (a[3], b[3]) == (2, 0)
    assert_same(a, b)


def test_imported_seeds(graph):
    """import_seeds of two concatenated batches, then backward (the
    data-parallel path in one process)."""
    def step(eng, emb, adam, t):
        out = eng.forward(emb)
        parts = []
        for name in t:
            eng.bpr(out, emb, *batch(name), 1e-4, grad_scale=0.5)
            parts.append([x.clone() for x in eng.export_seeds()])
        eng.import_seeds(*(torch.cat([p[i] for p in parts]) for i in range(3)))
        eng.backward(emb, adam=adam)
    ts = [("repeated", "ends"), ("single", "near_isolated")]
    a = two_steps(graph, 64, 3, True, ts, step=step, max_batch=8)
    b = two_steps(graph, 64, 3, False, ts, step=step, max_batch=8)
    assert (a[3], b[3]) == (2, 0)
    assert_same(a, b)


def edge_index_graph(inter):
    from furusato_recommend_amd.graph import Graph
    u, i = inter
    ei = np.stack([np.concatenate([u, i + NU]), np.concatenate([i + NU, u])])
    g = Graph.from_edge_index(ei, N, "cuda:0")
    g.n_users, g.m_items = NU, MI  # the training step's node numbering
    return g


FALLBACKS = {
    "edge_index": (edge_index_graph, None),
    "weights": (lambda it: make_graph(it, weight=1.0 + (np.arange(len(it[0])) % 5)), None),
    "r_adjusted": (lambda it: make_graph(it, r=0.3), None),
    "dropout": (make_graph, (0.5, 11)),
    "segments": (lambda it: make_graph(it, split=48), None),
}


@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_fallbacks_run_the_old_launch(inter, case):
    build, dropout = FALLBACKS[case]
    g = build(inter)
    if case == "segments":
        assert g.n_seg > 0
    ts = [batch("repeated"), batch("ends")]

    def step(eng, emb, adam, t):
        eng.train_step(emb, adam, *t, 1e-4, dropout=dropout)
    a = two_steps(g, 64, 3, True, ts, step=step)
    b = two_steps(g, 64, 3, False, ts, step=step)
    assert (a[3], b[3]) == (0, 0)
    assert_same(a, b)


def test_other_shapes_through_the_entry_are_mirec_propagate(graph):
    """mirec_propagate_seeded with no filter, and with an in_mask, is the
    plain launch."""
    import ctypes

    from furusato_recommend_amd import _lib
    eng = engine(graph, 64, 3, True)
    emb = table(graph, 64)
    t = batch("repeated")
    eng.compute_frontier(*t)
    out = eng.forward(emb, pruned=True)
    eng.bpr(out, emb, *t, 1e-4)
    res = []
    for filt, mask in ((None, None), (eng._seed_bits_struct(), eng.bm_self), (False, None)):
        p = _lib.Prop()
        xs = torch.full((N, 64), SENTINEL, device="cuda")
        rows = eng._hop_rows()
        p.dim, p.in_mode, p.divisor = 64, _lib.IN_SPARSE, 1.0
        p.slot, p.seed_in, p.seed = eng.slot.data_ptr(), eng.seed_p.data_ptr(), eng.seed_p.data_ptr()
        p.xs_out = xs.data_ptr()
        p.row_mask, p.row_list = rows["row_mask"].data_ptr(), rows["row_list"].data_ptr()
        p.row_count, p.row_list_cap = rows["row_count"].data_ptr(), rows["row_list_cap"]
        p.wide_list, p.wide_count = rows["wide_list"].data_ptr(), rows["wide_count"].data_ptr()
        p.narrow_max = eng.narrow_max
        p.in_mask = mask.data_ptr() if mask is not None else None
        if filt is False:
            _lib.check(_lib.lib.mirec_propagate(graph.csr_ptr(), ctypes.byref(p),
                                                _lib.stream_handle()))
        else:
            _lib.check(_lib.lib.mirec_propagate_seeded(
                graph.csr_ptr(), ctypes.byref(p), ctypes.byref(filt) if filt else None,
                _lib.stream_handle()))
        torch.cuda.synchronize()
        res.append(xs)
    assert torch.equal(res[0].view(torch.int32), res[2].view(torch.int32))
    assert torch.equal(res[1].view(torch.int32), res[2].view(torch.int32))


def test_graph_capture_of_a_seeded_step(graph):
    """One training step captured and replayed twice equals the same step
    issued twice eagerly (both replays are step 2 of the optimiser: the eager
    side rewinds its step count to match)."""
    from furusato_recommend_amd.engine import AdamState

    def setup():
        eng = engine(graph, 64, 3, True)
        emb = table(graph, 64)
        adam = AdamState(emb, lr=1e-2)
        t = batch("repeated")
        eng.train_step(emb, adam, *t, 1e-4)   # eager: prescale, allocations
        torch.cuda.synchronize()
        return eng, emb, adam, t

    eng, emb, adam, t = setup()
    for _ in range(2):
        adam.n_steps = 1
        eng.train_step(emb, adam, *t, 1e-4)
    torch.cuda.synchronize()
    eager = (emb.clone(), adam.exp_avg.clone(), adam.exp_avg_sq.clone())

    eng, emb, adam, t = setup()
    cg = torch.cuda.CUDAGraph()
    with counting() as n, torch.cuda.graph(cg):
        eng.train_step(emb, adam, *t, 1e-4)
    assert n[0] == 1
    cg.replay()
    cg.replay()
    torch.cuda.synchronize()
    for a, b in zip((emb, adam.exp_avg, adam.exp_avg_sq), eager):
        assert torch.equal(a, b)
