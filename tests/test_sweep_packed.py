"""Packed slot streams, user tiles above 64 KB and streaming Adam in the
per-wave column sweep (csrc/prop.hip; engine switches ``sweep_packed``,
``sweep_user_tile`` and ``adam_stream``).

None of the three may change one bit: a packed slot decodes to the (row,
column) pair of its 8-byte slot, a row's terms are added in ascending (column,
CSR position) order whatever tile the row lies in, and a non-temporal load or
store moves the same values.  So every case below is compared with
``torch.equal`` against one reference: 8-byte slots, unpaced, plain Adam.

The 3 000 x 700 graph of tests/test_prop_sweep_wave.py, L = 3, batch 64,
sizes forced small: several passes and bands, a ragged last tile."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
D, L, B = 64, 3, 64
# items: 30 tiles of 24 rows, 12 bands; users: 75 tiles of 40 rows, 11 bands;
# 3 workgroups: 10 and 25 passes
SIZES = dict(wave_items=(24, 256), wave_users=(40, 64), max_grid=3)


@pytest.fixture(scope="module")
def dataset():
    from furusato_recommend_amd import SyntheticBipartite
    return SyntheticBipartite(3000, 700, 40000, seed=1, test_frac=0)


def make_engine(ds, sizes=SIZES, packed=True, pace=None, adam_stream=False, use_sweep=True):
    from furusato_recommend_amd.engine import PropagationEngine
    from furusato_recommend_amd.graph import Graph
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    eng = PropagationEngine(g, D, L, B)
    eng.sweep_form, eng.sweep_users = "wave", True
    eng.sweep_packed = packed
    eng.set_sweep_sizes(**sizes)
    eng.sweep_pace, eng.adam_stream, eng.use_sweep = pace, adam_stream, use_sweep
    for lay in (eng.sweep_wave, eng.sweep_wave_users):
        assert (lay.desc.row_bits > 0) == packed
        assert lay.slot.element_size() == (4 if packed else 8)
        assert lay.slot.numel() == lay.desc.n_slots
    return g, eng


def triples(g, step):
    from furusato_recommend_amd.engine import sample_triples
    u = torch.empty(B, dtype=torch.int32, device="cuda")
    p, n = torch.empty_like(u), torch.empty_like(u)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    sample_triples(g, B, 0, step * B, u, p, n, err)
    return u, p, n


def run(ds, **kw):
    """The full forward's acc on every row, then two training steps: (acc,
    table, exp_avg, exp_avg_sq)."""
    from furusato_recommend_amd.engine import AdamState
    g, eng = make_engine(ds, **kw)
    torch.manual_seed(0)
    emb = (0.1 * torch.randn(g.n_nodes, D)).cuda()
    acc = eng.forward(emb).clone()
    adam = AdamState(emb, lr=1e-2)
    for s in range(2):
        eng.train_step(emb, adam, *triples(g, s), 1e-4)
    torch.cuda.synchronize()
    return acc, emb, adam.exp_avg, adam.exp_avg_sq


def assert_same(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.fixture(scope="module")
def reference(dataset):
    return run(dataset, packed=False)


@pytest.fixture(scope="module")
def default_pace():
    from furusato_recommend_amd.engine import SWEEP_PACE
    return SWEEP_PACE


def test_the_sweep_ran(dataset, reference):
    rows = run(dataset, packed=False, use_sweep=False)
    assert not torch.equal(rows[0], reference[0])


def test_packed_unpaced(dataset, reference):
    assert_same(run(dataset), reference)


def test_packed_paced_at_the_default_triples(dataset, reference, default_pace):
    assert_same(run(dataset, pace=default_pace), reference)
    assert_same(run(dataset, packed=False, pace=default_pace), reference)


@pytest.mark.parametrize("paced", [False, True])
def test_packed_single_workgroup(dataset, reference, default_pace, paced):
    sizes = dict(SIZES, max_grid=1)
    assert_same(run(dataset, sizes=sizes, pace=default_pace if paced else None), reference)


def test_packed_step_captured_and_replayed(dataset, default_pace):
    """One training step captured and replayed twice, packed against 8-byte
    (the fused Adam's scalars are launch arguments: both replays are step 2)."""
    from furusato_recommend_amd.engine import AdamState
    outs = []
    for packed in (False, True):
        g, eng = make_engine(dataset, packed=packed, pace=default_pace, adam_stream=packed)
        torch.manual_seed(0)
        emb = (0.1 * torch.randn(g.n_nodes, D)).cuda()
        adam = AdamState(emb, lr=1e-2)
        t = triples(g, 0)
        eng.train_step(emb, adam, *t, 1e-4)   # eager: prescale, allocations
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            eng.train_step(emb, adam, *t, 1e-4)
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
        outs.append((emb, adam.exp_avg, adam.exp_avg_sq))
    assert_same(outs[1], outs[0])


def full_launch(g, eng, x, wi, wu):
    """One full PRESCALED launch through mirec_propagate_sweep_wave."""
    from furusato_recommend_amd import _lib
    from furusato_recommend_amd._lib import IN_PRESCALED, check, lib
    out, xs = torch.zeros_like(x), torch.zeros_like(x)
    p = _lib.Prop()
    p.dim, p.in_mode, p.divisor = D, IN_PRESCALED, 1.0
    p.x_in, p.addend, p.out, p.xs_out = x.data_ptr(), x.data_ptr(), out.data_ptr(), xs.data_ptr()
    p.narrow_max = 64
    check(lib.mirec_propagate_sweep_wave(g.csr_ptr(), ctypes.byref(p), wi, wu,
                                         _lib.stream_handle()), "propagate")
    torch.cuda.synchronize()
    return out, xs


def test_descriptor_with_row_bits_0_still_runs(dataset):
    """row_bits == 0 is the 8-byte form, as every descriptor built before the
    field existed; the keyword that selects it leaves an engine with 8-byte
    slots and equal results."""
    g, e8 = make_engine(dataset, packed=False)
    _, e4 = make_engine(dataset, packed=True)
    assert e8.sweep_wave.desc.row_bits == 0 and e8.sweep_wave_users.desc.row_bits == 0
    assert e8.sweep_wave.slot.dtype == torch.int64
    assert e4.sweep_wave.desc.row_bits == 5 and e4.sweep_wave_users.desc.row_bits == 6
    x = (0.1 * torch.randn(g.n_nodes, D)).cuda()
    a = full_launch(g, e8, x, e8.sweep_wave.ptr(), e8.sweep_wave_users.ptr())
    b = full_launch(g, e4, x, e4.sweep_wave.ptr(), e4.sweep_wave_users.ptr())
    rows = full_launch(g, e8, x, None, None)
    assert_same(a, b)
    assert not torch.equal(a[0], rows[0])


@pytest.mark.parametrize("tile", [280, 320])
def test_user_tiles_above_64_kb(dataset, tile):
    big = dict(wave_items=(24, 256), wave_users=(tile, 64), max_grid=4)
    base = dict(big, wave_users=(256, 64))
    ref = run(dataset, sizes=base, packed=False)
    assert_same(run(dataset, sizes=big), ref)
    assert_same(run(dataset, sizes=big, packed=False), ref)


def test_tile_of_321_rows_is_refused(dataset):
    from furusato_recommend_amd import _lib
    with pytest.raises(ValueError):
        make_engine(dataset, sizes=dict(SIZES, wave_users=(321, 64)))
    # a hand-made descriptor: the launch falls back to the row kernel for the block
    g, eng = make_engine(dataset, sizes=dict(SIZES, wave_users=(320, 64)))
    bad = _lib.SweepWave.from_buffer_copy(eng.sweep_wave_users.desc)
    bad.tile_rows = 321
    x = (0.1 * torch.randn(g.n_nodes, D)).cuda()
    wi = eng.sweep_wave.ptr()
    fallback = full_launch(g, eng, x, wi, ctypes.byref(bad))
    rows = full_launch(g, eng, x, wi, None)
    swept = full_launch(g, eng, x, wi, eng.sweep_wave_users.ptr())
    assert_same(fallback, rows)
    assert not torch.equal(swept[0], rows[0])


def test_streaming_adam_swept(dataset, reference, default_pace):
    assert_same(run(dataset, adam_stream=True), reference)
    assert_same(run(dataset, adam_stream=True, pace=default_pace), reference)


def test_streaming_adam_row_kernel(dataset):
    off = run(dataset, use_sweep=False, adam_stream=False)
    on = run(dataset, use_sweep=False, adam_stream=True)
    assert_same(on, off)
