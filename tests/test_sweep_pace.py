"""Per-XCD pacing of the per-wave sweep (prop_sweep_wave_aux_kernel<.., kAuxPace>,
csrc/prop.hip; engine switch ``sweep_pace``).

The pacing touches no operand and no order of any sum: every comparison here
is ``torch.equal`` against the unpaced launches of the same layout.  It also
never waits UNTIL anything (a constant number of polls per band advance), so
a launch ends whatever its workspace holds; and the last workgroup to leave
zeroes the workspace again.

Small graph with the layouts forced small (18 item and 30 user tiles on at
most 16 workgroups: 2 workgroups per XCD label when the dispatcher deals them
round-robin, 2 passes of the user block, 12 and 11 bands)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
D, L, B = 64, 3, 64
SIZES = dict(wave_items=(40, 256), wave_users=(100, 64), max_grid=16)
PACE = {"items": (1, 1, 2), "users": (1, 1, 2)}


@pytest.fixture(scope="module")
def dataset():
    from furusato_recommend_amd import SyntheticBipartite
    return SyntheticBipartite(3000, 700, 40000, seed=1, test_frac=0)


def make_engine(ds, sizes=SIZES, dim=D, **graph_kw):
    from furusato_recommend_amd.engine import PropagationEngine
    from furusato_recommend_amd.graph import Graph
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0",
                                **graph_kw)
    eng = PropagationEngine(g, dim, L, B)
    eng.sweep_form, eng.sweep_users = "wave", True
    eng.set_sweep_sizes(**sizes)
    return g, eng


def triples(g, step):
    from furusato_recommend_amd.engine import sample_triples
    u = torch.empty(B, dtype=torch.int32, device="cuda")
    p, n = torch.empty_like(u), torch.empty_like(u)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    sample_triples(g, B, 0, step * B, u, p, n, err)
    return u, p, n


def run(ds, pace, sizes=SIZES, preset=None, dim=D, **graph_kw):
    """A full forward and two training steps: (acc, table, exp_avg,
    exp_avg_sq, workspace or None).  ``preset`` fills the workspace before
    every launch sequence."""
    from furusato_recommend_amd.engine import AdamState
    g, eng = make_engine(ds, sizes, dim, **graph_kw)
    eng.sweep_pace = pace
    if preset is not None:
        eng._pace_struct()  # allocates the workspace
        preset(eng._pace_ws)
    torch.manual_seed(0)
    emb = (0.1 * torch.randn(g.n_nodes, dim)).cuda()
    acc = eng.forward(emb).clone()
    adam = AdamState(emb, lr=1e-2)
    for s in range(2):
        if preset is not None:
            preset(eng._pace_ws)
        eng.train_step(emb, adam, *triples(g, s), 1e-4)
    torch.cuda.synchronize()
    return acc, emb, adam.exp_avg, adam.exp_avg_sq, eng._pace_ws


def assert_same(a, b):
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)


@pytest.fixture(scope="module")
def unpaced(dataset):
    return run(dataset, None)


def test_layouts_are_what_the_cases_assume(dataset):
    g, eng = make_engine(dataset)
    wi, wu = eng.sweep_wave.desc, eng.sweep_wave_users.desc
    assert wi.n_tiles == 18 and wu.n_tiles == 30 and wi.grid == 16 and wu.grid == 16
    assert -(-wi.n_src // wi.band_rows) == 12 and -(-wu.n_src // wu.band_rows) == 11


def test_paced_equals_unpaced(dataset, unpaced):
    paced = run(dataset, PACE)
    assert_same(paced, unpaced)
    assert int(paced[4].abs().max()) == 0  # the workspace zeroed itself


@pytest.mark.parametrize("max_grid", [1, 8, 2])
def test_paced_equals_unpaced_other_grids(dataset, unpaced, max_grid):
    """One workgroup per label (8), a single workgroup (1), grid < tiles (2).
    The grid only deals the tiles out: the unpaced result is the same for
    every grid, so the module's reference serves."""
    sizes = dict(SIZES, max_grid=max_grid)
    assert_same(run(dataset, None, sizes), unpaced)
    assert_same(run(dataset, PACE, sizes), unpaced)


def test_one_band_never_paces(dataset):
    """band_rows >= the source block: no band advance, the pacing path never
    runs (the workgroups still register, leave and zero the workspace)."""
    sizes = dict(wave_items=(40, 4096), wave_users=(100, 1024), max_grid=16)
    ref, paced = run(dataset, None, sizes), run(dataset, PACE, sizes)
    assert_same(paced, ref)
    assert int(paced[4].abs().max()) == 0


def test_maximum_throttling(dataset, unpaced):
    assert_same(run(dataset, {"items": (0, 1, 2), "users": (0, 1, 2)}), unpaced)


def test_one_block_paced(dataset, unpaced):
    assert_same(run(dataset, {"items": (1, 2, 1), "users": None}), unpaced)
    assert_same(run(dataset, {"items": None, "users": (2, 4, 0)}), unpaced)


def test_worst_case_workspace_terminates_and_changes_nothing(dataset, unpaced):
    """Every label's count preset to 2^20 workgroups with a sum of 0: every
    workgroup sees the largest possible lead at every advance and naps the
    full kPaceMaxNaps = 8 times, each nap 2 units of 512 clocks plus two
    polls (a few microseconds in all).  Nothing waits until anything, so the
    bound is a product of constants: at most 30 tiles x 11 advances per
    workgroup (max_grid 16: 2 tiles) x 8 naps x under 10 us < 27 ms for a
    single workgroup, far less here; the launch must end and stay bitwise
    equal.  (The preset counts are garbage the kernel cannot repair: only the
    results and termination are checked here.)"""
    def preset(ws):
        w = ws.view(-1, 32)
        w[:, 0] = 0
        w[0:16:2, 0] = 1 << 20            # items region: registered counts
        w[17:33:2, 0] = 1 << 20           # users region
    paced = run(dataset, {"items": (0, 1, 2), "users": (0, 1, 2)}, preset=preset)
    assert_same(paced, unpaced)


@pytest.mark.parametrize("launches", [1, 2, 5])
def test_workspace_zero_after_launches(dataset, launches):
    from furusato_recommend_amd._lib import IN_PRESCALED, lib
    g, eng = make_engine(dataset)
    eng.sweep_pace = PACE
    x = (0.1 * torch.randn(g.n_nodes, D)).cuda()
    out, xs = torch.empty_like(x), torch.empty_like(x)
    for _ in range(launches):
        eng._prop(in_mode=IN_PRESCALED, x_in=x, addend=x, out=out, xs_out=xs)
    torch.cuda.synchronize()
    assert eng._pace_ws.numel() * 4 == int(lib.mirec_sweep_pace_ws_bytes())
    assert int(eng._pace_ws.abs().max()) == 0


def test_graph_capture_of_a_paced_step(dataset):
    """One paced training step captured and replayed twice equals the same
    step issued twice eagerly (the fused Adam's scalars are launch arguments,
    so both replays are step 2 of the optimiser: the eager side rewinds its
    step count to match)."""
    from furusato_recommend_amd.engine import AdamState

    def setup():
        g, eng = make_engine(dataset)
        eng.sweep_pace = PACE
        torch.manual_seed(0)
        emb = (0.1 * torch.randn(g.n_nodes, D)).cuda()
        adam = AdamState(emb, lr=1e-2)
        t = triples(g, 0)
        eng.train_step(emb, adam, *t, 1e-4)   # eager: prescale, allocations
        torch.cuda.synchronize()
        return g, eng, emb, adam, t

    g, eng, emb, adam, t = setup()
    for _ in range(2):
        adam.n_steps = 1
        eng.train_step(emb, adam, *t, 1e-4)
    torch.cuda.synchronize()
    eager = (emb.clone(), adam.exp_avg.clone(), adam.exp_avg_sq.clone())

    g, eng, emb, adam, t = setup()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.train_step(emb, adam, *t, 1e-4)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip((emb, adam.exp_avg, adam.exp_avg_sq), eager):
        assert torch.equal(a, b)
    assert int(eng._pace_ws.abs().max()) == 0


def test_null_pace_is_the_unpaced_entry(dataset):
    """pace == NULL through the paced entry against
    mirec_propagate_sweep_wave, bitwise, on one full launch."""
    from furusato_recommend_amd import _lib
    from furusato_recommend_amd._lib import IN_PRESCALED, check, lib
    g, eng = make_engine(dataset)
    x = (0.1 * torch.randn(g.n_nodes, D)).cuda()
    outs = []
    for paced_entry in (True, False):
        out, xs = torch.zeros_like(x), torch.zeros_like(x)
        p = _lib.Prop()
        p.dim, p.in_mode, p.divisor = D, IN_PRESCALED, 1.0
        p.x_in, p.addend, p.out, p.xs_out = x.data_ptr(), x.data_ptr(), out.data_ptr(), \
            xs.data_ptr()
        p.narrow_max = 64
        wi, wu = eng.sweep_wave.ptr(), eng.sweep_wave_users.ptr()
        if paced_entry:
            check(lib.mirec_propagate_sweep_wave_paced(g.csr_ptr(), ctypes.byref(p), wi, wu, None,
                                                       _lib.stream_handle()))
        else:
            check(lib.mirec_propagate_sweep_wave(g.csr_ptr(), ctypes.byref(p), wi, wu,
                                                 _lib.stream_handle()))
        torch.cuda.synchronize()
        outs.append((out, xs))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert float(outs[0][0].abs().max()) > 0


def test_layouts_that_do_not_qualify_fall_back(dataset):
    """d = 32 and a weighted graph have no sweep layout: the paced entry is
    mirec_propagate, bit for bit, and never touches a workspace."""
    for kw in (dict(dim=32), dict(weight=np.random.default_rng(3).uniform(
            0.5, 2.0, len(dataset.trainUser)).astype(np.float32))):
        _, eng = make_engine(dataset, **kw)
        assert eng.sweep_wave is None and eng.sweep_wave_users is None
        ref, paced = run(dataset, None, **kw), run(dataset, PACE, **kw)
        assert_same(paced, ref)
        assert int(paced[4].abs().max()) == 0


def test_bad_pace_arguments_are_refused(dataset):
    g, eng = make_engine(dataset)
    x = (0.1 * torch.randn(g.n_nodes, D)).cuda()
    from furusato_recommend_amd._lib import IN_PRESCALED
    for bad in ((1, 1, 17), (-1, 1, 1), (1, -1, 1)):
        eng.sweep_pace = {"items": bad, "users": None}
        with pytest.raises(Exception):
            eng._prop(in_mode=IN_PRESCALED, x_in=x, addend=x, out=torch.empty_like(x))
