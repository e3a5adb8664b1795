"""The masked form of the per-wave column sweep: the in-masked backward launch
of a pruned step (``in_mask`` = F1, every row; csrc/prop.hip sweep_wave_work's
INMASK, ``mirec_propagate_sweep_wave_masked``, engine switch ``sweep_inmask``;
DESIGN.md §27).

Exact oracle.  A masked-out slot becomes padding and a row's passing terms are
added in stream order to accumulators that start at +0.0, so the masked sweep
of ``x`` under mask M must equal, bit for bit, the UNMASKED sweep (same layout,
same pacing) of a copy of ``x`` whose rows outside M are +0.0.  The masked run
gets NaN in the rows outside M: any use of a masked-out row poisons its result.
A block that is not asked for runs the row kernel on its row range and must
equal ``mirec_propagate`` with the same mask bit for bit (3 000 % 4 == 0: the
item rows start a wave of the row kernel).

The 3 000 x 700 graph of tests/test_sweep_packed.py.  Item tiles of 8, 196 and
280 rows all leave a ragged last tile (700 = 87 x 8 + 4); 3 000 = 375 x 8, so
the case with tiles of 8 rows also runs the user block at 7 rows (428 x 7 + 4),
where it has one too."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
D, B = 64, 64
NU, MI = 3000, 700
N = NU + MI
BAND_I, BAND_U = 256, 64           # 12 bands of users, 11 bands of items
ITEMS, USERS, BOTH = 1, 2, 3
PACE = {"items": (8, 16, 16), "users": (4, 4, 16)}


@pytest.fixture(scope="module")
def dataset():
    from furusato_recommend_amd import SyntheticBipartite
    return SyntheticBipartite(NU, MI, 40000, seed=1, test_frac=0)


@pytest.fixture(scope="module")
def graph(dataset):
    from furusato_recommend_amd.graph import Graph
    ds = dataset
    return Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")


def make_engine(g, tile=24, grid=3, L=3, packed=True, pace=None, dim=D, tile_users=None):
    from furusato_recommend_amd.engine import PropagationEngine
    eng = PropagationEngine(g, dim, L, B)
    eng.sweep_form, eng.sweep_users = "wave", True
    eng.sweep_packed = packed
    eng.set_sweep_sizes(wave_items=(tile, BAND_I), wave_users=(tile_users or tile, BAND_U),
                        max_grid=grid)
    eng.sweep_pace = pace
    return eng


def triples(g, step):
    from furusato_recommend_amd.engine import sample_triples
    u = torch.empty(B, dtype=torch.int32, device="cuda")
    p, n = torch.empty_like(u), torch.empty_like(u)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    sample_triples(g, B, 0, step * B, u, p, n, err)
    return u, p, n


@pytest.fixture(scope="module")
def inputs():
    """x, and the seed rows of the launch as the second backward layer passes
    them: slot >= 0 on a few nodes of both blocks, ``seed`` added to their rows."""
    gen = torch.Generator().manual_seed(5)
    x = (0.1 * torch.randn(N, D, generator=gen)).cuda()
    nodes = torch.randperm(N, generator=gen)[:97]
    slot = torch.full((N,), -1, dtype=torch.int32)
    slot[nodes] = torch.arange(97, dtype=torch.int32)
    seed = torch.randn(97, D, generator=gen).cuda()
    return x, slot.cuda(), seed


def launch(g, eng, inputs, x, mask, entry, blocks=0, row_mask=None, dim=D):
    """One launch of the second backward layer's shape (PRESCALED, seed,
    xs_out, no out): 'masked' = mirec_propagate_sweep_wave_masked, 'paced' =
    mirec_propagate_sweep_wave_paced, 'rows' = mirec_propagate."""
    from furusato_recommend_amd import _lib
    from furusato_recommend_amd._lib import IN_PRESCALED, check, lib
    _, slot, seed = inputs
    xs = torch.full((N, dim), 7.0, device="cuda")
    p = _lib.Prop()
    p.dim, p.in_mode, p.divisor, p.narrow_max = dim, IN_PRESCALED, 1.0, 64
    p.x_in, p.xs_out = x.data_ptr(), xs.data_ptr()
    if dim == D:
        p.slot, p.seed = slot.data_ptr(), seed.data_ptr()
    p.in_mask = mask.data_ptr() if mask is not None else None
    p.row_mask = row_mask.data_ptr() if row_mask is not None else None
    wi, wu = eng.sweep_wave, eng.sweep_wave_users
    wi, wu = (w.ptr() if w is not None else None for w in (wi, wu))
    pace = eng._pace_struct()
    pace = ctypes.byref(pace) if pace is not None else None
    st = _lib.stream_handle()
    if entry == "masked":
        check(lib.mirec_propagate_sweep_wave_masked(g.csr_ptr(), ctypes.byref(p), wi, wu, pace,
                                                    blocks, st), "propagate")
    elif entry == "paced":
        check(lib.mirec_propagate_sweep_wave_paced(g.csr_ptr(), ctypes.byref(p), wi, wu, pace, st),
              "propagate")
    else:
        check(lib.mirec_propagate(g.csr_ptr(), ctypes.byref(p), st), "propagate")
    torch.cuda.synchronize()
    return xs


def neighbours(g, rows):
    rp, col = g.rowptr_host, g.col_host
    return np.unique(np.concatenate([col[rp[r]:rp[r + 1]] for r in rows] or [np.empty(0, int)]))


def masks(g, eng):
    """name -> byte map over the nodes (uint8 [N], on the device)."""
    out = {"all": np.ones(N, np.uint8), "empty": np.zeros(N, np.uint8)}
    for name, node in (("one_user", 1234), ("one_item", NU + 321)):
        out[name] = np.zeros(N, np.uint8)
        out[name][node] = 1
    eng.compute_frontier(*triples(g, 0))
    torch.cuda.synchronize()
    out["frontier"] = eng.bm_hop.view(torch.uint8)[:N].cpu().numpy().copy()
    assert 0 < out["frontier"][:NU].sum() < NU and 0 < out["frontier"][NU:].sum() < MI
    # every set node in the last band of its block: the first slot of nearly
    # every batch fails and whole bands carry no passing entry
    last = np.zeros(N, np.uint8)
    last[(NU - 1) // BAND_I * BAND_I:NU] = 1
    last[NU + (MI - 1) // BAND_U * BAND_U:] = 1
    out["last_band"] = last
    # every stream that wave 3 of workgroup 0 walks, in both blocks, is left
    # without a passing entry: no source of its rows is set
    hollow = np.ones(N, np.uint8)
    for lay in (eng.sweep_wave, eng.sweep_wave_users):
        d = lay.desc
        rows = [d.row0 + t * d.tile_rows + 3 * d.wave_rows + i
                for t in range(0, d.n_tiles, d.grid) for i in range(d.wave_rows)
                if 3 * d.wave_rows + i < d.tile_rows
                and t * d.tile_rows + 3 * d.wave_rows + i < d.n_rows]
        assert rows
        hollow[neighbours(g, rows)] = 0
    out["hollow_wave"] = hollow
    return {k: torch.from_numpy(v).cuda() for k, v in out.items()}


@pytest.mark.parametrize("grid", [1, 2, 16])
@pytest.mark.parametrize("tile", [8, 196, 280])
def test_masked_sweep_equals_the_sweep_of_zeroed_rows(graph, inputs, tile, grid):
    g, x = graph, inputs[0]
    for paced, tile_users in [(p, t) for t in ((8, 7) if tile == 8 else (tile,))
                              for p in (False, True)]:
        eng = make_engine(g, tile, grid, pace=PACE if paced else None, tile_users=tile_users)
        assert eng.sweep_wave.desc.row_bits > 0 and eng.sweep_wave_users.desc.row_bits > 0
        assert eng.sweep_wave.desc.n_rows % tile != 0
        assert tile_users == 8 or eng.sweep_wave_users.desc.n_rows % tile_users != 0
        plain = launch(g, eng, inputs, x, None, "paced")
        for name, m in masks(g, eng).items():
            keep = m.bool()[:, None]
            x_nan = torch.where(keep, x, torch.full_like(x, float("nan")))
            x_zero = torch.where(keep, x, torch.zeros_like(x))
            ref = launch(g, eng, inputs, x_zero, None, "paced")
            rows = launch(g, eng, inputs, x_nan, m, "rows")
            assert not torch.isnan(ref).any() and not torch.isnan(rows).any()
            if name == "all":
                assert torch.equal(ref, plain)
            for blocks in (ITEMS, USERS, BOTH):
                got = launch(g, eng, inputs, x_nan, m, "masked", blocks)
                for block, lo, hi in ((USERS, 0, NU), (ITEMS, NU, N)):
                    want = ref if blocks & block else rows
                    assert torch.equal(got[lo:hi], want[lo:hi]), (name, paced, blocks, block)
            if paced:  # the last workgroup to leave zeroed its region
                assert int(eng._pace_ws.abs().sum()) == 0


def test_the_masked_sweep_ran(graph, inputs):
    """The swept rows differ from the row kernel's somewhere (wide rows are
    summed in another order): the exact cases above did not compare the row
    kernel with itself."""
    g, x = graph, inputs[0]
    eng = make_engine(g)
    m = masks(g, eng)["frontier"]
    rows = launch(g, eng, inputs, x, m, "rows")
    both = launch(g, eng, inputs, x, m, "masked", BOTH)
    assert not torch.equal(both[:NU], rows[:NU]) or not torch.equal(both[NU:], rows[NU:])
    assert torch.allclose(both, rows, rtol=0, atol=1e-5)


def test_against_the_row_kernel_in_fp64(graph, inputs):
    """Both kernels sum the same fp32 terms in a different order; against the
    fp64 sum of those terms the masked sweep's max|err| / max|ref| must not
    exceed twice the row kernel's."""
    g, (x, slot, seed) = graph, inputs
    eng = make_engine(g)
    m = masks(g, eng)["frontier"]
    rp = torch.from_numpy(g.rowptr_host.astype(np.int64))
    col = torch.from_numpy(g.col_host.astype(np.int64))
    row = torch.repeat_interleave(torch.arange(N), rp[1:] - rp[:-1])
    x64 = x.double().cpu() * m.cpu().double()[:, None]
    s = torch.zeros(N, D, dtype=torch.float64).index_add_(0, row, x64[col])
    dinv = g.dinv.double().cpu()[:, None]
    z = dinv * s
    sl = slot.cpu().long()
    z[sl >= 0] += seed.double().cpu()[sl[sl >= 0]]
    ref = dinv * z

    def rel(a):
        return float((a.double().cpu() - ref).abs().max() / ref.abs().max())
    e_rows = rel(launch(g, eng, inputs, x, m, "rows"))
    e_sweep = rel(launch(g, eng, inputs, x, m, "masked", BOTH))
    print(f"fp64: row kernel rel {e_rows:.3e}, masked sweep rel {e_sweep:.3e}")
    assert e_sweep <= 2 * e_rows


def test_blocks_0_and_unqualified_launches_are_the_row_kernel(graph, inputs):
    """blocks == 0, a row_mask and d != 64 run the old launch, bitwise
    mirec_propagate; 8-byte slots run the masked sweep, bitwise the packed one."""
    g, x = graph, inputs[0]
    eng = make_engine(g)
    m = masks(g, eng)["frontier"]
    rows = launch(g, eng, inputs, x, m, "rows")
    assert torch.equal(launch(g, eng, inputs, x, m, "masked", 0), rows)
    assert torch.equal(launch(g, eng, inputs, x, m, "paced"), rows)
    rm = (torch.arange(N, device="cuda") % 3 != 0).to(torch.uint8)
    a = launch(g, eng, inputs, x, m, "masked", BOTH, row_mask=rm)
    assert torch.equal(a, launch(g, eng, inputs, x, m, "rows", row_mask=rm))
    assert torch.equal(a[rm == 0], torch.full_like(a[rm == 0], 7.0))
    e8 = make_engine(g, packed=False)
    assert e8.sweep_wave.desc.row_bits == 0
    assert torch.equal(launch(g, e8, inputs, x, m, "masked", BOTH),
                       launch(g, eng, inputs, x, m, "masked", BOTH))
    x32 = x[:, :32].contiguous()
    a = launch(g, eng, inputs, x32, m, "masked", BOTH, dim=32)
    assert torch.equal(a, launch(g, eng, inputs, x32, m, "rows", dim=32))
    # an unknown block bit is refused
    with pytest.raises(Exception):
        launch(g, eng, inputs, x, m, "masked", 4)


def run_steps(g, L, inmask, n_steps=2, dropout=None, dim=D, **kw):
    """(losses, table, exp_avg, exp_avg_sq) after ``n_steps`` training steps."""
    from furusato_recommend_amd.engine import AdamState
    eng = make_engine(g, L=L, pace=PACE, dim=dim, **kw)
    eng.sweep_inmask = inmask
    torch.manual_seed(0)
    emb = (0.1 * torch.randn(g.n_nodes, dim)).cuda()
    adam = AdamState(emb, lr=1e-2)
    losses = []
    for s in range(n_steps):
        drop = (dropout, 11 + s) if dropout is not None else None
        losses.append(eng.train_step(emb, adam, *triples(g, s), 1e-4, dropout=drop).clone())
    torch.cuda.synchronize()
    return torch.stack(losses).reshape(-1), emb, adam.exp_avg, adam.exp_avg_sq


def replay_fp64(ds, g, L, n_steps=2):
    """The same steps in float64 on the CPU (oracle.lightgcn_oracle's loss,
    torch.optim.Adam)."""
    from oracle import lightgcn_oracle as O
    torch.manual_seed(0)
    emb = torch.nn.Parameter((0.1 * torch.randn(g.n_nodes, D)).double())
    ei = O.edge_index(ds.trainUser, ds.trainItem, NU)
    div = O.degree_div(ei, N).double()
    opt = torch.optim.Adam([emb], lr=1e-2)
    losses = []
    for s in range(n_steps):
        u, p, n = (t.cpu().long() for t in triples(g, s))
        opt.zero_grad()
        loss, reg = O.bpr_loss(emb, ei, NU, L, u, p, n, div)
        loss = loss + 1e-4 * reg
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    st = opt.state[emb]
    return torch.stack(losses), emb.detach(), st["exp_avg"], st["exp_avg_sq"]


@pytest.mark.parametrize("L", [2, 3])
def test_two_training_steps_both_against_off(dataset, graph, L):
    """Loss, table and both moments of two steps with the switch 'both' lie as
    close to a float64 replay as twice what 'off' (the row kernel) does."""
    ref = replay_fp64(dataset, graph, L)
    off = run_steps(graph, L, "off")
    both = run_steps(graph, L, "both")
    assert not all(torch.equal(a, b) for a, b in zip(off, both))
    for name, r, a, b in zip(("loss", "table", "exp_avg", "exp_avg_sq"), ref, off, both):
        scale = float(r.abs().max())
        e_off = float((a.double().cpu() - r).abs().max()) / scale
        e_both = float((b.double().cpu() - r).abs().max()) / scale
        print(f"L={L} {name}: off rel {e_off:.3e}, both rel {e_both:.3e}")
        assert e_both <= 2 * e_off, name


@pytest.mark.parametrize("L", [2, 3])
def test_steps_with_off_equal_mirec_propagate_bitwise(graph, monkeypatch, L):
    """With 'off' the masked entry is never called, and every array of two
    steps equals, bit for bit, the steps whose in-masked launch goes through
    mirec_propagate itself (what the launch ran before the switch existed)."""
    from furusato_recommend_amd import engine
    calls = []

    def never(*a):
        raise AssertionError("the masked entry ran with sweep_inmask = 'off'")
    monkeypatch.setattr(engine.lib, "mirec_propagate_sweep_wave_masked", never, raising=False)
    off = run_steps(graph, L, "off")

    def rows(csr, p, items, users, pace, blocks, stream):
        calls.append(blocks)
        return engine.lib.mirec_propagate(csr, p, stream)
    monkeypatch.setattr(engine.lib, "mirec_propagate_sweep_wave_masked", rows, raising=False)
    via_rows = run_steps(graph, L, "both")
    assert calls == [BOTH, BOTH]  # one in-masked launch per step
    for a, b in zip(off, via_rows):
        assert torch.equal(a, b)


@pytest.mark.parametrize("case", ["dim32", "weighted", "dropout"])
def test_steps_that_do_not_qualify_equal_off_bitwise(dataset, graph, case):
    from furusato_recommend_amd.graph import Graph
    g, kw = graph, {}
    if case == "weighted":
        ds = dataset
        w = np.random.default_rng(3).uniform(0.5, 2.0, len(ds.trainUser)).astype(np.float32)
        g = Graph.from_interactions(ds.trainUser, ds.trainItem, NU, MI, "cuda:0", weight=w)
    elif case == "dim32":
        kw = dict(dim=32)
    else:
        kw = dict(dropout=0.7)
    off = run_steps(g, 3, "off", **kw)
    both = run_steps(g, 3, "both", **kw)
    for a, b in zip(off, both):
        assert torch.equal(a, b)


def test_steps_with_8_byte_slots_and_in_the_group_form_equal_the_packed_wave_form(graph):
    """8-byte slots decode to the same slots; the group form (item rows swept,
    user rows by the row kernel) borrows the wave form's item layout for its
    in-masked launch: with "items" all three train to the same bits."""
    from furusato_recommend_amd.engine import AdamState
    outs = []
    for form, packed in (("wave", True), ("wave", False), ("group", True)):
        eng = make_engine(graph, packed=packed)
        eng.set_sweep_sizes(200, 7, 256, wave_items=(200, BAND_I), wave_users=(100, BAND_U),
                            max_grid=8)
        eng.sweep_form, eng.sweep_users, eng.sweep_inmask = form, False, "items"
        assert eng.sweep_wave is not None and (form == "wave" or eng.sweep is not None)
        torch.manual_seed(0)
        emb = (0.1 * torch.randn(graph.n_nodes, D)).cuda()
        adam = AdamState(emb, lr=1e-2)
        for s in range(2):
            eng.train_step(emb, adam, *triples(graph, s), 1e-4)
        torch.cuda.synchronize()
        outs.append((emb, adam.exp_avg, adam.exp_avg_sq))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)


def test_step_captured_and_replayed_twice(graph):
    """A step with the switch 'both' captured and replayed twice, against the
    same three steps run eagerly (the fused Adam's scalars are launch
    arguments: both replays are step 2)."""
    from furusato_recommend_amd.engine import AdamState
    g, outs = graph, []
    t = triples(g, 0)
    for captured in (False, True):
        eng = make_engine(g, pace=PACE)
        eng.sweep_inmask = "both"
        torch.manual_seed(0)
        emb = (0.1 * torch.randn(g.n_nodes, D)).cuda()
        adam = AdamState(emb, lr=1e-2)
        eng.train_step(emb, adam, *t, 1e-4)
        torch.cuda.synchronize()
        if captured:
            graph_ = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph_):
                eng.train_step(emb, adam, *t, 1e-4)
            graph_.replay()
            graph_.replay()
        else:
            for _ in range(2):
                adam.n_steps = 1
                eng.train_step(emb, adam, *t, 1e-4)
        torch.cuda.synchronize()
        outs.append((emb, adam.exp_avg, adam.exp_avg_sq))
        assert int(eng._pace_ws.abs().sum()) == 0
    for a, b in zip(*outs):
        assert torch.equal(a, b)
