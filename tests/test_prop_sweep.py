"""Column sweep of the item rows (prop_sweep_kernel, csrc/prop.hip): with the
engine switch ``use_sweep`` on, full PRESCALED launches gather the item rows in
ascending source column through LDS accumulators; off, every row goes through
the row kernel.  Only the summation order differs, so both agree to the 1e-5
that tests/test_gpu_parity.py uses for such pairs, the sweep is deterministic,
and launches or graphs that do not qualify are bit-identical either way.

Small graphs with the tile, group and band sizes forced small, so that the
sweep spans many bands, several tiles (the last one ragged) and several rows
per lane group."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-5  # summation order only (tests/test_gpu_parity.py)
D, L = 64, 3


def rel(a, b):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def host_forward(g, x, n_layers):
    """(x_0 + ... + x_L) / (L + 1), x_l = D^-1/2 A D^-1/2 x_{l-1}, in float64."""
    rp, col = g.rowptr_host, g.col_host
    deg = np.diff(rp).astype(np.float64)
    dinv = np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1.0)), 0.0)[:, None]
    rows = np.repeat(np.arange(g.n_nodes), np.diff(rp))
    cur = x.astype(np.float64)
    acc = cur.copy()
    for _ in range(n_layers):
        y = np.zeros_like(cur)
        np.add.at(y, rows, (dinv * cur)[col])
        cur = dinv * y
        acc += cur
    return acc / (n_layers + 1)


def make_engine(u, i, nu, mi, sizes, dim=D, layers=L, split=None, batch=64):
    from furusato_recommend_amd.engine import PropagationEngine
    from furusato_recommend_amd.graph import DEFAULT_SPLIT, Graph
    g = Graph.from_interactions(u, i, nu, mi, "cuda:0",
                                split=DEFAULT_SPLIT if split is None else split)
    eng = PropagationEngine(g, dim, layers, batch)
    if sizes is not None:
        eng.set_sweep_sizes(*sizes)
    return g, eng


@pytest.fixture(scope="module")
def uniform():
    from furusato_recommend_amd import SyntheticBipartite
    ds = SyntheticBipartite(3000, 700, 40000, seed=1, test_frac=0)
    nu, mi = ds.n_users, ds.m_items
    # 200-row tiles (4 tiles, the last of 100 rows), 7 rows per group (29
    # groups, the last of 4 rows), 256-user bands (12 bands)
    g, eng = make_engine(ds.trainUser, ds.trainItem, nu, mi, (200, 7, 256))
    d = eng.sweep.desc
    assert d.n_tiles >= 3 and d.group_rows > 1 and -(-nu // d.band_rows) >= 10
    torch.manual_seed(0)
    x = (0.1 * torch.randn(nu + mi, D)).cuda()
    return g, eng, x, host_forward(g, x.cpu().numpy(), L)


def hand_graph():
    """37 users x 11 items: item 0 has no edges, item 1 only users of the band
    [8, 16), item 2 the same user twice; neither count is a multiple of the
    band (8) or tile (4) size."""
    rng = np.random.default_rng(2)
    u = [9, 12, 8, 15, 12] + [3, 20, 3, 36] + rng.integers(0, 37, 60).tolist()
    i = [1] * 5 + [2] * 4 + rng.integers(3, 11, 60).tolist()
    return np.array(u), np.array(i), 37, 11


def forward_pair(eng, x):
    eng.use_sweep = True
    eng.invalidate_prescaled()
    on = eng.forward(x).clone()
    eng.use_sweep = False
    eng.invalidate_prescaled()
    off = eng.forward(x).clone()
    eng.use_sweep = True
    torch.cuda.synchronize()
    return on, off


def test_forward_matches_row_kernel_and_float64(uniform):
    g, eng, x, ref = uniform
    on, off = forward_pair(eng, x)
    r_pair, r_ref, r_off = rel(on, off), rel(on, ref), rel(off, ref)
    print(f"sweep vs row kernel {r_pair:.2e}; vs float64: sweep {r_ref:.2e}, rows {r_off:.2e}")
    assert not torch.equal(on[g.n_users:], off[g.n_users:])  # the sweep did run
    assert r_pair < TOL and r_ref < TOL


def test_forward_hand_built_graph():
    u, i, nu, mi = hand_graph()
    g, eng = make_engine(u, i, nu, mi, (4, 2, 8))
    assert eng.sweep.desc.n_tiles == 3 and eng.sweep.desc.groups == 2
    torch.manual_seed(1)
    x = torch.randn(nu + mi, D).cuda()
    on, off = forward_pair(eng, x)
    ref = host_forward(g, x.cpu().numpy(), L)
    r_pair, r_ref = rel(on, off), rel(on, ref)
    print(f"hand graph: sweep vs row kernel {r_pair:.2e}, vs float64 {r_ref:.2e}")
    assert r_pair < TOL and r_ref < TOL
    # the empty item's layers are zero: its output is x_0 / (L + 1) exactly as before
    assert torch.equal(on[nu], off[nu])


def train_two_steps(uniform_ds, use_sweep):
    from furusato_recommend_amd.engine import AdamState, sample_triples
    ds, sizes = uniform_ds
    g, eng = make_engine(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, sizes)
    eng.use_sweep = use_sweep
    torch.manual_seed(0)
    emb = (0.1 * torch.randn(g.n_nodes, D)).cuda()
    adam = AdamState(emb, lr=1e-2)
    B = 64
    u = torch.empty(B, dtype=torch.int32, device="cuda")
    p, n = torch.empty_like(u), torch.empty_like(u)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    losses = []
    for s in range(2):
        sample_triples(g, B, 0, s * B, u, p, n, err)
        losses.append(float(eng.train_step(emb, adam, u, p, n, 1e-4)))
    torch.cuda.synchronize()
    return emb, adam.exp_avg, adam.exp_avg_sq, losses


def test_training_and_determinism():
    from furusato_recommend_amd import SyntheticBipartite
    ds = (SyntheticBipartite(3000, 700, 40000, seed=1, test_frac=0), (200, 7, 256))
    on = train_two_steps(ds, True)
    on2 = train_two_steps(ds, True)
    off = train_two_steps(ds, False)
    for name, a, b in zip(("table", "exp_avg", "exp_avg_sq"), on, off):
        r = rel(a, b)
        print(f"train {name}: sweep vs row kernel {r:.2e}")
        assert r < TOL
    print("losses", on[3], off[3])
    assert np.allclose(on[3], off[3], rtol=1e-5, atol=0)
    for a, b in zip(on[:3], on2[:3]):  # determinism: the same bits twice
        assert torch.equal(a, b)
    assert on[3] == on2[3]


def test_forward_determinism(uniform):
    _, eng, x, _ = uniform
    a = eng.forward(x).clone()
    eng.invalidate_prescaled()
    b = eng.forward(x).clone()
    assert torch.equal(a, b)


def test_fallback_long_row():
    u, i, nu, mi = hand_graph()
    g, eng = make_engine(u, i, nu, mi, (4, 2, 8), split=4)
    assert g.n_long > 0 and eng.sweep is None
    x = torch.randn(nu + mi, D).cuda()
    on, off = forward_pair(eng, x)
    assert torch.equal(on, off)


def test_fallback_edge_index_graph():
    from furusato_recommend_amd.engine import PropagationEngine
    from furusato_recommend_amd.graph import Graph
    u, i, nu, mi = hand_graph()
    ei = np.stack([np.concatenate([u, nu + i]), np.concatenate([nu + i, u])])
    g = Graph.from_edge_index(ei, nu + mi, "cuda:0")
    eng = PropagationEngine(g, D, L, 8)
    eng.set_sweep_sizes(4, 2, 8)
    assert eng.sweep is None
    x = torch.randn(nu + mi, D).cuda()
    on, off = forward_pair(eng, x)
    assert torch.equal(on, off)


@pytest.mark.parametrize("dim", [4, 8, 16, 32, 128, 256])
def test_fallback_other_widths(dim):
    """Widths without a sweep kernel (only d = 64 has one) run the row kernel."""
    u, i, nu, mi = hand_graph()
    g, eng = make_engine(u, i, nu, mi, (4, 2, 8), dim=dim)
    assert eng.sweep is None
    x = torch.randn(nu + mi, dim).cuda()
    on, off = forward_pair(eng, x)
    assert torch.equal(on, off)
