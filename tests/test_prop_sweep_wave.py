"""The per-wave form of the column sweep (prop_sweep_wave_kernel, csrc/prop.hip;
engine switches ``sweep_form`` and ``sweep_users``).

Item rows: both forms add a row's terms one at a time in ascending source
column, so the wave form equals the group form bit for bit.  User rows
(``sweep_users``): the same kernel over a layout with ``src0 = n_users``, in
several passes; against the row kernel only the summation order differs
(1e-5, as tests/test_gpu_parity.py and test_prop_sweep.py).  Launches and
graphs that do not qualify are bit-identical whatever the switches say.

Small graphs with the sizes forced small: several tiles (a ragged last one),
waves with several rows, at least 10 bands, and a capped grid so that the
user tiles take 4 passes, the last one ragged."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-5  # summation order only (tests/test_gpu_parity.py)
D, L = 64, 3
# group form (tile, rows per group, band); wave form (tile, band) per block
GROUP = (200, 7, 256)
WAVE = dict(wave_items=(200, 256), wave_users=(100, 64), max_grid=8)


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


def make_engine(u, i, nu, mi, group=None, wave=None, dim=D, split=None, batch=64, **graph_kw):
    from furusato_recommend_amd.engine import PropagationEngine
    from furusato_recommend_amd.graph import DEFAULT_SPLIT, Graph
    g = Graph.from_interactions(u, i, nu, mi, "cuda:0",
                                split=DEFAULT_SPLIT if split is None else split, **graph_kw)
    eng = PropagationEngine(g, dim, L, batch)
    eng.sweep_form = "wave"
    eng.sweep_users = True
    if group is not None:
        eng.set_sweep_sizes(*group, **(wave or {}))
    return g, eng


def forward(eng, x, form="wave", users=False, use_sweep=True):
    eng.use_sweep, eng.sweep_form, eng.sweep_users = use_sweep, form, users
    eng.invalidate_prescaled()
    out = eng.forward(x).clone()
    torch.cuda.synchronize()
    eng.use_sweep = True
    return out


def hand_graph():
    """37 users x 11 items: item 0 has no edges, item 1 only users of the band
    [8, 16), item 2 the same user twice; neither count is a multiple of the
    band (8) or tile (4) size."""
    rng = np.random.default_rng(2)
    u = [9, 12, 8, 15, 12] + [3, 20, 3, 36] + rng.integers(0, 37, 60).tolist()
    i = [1] * 5 + [2] * 4 + rng.integers(3, 11, 60).tolist()
    return np.array(u), np.array(i), 37, 11


HAND = dict(group=(4, 2, 8), wave=dict(wave_items=(4, 8), wave_users=(10, 2), max_grid=2))


@pytest.fixture(scope="module")
def dataset():
    from furusato_recommend_amd import SyntheticBipartite
    return SyntheticBipartite(3000, 700, 40000, seed=1, test_frac=0)


@pytest.fixture(scope="module")
def uniform(dataset):
    ds = dataset
    nu, mi = ds.n_users, ds.m_items
    g, eng = make_engine(ds.trainUser, ds.trainItem, nu, mi, GROUP, WAVE)
    wi, wu = eng.sweep_wave.desc, eng.sweep_wave_users.desc
    assert wi.n_tiles == 4 and wi.wave_rows == 25 and -(-nu // wi.band_rows) >= 10
    # 30 user tiles on 8 workgroups: 4 passes, 6 tiles in the last; 11 bands
    assert wu.n_tiles == 30 and wu.grid == 8 and wu.src0 == nu and -(-mi // wu.band_rows) >= 10
    torch.manual_seed(0)
    x = (0.1 * torch.randn(nu + mi, D)).cuda()
    outs = {"ref": host_forward(g, x.cpu().numpy(), L),
            "rows": forward(eng, x, use_sweep=False),
            "group": forward(eng, x, "group"),
            "wave": forward(eng, x, "wave"),
            "both": forward(eng, x, "wave", users=True)}
    return g, eng, x, outs


def test_item_rows_bitwise_equal_to_group_form(uniform):
    g, _, _, o = uniform
    assert not torch.equal(o["wave"][g.n_users:], o["rows"][g.n_users:])  # the sweep did run
    assert torch.equal(o["wave"], o["group"])


def test_item_rows_hand_built_graph():
    u, i, nu, mi = hand_graph()
    g, eng = make_engine(u, i, nu, mi, **HAND)
    assert eng.sweep_wave.desc.n_tiles == 3 and eng.sweep_wave.desc.wave_rows == 1
    torch.manual_seed(1)
    x = torch.randn(nu + mi, D).cuda()
    wave, group, rows = (forward(eng, x, "wave"), forward(eng, x, "group"),
                         forward(eng, x, use_sweep=False))
    assert torch.equal(wave, group)
    assert torch.equal(wave[nu], rows[nu])  # the empty item: x_0 / (L + 1) exactly
    both = forward(eng, x, "wave", users=True)
    ref = host_forward(g, x.cpu().numpy(), L)
    r_pair, r_ref = rel(both, rows), rel(both, ref)
    print(f"hand graph, both blocks: vs row kernel {r_pair:.2e}, vs float64 {r_ref:.2e}")
    assert r_pair < TOL and r_ref < TOL


def test_user_block_matches_row_kernel_and_float64(uniform):
    g, _, _, o = uniform
    r_pair, r_ref, r_rows = rel(o["both"], o["rows"]), rel(o["both"], o["ref"]), \
        rel(o["rows"], o["ref"])
    print(f"both blocks vs row kernel {r_pair:.2e}; vs float64: swept {r_ref:.2e}, "
          f"rows {r_rows:.2e}")
    assert not torch.equal(o["both"][:g.n_users], o["rows"][:g.n_users])  # the path ran
    assert not torch.equal(o["both"][:g.n_users], o["wave"][:g.n_users])
    assert r_pair < TOL and r_ref < TOL


def train_two_steps(ds, form, users, use_sweep=True):
    from furusato_recommend_amd.engine import AdamState, sample_triples
    g, eng = make_engine(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, GROUP, WAVE)
    eng.use_sweep, eng.sweep_form, eng.sweep_users = use_sweep, form, users
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


@pytest.fixture(scope="module")
def trained(dataset):
    return {"rows": train_two_steps(dataset, "group", False, use_sweep=False),
            "group": train_two_steps(dataset, "group", False),
            "wave": train_two_steps(dataset, "wave", False),
            "both": train_two_steps(dataset, "wave", True)}


def test_training_item_rows_bitwise_equal_to_group_form(trained):
    """Two steps, the fused-Adam launch's table and moments included: with the
    item rows equal bit for bit and the user rows from the same row kernel,
    everything is."""
    for a, b in zip(trained["wave"][:3], trained["group"][:3]):
        assert torch.equal(a, b)
    assert trained["wave"][3] == trained["group"][3]


def test_training_user_block(trained):
    for name, a, b in zip(("table", "exp_avg", "exp_avg_sq"), trained["both"], trained["rows"]):
        r = rel(a, b)
        print(f"train {name}: both blocks swept vs row kernel {r:.2e}")
        assert r < TOL
    assert not torch.equal(trained["both"][0], trained["wave"][0])  # the user path ran
    assert np.allclose(trained["both"][3], trained["rows"][3], rtol=1e-5, atol=0)


def test_determinism(uniform, trained, dataset):
    _, eng, x, o = uniform
    assert torch.equal(forward(eng, x, "wave", users=True), o["both"])
    assert torch.equal(forward(eng, x, "wave"), o["wave"])
    again = train_two_steps(dataset, "wave", True)
    for a, b in zip(again[:3], trained["both"][:3]):
        assert torch.equal(a, b)
    assert again[3] == trained["both"][3]


def assert_switches_do_nothing(eng, x):
    rows = forward(eng, x, use_sweep=False)
    for form, users in (("group", False), ("wave", False), ("wave", True)):
        assert torch.equal(forward(eng, x, form, users), rows)


def test_fallback_long_row():
    u, i, nu, mi = hand_graph()
    g, eng = make_engine(u, i, nu, mi, split=4, **HAND)
    assert g.n_long > 0 and eng.sweep_wave is None and eng.sweep_wave_users is None
    assert_switches_do_nothing(eng, torch.randn(nu + mi, D).cuda())


def test_fallback_edge_index_graph():
    from furusato_recommend_amd.engine import PropagationEngine
    from furusato_recommend_amd.graph import Graph
    u, i, nu, mi = hand_graph()
    ei = np.stack([np.concatenate([u, nu + i]), np.concatenate([nu + i, u])])
    g = Graph.from_edge_index(ei, nu + mi, "cuda:0")
    eng = PropagationEngine(g, D, L, 8)
    eng.sweep_form, eng.sweep_users = "wave", True
    eng.set_sweep_sizes(*HAND["group"], **HAND["wave"])
    assert eng.sweep_wave is None and eng.sweep_wave_users is None
    assert_switches_do_nothing(eng, torch.randn(nu + mi, D).cuda())


@pytest.mark.parametrize("dim", [32, 128])
def test_fallback_other_widths(dim):
    u, i, nu, mi = hand_graph()
    g, eng = make_engine(u, i, nu, mi, dim=dim, **HAND)
    assert eng.sweep_wave is None and eng.sweep_wave_users is None
    assert_switches_do_nothing(eng, torch.randn(nu + mi, dim).cuda())


def test_fallback_weighted_graph():
    u, i, nu, mi = hand_graph()
    w = np.random.default_rng(3).uniform(0.5, 2.0, len(u)).astype(np.float32)
    g, eng = make_engine(u, i, nu, mi, weight=w, **HAND)
    assert g.val is not None and eng.sweep_wave is None and eng.sweep_wave_users is None
    assert_switches_do_nothing(eng, torch.randn(nu + mi, D).cuda())


def test_item_block_inside_l2_gets_no_user_layout():
    """Default sizes: 17 000 user rows (4.35 MB) exceed one L2, so the item
    rows are swept; 300 item rows (77 KB) fit, so the user rows are not."""
    from furusato_recommend_amd import SyntheticBipartite
    ds = SyntheticBipartite(17000, 300, 60000, seed=3, test_frac=0)
    g, eng = make_engine(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items)
    assert eng.sweep is not None and eng.sweep_wave is not None
    assert eng.sweep_wave_users is None
    x = (0.1 * torch.randn(g.n_nodes, D)).cuda()
    wave = forward(eng, x, "wave")
    assert torch.equal(forward(eng, x, "wave", users=True), wave)
    assert torch.equal(wave, forward(eng, x, "group"))
    assert not torch.equal(wave, forward(eng, x, use_sweep=False))
