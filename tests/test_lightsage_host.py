"""Host checks of tests/lightsage_common.py (no device): the two restatements
of the hop agree, the closed-form backward is float64 autograd's, the tree
forward at a covering fanout is the dense full-graph form, the case lists
contain what tests/test_lightsage_kernels.py claims, and the package names the
hop (header, binding, registry)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import dropout_common as dc
from tests import gat_common as gc
from tests import lightsage_common as lc
from tests.conftest import ROOT

CASES = lc.kernel_cases()
SMALL = [i for i, c in enumerate(CASES) if c["n_t"] * c["k"] * c["dim"] <= 37 * 25 * 64]
SYMBOLS = ("mirec_fanout_resmean_gather", "mirec_fanout_resmean", "mirec_fanout_resmean_bwd")


def _inputs(c):
    rng = np.random.default_rng([c["n_t"], c["k"], c["dim"], 3])
    n_t, k, dim = c["n_t"], c["k"], c["dim"]
    xs = rng.standard_normal((n_t, dim)).astype(np.float32)
    xc = rng.standard_normal((n_t * k, dim)).astype(np.float32)
    g = rng.standard_normal((n_t, dim)).astype(np.float32)
    mask, scale = dc.fanout_mask(c["p"], c["seed"], n_t * k, dim)
    return xs, xc, g, dc.fanout_ids(c), mask, scale


@pytest.mark.parametrize("i", SMALL)
def test_the_two_restatements_agree(i):
    c = CASES[i]
    xs, xc, _, valid, mask, scale = _inputs(c)
    a, A, cnt = lc.hop_loop(xs, xc, valid, c["k"], mask, scale)
    b = lc.hop_edges(torch.from_numpy(xs).double(), torch.from_numpy(xc).double(), valid, c["k"],
                     mask, scale).numpy()
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(a).max())
    assert np.array_equal(cnt, (valid >= 0).reshape(c["n_t"], c["k"]).sum(1))
    assert (A >= np.abs(a) - 1e-12).all()
    # valid = None: every slot counts
    a0, _, cnt0 = lc.hop_loop(xs, xc, None, c["k"], mask, scale)
    b0 = lc.hop_edges(torch.from_numpy(xs).double(), torch.from_numpy(xc).double(), None, c["k"],
                      mask, scale).numpy()
    assert np.abs(a0 - b0).max() <= 1e-12 * max(1.0, np.abs(a0).max()) and (cnt0 == c["k"]).all()
    # a target without a valid child keeps its self row
    none = cnt == 0
    assert np.array_equal(a[none], xs[none].astype(np.float64))


@pytest.mark.parametrize("i", SMALL)
def test_closed_form_backward_is_autograd(i):
    c = CASES[i]
    xs, xc, g, valid, mask, scale = _inputs(c)
    ts = torch.from_numpy(xs).double().requires_grad_(True)
    tc = torch.from_numpy(xc).double().requires_grad_(True)
    out = lc.hop_edges(ts, tc, valid, c["k"], mask, scale)
    gs, gch = torch.autograd.grad(out, [ts, tc], torch.from_numpy(g).double())
    ws, wc = lc.backward_closed(g, valid, c["k"], mask, scale)
    assert np.abs(gs.numpy() - ws).max() <= 1e-12
    assert np.abs(gch.numpy() - wc).max() <= 1e-12 * max(1.0, np.abs(wc).max())
    assert not wc[valid < 0].any()
    if c["p"] > 0:
        assert (wc[valid >= 0] == 0).any() and (wc[valid >= 0] != 0).any()


def test_bounds_hold_the_float32_rounding_of_the_reference():
    c = CASES[3]
    xs, xc, g, valid, mask, scale = _inputs(c)
    out, A, cnt = lc.hop_loop(xs, xc, valid, c["k"], mask, scale)
    b = lc.fwd_bound(A, cnt)
    assert b.shape == out.shape and (b[A > 0] > 0).all()
    assert (np.abs(out.astype(np.float32) - out) <= b).all()
    assert b.max() <= 1e-5 * np.abs(out).max()        # far inside the model's 1e-4 bar
    _, wc = lc.backward_closed(g, valid, c["k"], mask, scale)
    assert (np.abs(wc.astype(np.float32) - wc) <= lc.bwd_bound(wc)).all()


def test_tree_forward_at_a_covering_fanout_is_the_dense_form():
    u, i, nu, mi = gc.small_graph_edges()
    rowptr, col = gc.host_csr(u, i, nu, mi)
    n, kmax, L = nu + mi, int(np.diff(rowptr).max()), 2
    assert np.diff(rowptr).min() == 0
    depths = [0, 1, 2, 2]                       # SampleTree.canonical_layout(2)
    children = {(0, 1): 1, (1, 2): 2, (0, 2): 3}

    def kids(parents):
        out = np.full((len(parents), kmax), -1, np.int32)
        for r, p in enumerate(parents):
            if p >= 0:
                nb = col[rowptr[p]:rowptr[p + 1]]
                out[r, :len(nb)] = nb
        return out.reshape(-1)

    groups = [np.arange(n, dtype=np.int32), None, None, None]
    groups[1] = kids(groups[0])
    groups[2] = kids(groups[1])
    groups[3] = kids(groups[0])
    table = torch.from_numpy(np.random.default_rng(1).standard_normal((n, 8)))
    emb = lc.tree_forward(table, groups, depths, children, L, [kmax, kmax])
    full = lc.dense_full(table, rowptr, col, L)
    assert float((emb - full).abs().max()) <= 1e-12
    # dropout changes it, and the same seed repeats it
    a = lc.tree_forward(table, groups, depths, children, L, [kmax, kmax], 0.3, 7)
    b = lc.tree_forward(table, groups, depths, children, L, [kmax, kmax], 0.3, 7)
    assert torch.equal(a, b) and not torch.equal(a, emb)


def test_case_lists_contain_what_they_claim():
    d4 = {c["dim"] // 4 for c in CASES}
    assert {1, 2, 3, 16, 64, 65, 128} <= d4
    ks = {c["k"] for c in CASES}
    assert {1, 5, 8, 9, 25, 64, 70} <= ks and max(ks) == 70      # across the batch of 8
    assert {c["p"] for c in CASES} == {0.0, 0.3, 0.5}
    assert {c["seed"] for c in CASES} == set(dc.SEEDS) and max(dc.SEEDS) > 1 << 63
    shapes = {(c["n_t"], c["k"], c["dim"]) for c in CASES}
    assert (1, 1, 64) in shapes and (1, 25, 8) in shapes
    assert any(c["n_t"] * c["dim"] // 4 > 256 for c in CASES)    # more than one block
    for c in CASES:
        ids = dc.fanout_ids(c).reshape(c["n_t"], c["k"])
        sid = lc.self_ids(c)
        assert sid[0] == -1 and sid.min() >= -1 and sid.max() < c["n_rows"]
        assert (sid[1:] >= 0).sum() >= c["n_t"] - 2
        if c["n_t"] >= 4:
            assert (ids[0] < 0).all() and (ids[1] >= 0).sum() == 1 and ids[1, -1] >= 0
            assert (ids[2] >= 0).all() and (ids[3] >= 0).all()
            assert c["k"] < 2 or ids[3, -1] == ids[3, 0]
        else:
            assert (ids[0] >= 0).any()           # a -1 self row with a valid child
    extra = CASES[-1]
    assert extra["neg_self"] == (0, 2) and lc.self_ids(extra)[2] == -1
    assert (dc.fanout_ids(extra).reshape(37, 5)[2] >= 0).all()
    assert len(CASES) == len(dc.fanout_cases()) + 1


def test_seed_of_wraps_like_the_device_argument():
    assert lc.seed_of(3, 0, 0) == 3_000_009
    assert lc.seed_of(3, 2, 1) == 3_000_009 + 263
    assert lc.seed_of(1 << 62, 1, 0) == ((1 << 62) * 1_000_003 + 131) % (1 << 64)


def test_the_package_names_the_hop():
    src = open(os.path.join(ROOT, "include", "mirec.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    from furusato_recommend_amd import _lib
    for s in SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", code), s
        assert s in _lib.SIGNATURES and hasattr(_lib.lib, s)
    assert "mirec_fanout_resmean_gather" in src.split("Element index:")[1].split("seed_base")[0]
    mk = open(os.path.join(ROOT, "furusato_recommend_amd", "csrc", "Makefile")).read()
    assert "lightsage.hip" in re.search(r"HIP_SRCS := (.*)", mk).group(1).split()


def test_the_registry_has_the_model():
    import furusato_recommend_amd as pkg
    from furusato_recommend_amd import lightsage
    assert pkg.MODELS["lightsage"] is lightsage.LightSAGE is pkg.LightSAGE
    assert "LightSAGE" in pkg.__all__
    assert lightsage.LightSAGE.HEAVY_SLICE == 1 and lightsage.FUSED_HOP in (True, False)
    assert pkg.MODELS["sage"] is pkg.GraphSAGE and pkg.MODELS["gnn"] is pkg.GNN


def test_config_errors_need_no_device():
    from furusato_recommend_amd import LightSAGE
    with pytest.raises(ValueError, match="one size per layer"):
        LightSAGE({"layer": 2, "fanouts": [3]}, type("D", (), {"n_users": 3, "m_items": 2}))
