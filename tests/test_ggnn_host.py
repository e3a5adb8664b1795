"""Host checks of the gated graph hop's float64 restatement
(tests/ggnn_common.py) and of what the package says about it without a GPU:
the two forms of the gate and of the hop agree, the closed-form backward is
float64 autograd, the bounds and case lists are what the GPU tests assume, and
the model and the C ABI name the new hop."""
import os
import re

import numpy as np
import pytest
import torch

from tests import gat_common as gc
from tests import ggnn_common as gg
from tests.conftest import ROOT

ALL_CASES = gg.CASES + [gg.STRIDE_CASE]
SMALL = [c for c in gg.CASES if c[0] * c[1] <= 33 * 64]


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _cell_inputs(n, d, seed=0, scale=1.0):
    rng = np.random.default_rng([n, d, seed])
    a = rng.standard_normal((n, d)).astype(np.float32).astype(np.float64) * scale
    h = rng.standard_normal((n, d)).astype(np.float32).astype(np.float64) * scale
    return a, h, gg.make_conv(d, seed, scale)


@pytest.mark.parametrize("case", SMALL, ids=str)
@pytest.mark.parametrize("scale", [1.0, 6.0])
def test_the_two_gate_forms_agree(case, scale):
    n, d = case
    a, h, (_, w_ih, w_hh, b_ih, b_hh) = _cell_inputs(n, d, scale=scale)
    gi = a @ w_ih.numpy().T + b_ih.numpy()
    gh = h @ w_hh.numpy().T + b_hh.numpy()
    got = gg.gate_np(gi, gh, h)
    want = gg.cell_torch(_t(a), _t(h), w_ih, w_hh, b_ih, b_hh).numpy()
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert np.array_equal(gg.gate_np(gi, gh, h, relu=True), np.maximum(got, 0.0))


@pytest.mark.parametrize("mode", gc.VALID_MODES)
@pytest.mark.parametrize("shape", [(1, 1, 4), (5, 3, 12), (9, 10, 16)], ids=str)
def test_the_two_hop_forms_agree(shape, mode):
    n_t, k, d = shape
    rng = np.random.default_rng([n_t, k, d, gc.VALID_MODES.index(mode)])
    xc = rng.standard_normal((n_t * k, d))
    xs = rng.standard_normal((n_t, d))
    if mode == "null":
        valid = None
    elif mode == "all":
        valid = rng.integers(0, 99, n_t * k).astype(np.int32)
    elif mode == "none":
        valid = np.full(n_t * k, -1, np.int32)
    else:
        v = rng.integers(0, 99, (n_t, k)).astype(np.int32)
        v[rng.random((n_t, k)) < 0.3] = -1
        v[-1] = -1                              # the last target without a valid child
        valid = v.reshape(-1)
    conv = gg.make_conv(d)
    loop = gg.hop_loop(xc, xs, valid, k, [p.numpy() for p in conv])
    edges = gg.tree_level(_t(xc), _t(xs), valid, k, conv).numpy()
    assert np.abs(loop - edges).max() <= 1e-12 * max(1.0, np.abs(edges).max())
    if mode in ("none", "some"):
        # a target without a valid child: a = 0, the cell on (0, x)
        t = n_t - 1
        _, w_ih, w_hh, b_ih, b_hh = conv
        lone = gg.cell_torch(torch.zeros(1, d, dtype=torch.float64), _t(xs[t:t + 1]), w_ih, w_hh,
                             b_ih, b_hh).numpy()
        assert np.abs(loop[t] - lone[0]).max() <= 1e-12


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", [(3, 12), (33, 64)], ids=str)
def test_closed_form_backward_is_autograd(case, relu):
    n, d = case
    a, h, (_, w_ih, w_hh, b_ih, b_hh) = _cell_inputs(n, d, seed=3, scale=2.0)
    leaves = [x.clone().requires_grad_(True) for x in (_t(a), _t(h), w_ih, w_hh, b_ih, b_hh)]
    out = gg.cell_torch(*leaves)
    if relu:
        out = out.relu()
    g = np.random.default_rng(5).standard_normal((n, d))
    want = torch.autograd.grad(out, leaves, _t(g))
    gi = a @ w_ih.numpy().T + b_ih.numpy()
    gh = h @ w_hh.numpy().T + b_hh.numpy()
    mask = gg.gate_np(gi, gh, h) > 0 if relu else None
    d_gi, d_gh, d_h = gg.backward_closed(g, gi, gh, h, mask)
    got = [d_gi @ w_ih.numpy(), d_h + d_gh @ w_hh.numpy(), d_gi.T @ a, d_gh.T @ h,
           d_gi.sum(0), d_gh.sum(0)]
    for name, x, y in zip(("a", "h", "w_ih", "w_hh", "b_ih", "b_hh"), got, want):
        y = y.numpy()
        assert np.abs(x - y).max() <= 1e-12 * max(1.0, np.abs(y).max()), name


def test_model_forward_is_the_hop_per_level():
    """Two layers on an explicit tree equal the per-level loop form."""
    from furusato_recommend_amd.graphsage import SampleTree
    L, sizes, d = 2, [3, 2], 8
    depths, children = SampleTree.canonical_layout(L)
    rng = np.random.default_rng(1)
    groups = [rng.integers(-1, 20, 4).astype(np.int32)]
    groups[0][0] = 5
    order = sorted(children.items(), key=lambda kv: kv[1])
    groups += [None] * len(order)
    for (gi, hop), ci in order:
        groups[ci] = rng.integers(-1, 20, len(groups[gi]) * sizes[hop - 1]).astype(np.int32)
    table = _t(rng.standard_normal((20, d)))
    convs = [gg.make_conv(d, seed=s) for s in range(L)]
    got = gg.model_forward(table, convs, groups, depths, children, L, sizes).numpy()
    rows = [np.where(g[:, None] >= 0, table.numpy()[np.maximum(g, 0)], 0.0) for g in groups]
    for i in range(L):
        hop = L - i
        new = list(rows)
        for gi, dep in enumerate(depths):
            if dep > hop - 1:
                continue
            ci = children[(gi, hop)]
            new[gi] = gg.hop_loop(rows[ci], rows[gi], groups[ci], sizes[hop - 1],
                                  [p.numpy() for p in convs[i]], relu=i != L - 1)
        rows = new
    assert np.abs(got - rows[0]).max() <= 1e-12 * max(1.0, np.abs(got).max())


def test_saturated_inputs_have_finite_references_and_bounds():
    case = (33, 64)
    s = gg.make_saturated(case)
    pre = np.abs(np.concatenate([s["gi"].ravel(), s["gh"][:, 2 * 64:].ravel()]))
    assert set(np.unique(pre)) == {90.0, 1e4}
    r, z, n, x_r, x_z, x_n = gg.gates_np(s["gi"], s["gh"])
    assert set(np.unique(np.abs(x_r))) <= {90.0, 1e4} and (x_n == 0).any()
    out = gg.gate_np(s["gi"], s["gh"], s["h"], relu=True)
    mask = out.astype(np.float32) > 0
    refs = gg.backward_closed(s["g"], s["gi"], s["gh"], s["h"], mask)
    bounds, raw = gg.bwd_bounds(s["g"], s["gi"], s["gh"], s["h"], mask, refs)
    for a in (out, gg.fwd_bounds(s["gi"], s["gh"], s["h"], out), *refs, *bounds, *raw):
        assert np.isfinite(a).all()


@pytest.mark.parametrize("scale", gg.SCALES)
def test_bounds_are_positive_and_below_the_cap(scale):
    case = (33, 64)
    s = gg.make_inputs(case, scale)
    out = gg.gate_np(s["gi"], s["gh"], s["h"])
    b = gg.fwd_bounds(s["gi"], s["gh"], s["h"], out)
    assert (b > 0).all() and b.max() <= gg.CAP * np.abs(out).max()
    # the float64 -> float32 rounding of the reference alone sits inside it
    assert (np.abs(out.astype(np.float32) - out) <= b).all()
    refs = gg.backward_closed(s["g"], s["gi"], s["gh"], s["h"])
    bounds, raw = gg.bwd_bounds(s["g"], s["gi"], s["gh"], s["h"], None, refs)
    for bd, rw, ref in zip(bounds, raw, refs):
        assert (bd > 0).all() and (bd <= rw).all()
        assert bd.max() <= gg.CAP * np.abs(ref).max()
        assert (np.abs(ref.astype(np.float32) - ref) <= bd).all()
    bb = gg.bias_bounds(raw[0], refs[0])
    assert bb.shape == (3 * 64,) and (bb > 0).all()


def test_case_lists_cover_the_kernel_paths():
    src = open(os.path.join(ROOT, "furusato_recommend_amd", "csrc", "ggnn.hip")).read()
    assert int(re.search(r"kGruMaxBlocks = (\d+);", src).group(1)) == gg.MAX_BLOCKS
    n, d = gg.STRIDE_CASE
    assert -(-n // gg.rows_per_block(d)) > gg.MAX_BLOCKS
    assert all(-(-n // gg.rows_per_block(d)) < gg.MAX_BLOCKS for n, d in gg.CASES)
    ds = [d for _, d in gg.CASES]
    assert any(d // 4 & (d // 4 - 1) for d in ds)            # idle lanes in a row's group
    assert any(n > gg.rows_per_block(d) for n, d in gg.CASES)  # more than one block
    assert any(n % gg.rows_per_block(d) for n, d in gg.CASES)  # a ragged last block
    assert [gg.rows_per_block(d) for d in (4, 12, 64, 128, 256)] == [256, 64, 16, 8, 4]


def test_the_package_names_the_hop():
    from furusato_recommend_amd import _lib, gnn
    assert "ggnn" in gnn.CONVS and gnn.CONVS[0] == "gat"
    assert "mirec_gru_gate" in _lib.SIGNATURES and "mirec_gru_gate_bwd" in _lib.SIGNATURES


def test_other_convs_are_still_refused():
    from furusato_recommend_amd import GNN
    for conv in ("gcn", "sage", "transformer"):
        with pytest.raises(ValueError, match="gat"):
            GNN({"conv": conv}, None)
