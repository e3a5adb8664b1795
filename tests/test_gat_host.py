"""Host checks of the graph-attention restatement (tests/gat_common.py), of the
case lists of tests/test_gat_kernels.py, and of the library's new surface
(the registry entry and the exported symbols).  No GPU."""
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import gat_common as gc
from tests.conftest import LIB

SYMBOLS = ("mirec_fanout_gat", "mirec_fanout_gat_bwd_work_floats", "mirec_fanout_gat_bwd",
           "mirec_csr_gat")
ALL_CASES = gc.CASES + [gc.STRIDE_CASE]


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _both_forms(case, mode, scale):
    n_t, k, H, C = case
    d = gc.make_inputs(case, mode, scale)
    out1, alpha1, s1 = gc.tree_loop(d["zc"], d["zs"], d["valid"], d["a_src"], d["a_dst"],
                                    d["bias"], k, H)
    z = torch.cat([_t(d["zc"]), _t(d["zs"])])
    ei = gc.tree_edges(d["valid"], n_t, k)
    out2, alpha2, _ = gc.edge_softmax(z, ei, _t(d["a_src"]), _t(d["a_dst"]), _t(d["bias"]), H)
    return d, (out1, alpha1, s1), (out2[n_t * k:].numpy(), alpha2.numpy(), ei.numpy())


@pytest.mark.parametrize("case", gc.CASES, ids=str)
@pytest.mark.parametrize("mode", gc.VALID_MODES)
@pytest.mark.parametrize("scale", gc.SCALES)
def test_two_forms_agree(case, mode, scale):
    n_t, k, H, C = case
    d, (out1, alpha1, _), (out2, alpha2, ei) = _both_forms(case, mode, scale)
    ref = max(np.abs(out1).max(), 1e-300)
    assert np.abs(out1 - out2).max() <= 1e-12 * ref
    # the edge form's alpha per edge against the loop form's per slot
    E = ei.shape[1]
    t, c = (ei[1] - n_t * k), (ei[0] - (ei[1] - n_t * k) * k)
    assert np.abs(alpha2[:E] - alpha1[t, c]).max(initial=0.0) <= 1e-12
    self_alpha = alpha2[E + n_t * k:]
    assert np.abs(self_alpha - alpha1[:, k]).max() <= 1e-12
    assert np.allclose(alpha1.sum(1), 1.0, atol=1e-12)


@pytest.mark.parametrize("case", gc.CASES[:4] + gc.CASES[5:], ids=str)
@pytest.mark.parametrize("mode", ("null", "some"))
def test_closed_form_backward_is_autograd(case, mode):
    n_t, k, H, C = case
    d = gc.make_inputs(case, mode, 1.0)
    ts = {n: _t(d[n]).requires_grad_(True) for n in ("zc", "zs", "a_src", "a_dst", "bias")}
    out = gc.tree_level(ts["zc"], ts["zs"], d["valid"], ts["a_src"], ts["a_dst"], ts["bias"], k, H)
    out.backward(_t(d["g"]))
    _, alpha, s = gc.tree_loop(d["zc"], d["zs"], d["valid"], d["a_src"], d["a_dst"], d["bias"],
                               k, H)
    got = gc.backward_closed(d["g"], d["zc"], d["zs"], d["valid"], d["a_src"], d["a_dst"], alpha,
                             s, k, H)
    for name, a in zip(("zc", "zs", "a_src", "a_dst"), got):
        want = ts[name].grad.numpy()
        assert np.abs(a - want).max() <= 1e-11 * max(np.abs(want).max(), 1.0), name
    assert np.allclose(ts["bias"].grad.numpy(), d["g"].astype(np.float64).sum(0), rtol=1e-13)
    # rows of invalid slots get exactly nothing
    ok = gc.valid_mask(d["valid"], n_t, k).reshape(-1)
    assert np.all(got[0][~ok] == 0.0)


def test_hand_cases():
    rng = np.random.default_rng(1)
    z = rng.standard_normal((1, 8))
    a_s, a_d, b = rng.standard_normal(8), rng.standard_normal(8), rng.standard_normal(8)
    # k = 1, the child row equal to the self row: alpha = 1/2, 1/2
    out, alpha, _ = gc.tree_loop(z, z, None, a_s, a_d, b, 1, 2)
    assert np.allclose(alpha, 0.5, atol=1e-15) and np.allclose(out, z + b, atol=1e-15)
    # every slot invalid: out = z_self + bias
    zc = rng.standard_normal((3, 8))
    out, alpha, _ = gc.tree_loop(zc, z, np.full(3, -1, np.int32), a_s, a_d, b, 3, 2)
    assert np.array_equal(out, z + b) and np.all(alpha[:, :3] == 0) and np.all(alpha[:, 3] == 1)
    # a repeated child id counts twice: slots (r, r, q) against edges (r, q)
    # with the logit of r raised by log 2
    r, q = rng.standard_normal(8), rng.standard_normal(8)
    out3, alpha3, s3 = gc.tree_loop(np.stack([r, r, q]), z, np.array([5, 5, 9], np.int32), a_s,
                                    a_d, None, 3, 1)
    assert np.allclose(alpha3[0, 0], alpha3[0, 1])
    e = np.where(s3[0, :, 0] > 0, s3[0, :, 0], 0.2 * s3[0, :, 0])
    w = np.exp(np.array([e[0] + np.log(2.0), e[2], e[3]]))
    w /= w.sum()
    assert np.allclose(out3[0], w[0] * r + w[1] * q + w[2] * z[0], atol=1e-14)


def test_case_list_contains_what_it_claims():
    pos = neg = 0
    overflow = False
    for case in gc.CASES:
        n_t, k, H, C = case
        for scale in gc.SCALES:
            d = gc.make_inputs(case, "null", scale)
            _, _, s = gc.tree_loop(d["zc"], d["zs"], None, d["a_src"], d["a_dst"], None, k, H)
            pos += int((s > 0).sum())
            neg += int((s < 0).sum())
            if scale == 30.0 and s.max() > 88.73:   # exp(88.73) > float32 max
                overflow = True
        v = gc.make_inputs(case, "some", 1.0)["valid"].reshape(n_t, k)
        assert np.all(v[-1] < 0)                    # a target without a valid child
        if n_t > 1 and k > 1:
            assert (v < 0).any() and (v >= 0).any()
    assert pos > 100 and neg > 100 and overflow
    # the scale-30 logits have the spread the issue names (std about 170 for
    # the source dot at C = 32)
    d = gc.make_inputs((65, 25, 4, 32), "null", 30.0)
    dots = (d["zc"].astype(np.float64).reshape(-1, 4, 32) * d["a_src"].reshape(1, 4, 32)).sum(-1)
    assert 100 < dots.std() < 260
    # workgroup boundaries: several blocks with a ragged tail, one block, and
    # (the extra case) more blocks than the backward's partial-sum limit
    per = {c: gc.lanes(c[2], c[3])[2] for c in ALL_CASES}
    assert any(c[0] > per[c] and c[0] % per[c] for c in gc.CASES)
    assert any(c[0] < per[c] for c in gc.CASES)
    assert -(-gc.STRIDE_CASE[0] // per[gc.STRIDE_CASE]) > gc.MAX_BLOCKS
    assert all(gc.bwd_blocks(c[0], c[2], c[3]) < gc.MAX_BLOCKS for c in gc.CASES)
    # head layouts: one lane per head up to eight; a full 64-lane group
    assert {c[3] // 4 for c in gc.CASES} >= {1, 2, 4, 8}
    assert any(gc.lanes(c[2], c[3])[0] == 64 for c in gc.CASES)
    assert any(c[1] == 64 for c in gc.CASES) and any(c[1] % gc.BATCH for c in gc.CASES)


def test_csr_graphs_contain_what_they_claim():
    u, i, nu, mi = gc.csr_graph_edges()
    rowptr, col = gc.host_csr(u, i, nu, mi)
    deg = np.diff(rowptr)
    assert (nu, mi) == (37, 11) and deg[nu + 10] == 0 and deg[36] == 1 and deg[nu] >= 300
    assert len(set(zip(u.tolist(), i.tolist()))) < len(u)        # duplicate edges
    assert col.min() >= 0 and col.max() < nu + mi
    # the library's own builder keeps the same rows (multi-edges included)
    from furusato_recommend_amd._lib import lib
    rp2 = np.empty(nu + mi + 1, np.int64)
    col2 = np.empty(2 * len(u), np.int32)
    dinv = np.empty(nu + mi, np.float32)
    assert lib.mirec_csr_bipartite(u.ctypes.data, i.ctypes.data, len(u), nu, mi,
                                   rp2.ctypes.data, col2.ctypes.data, dinv.ctypes.data) == 0
    assert np.array_equal(rp2, rowptr)
    for r in range(nu + mi):
        assert sorted(col2[rp2[r]:rp2[r + 1]]) == sorted(col[rowptr[r]:rowptr[r + 1]])
    u, i, nu, mi = gc.small_graph_edges()
    deg = np.diff(gc.host_csr(u, i, nu, mi)[0])
    assert 8 < deg.max() <= 64 and deg[nu + 6] == 0 and len(set(zip(u.tolist(), i.tolist()))) < len(u)


def test_dense_full_is_the_edge_form():
    u, i, nu, mi = gc.small_graph_edges()
    rowptr, col = gc.host_csr(u, i, nu, mi)
    n = nu + mi
    rng = np.random.default_rng(3)
    z, a_s, a_d, b = (rng.standard_normal(s) for s in ((n, 16), 16, 16, 16))
    dst = np.repeat(np.arange(n), np.diff(rowptr))
    ei = torch.from_numpy(np.stack([col.astype(np.int64), dst]))
    want = gc.edge_softmax(_t(z), ei, _t(a_s), _t(a_d), _t(b), 4)[0].numpy()
    got, bound = gc.dense_full(z, rowptr, col, a_s, a_d, b, 4)
    assert np.abs(got - want).max() <= 1e-12 and (bound > 0).all()


def test_bounds_are_positive_and_capped():
    case = (33, 10, 4, 16)
    n_t, k, H, C = case
    for scale in gc.SCALES:
        d = gc.make_inputs(case, "some", scale)
        out, alpha, s = gc.tree_loop(d["zc"], d["zs"], d["valid"], d["a_src"], d["a_dst"],
                                     d["bias"], k, H)
        b_out, b_alpha = gc.fwd_bounds(d["zc"], d["zs"], d["valid"], d["a_src"], d["a_dst"],
                                       d["bias"], k, H, alpha, s, out)
        assert (b_out > 0).all() and b_out.max() <= gc.CAP * np.abs(out).max()
        assert b_alpha.max() <= gc.CAP
        a32 = alpha.astype(np.float32)
        refs = gc.backward_closed(d["g"], d["zc"], d["zs"], d["valid"], d["a_src"], d["a_dst"],
                                  a32, s, k, H)
        for b, r in zip(gc.bwd_bounds(d["g"], d["zc"], d["zs"], d["valid"], d["a_src"],
                                      d["a_dst"], a32, s, k, H, refs), refs):
            assert b.shape == r.shape and (b >= 0).all() and b.max() <= gc.CAP * np.abs(r).max()


def test_registry_and_symbols():
    """Fails before this feature: the 'gnn' entry and the four entry points."""
    from furusato_recommend_amd import _lib
    from furusato_recommend_amd.register import MODELS
    assert "gnn" in MODELS and MODELS["gnn"].__name__ == "GNN"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (mirec_\w+)", out))
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and s in exported, s
    assert _lib.lib.mirec_fanout_gat_bwd_work_floats(257, 3, 4, 8) == \
        gc.bwd_blocks(257, 4, 8) * 2 * 32
    # shapes outside the limits: -1, and the error code with nothing launched
    for k, H, C in ((0, 4, 8), (65, 4, 8), (3, 9, 4), (3, 4, 6), (3, 8, 36), (3, 0, 4)):
        assert _lib.lib.mirec_fanout_gat_bwd_work_floats(5, k, H, C) == -1
        assert _lib.lib.mirec_fanout_gat(None, None, None, None, None, None, 5, k, H, C, 0.2,
                                         None, None, None) == 1
