"""Host checks of the dot-product attention restatement (tests/tattn_common.py),
of the case lists of tests/test_tattn_kernels.py, and of the library's new
surface (the registry entry, the exported symbols, and the argument checks of
the three entry points, which come before any device call).  No GPU."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import gat_common as gc
from tests import tattn_common as tc
from tests.conftest import LIB

SYMBOLS = ("mirec_fanout_tattn", "mirec_fanout_tattn_bwd", "mirec_csr_tattn")
ERR_ARG = 1


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _both_forms(case, mode, scale):
    n_t, k, H, C = case
    d = tc.make_inputs(case, mode, scale)
    out1, alpha1, s1 = tc.tree_loop(d["q"], d["skip"], d["key"], d["val"], d["valid"], k, H)
    D = H * C
    zc, zt = torch.zeros(n_t * k, D, dtype=torch.float64), torch.zeros(n_t, D, dtype=torch.float64)
    ei = tc.tree_edges(d["valid"], n_t, k)
    out2, alpha2 = tc.edge_attention(torch.cat([zc, _t(d["q"])]), torch.cat([_t(d["key"]), zt]),
                                     torch.cat([_t(d["val"]), zt]),
                                     torch.cat([zc, _t(d["skip"])]), ei, H)
    return d, (out1, alpha1, s1), (out2[n_t * k:].numpy(), alpha2.numpy(), ei.numpy())


@pytest.mark.parametrize("case", tc.CASES, ids=str)
@pytest.mark.parametrize("mode", tc.VALID_MODES)
@pytest.mark.parametrize("scale", tc.SCALES)
def test_two_forms_agree(case, mode, scale):
    n_t, k, H, C = case
    d, (out1, alpha1, _), (out2, alpha2, ei) = _both_forms(case, mode, scale)
    ref = max(np.abs(out1).max(), 1e-300)
    assert np.abs(out1 - out2).max() <= 1e-12 * ref
    # the edge form's alpha per edge against the loop form's per slot
    t, c = (ei[1] - n_t * k), (ei[0] - (ei[1] - n_t * k) * k)
    assert np.abs(alpha2 - alpha1[t, c]).max(initial=0.0) <= 1e-12
    has = tc.valid_mask(d["valid"], n_t, k).any(1)
    assert np.allclose(alpha1.sum(1)[has], 1.0, atol=1e-12) and np.all(alpha1[~has] == 0.0)


@pytest.mark.parametrize("case", tc.CASES, ids=str)
@pytest.mark.parametrize("mode", ("null", "some"))
def test_closed_form_backward_is_autograd(case, mode):
    n_t, k, H, C = case
    d = tc.make_inputs(case, mode, 1.0)
    ts = {n: _t(d[n]).requires_grad_(True) for n in ("q", "skip", "key", "val")}
    out = tc.tree_level(ts["q"], ts["skip"], ts["key"], ts["val"], d["valid"], k, H)
    out.backward(_t(d["g"]))
    _, alpha, _ = tc.tree_loop(d["q"], d["skip"], d["key"], d["val"], d["valid"], k, H)
    got = tc.backward_closed(d["g"], d["q"], d["key"], d["val"], d["valid"], alpha, k, H)
    for name, a in zip(("q", "key", "val"), got):
        want = ts[name].grad.numpy()
        assert np.abs(a - want).max() <= 1e-11 * max(np.abs(want).max(), 1.0), name
    assert np.array_equal(ts["skip"].grad.numpy(), d["g"].astype(np.float64))
    # rows of invalid slots get exactly nothing
    ok = tc.valid_mask(d["valid"], n_t, k).reshape(-1)
    assert np.all(got[1][~ok] == 0.0) and np.all(got[2][~ok] == 0.0)


def test_hand_cases():
    rng = np.random.default_rng(1)
    q, skip = rng.standard_normal((1, 8)), rng.standard_normal((1, 8))
    # k = 1: alpha = 1, out = the value row + skip
    key, val = rng.standard_normal((1, 8)), rng.standard_normal((1, 8))
    out, alpha, _ = tc.tree_loop(q, skip, key, val, None, 1, 2)
    assert np.all(alpha == 1.0) and np.allclose(out, val + skip, atol=1e-15)
    # every slot invalid: out = skip exactly, and nothing flows to the children
    key, val = rng.standard_normal((3, 8)), rng.standard_normal((3, 8))
    none = np.full(3, -1, np.int32)
    out, alpha, _ = tc.tree_loop(q, skip, key, val, none, 3, 2)
    assert np.array_equal(out, skip) and np.all(alpha == 0)
    g = rng.standard_normal((1, 8))
    gq, gk, gv = tc.backward_closed(g, q, key, val, none, alpha, 3, 2)
    assert np.all(gq == 0) and np.all(gk == 0) and np.all(gv == 0)
    ts = [_t(x).requires_grad_(True) for x in (q, skip, key, val)]
    tc.tree_level(*ts, none, 3, 2).backward(_t(g))
    assert np.array_equal(ts[1].grad.numpy(), g)
    assert all(float(t.grad.abs().max()) == 0.0 for t in (ts[0], ts[2], ts[3]))
    # a repeated child id counts twice: slots (r, r, p) against edges (r, p)
    # with the logit of r raised by log 2
    kr, kp, vr, vp = (rng.standard_normal(8) for _ in range(4))
    out3, alpha3, s3 = tc.tree_loop(q, None, np.stack([kr, kr, kp]), np.stack([vr, vr, vp]),
                                    np.array([5, 5, 9], np.int32), 3, 1)
    assert np.allclose(alpha3[0, 0], alpha3[0, 1])
    w = np.exp(np.array([s3[0, 0, 0] + np.log(2.0), s3[0, 2, 0]]))
    w /= w.sum()
    assert np.allclose(out3[0], w[0] * vr + w[1] * vp, atol=1e-14)
    assert np.isclose(alpha3[0, 0, 0] + alpha3[0, 1, 0], w[0])
    # the logit is the scaled dot: 1 / sqrt(C) as the float32 the kernel gets
    assert np.isclose(s3[0, 2, 0], float(q[0] @ kp) * float(np.float32(1 / np.sqrt(8))), rtol=1e-15)


def _max_logit(case, mode, scale):
    n_t, k, H, C = case
    d = tc.make_inputs(case, mode, scale)
    _, _, s = tc.tree_loop(d["q"], None, d["key"], d["val"], d["valid"], k, H)
    ok = tc.valid_mask(d["valid"], n_t, k)
    return s[ok].max() if ok.any() else -np.inf, s[ok]


def test_case_list_contains_what_it_claims():
    assert tc.CASES == [(1, 1, 1, 4), (3, 5, 8, 4), (33, 10, 8, 8), (65, 25, 8, 16),
                        (7, 64, 8, 32), (257, 3, 4, 8), (5, 7, 2, 12), (9, 9, 5, 20)]
    assert tc.SCALES == (1.0, 60.0) and tc.VALID_MODES == ("null", "all", "none", "some")
    for case in tc.CASES:
        n_t, k, H, C = case
        # at variance 60 exp without the max subtraction overflows float32 in
        # every case but the single-logit one, in every mode with a child
        if case != (1, 1, 1, 4):
            for mode in ("null", "all", "some"):
                top, _ = _max_logit(case, mode, 60.0)
                assert top > tc.OVERFLOW, (case, mode, top)
        v = tc.make_inputs(case, "some", 1.0)["valid"].reshape(n_t, k)
        assert np.all(v[-1] < 0)                    # a target without a valid child
        if n_t > 1 and k > 1:
            assert (v < 0).any() and (v >= 0).any()
    # the variance-60 logits have the spread the issue names (std about 60)
    _, s = _max_logit((65, 25, 8, 16), "null", 60.0)
    assert 45 < s.std() < 75
    # workgroup boundaries: several blocks with a ragged tail, and one block
    per = {c: tc.lanes(c[2], c[3])[2] for c in tc.CASES}
    assert any(c[0] > per[c] and c[0] % per[c] for c in tc.CASES)
    assert any(c[0] < per[c] for c in tc.CASES)
    # head layouts: one lane per head up to eight; a full 64-lane group; a head
    # width whose lanes are not a power of two; idle lanes inside a group
    assert {c[3] // 4 for c in tc.CASES} >= {1, 2, 4, 8, 3, 5}
    assert any(tc.lanes(c[2], c[3])[0] == 64 for c in tc.CASES)
    assert any(tc.lanes(c[2], c[3])[0] < tc.lanes(c[2], c[3])[1] for c in tc.CASES)
    assert any(c[1] == 64 for c in tc.CASES) and any(c[1] % tc.BATCH for c in tc.CASES)
    assert any(c[1] > tc.BATCH and c[1] % tc.BATCH for c in tc.CASES)


def test_dense_full_is_the_edge_form():
    u, i, nu, mi = gc.small_graph_edges()
    rowptr, col = gc.host_csr(u, i, nu, mi)
    n = nu + mi
    rng = np.random.default_rng(3)
    q, skip, key, val = (rng.standard_normal((n, 16)) for _ in range(4))
    dst = np.repeat(np.arange(n), np.diff(rowptr))
    ei = torch.from_numpy(np.stack([col.astype(np.int64), dst]))
    want = tc.edge_attention(_t(q), _t(key), _t(val), _t(skip), ei, 4)[0].numpy()
    got, bound = tc.dense_full(q, skip, key, val, rowptr, col, 4)
    assert np.abs(got - want).max() <= 1e-12 and (bound > 0).all()
    assert np.array_equal(got[nu + 6], skip[nu + 6])            # the isolated item


def test_bounds_are_positive_and_capped():
    case = (33, 10, 8, 8)
    n_t, k, H, C = case
    for scale in tc.SCALES:
        d = tc.make_inputs(case, "some", scale)
        args = (d["q"], d["skip"], d["key"], d["val"], d["valid"], k, H)
        out, alpha, s = tc.tree_loop(*args)
        b_out, b_alpha = tc.fwd_bounds(*args, alpha, s, out)
        assert (b_out > 0).all() and b_out.max() <= tc.CAP * np.abs(out).max()
        assert b_alpha.max() <= tc.CAP and tc.CAP * np.abs(out).max() >= tc.TINY
        a32 = alpha.astype(np.float32)
        refs = tc.backward_closed(d["g"], d["q"], d["key"], d["val"], d["valid"], a32, k, H)
        bounds = tc.bwd_bounds(d["g"], d["q"], d["key"], d["val"], d["valid"], a32, k, H, refs)
        for b, r in zip(bounds, refs):
            assert b.shape == r.shape and (b >= 0).all() and b.max() <= tc.CAP * np.abs(r).max()
        ok = tc.valid_mask(d["valid"], n_t, k).reshape(-1)
        assert np.all(bounds[1][~ok] == 0) and np.all(bounds[2][~ok] == 0)


# ------------------------------------------- the library's surface, no device
def test_registry_and_symbols():
    """Fails before this feature: the 'tgrec' entry and the three entry points."""
    import furusato_recommend_amd
    from furusato_recommend_amd import _lib
    from furusato_recommend_amd.register import MODELS
    assert MODELS["tgrec"] is furusato_recommend_amd.TGRec
    assert "TGRec" in furusato_recommend_amd.__all__
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (mirec_\w+)", out))
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and s in exported, s


P = 0x10000  # a 16-byte aligned address nobody reads: every call below is refused first


def _fwd(k=5, H=2, C=4, n_t=3, ld_q=None, ld_kv=None, ptrs=None):
    from furusato_recommend_amd._lib import lib
    D = H * C
    q, skip, key, val, out, alpha = ptrs or (P,) * 6
    return lib.mirec_fanout_tattn(q, skip, D if ld_q is None else ld_q, key, val,
                                  D if ld_kv is None else ld_kv, None, n_t, k, H, C, 0.5, out,
                                  alpha, None)


def _bwd(k=5, H=2, C=4, n_t=3, ld=None, ptrs=None):
    from furusato_recommend_amd._lib import lib
    D = H * C
    ld = dict(dict(q=D, kv=D, gq=D, gkv=D), **(ld or {}))
    g, q, key, val, alpha, gq, gs, gk, gv = ptrs or (P,) * 9
    return lib.mirec_fanout_tattn_bwd(g, q, ld["q"], key, val, ld["kv"], None, alpha, n_t, k, H,
                                      C, 0.5, gq, gs, ld["gq"], gk, gv, ld["gkv"], None)


def _csr(H=2, C=4, n_rows=3, ld_q=None, ld_kv=None, ptrs=None):
    from furusato_recommend_amd._lib import CSR, lib
    D = H * C
    csr = CSR(rowptr=P, col=P, n_rows=n_rows, nnz=0)
    q, skip, key, val, out = ptrs or (P,) * 5
    return lib.mirec_csr_tattn(ctypes.byref(csr), q, skip, D if ld_q is None else ld_q, key, val,
                               D if ld_kv is None else ld_kv, H, C, 0.5, out, None)


@pytest.mark.parametrize("bad", [dict(C=6), dict(H=9), dict(H=5, C=52), dict(k=0), dict(k=65)],
                         ids=str)
def test_out_of_range_shapes_are_refused_without_a_device(bad):
    """C = 6, H = 9, H·C = 260, k = 0, k = 65."""
    if bad == dict(H=5, C=52):
        assert 5 * 52 == 260
    assert _fwd(**bad) == ERR_ARG and _bwd(**bad) == ERR_ARG
    if "k" not in bad:
        assert _csr(**bad) == ERR_ARG


def test_strides_and_alignment_are_refused_without_a_device():
    D = 8
    for ld in (D - 4, D + 2):            # below D; not a multiple of 4
        assert _fwd(ld_q=ld) == ERR_ARG and _fwd(ld_kv=ld) == ERR_ARG
        for name in ("q", "kv", "gq", "gkv"):
            assert _bwd(ld={name: ld}) == ERR_ARG, (name, ld)
        assert _csr(ld_q=ld) == ERR_ARG and _csr(ld_kv=ld) == ERR_ARG
    for n, call in ((6, _fwd), (9, _bwd), (5, _csr)):
        for bad in range(n):             # one misaligned pointer at a time
            ptrs = tuple(P + 4 if j == bad else P for j in range(n))
            assert call(ptrs=ptrs) == ERR_ARG, (call.__name__, bad)
    # NaN scale
    from furusato_recommend_amd._lib import lib
    assert lib.mirec_fanout_tattn(P, P, D, P, P, D, None, 3, 5, 2, 4, float("nan"), P, P,
                                  None) == ERR_ARG


def test_no_targets_is_ok_without_a_device():
    assert _fwd(n_t=0) == 0 and _bwd(n_t=0) == 0 and _csr(n_rows=0) == 0
    assert _fwd(n_t=-1) == ERR_ARG and _bwd(n_t=-1) == ERR_ARG
