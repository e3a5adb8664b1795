"""The SASRec row tail with dropout_p > 0, through the C ABI, against the
host-made mask of tests/dropout_common.py: mirec_resnorm_fwd / _bwd
(csrc/resnorm.hip) and the forms with the Linear inside, mirec_gemm_resnorm
and mirec_gemm_nn_resnorm_bwd (csrc/gemm.hip).  The arithmetic around the mask
is covered at p = 0 by test_resnorm_rows_match_torch; here the mask is the
subject: which elements are dropped (exactly), under which key (seed_base NULL
or given), and that it is the same mask forward and backward.

Conventions (tests/test_ssm_shared_kernels.py's): outputs start as one NaN
bit pattern in buffers longer than what is written, the excess is compared
bitwise, every call runs twice into fresh buffers and must repeat bitwise.

Tolerance: none is measured.  u = 2^-24, gamma(n) = n u / (1 - n u).
  mask       out = where(mask, z * scale, 0) with res = bias = NULL is one
             float32 multiply: bitwise.  d_z = where(mask, d_res * scale, 0)
             from the kernel's own d_res likewise.
  forward    out = res + mask * scale * (z + bias) (then ReLU, 1-Lipschitz):
             three roundings, gamma(3) * (scale * (|z| + |bias|) + |res|)
  d_bias     a column sum of n values of d_z, any order: gamma(n + 1) * sum
             |d_z| against the float64 sum of the kernel's own d_z
  y, mean, rstd  against a float64 LayerNorm of the kernel's own out with the
             measure and constant of test_resnorm_rows_match_torch (max |a - b|
             / max |b| < 1e-4): unchanged arithmetic, shown to be unchanged.

Shapes: dropout_common.rowtail_cases (every lanes-per-row / columns-per-lane
shape of the dispatch — the host file asserts it — n = 1 and 67, every
seed_base kind);
tests/test_dropout_host.py holds their coverage.

Measured on an MI355X, the largest err / bound over all cases (how much room
the derived bounds leave; they are not set by it):

    mirec_resnorm_fwd out            0.73
    mirec_resnorm_bwd d_bias         0.04
    mirec_gemm_nn_resnorm_bwd d_bias 0.02
    y / mean / rstd (of 1e-4)        0.005
"""
import numpy as np
import pytest
import torch

from tests import dropout_common as dc

pytestmark = pytest.mark.gpu

CANARY = 0x7FC5A5A5
PAD = 13
EPS = 1e-5
TOL = 1e-4          # tests/test_gpu_parity.py's, for the LayerNorm outputs
KR = 32
CASES = dc.rowtail_cases()
FUSED = dc.fused_rowtail_cases()


def _cid(c):
    b = "null" if c["base"] is None else ("big" if c["base"] > 1 else str(c["base"]))
    return f"n{c['n']}d{c['d']}p{c['p']}b{b}"


# ------------------------------------------------------------------ plumbing
def _api():
    from furusato_recommend_amd import _lib
    return _lib.lib, _lib.stream_handle()


def _canary_f32(n):
    return torch.full((n + PAD,), CANARY, dtype=torch.int32, device="cuda").view(torch.float32)


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _split(buf, n, shape):
    a = _np(buf)
    return a[:n].reshape(shape), bool(np.all(_bits(a[n:]) == CANARY))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _base_dev(base):
    """*seed_base on the device (None: the NULL pointer)."""
    if base is None:
        return None
    return torch.from_numpy(np.array([base], np.uint64).view(np.int64)).cuda()


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def _check_bound(tag, got, ref, bound):
    """Every element written (no NaN canary left, nothing non-finite) and
    within its bound; NaN fails both assertions."""
    got = np.asarray(got)
    assert np.isfinite(got).all(), (tag, np.argwhere(~np.isfinite(got))[:5].tolist())
    err = np.abs(got.astype(np.float64) - ref)
    bound = np.broadcast_to(bound, err.shape)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print(f"[rowtail] {tag}: max err / bound = {ratio:.4f}")
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0 and np.isfinite(ratio), (tag, bad[:5].tolist(), float(err.max()), ratio)


def _masked(mask, v, scale):
    """where(mask, v * scale, +0) in float32 (one multiply)."""
    assert v.dtype == np.float32 and scale.dtype == np.float32
    return np.where(mask, v * scale, np.float32(0)).astype(np.float32)


def _fwd(lib, st, c, z, res=None, bias=None, gamma=None, beta=None, relu=0, norm=False,
         base="case"):
    """mirec_resnorm_fwd into fresh canary buffers: dict of host arrays."""
    n, d = c["n"], c["d"]
    sb = _base_dev(c["base"] if base == "case" else base)
    out = _canary_f32(n * d)
    y, mean, rstd = (_canary_f32(n * d), _canary_f32(n), _canary_f32(n)) if norm else (None,) * 3
    rc = lib.mirec_resnorm_fwd(_ptr(res), z.data_ptr(), _ptr(bias), _ptr(gamma), _ptr(beta), n, d,
                               relu, c["p"], c["seed"], _ptr(sb), EPS, out.data_ptr(), _ptr(y),
                               _ptr(mean), _ptr(rstd), st)
    assert rc == 0
    r = {}
    for name, buf, cnt, shape in (("out", out, n * d, (n, d)), ("y", y, n * d, (n, d)),
                                  ("mean", mean, n, (n,)), ("rstd", rstd, n, (n,))):
        if buf is not None:
            r[name], clean = _split(buf, cnt, shape)
            assert clean and np.isfinite(r[name]).all(), name
    return r


def _same(r1, r2):
    assert r1.keys() == r2.keys()
    for k in r1:
        assert np.array_equal(_bits(r1[k]), _bits(r2[k])), k


def _layer_norm64(out, gamma, beta):
    o = out.astype(np.float64)
    mu = o.mean(1)
    rs = 1.0 / np.sqrt(o.var(1) + EPS)
    return (o - mu[:, None]) * rs[:, None] * gamma.astype(np.float64) + beta.astype(np.float64), mu, rs


# ------------------------------------------------------------ mirec_resnorm_fwd
@pytest.mark.parametrize("c", CASES, ids=_cid)
def test_resnorm_fwd_mask_is_the_host_mask(c):
    """res = bias = NULL, no ReLU, z in [0.5, 1.5]: out is bitwise
    where(mask, z * scale, 0) under the case's key."""
    lib, st = _api()
    n, d = c["n"], c["d"]
    rng = np.random.default_rng([n, d, 1])
    z = rng.uniform(0.5, 1.5, (n, d)).astype(np.float32)
    mask, scale = dc.rowtail_mask(c["p"], c["seed"], n, d, c["base"])
    z_d = _dev(z)
    r1, r2 = _fwd(lib, st, c, z_d), _fwd(lib, st, c, z_d)
    _same(r1, r2)
    assert np.array_equal(r1["out"] != 0, mask)
    assert np.array_equal(_bits(r1["out"]), _bits(_masked(mask, z, scale)))


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("c", CASES, ids=_cid)
def test_resnorm_fwd_full_row_tail(c, relu):
    """With res, bias, ReLU and LayerNorm: out against float64 with the host
    mask; y / mean / rstd against the float64 LayerNorm of the kernel's out."""
    lib, st = _api()
    n, d = c["n"], c["d"]
    rng = np.random.default_rng([n, d, 2, relu])
    z, res = (rng.standard_normal((n, d)).astype(np.float32) for _ in range(2))
    bias = (0.1 * rng.standard_normal(d)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, d).astype(np.float32)
    beta = rng.uniform(-0.2, 0.2, d).astype(np.float32)
    mask, scale = dc.rowtail_mask(c["p"], c["seed"], n, d, c["base"])
    dev = [_dev(a) for a in (z, res, bias, gamma, beta)]
    args = dict(res=dev[1], bias=dev[2], gamma=dev[3], beta=dev[4], relu=relu, norm=True)
    r1, r2 = _fwd(lib, st, c, dev[0], **args), _fwd(lib, st, c, dev[0], **args)
    _same(r1, r2)
    zb = z.astype(np.float64) + bias.astype(np.float64)
    pre = res.astype(np.float64) + np.where(mask, float(scale) * zb, 0.0)
    ref = np.maximum(pre, 0.0) if relu else pre
    A = float(scale) * (np.abs(z).astype(np.float64) + np.abs(bias).astype(np.float64)) \
        + np.abs(res).astype(np.float64)
    _check_bound(f"out {_cid(c)} relu{relu}", r1["out"], ref, dc.gamma(3) * A)
    y64, mu64, rs64 = _layer_norm64(r1["out"], gamma, beta)
    errs = [rel(r1["y"], y64), rel(r1["mean"], mu64), rel(r1["rstd"], rs64)]
    print(f"[rowtail] ln {_cid(c)} relu{relu}: max rel / 1e-4 = {max(errs) / TOL:.4f}")
    assert all(e < TOL for e in errs), errs


# ------------------------------------------------------------ mirec_resnorm_bwd
def _bwd_inputs(n, d, tag):
    rng = np.random.default_rng([n, d, 3, tag])
    out = rng.standard_normal((n, d)).astype(np.float32)
    mean = out.mean(1, dtype=np.float32)
    rstd = (1.0 / np.sqrt(out.astype(np.float64).var(1) + EPS)).astype(np.float32)
    g_y, g_out = (rng.standard_normal((n, d)).astype(np.float32) for _ in range(2))
    gamma = rng.uniform(0.5, 1.5, d).astype(np.float32)
    return out, mean, rstd, g_y, g_out, gamma


def _check_bwd(tag, c, d_res, d_z, d_bias):
    n, d = c["n"], c["d"]
    mask, scale = dc.rowtail_mask(c["p"], c["seed"], n, d, c["base"])
    assert (d_res != 0).mean() > 0.3                       # (ReLU zeroes about half)
    assert np.array_equal(_bits(d_z), _bits(_masked(mask, d_res, scale)))
    assert np.array_equal(d_z != 0, mask & (d_res != 0))
    dz64 = d_z.astype(np.float64)
    _check_bound(f"{tag} {_cid(c)}", d_bias, dz64.sum(0), dc.gamma(n + 1) * np.abs(dz64).sum(0))


@pytest.mark.parametrize("c", CASES, ids=_cid)
def test_resnorm_bwd_applies_the_forward_mask(c):
    """d_z is bitwise where(mask, d_res * scale, 0) of the kernel's own d_res
    (ReLU and LayerNorm backward in front of it), d_bias the column sum."""
    lib, st = _api()
    n, d = c["n"], c["d"]
    out, mean, rstd, g_y, g_out, gamma = _bwd_inputs(n, d, 0)
    dev = [_dev(a) for a in (g_y, g_out, out, mean, rstd, gamma)]
    sb = _base_dev(c["base"])
    nw = int(lib.mirec_resnorm_work_floats(n, d))
    assert nw >= 3 * d
    runs = []
    for _ in range(2):
        d_res, d_z, work = _canary_f32(n * d), _canary_f32(n * d), _canary_f32(nw)
        sums = [_canary_f32(d) for _ in range(3)]
        rc = lib.mirec_resnorm_bwd(*[t.data_ptr() for t in dev], n, d, 1, c["p"], c["seed"],
                                   _ptr(sb), d_res.data_ptr(), d_z.data_ptr(), work.data_ptr(),
                                   *[t.data_ptr() for t in sums], st)
        assert rc == 0
        r = {}
        for name, buf, cnt, shape in (("d_res", d_res, n * d, (n, d)), ("d_z", d_z, n * d, (n, d)),
                                      ("d_gamma", sums[0], d, (d,)), ("d_beta", sums[1], d, (d,)),
                                      ("d_bias", sums[2], d, (d,))):
            r[name], clean = _split(buf, cnt, shape)
            assert clean and np.isfinite(r[name]).all(), name
        assert _split(work, nw, (nw,))[1]
        runs.append(r)
    _same(*runs)
    _check_bwd("d_bias", c, runs[0]["d_res"], runs[0]["d_z"], runs[0]["d_bias"])


# ----------------------------------------------------- seed_base, every kind
@pytest.mark.parametrize("base", [None, 0, 1, (1 << 63) + 5],
                         ids=["null", "0", "1", "big"])
def test_seed_base_selects_the_key_forward_and_backward(base):
    """*seed_base = b: the mask under run_key(key, b); NULL: under key (so b =
    0 is not NULL) — the same in mirec_resnorm_fwd and mirec_resnorm_bwd."""
    lib, st = _api()
    c = dict(n=67, d=36, p=0.3, seed=123, base=base)
    n, d = c["n"], c["d"]
    mask, scale = dc.rowtail_mask(c["p"], c["seed"], n, d, base)
    for other in {None, 0, 1, (1 << 63) + 5} - {base}:
        assert not np.array_equal(mask, dc.rowtail_mask(c["p"], c["seed"], n, d, other)[0])
    rng = np.random.default_rng(9)
    z = rng.uniform(0.5, 1.5, (n, d)).astype(np.float32)
    z_d = _dev(z)
    r = _fwd(lib, st, c, z_d)
    assert np.array_equal(_bits(r["out"]), _bits(_masked(mask, z, scale)))
    # backward without LayerNorm / ReLU: d_res = g_out, d_z = mask * scale * g_out
    g_out = rng.uniform(0.5, 1.5, (n, d)).astype(np.float32)
    d_res, d_z = _canary_f32(n * d), _canary_f32(n * d)
    sb, g_d = _base_dev(base), _dev(g_out)
    rc = lib.mirec_resnorm_bwd(None, g_d.data_ptr(), z_d.data_ptr(), None, None, None,
                               n, d, 0, c["p"], c["seed"], _ptr(sb), d_res.data_ptr(),
                               d_z.data_ptr(), None, None, None, None, st)
    assert rc == 0
    (a, ca), (b, cb) = _split(d_res, n * d, (n, d)), _split(d_z, n * d, (n, d))
    assert ca and cb and np.array_equal(_bits(a), _bits(g_out))
    assert np.array_equal(_bits(b), _bits(_masked(mask, g_out, scale)))


# ---------------------------------------------------------- the fused forms
@pytest.mark.parametrize("c", FUSED, ids=_cid)
def test_gemm_resnorm_mask_is_the_host_mask(c):
    """mirec_gemm_resnorm with A, W > 0 (so z > 0), res = bias = NULL, no
    ReLU: the zero pattern of out is the host mask."""
    lib, st = _api()
    n, d = c["n"], c["d"]
    rng = np.random.default_rng([n, 4])
    A = rng.uniform(0.5, 1.5, (n, KR)).astype(np.float32)
    W = (rng.uniform(0.5, 1.5, (d, KR)) / KR).astype(np.float32)
    mask, scale = dc.rowtail_mask(c["p"], c["seed"], n, d, c["base"])
    A_d, W_d, sb = _dev(A), _dev(W), _base_dev(c["base"])
    outs = []
    for _ in range(2):
        out = _canary_f32(n * d)
        rc = lib.mirec_gemm_resnorm(A_d.data_ptr(), W_d.data_ptr(), n, KR, d, None, None, None,
                                    None, 0, c["p"], c["seed"], _ptr(sb), EPS, out.data_ptr(),
                                    None, None, None, st)
        assert rc == 0
        o, clean = _split(out, n * d, (n, d))
        assert clean
        outs.append(o)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    assert np.array_equal(outs[0] != 0, mask)
    # kept values: z * scale, z the f32-accurate product (its own tests hold it)
    z64 = A.astype(np.float64) @ W.astype(np.float64).T
    assert rel(outs[0][mask], (float(scale) * z64)[mask]) < 1e-6


@pytest.mark.parametrize("c", FUSED, ids=_cid)
def test_gemm_nn_resnorm_bwd_applies_the_forward_mask(c):
    """mirec_gemm_nn_resnorm_bwd: d_z bitwise where(mask, d_res * scale, 0) of
    its own d_res, d_bias the column sum of its d_z."""
    lib, st = _api()
    n, d = c["n"], c["d"]
    out, mean, rstd, _, g_out, gamma = _bwd_inputs(n, d, 1)
    rng = np.random.default_rng([n, 5])
    A = rng.standard_normal((n, KR)).astype(np.float32)
    W = (rng.standard_normal((KR, d)) * KR ** -0.5).astype(np.float32)
    dev = [_dev(a) for a in (A, W, g_out, out, mean, rstd, gamma)]
    sb = _base_dev(c["base"])
    nw = int(lib.mirec_gemm_nn_resnorm_bwd_work_floats(n, d))
    assert nw >= 3 * d
    runs = []
    for _ in range(2):
        d_res, d_z, work = _canary_f32(n * d), _canary_f32(n * d), _canary_f32(nw)
        sums = [_canary_f32(d) for _ in range(3)]
        rc = lib.mirec_gemm_nn_resnorm_bwd(dev[0].data_ptr(), dev[1].data_ptr(), n, KR, d,
                                           *[t.data_ptr() for t in dev[2:]], 1, c["p"], c["seed"],
                                           _ptr(sb), d_res.data_ptr(), d_z.data_ptr(),
                                           work.data_ptr(), *[t.data_ptr() for t in sums], st)
        assert rc == 0
        r = {}
        for name, buf, cnt, shape in (("d_res", d_res, n * d, (n, d)), ("d_z", d_z, n * d, (n, d)),
                                      ("d_gamma", sums[0], d, (d,)), ("d_beta", sums[1], d, (d,)),
                                      ("d_bias", sums[2], d, (d,))):
            r[name], clean = _split(buf, cnt, shape)
            assert clean and np.isfinite(r[name]).all(), name
        assert _split(work, nw, (nw,))[1]
        runs.append(r)
    _same(*runs)
    _check_bwd("d_bias fused", c, runs[0]["d_res"], runs[0]["d_z"], runs[0]["d_bias"])
