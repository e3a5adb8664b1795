"""csrc/gat.hip called directly through the C ABI against the float64
restatement of tests/gat_common.py: mirec_fanout_gat, mirec_fanout_gat_bwd and
mirec_csr_gat.

Conventions (tests/test_sage_kernels.py's).  Every output buffer is one
quiet-NaN bit pattern before the call, with PAD canary floats before and after
the part the kernel should write; the canaries are compared bitwise.  Every
call runs twice into fresh buffers and must repeat bitwise — the parameter
gradients included, which are ordered sums.  Slots of alpha and rows of
grad_z_child that belong to an invalid child are exactly 0.

Cases: gat_common.CASES x valid in {NULL, all valid, all -1, ~30 % -1} x input
variance {1, 30} (at 30 the logits have a standard deviation of about 170 and
exp without the max subtraction overflows float32), plus STRIDE_CASE for the
backward's second grid-stride round; tests/test_gat_host.py holds their
coverage.  The backward is given the float32-rounded reference alpha, so it
is tested on its own.

Tolerance: the bounds derived in gat_common's docstring (logit error, one
explicit exp constant, gamma(m) * A for the sums), capped at 1e-4 * max
|reference| of the tensor.  Nothing is measured into them.  The largest err /
bound over all cases of an output, measured on an MI355X (how much room the
bound leaves; it does not set it), is printed per case and recorded in
DESIGN.md section 21:

    out 0.10   alpha 0.09   grad_z_child 0.50   grad_z_self 0.11
    grad_att_src 0.03   grad_att_dst 0.02   csr out 0.03   csr logits 0.27
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import gat_common as gc

pytestmark = pytest.mark.gpu

CANARY = 0x7FC5A5A5
PAD = 64   # floats: whole rows of every case fit, and 16-byte alignment is kept
ERR_ARG = 1
COMBOS = [(c, m, s) for c in gc.CASES for m in gc.VALID_MODES for s in gc.SCALES]


def _cid(x):
    c, m, s = x
    return f"t{c[0]}k{c[1]}h{c[2]}c{c[3]}-{m}-v{int(s)}"


def _api():
    from furusato_recommend_amd import _lib
    return _lib.lib, _lib.stream_handle()


class Out:
    """A device buffer of n floats with PAD canary floats on both sides."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), CANARY, dtype=torch.int32,
                              device="cuda").view(torch.float32)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * PAD

    def get(self, shape):
        """(the written part, True iff both canary runs are untouched)."""
        torch.cuda.synchronize()
        a = self.buf.cpu().numpy().copy()
        bits = a.view(np.int32)
        clean = bool(np.all(bits[:PAD] == CANARY) and np.all(bits[PAD + self.n:] == CANARY))
        return a[PAD:PAD + self.n].reshape(shape), clean

    def untouched(self):
        torch.cuda.synchronize()
        return bool(np.all(self.buf.cpu().numpy().view(np.int32) == CANARY))


def _dev(a, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()


def _p(t):
    return None if t is None else t.data_ptr()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check(tag, got, ref, bound, worst):
    got = np.asarray(got)
    assert np.isfinite(got).all(), (tag, np.argwhere(~np.isfinite(got))[:5].tolist())
    err = np.abs(got.astype(np.float64) - ref)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    worst[tag] = ratio
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0 and np.isfinite(ratio), (tag, bad[:5].tolist(), float(err.max()), ratio)


# ---------------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def _ref(case, mode, scale):
    """Inputs and float64 references of one combination, computed once."""
    n_t, k, H, C = case
    d = gc.make_inputs(case, mode, scale)
    args = (d["zc"], d["zs"], d["valid"], d["a_src"], d["a_dst"])
    out, alpha, s = gc.tree_loop(*args, d["bias"], k, H)
    b_out, b_alpha = gc.fwd_bounds(*args, d["bias"], k, H, alpha, s, out)
    a32 = alpha.astype(np.float32)
    grads = gc.backward_closed(d["g"], *args, a32, s, k, H)
    b_grads = gc.bwd_bounds(d["g"], *args, a32, s, k, H, grads)
    for a in list(d.values()) + [out, alpha, a32, b_out, b_alpha, *grads, *b_grads]:
        if a is not None:
            a.setflags(write=False)
    return dict(d=d, out=out, alpha=alpha, a32=a32, b_out=b_out, b_alpha=b_alpha, grads=grads,
                b_grads=b_grads, ok=gc.valid_mask(d["valid"], n_t, k))


def _run_fwd(case, d, keep_alpha=True, bias=True):
    lib, st = _api()
    n_t, k, H, C = case
    D = H * C
    dev = {n: _dev(d[n]) for n in ("zc", "zs", "a_src", "a_dst", "bias")}
    valid = _dev(d["valid"], np.int32)
    out, alpha = Out(n_t * D), Out(n_t * (k + 1) * H)
    rc = lib.mirec_fanout_gat(_p(dev["zc"]), _p(dev["zs"]), _p(valid), _p(dev["a_src"]),
                              _p(dev["a_dst"]), _p(dev["bias"]) if bias else None, n_t, k, H, C,
                              gc.SLOPE, out.ptr, alpha.ptr if keep_alpha else None, st)
    assert rc == 0
    return out, alpha


def _run_bwd(case, d, a32):
    lib, st = _api()
    n_t, k, H, C = case
    D = H * C
    dev = {n: _dev(d[n]) for n in ("g", "zc", "zs", "a_src", "a_dst")}
    valid, alpha = _dev(d["valid"], np.int32), _dev(a32)
    nw = lib.mirec_fanout_gat_bwd_work_floats(n_t, k, H, C)
    assert nw == gc.bwd_blocks(n_t, H, C) * 2 * D
    outs = [Out(n_t * k * D), Out(n_t * D), Out(D), Out(D)]
    work = Out(nw)
    rc = lib.mirec_fanout_gat_bwd(_p(dev["g"]), _p(dev["zc"]), _p(dev["zs"]), _p(valid),
                                  _p(dev["a_src"]), _p(dev["a_dst"]), _p(alpha), n_t, k, H, C,
                                  gc.SLOPE, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr,
                                  work.ptr, st)
    assert rc == 0
    return outs, work


# ------------------------------------------------------------------- forward
@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_fanout_gat_forward(combo):
    case, mode, scale = combo
    n_t, k, H, C = case
    r = _ref(*combo)
    worst = {}
    runs = []
    for _ in range(2):
        out, alpha = _run_fwd(case, r["d"])
        o, c1 = out.get((n_t, H * C))
        a, c2 = alpha.get((n_t, k + 1, H))
        assert c1 and c2, "canary overwritten"
        runs.append((o, a))
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0]))
    assert np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))
    o, a = runs[0]
    _check("out", o, r["out"], r["b_out"], worst)
    _check("alpha", a, r["alpha"], r["b_alpha"], worst)
    assert np.all(_bits(a[:, :k][~r["ok"]]) == 0), "alpha of an invalid slot is not +0"
    none = ~r["ok"].any(1)
    want = (r["d"]["zs"] + r["d"]["bias"])[none]        # float32: z_self + bias exactly
    assert np.array_equal(_bits(o[none]), _bits(want))
    assert np.all(a[none, k] == 1.0)
    print(f"[gat] fwd {_cid(combo)}: err/bound out {worst['out']:.4f} alpha {worst['alpha']:.4f}")


def test_fanout_gat_without_alpha_or_bias():
    case, mode, scale = (33, 10, 4, 16), "some", 1.0
    r = _ref(case, mode, scale)
    full, _ = _run_fwd(case, r["d"])
    o1, _ = full.get((33, 64))
    out, alpha = _run_fwd(case, r["d"], keep_alpha=False)
    o2, clean = out.get((33, 64))
    assert clean and alpha.untouched() and np.array_equal(_bits(o1), _bits(o2))
    out, _ = _run_fwd(case, r["d"], bias=False)
    o3, clean = out.get((33, 64))
    ref = r["out"] - r["d"]["bias"].astype(np.float64)
    assert clean
    _check("out", o3, ref, r["b_out"], {})


# ------------------------------------------------------------------ backward
NAMES = ("grad_z_child", "grad_z_self", "grad_att_src", "grad_att_dst")


def _bwd_case(case, mode, scale):
    n_t, k, H, C = case
    D = H * C
    r = _ref(case, mode, scale)
    shapes = [(n_t * k, D), (n_t, D), (D,), (D,)]
    runs = []
    for _ in range(2):
        outs, work = _run_bwd(case, r["d"], r["a32"])
        got = []
        for o, sh in zip(outs, shapes):
            a, clean = o.get(sh)
            assert clean, "canary overwritten"
            got.append(a)
        assert work.get((work.n,))[1], "canary around the workspace overwritten"
        runs.append(got)
    for a, b, name in zip(runs[0], runs[1], NAMES):
        assert np.array_equal(_bits(a), _bits(b)), f"{name} differs between two runs"
    worst = {}
    for name, got, ref, bound in zip(NAMES, runs[0], r["grads"], r["b_grads"]):
        _check(name, got, ref, bound, worst)
    gzc = runs[0][0].reshape(n_t, k, D)
    assert np.all(_bits(gzc[~r["ok"]]) == 0), "grad_z_child of an invalid slot is not +0"
    print(f"[gat] bwd {_cid((case, mode, scale))}: err/bound " +
          " ".join(f"{n} {worst[n]:.4f}" for n in NAMES))


@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_fanout_gat_backward(combo):
    _bwd_case(*combo)


def test_backward_second_grid_round():
    """More targets than the partial-sum blocks take in one round."""
    _bwd_case(gc.STRIDE_CASE, "some", 1.0)


def test_forward_and_backward_chain():
    """The backward on the forward kernel's own alpha (the pair as autograd
    uses it) against float64 end to end, by max-norm per tensor at 1e-4."""
    case = (65, 25, 4, 32)
    n_t, k, H, C = case
    r = _ref(case, "some", 1.0)
    _, alpha = _run_fwd(case, r["d"])
    a, _ = alpha.get((n_t, k + 1, H))
    outs, _ = _run_bwd(case, r["d"], a)
    d = r["d"]
    _, al64, s = gc.tree_loop(d["zc"], d["zs"], d["valid"], d["a_src"], d["a_dst"], None, k, H)
    refs = gc.backward_closed(d["g"], d["zc"], d["zs"], d["valid"], d["a_src"], d["a_dst"], al64,
                              s, k, H)
    for o, ref, name in zip(outs, refs, NAMES):
        got, clean = o.get(ref.shape)
        assert clean
        assert np.abs(got - ref).max() <= gc.CAP * np.abs(ref).max(), name


# --------------------------------------------------------------- bad shapes
BAD = [dict(k=0), dict(k=65), dict(k=-1), dict(H=0), dict(H=9), dict(C=6), dict(C=0), dict(C=2),
       dict(H=8, C=36), dict(n_t=-1)]


@pytest.mark.parametrize("bad", BAD, ids=str)
def test_out_of_range_shapes_are_refused(bad):
    lib, st = _api()
    n_t, k, H, C = bad.get("n_t", 3), bad.get("k", 5), bad.get("H", 4), bad.get("C", 4)
    n = 4096
    ins = [torch.zeros(n, device="cuda") for _ in range(7)]
    valid = torch.zeros(n, dtype=torch.int32, device="cuda")
    outs = [Out(n) for _ in range(7)]
    rc = lib.mirec_fanout_gat(_p(ins[0]), _p(ins[1]), _p(valid), _p(ins[2]), _p(ins[3]),
                              _p(ins[4]), n_t, k, H, C, gc.SLOPE, outs[0].ptr, outs[1].ptr, st)
    assert rc == ERR_ARG
    assert lib.mirec_fanout_gat_bwd_work_floats(n_t, k, H, C) == -1
    rc = lib.mirec_fanout_gat_bwd(_p(ins[5]), _p(ins[0]), _p(ins[1]), _p(valid), _p(ins[2]),
                                  _p(ins[3]), _p(ins[6]), n_t, k, H, C, gc.SLOPE, outs[2].ptr,
                                  outs[3].ptr, outs[4].ptr, outs[5].ptr, outs[6].ptr, st)
    assert rc == ERR_ARG
    if "k" not in bad and "n_t" not in bad:
        from furusato_recommend_amd._lib import CSR
        rowptr = torch.zeros(4, dtype=torch.int64, device="cuda")
        csr = CSR(rowptr=rowptr.data_ptr(), col=valid.data_ptr(), n_rows=3, nnz=0)
        rc = lib.mirec_csr_gat(ctypes.byref(csr), _p(ins[0]), _p(ins[2]), _p(ins[3]), _p(ins[4]),
                               H, C, gc.SLOPE, outs[0].ptr, outs[1].ptr, st)
        assert rc == ERR_ARG
    assert all(o.untouched() for o in outs)


# ----------------------------------------------------------------- CSR form
def _device_csr(rowptr, col):
    from furusato_recommend_amd._lib import CSR
    rp, cl = _dev(rowptr, np.int64), _dev(col, np.int32)
    csr = CSR(rowptr=rp.data_ptr(), col=cl.data_ptr(), n_rows=len(rowptr) - 1, nnz=len(col))
    return csr, (rp, cl)


def _csr_inputs(n, H, C, scale, seed):
    rng = np.random.default_rng([n, H, C, int(scale), seed])
    sd = np.sqrt(scale)
    return tuple((rng.standard_normal(s) * sd).astype(np.float32)
                 for s in ((n, H * C), H * C, H * C, H * C))


def _run_csr(csr, z, a_s, a_d, b, H, C):
    lib, st = _api()
    n = z.shape[0]
    dz, ds, dd, db = _dev(z), _dev(a_s), _dev(a_d), _dev(b)
    out, logits = Out(n * H * C), Out(n * 2 * H)
    assert lib.mirec_csr_gat(ctypes.byref(csr), _p(dz), _p(ds), _p(dd), _p(db), H, C, gc.SLOPE,
                             out.ptr, logits.ptr, st) == 0
    o, c1 = out.get((n, H * C))
    lg, c2 = logits.get((n, 2 * H))
    assert c1 and c2, "canary overwritten"
    return o, lg


@pytest.mark.parametrize("H,C", [(4, 16), (1, 4), (8, 32), (2, 12)], ids=str)
@pytest.mark.parametrize("scale", gc.SCALES)
def test_csr_gat(H, C, scale):
    """The 37 x 11 graph (duplicates, an isolated item, a degree-1 user, a
    hub of degree 324).  The kernel has one path for every degree (one lane
    group walks the row in batches of 8), which the hub, the degree-1 row and
    the empty row all take: ragged tails 324 % 8 = 4, 1, 0.  (2, 12) is the
    head width whose lanes are not a power of two."""
    u, i, nu, mi = gc.csr_graph_edges()
    rowptr, col = gc.host_csr(u, i, nu, mi)
    n = nu + mi
    z, a_s, a_d, b = _csr_inputs(n, H, C, scale, 1)
    ref, bound = gc.dense_full(z, rowptr, col, a_s, a_d, b, H)
    bound = np.minimum(bound, gc.CAP * np.abs(ref).max())
    csr, keep = _device_csr(rowptr, col)
    o1, lg1 = _run_csr(csr, z, a_s, a_d, b, H, C)
    o2, lg2 = _run_csr(csr, z, a_s, a_d, b, H, C)
    assert np.array_equal(_bits(o1), _bits(o2)) and np.array_equal(_bits(lg1), _bits(lg2))
    worst = {}
    _check("csr out", o1, ref, bound, worst)
    iso = nu + 10
    assert np.array_equal(_bits(o1[iso]), _bits(z[iso] + b))     # degree 0: z_r + bias
    z64 = z.astype(np.float64).reshape(n, H, C)
    want = np.concatenate([(z64 * a_s.reshape(1, H, C)).sum(-1),
                           (z64 * a_d.reshape(1, H, C)).sum(-1)], 1)
    absd = np.concatenate([np.abs(z64 * a_s.reshape(1, H, C)).sum(-1),
                           np.abs(z64 * a_d.reshape(1, H, C)).sum(-1)], 1)
    _check("csr logits", lg1, want, gc.gamma(C + 1) * absd, worst)
    print(f"[gat] csr h{H}c{C} v{int(scale)}: err/bound {worst}")


def test_tree_kernel_equals_csr_kernel():
    """Sampling without replacement at a fanout above the largest degree
    returns every neighbour, so the one-layer tree kernel on the sampled
    children computes the CSR kernel's rows."""
    from furusato_recommend_amd._lib import lib
    st = _api()[1]
    u, i, nu, mi = gc.small_graph_edges()
    rowptr, col = gc.host_csr(u, i, nu, mi)
    n, H, C, k = nu + mi, 4, 8, 64
    assert np.diff(rowptr).max() <= k
    z, a_s, a_d, b = _csr_inputs(n, H, C, 1.0, 2)
    csr, keep = _device_csr(rowptr, col)
    full, _ = _run_csr(csr, z, a_s, a_d, b, H, C)
    nodes = torch.arange(n, dtype=torch.int32, device="cuda")
    ch = torch.empty(n * k, dtype=torch.int32, device="cuda")
    assert lib.mirec_sample_fanout_norep(ctypes.byref(csr), nodes.data_ptr(), n, k,
                                         ctypes.c_uint64(5), ctypes.c_uint64(0), ch.data_ptr(),
                                         st) == 0
    ids = ch.cpu().numpy()
    for r in range(n):   # all neighbours, in row order, then -1
        deg = rowptr[r + 1] - rowptr[r]
        assert np.array_equal(ids[r * k: r * k + deg], col[rowptr[r]:rowptr[r + 1]])
        assert np.all(ids[r * k + deg:(r + 1) * k] == -1)
    zc = np.where(ids[:, None] >= 0, z[np.maximum(ids, 0)], 0).astype(np.float32)
    d = dict(zc=zc, zs=z, a_src=a_s, a_dst=a_d, bias=b, valid=ids)
    out, _ = _run_fwd((n, k, H, C), d)
    tree, clean = out.get((n, H * C))
    assert clean
    ref, bound = gc.dense_full(z, rowptr, col, a_s, a_d, b, H)
    bound = np.minimum(bound, gc.CAP * np.abs(ref).max())
    _check("tree", tree, ref, bound, {})
    _check("csr", full, ref, bound, {})
    assert np.all(np.abs(tree.astype(np.float64) - full) <= 2 * bound)
