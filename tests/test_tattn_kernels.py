"""csrc/tattn.hip called directly through the C ABI against the float64
restatement of tests/tattn_common.py: mirec_fanout_tattn,
mirec_fanout_tattn_bwd and mirec_csr_tattn.

Conventions (tests/test_gat_kernels.py's).  Every output buffer is one
quiet-NaN bit pattern before the call, with PAD canary floats before and after
the part the kernel should write; the canaries are compared bitwise.  Every
call runs twice into fresh buffers and must repeat bitwise.  Slots of alpha
and rows of grad_key / grad_value that belong to an invalid child are exactly
0; a target without a valid child gets its skip row bit for bit.

Cases: tattn_common.CASES x valid in {NULL, all valid, all -1, ~30 % -1 with
the last target childless} x input variance {1, 60} (at 60 the logits have a
standard deviation of about 60 and exp without the max subtraction overflows
float32; tests/test_tattn_host.py holds that for every case).  No kernel has a
capped grid or a grid-stride loop, so there is no second-round case.  The
backward is given the float32-rounded reference alpha, so it is tested on its
own.

Layouts: every case runs with contiguous separate buffers (every stride D) and
with fused buffers (every stride 2 D: key at +0 and value at +D of one [n_t k,
2 D] buffer, query at +0 and skip at +D of one [n_t, 2 D] buffer, the
gradients the same way); the two must agree bitwise.  Where the kernel must
not write into a fused buffer (the skip half without grad_skip) that half
keeps the canary.

Tolerance: the bounds derived in tattn_common's docstring (logit error, one
explicit exp constant, gamma(m) * A for the sums), capped at 1e-4 * max
|reference| of the tensor.  Nothing is measured into them.  The largest err /
bound of every output is printed per case; DESIGN.md section 22 records the
largest over all cases as measured on an MI355X.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import gat_common as gc
from tests import tattn_common as tc

pytestmark = pytest.mark.gpu

CANARY = 0x7FC5A5A5
PAD = 64   # floats: whole rows of every case fit, and 16-byte alignment is kept
ERR_ARG = 1
COMBOS = [(c, m, s) for c in tc.CASES for m in tc.VALID_MODES for s in tc.SCALES]
LAYOUTS = ("contig", "fused")


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


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check(tag, got, ref, bound, worst):
    got = np.asarray(got)
    assert np.isfinite(got).all(), (tag, np.argwhere(~np.isfinite(got))[:5].tolist())
    err = np.abs(got.astype(np.float64) - ref)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    worst[tag] = max(worst.get(tag, 0.0), ratio)
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0 and np.isfinite(ratio), (tag, bad[:5].tolist(), float(err.max()), ratio)


# ---------------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def _ref(case, mode, scale):
    """Inputs and float64 references of one combination, computed once."""
    n_t, k, H, C = case
    d = tc.make_inputs(case, mode, scale)
    args = (d["q"], d["skip"], d["key"], d["val"], d["valid"], k, H)
    out, alpha, s = tc.tree_loop(*args)
    b_out, b_alpha = tc.fwd_bounds(*args, alpha, s, out)
    a32 = alpha.astype(np.float32)
    grads = tc.backward_closed(d["g"], d["q"], d["key"], d["val"], d["valid"], a32, k, H)
    b_grads = tc.bwd_bounds(d["g"], d["q"], d["key"], d["val"], d["valid"], a32, k, H, grads)
    for a in list(d.values()) + [out, alpha, a32, b_out, b_alpha, *grads, *b_grads]:
        if a is not None:
            a.setflags(write=False)
    return dict(d=d, out=out, alpha=alpha, a32=a32, b_out=b_out, b_alpha=b_alpha, grads=grads,
                b_grads=b_grads, ok=tc.valid_mask(d["valid"], n_t, k))


def _pair(a, b, layout):
    """Device rows (a | b): (pointer of a, pointer of b, stride in floats,
    the tensors to keep alive)."""
    D = a.shape[1]
    if layout == "contig":
        ta, tb = _dev(a), _dev(b)
        return ta.data_ptr(), tb.data_ptr(), D, (ta, tb)
    t = _dev(np.concatenate([a, b], axis=1))
    return t.data_ptr(), t.data_ptr() + 4 * D, 2 * D, (t,)


class OutPair:
    """Two output row sets [n, D] in the layout: separate canary-padded
    buffers, or the halves of one canary-padded [n, 2 D] buffer."""

    def __init__(self, n, D, layout):
        self.n, self.D, self.layout = n, D, layout
        if layout == "contig":
            self.a, self.b = Out(n * D), Out(n * D)
            self.pa, self.pb, self.ld = self.a.ptr, self.b.ptr, D
        else:
            self.a = self.b = Out(n * 2 * D)
            self.pa, self.pb, self.ld = self.a.ptr, self.a.ptr + 4 * D, 2 * D

    def get(self):
        """(rows a, rows b, canaries clean); a half nobody wrote comes back as
        the canary pattern."""
        if self.layout == "contig":
            a, c1 = self.a.get((self.n, self.D))
            b, c2 = self.b.get((self.n, self.D))
            return a, b, c1 and c2
        ab, clean = self.a.get((self.n, 2 * self.D))
        return ab[:, :self.D].copy(), ab[:, self.D:].copy(), clean


def _run_fwd(case, d, layout="contig", skip=True, keep_alpha=True):
    lib, st = _api()
    n_t, k, H, C = case
    pq, ps, ld_q, keep1 = _pair(d["q"], d["skip"], layout)
    pk, pv, ld_kv, keep2 = _pair(d["key"], d["val"], layout)
    valid = _dev(d["valid"], np.int32)
    out, alpha = Out(n_t * H * C), Out(n_t * k * H)
    rc = lib.mirec_fanout_tattn(pq, ps if skip else None, ld_q, pk, pv, ld_kv,
                                None if valid is None else valid.data_ptr(), n_t, k, H, C,
                                float(tc.kernel_scale(C)), out.ptr,
                                alpha.ptr if keep_alpha else None, st)
    assert rc == 0
    torch.cuda.synchronize()
    return out, alpha


def _run_bwd(case, d, a32, layout="contig", grad_skip=True):
    lib, st = _api()
    n_t, k, H, C = case
    D = H * C
    g, alpha = _dev(d["g"]), _dev(a32)
    pq, _, ld_q, keep1 = _pair(d["q"], d["skip"], layout)
    pk, pv, ld_kv, keep2 = _pair(d["key"], d["val"], layout)
    valid = _dev(d["valid"], np.int32)
    gqs, gkv = OutPair(n_t, D, layout), OutPair(n_t * k, D, layout)
    rc = lib.mirec_fanout_tattn_bwd(g.data_ptr(), pq, ld_q, pk, pv, ld_kv,
                                    None if valid is None else valid.data_ptr(),
                                    alpha.data_ptr(), n_t, k, H, C, float(tc.kernel_scale(C)),
                                    gqs.pa, gqs.pb if grad_skip else None, gqs.ld, gkv.pa, gkv.pb,
                                    gkv.ld, st)
    assert rc == 0
    torch.cuda.synchronize()
    return gqs, gkv


# ------------------------------------------------------------------- forward
@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_fanout_tattn_forward(combo):
    case, mode, scale = combo
    n_t, k, H, C = case
    r = _ref(*combo)
    worst = {}
    runs = []
    for layout in LAYOUTS:
        for _ in range(2):
            out, alpha = _run_fwd(case, r["d"], layout)
            o, c1 = out.get((n_t, H * C))
            a, c2 = alpha.get((n_t, k, H))
            assert c1 and c2, "canary overwritten"
            runs.append((o, a))
    for o, a in runs[1:]:   # two runs, and the two layouts, agree bitwise
        assert np.array_equal(_bits(runs[0][0]), _bits(o))
        assert np.array_equal(_bits(runs[0][1]), _bits(a))
    o, a = runs[0]
    _check("out", o, r["out"], r["b_out"], worst)
    _check("alpha", a, r["alpha"], r["b_alpha"], worst)
    assert np.all(_bits(a[~r["ok"]]) == 0), "alpha of an invalid slot is not +0"
    none = ~r["ok"].any(1)
    assert mode not in ("none", "some") or none.any()
    assert mode != "none" or none.all()
    assert np.array_equal(_bits(o[none]), _bits(r["d"]["skip"][none])), "not the skip row"
    print(f"[tattn] fwd {_cid(combo)}: err/bound out {worst['out']:.4f} alpha {worst['alpha']:.4f}")


# ------------------------------------------------------------------ backward
NAMES = ("grad_query", "grad_key", "grad_value")


@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_fanout_tattn_backward(combo):
    case, mode, scale = combo
    n_t, k, H, C = case
    D = H * C
    r = _ref(*combo)
    runs = []
    for layout in LAYOUTS:
        for _ in range(2):
            gqs, gkv = _run_bwd(case, r["d"], r["a32"], layout)
            gq, gs, c1 = gqs.get()
            gk, gv, c2 = gkv.get()
            assert c1 and c2, "canary overwritten"
            runs.append((gq, gk, gv, gs))
    for other in runs[1:]:
        for a, b, name in zip(runs[0], other, NAMES + ("grad_skip",)):
            assert np.array_equal(_bits(a), _bits(b)), f"{name} differs between runs / layouts"
    gq, gk, gv, gs = runs[0]
    worst = {}
    for name, got, ref, bound in zip(NAMES, (gq, gk, gv), r["grads"], r["b_grads"]):
        _check(name, got, ref, bound, worst)
    assert np.array_equal(_bits(gs), _bits(r["d"]["g"])), "grad_skip is not grad_out"
    bad = ~r["ok"].reshape(-1)
    assert np.all(_bits(gk[bad]) == 0) and np.all(_bits(gv[bad]) == 0), \
        "gradient rows of an invalid slot are not +0"
    assert np.all(_bits(gq[~r["ok"].any(1)]) == 0), "grad_query of a childless target is not +0"
    print(f"[tattn] bwd {_cid(combo)}: err/bound " +
          " ".join(f"{n} {worst[n]:.4f}" for n in NAMES))


# ------------------------------------------------- NULL skip / alpha / grad_skip
def test_null_pointer_variants():
    case, mode, scale = (33, 10, 8, 8), "some", 1.0
    n_t, k, H, C = case
    D = H * C
    r = _ref(case, mode, scale)
    d = r["d"]
    full, _ = _run_fwd(case, d)
    o1, _ = full.get((n_t, D))
    for layout in LAYOUTS:
        # alpha = NULL: the same out, the alpha buffer untouched
        out, alpha = _run_fwd(case, d, layout, keep_alpha=False)
        o2, clean = out.get((n_t, D))
        assert clean and alpha.untouched() and np.array_equal(_bits(o1), _bits(o2))
        # skip = NULL: the aggregate alone; a childless target gets +0
        out, _ = _run_fwd(case, d, layout, skip=False)
        o3, clean = out.get((n_t, D))
        assert clean
        ref = r["out"] - d["skip"].astype(np.float64)
        _check("out", o3, ref, r["b_out"], {})
        assert np.all(_bits(o3[~r["ok"].any(1)]) == 0)
    # grad_skip = NULL: the other three unchanged, nothing written for skip
    want_q, want_s, _ = _run_bwd(case, d, r["a32"])[0].get()
    for layout in LAYOUTS:
        gqs, gkv = _run_bwd(case, d, r["a32"], layout, grad_skip=False)
        gq, gs, clean = gqs.get()
        assert clean and np.array_equal(_bits(gq), _bits(want_q))
        if layout == "contig":
            assert gqs.b.untouched()
        else:   # the skip half of every fused row keeps the canary
            assert np.all(_bits(gs) == CANARY)
    assert np.array_equal(_bits(want_s), _bits(d["g"]))


def test_padded_stride_leaves_the_row_tails_alone():
    """A stride above 2 D (rows of 2 D + 4 floats): the four floats after each
    gradient row keep the canary."""
    lib, st = _api()
    case = (33, 10, 8, 8)
    n_t, k, H, C = case
    D = H * C
    ld = 2 * D + 4
    r = _ref(case, "some", 1.0)
    d = r["d"]

    def rows(a, b):
        n = a.shape[0]
        buf = np.zeros((n, ld), np.float32)
        buf[:, :D], buf[:, D:2 * D] = a, b
        return _dev(buf)

    qs, kv = rows(d["q"], d["skip"]), rows(d["key"], d["val"])
    valid, g, alpha = _dev(d["valid"], np.int32), _dev(d["g"]), _dev(r["a32"])
    out = Out(n_t * D)
    assert lib.mirec_fanout_tattn(qs.data_ptr(), qs.data_ptr() + 4 * D, ld, kv.data_ptr(),
                                  kv.data_ptr() + 4 * D, ld, valid.data_ptr(), n_t, k, H, C,
                                  float(tc.kernel_scale(C)), out.ptr, None, st) == 0
    o, clean = out.get((n_t, D))
    assert clean
    _check("out", o, r["out"], r["b_out"], {})
    gqs, gkv = Out(n_t * ld), Out(n_t * k * ld)
    assert lib.mirec_fanout_tattn_bwd(g.data_ptr(), qs.data_ptr(), ld, kv.data_ptr(),
                                      kv.data_ptr() + 4 * D, ld, valid.data_ptr(),
                                      alpha.data_ptr(), n_t, k, H, C, float(tc.kernel_scale(C)),
                                      gqs.ptr, gqs.ptr + 4 * D, ld, gkv.ptr, gkv.ptr + 4 * D, ld,
                                      st) == 0
    a, c1 = gqs.get((n_t, ld))
    b, c2 = gkv.get((n_t * k, ld))
    assert c1 and c2
    assert np.all(_bits(a[:, 2 * D:]) == CANARY) and np.all(_bits(b[:, 2 * D:]) == CANARY)
    for got, ref, bound in zip((a[:, :D], b[:, :D], b[:, D:2 * D]), r["grads"], r["b_grads"]):
        _check("grad", got, ref, bound, {})
    assert np.array_equal(_bits(a[:, D:2 * D]), _bits(d["g"]))


def test_forward_and_backward_chain():
    """tconv.fanout_tattn forward then backward (the pair as autograd uses it:
    fused buffers, the forward kernel's own alpha) against float64 autograd of
    the edge-list form, by max-norm per tensor at 1e-4."""
    from furusato_recommend_amd.tconv import fanout_tattn
    case = (65, 25, 8, 16)
    n_t, k, H, C = case
    D = H * C
    d = _ref(case, "some", 1.0)["d"]
    kv = _dev(np.concatenate([d["key"], d["val"]], 1)).requires_grad_(True)
    qs = _dev(np.concatenate([d["q"], d["skip"]], 1)).requires_grad_(True)
    out = fanout_tattn(kv, qs, _dev(d["valid"], np.int32), k, H)
    out.backward(_dev(d["g"]))
    ts = {n: torch.from_numpy(d[n].astype(np.float64)).requires_grad_(True)
          for n in ("q", "skip", "key", "val")}
    ref = tc.tree_level(ts["q"], ts["skip"], ts["key"], ts["val"], d["valid"], k, H)
    ref.backward(torch.from_numpy(d["g"].astype(np.float64)))
    got = {"out": out.detach(), "q": qs.grad[:, :D], "skip": qs.grad[:, D:],
           "key": kv.grad[:, :D], "val": kv.grad[:, D:]}
    want = dict({n: t.grad for n, t in ts.items()}, out=ref.detach())
    for name in got:
        a, b = got[name].double().cpu().numpy(), want[name].numpy()
        rel = np.abs(a - b).max() / np.abs(b).max()
        print(f"[tattn] chain {name}: rel {rel:.2e}")
        assert rel <= tc.CAP, (name, rel)


# --------------------------------------------------------------- bad shapes
BAD = [dict(k=0), dict(k=65), dict(H=9), dict(C=6), dict(H=5, C=52), dict(n_t=-1), dict(ld=4),
       dict(ld=18)]


@pytest.mark.parametrize("bad", BAD, ids=str)
def test_refused_calls_launch_nothing(bad):
    lib, st = _api()
    n_t, k, H, C = bad.get("n_t", 3), bad.get("k", 5), bad.get("H", 4), bad.get("C", 4)
    ld = bad.get("ld", max(H * C, 4))
    n = 4096
    ins = [torch.zeros(n, device="cuda") for _ in range(6)]
    valid = torch.zeros(n, dtype=torch.int32, device="cuda")
    outs = [Out(n) for _ in range(6)]
    p = [t.data_ptr() for t in ins]
    assert lib.mirec_fanout_tattn(p[0], p[1], ld, p[2], p[3], ld, valid.data_ptr(), n_t, k, H, C,
                                  0.5, outs[0].ptr, outs[1].ptr, st) == ERR_ARG
    assert lib.mirec_fanout_tattn_bwd(p[4], p[0], ld, p[2], p[3], ld, valid.data_ptr(), p[5], n_t,
                                      k, H, C, 0.5, outs[2].ptr, outs[3].ptr, ld, outs[4].ptr,
                                      outs[5].ptr, ld, st) == ERR_ARG
    if "k" not in bad and "n_t" not in bad:
        from furusato_recommend_amd._lib import CSR
        rowptr = torch.zeros(4, dtype=torch.int64, device="cuda")
        csr = CSR(rowptr=rowptr.data_ptr(), col=valid.data_ptr(), n_rows=3, nnz=0)
        assert lib.mirec_csr_tattn(ctypes.byref(csr), p[0], p[1], ld, p[2], p[3], ld, H, C, 0.5,
                                   outs[0].ptr, st) == ERR_ARG
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
    return tuple((rng.standard_normal((n, H * C)) * sd).astype(np.float32) for _ in range(4))


def _run_csr(csr, q, skip, key, val, H, C, layout="fused"):
    lib, st = _api()
    n = q.shape[0]
    pq, ps, ld_q, keep1 = _pair(q, skip, layout)
    pk, pv, ld_kv, keep2 = _pair(key, val, layout)
    out = Out(n * H * C)
    assert lib.mirec_csr_tattn(ctypes.byref(csr), pq, ps, ld_q, pk, pv, ld_kv, H, C,
                               float(tc.kernel_scale(C)), out.ptr, st) == 0
    o, clean = out.get((n, H * C))
    assert clean, "canary overwritten"
    return o


@pytest.mark.parametrize("H,C", [(8, 4), (8, 16), (2, 12), (4, 32)], ids=str)
@pytest.mark.parametrize("scale", tc.SCALES)
def test_csr_tattn(H, C, scale):
    """The 37 x 11 graph (duplicates, an isolated item, a degree-1 user, a
    hub of degree 324).  The kernel has one path for every degree (one lane
    group walks the row in batches of 8, its lanes exchanging inside the
    loop), which the hub, the degree-1 row and the empty row all take beside
    each other in one wave: ragged tails 324 % 8 = 4, 1, 0.  (2, 12) is the
    head width whose lanes are not a power of two."""
    u, i, nu, mi = gc.csr_graph_edges()
    rowptr, col = gc.host_csr(u, i, nu, mi)
    n = nu + mi
    q, skip, key, val = _csr_inputs(n, H, C, scale, 1)
    ref, bound = tc.dense_full(q, skip, key, val, rowptr, col, H)
    bound = np.minimum(bound, tc.CAP * np.abs(ref).max())
    csr, keep = _device_csr(rowptr, col)
    o1 = _run_csr(csr, q, skip, key, val, H, C)
    o2 = _run_csr(csr, q, skip, key, val, H, C)
    o3 = _run_csr(csr, q, skip, key, val, H, C, layout="contig")
    assert np.array_equal(_bits(o1), _bits(o2)) and np.array_equal(_bits(o1), _bits(o3))
    worst = {}
    _check("csr out", o1, ref, bound, worst)
    iso = nu + 10
    assert np.array_equal(_bits(o1[iso]), _bits(skip[iso]))     # degree 0: the skip row
    print(f"[tattn] csr h{H}c{C} v{int(scale)}: err/bound {worst}")


def test_csr_tattn_skips_entries_outside_the_graph():
    """col entries outside [0, n_rows) are skipped: a row made of them alone
    is an isolated row."""
    H, C, n = 4, 8, 5
    rowptr = np.array([0, 2, 5, 5, 6, 8], np.int64)
    col = np.array([1, 4, -1, 2, 7, 9, 0, 5], np.int32)        # row 3: only 9; 5 == n
    q, skip, key, val = _csr_inputs(n, H, C, 1.0, 4)
    keep = (col >= 0) & (col < n)
    rp2 = np.concatenate([[0], np.cumsum([keep[rowptr[r]:rowptr[r + 1]].sum() for r in range(n)])])
    ref, bound = tc.dense_full(q, skip, key, val, rp2.astype(np.int64), col[keep], H)
    csr, hold = _device_csr(rowptr, col)
    o = _run_csr(csr, q, skip, key, val, H, C)
    _check("csr out", o, ref, np.minimum(bound, tc.CAP * np.abs(ref).max()), {})
    assert np.array_equal(_bits(o[3]), _bits(skip[3]))
    assert np.array_equal(_bits(o[2]), _bits(skip[2]))


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
    q, skip, key, val = _csr_inputs(n, H, C, 1.0, 2)
    csr, keep = _device_csr(rowptr, col)
    full = _run_csr(csr, q, skip, key, val, H, C)
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

    def gather(x):
        return np.where(ids[:, None] >= 0, x[np.maximum(ids, 0)], 0).astype(np.float32)

    d = dict(q=q, skip=skip, key=gather(key), val=gather(val), valid=ids)
    out, _ = _run_fwd((n, k, H, C), d, "fused")
    tree, clean = out.get((n, H * C))
    assert clean
    ref, bound = tc.dense_full(q, skip, key, val, rowptr, col, H)
    bound = np.minimum(bound, tc.CAP * np.abs(ref).max())
    _check("tree", tree, ref, bound, {})
    _check("csr", full, ref, bound, {})
    assert np.all(np.abs(tree.astype(np.float64) - full) <= 2 * bound)
