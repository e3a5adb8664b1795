"""csrc/ggnn.hip called directly through the C ABI against the float64
restatement of tests/ggnn_common.py: mirec_gru_gate and mirec_gru_gate_bwd.

Conventions (tests/test_gat_kernels.py's).  Every output buffer is one
quiet-NaN bit pattern before the call, with PAD canary floats before and after
the part the kernel should write; the canaries are compared bitwise.  Every
call runs twice into fresh buffers and must repeat bitwise — the bias
gradients included, which are ordered column sums (linear.col_sums) of the
backward's grad_gi / grad_gh.

Cases: ggnn_common.CASES x ReLU {off, on} x input variance {1, 30}, the
saturated case (pre-activations from {+-90, +-1e4}: every output and gradient
finite and within its bound) and STRIDE_CASE for the second round of the
grid-stride loop; tests/test_ggnn_host.py holds their coverage.  The backward
takes the forward's float32 ``out`` from the kernel and its reference takes
the ReLU mask from that same ``out``, so it is tested on its own.

Tolerance: the bounds derived in ggnn_common's docstring (one explicit
constant each for the hardware exp2 and reciprocal, the errors carried
through r, z, n), capped at 1e-4 * max |reference| of the tensor.  Nothing is
measured into them.  The largest err / bound over all cases of an output,
measured on an MI355X (how much room the bound leaves; it does not set it), is
printed per case and recorded in DESIGN.md section 25:

    out 0.79   grad_gi 0.61   grad_gh 0.61   grad_h 0.43
    grad_bias_ih 0.44   grad_bias_hh 0.44
"""
import functools

import numpy as np
import pytest
import torch

from tests import ggnn_common as gg

pytestmark = pytest.mark.gpu

CANARY = 0x7FC5A5A5
PAD = 64   # floats: 16-byte alignment is kept
ERR_ARG = 1
COMBOS = [(c, r, s) for c in gg.CASES for r in (False, True) for s in gg.SCALES]


def _cid(x):
    c, r, s = x
    return f"n{c[0]}d{c[1]}-{'relu' if r else 'lin'}-v{int(s)}"


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

    def dev(self, shape):
        return self.buf[PAD:PAD + self.n].view(shape)

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


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()


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
def _inputs(case, scale):
    d = gg.make_saturated(case) if scale == "sat" else gg.make_inputs(case, scale)
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _fwd_ref(case, scale, relu):
    d = _inputs(case, scale)
    ref = gg.gate_np(d["gi"], d["gh"], d["h"], relu)
    bound = gg.fwd_bounds(d["gi"], d["gh"], d["h"], ref)
    ref.setflags(write=False)
    bound.setflags(write=False)
    return ref, bound


def _run_fwd(case, d, relu):
    lib, st = _api()
    n, dim = case
    dev = [_dev(d[k]) for k in ("gi", "gh", "h")]
    out = Out(n * dim)
    rc = lib.mirec_gru_gate(*(t.data_ptr() for t in dev), n, dim, int(relu), out.ptr, st)
    assert rc == 0
    return out


def _run_bwd(case, d, out32):
    """out32: the forward's float32 output (the ReLU mask) or None."""
    from furusato_recommend_amd.linear import col_sums
    lib, st = _api()
    n, dim = case
    dev = [_dev(d[k]) for k in ("g", "gi", "gh", "h")]
    o = None if out32 is None else _dev(out32)
    outs = Out(3 * n * dim), Out(3 * n * dim), Out(n * dim)
    rc = lib.mirec_gru_gate_bwd(*(t.data_ptr() for t in dev), None if o is None else o.data_ptr(),
                                n, dim, outs[0].ptr, outs[1].ptr, outs[2].ptr, st)
    assert rc == 0
    sums = [col_sums(outs[i].dev((n, 3 * dim))).cpu().numpy() for i in (0, 1)]
    return outs, sums


def _fwd_case(case, relu, scale):
    n, dim = case
    d = _inputs(case, scale)
    ref, bound = _fwd_ref(case, scale, relu)
    worst = {}
    (got, clean), (again, clean2) = (_run_fwd(case, d, relu).get((n, dim)) for _ in range(2))
    assert clean and clean2
    assert np.array_equal(_bits(got), _bits(again))
    _check("out", got, ref, bound, worst)
    if relu:
        assert (got >= 0).all()
    print(f"[ggnn fwd {case} relu={relu} v={scale}] err/bound " +
          "  ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    return got


def _bwd_case(case, relu, scale):
    n, dim = case
    d = _inputs(case, scale)
    out32 = _run_fwd(case, d, True).get((n, dim))[0] if relu else None
    mask = None if out32 is None else out32 > 0
    refs = gg.backward_closed(d["g"], d["gi"], d["gh"], d["h"], mask)
    bounds, raw = gg.bwd_bounds(d["g"], d["gi"], d["gh"], d["h"], mask, refs)
    worst = {}
    runs = []
    for _ in range(2):
        outs, sums = _run_bwd(case, d, out32)
        got = [o.get(s) for o, s in zip(outs, ((n, 3 * dim), (n, 3 * dim), (n, dim)))]
        assert all(clean for _, clean in got)
        runs.append([a for a, _ in got] + sums)
    for a, b in zip(*runs):
        assert np.array_equal(_bits(a), _bits(b))
    names = ("grad_gi", "grad_gh", "grad_h")
    for name, got, ref, bound in zip(names, runs[0], refs, bounds):
        _check(name, got, ref, bound, worst)
    if mask is not None:
        # exactly 0 where the ReLU stopped the gradient
        dead = np.tile(~mask, (1, 3))
        assert not runs[0][0][dead].any() and not runs[0][1][dead].any()
        assert not runs[0][2][~mask].any()
    for name, got, ref, rw in zip(("grad_bias_ih", "grad_bias_hh"), runs[0][3:], refs, raw):
        _check(name, got, ref.sum(0), gg.bias_bounds(rw, ref), worst)
    print(f"[ggnn bwd {case} relu={relu} v={scale}] err/bound " +
          "  ".join(f"{k} {v:.2f}" for k, v in worst.items()))


# --------------------------------------------------------------------- tests
@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_forward(combo):
    _fwd_case(*combo)


@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_backward(combo):
    _bwd_case(*combo)


@pytest.mark.parametrize("case", [(33, 64), (3, 12)], ids=str)
def test_saturated_pre_activations_stay_finite(case):
    for relu in (False, True):
        _fwd_case(case, relu, "sat")
        _bwd_case(case, relu, "sat")


def test_grid_stride_round():
    _fwd_case(gg.STRIDE_CASE, True, 1.0)
    _bwd_case(gg.STRIDE_CASE, True, 1.0)


def test_the_largest_finite_pre_activations():
    """+-3e38 in every pre-activation (their sums stay finite): out and the
    gradients are finite."""
    n, dim = 2, 8
    big = np.float32(3e38)
    rng = np.random.default_rng(9)
    sg = lambda *s: rng.choice([-1.0, 1.0], s).astype(np.float32)  # noqa: E731
    gi = sg(n, 3 * dim) * big
    d = dict(gi=gi, gh=np.zeros_like(gi), h=sg(n, dim), g=sg(n, dim))
    d["gh"][:, 2 * dim:] = sg(n, dim) * np.float32(1e-3)
    got, clean = _run_fwd((n, dim), d, False).get((n, dim))
    assert clean and np.isfinite(got).all()
    outs, _ = _run_bwd((n, dim), d, None)
    for o, s in zip(outs, ((n, 3 * dim), (n, 3 * dim), (n, dim))):
        a, clean = o.get(s)
        assert clean and np.isfinite(a).all()


def test_autograd_function_and_shape_checks():
    from furusato_recommend_amd.ggnn import gru_gate
    case = (33, 64)
    d = _inputs(case, 1.0)
    gi, gh, h = (_dev(d[k]).requires_grad_(True) for k in ("gi", "gh", "h"))
    out = gru_gate(gi, gh, h, relu=True)
    ref, bound = _fwd_ref(case, 1.0, True)
    assert (np.abs(out.detach().cpu().numpy() - ref) <= bound).all()
    out.backward(_dev(d["g"]))
    mask = out.detach().cpu().numpy() > 0
    refs = gg.backward_closed(d["g"], d["gi"], d["gh"], d["h"], mask)
    bounds, _ = gg.bwd_bounds(d["g"], d["gi"], d["gh"], d["h"], mask, refs)
    for t, ref, b in zip((gi, gh, h), refs, bounds):
        assert (np.abs(t.grad.cpu().numpy() - ref) <= b).all()
    with pytest.raises(ValueError):
        gru_gate(gi[:, :-4], gh[:, :-4], h)            # gi is not [n, 3d]
    with pytest.raises(ValueError):
        gru_gate(gi.cpu(), gh.cpu(), h.cpu())
    with pytest.raises(ValueError):
        gru_gate(gi.double(), gh.double(), h.double())
    with pytest.raises(ValueError):
        gru_gate(gi[:, :18], gh[:, :18], h[:, :6])     # d % 4


def test_bad_arguments_launch_nothing():
    lib, st = _api()
    n, dim = 5, 8
    d = gg.make_inputs((n, dim), 1.0)
    gi, gh, h, g = (_dev(d[k]) for k in ("gi", "gh", "h", "g"))
    out = Out(n * dim)
    outs = Out(3 * n * dim), Out(3 * n * dim), Out(n * dim)
    p = [t.data_ptr() for t in (gi, gh, h)]
    for bad_dim in (0, 6, -4, 1028):
        assert lib.mirec_gru_gate(*p, n, bad_dim, 0, out.ptr, st) == ERR_ARG
        assert lib.mirec_gru_gate_bwd(g.data_ptr(), *p, None, n, bad_dim, outs[0].ptr,
                                      outs[1].ptr, outs[2].ptr, st) == ERR_ARG
    assert lib.mirec_gru_gate(*p, -1, dim, 0, out.ptr, st) == ERR_ARG
    assert lib.mirec_gru_gate(p[0] + 4, p[1], p[2], n, dim, 0, out.ptr, st) == ERR_ARG
    assert lib.mirec_gru_gate(p[0], p[1], p[2], n, dim, 0, out.ptr + 4, st) == ERR_ARG
    assert lib.mirec_gru_gate(None, p[1], p[2], n, dim, 0, out.ptr, st) == ERR_ARG
    assert lib.mirec_gru_gate_bwd(g.data_ptr(), *p, None, n, dim, outs[0].ptr, None,
                                  outs[2].ptr, st) == ERR_ARG
    assert lib.mirec_gru_gate_bwd(g.data_ptr(), *p, None, n, dim, outs[0].ptr, outs[1].ptr + 8,
                                  outs[2].ptr, st) == ERR_ARG
    # no rows: nothing to do, nothing written
    assert lib.mirec_gru_gate(*p, 0, dim, 1, out.ptr, st) == 0
    assert lib.mirec_gru_gate_bwd(g.data_ptr(), *p, None, 0, dim, outs[0].ptr, outs[1].ptr,
                                  outs[2].ptr, st) == 0
    assert out.untouched() and all(o.untouched() for o in outs)
