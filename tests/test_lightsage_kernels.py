"""csrc/lightsage.hip called directly through the C ABI against float64 numpy
with the host-made dropout mask: mirec_fanout_resmean_gather,
mirec_fanout_resmean and mirec_fanout_resmean_bwd.

Conventions (tests/test_sage_kernels.py's).  Every output buffer starts as one
quiet-NaN bit pattern and is longer than what the kernel should write; the
excess is compared bitwise.  Every call runs twice into fresh buffers and must
repeat bitwise.

Tolerance: none is measured.  Which elements are dropped is an integer
function of (seed, element index) restated on the host and compared exactly;
a forward value is held to gamma(cnt + 5) * (|self| + sum |term|), a kept
element of the backward to gamma(4) * |ref| (tests/lightsage_common.py's
docstring); grad_self is a copy and is compared bitwise.

Shapes: lightsage_common.kernel_cases — dropout_common.fanout_cases with
fanout_ids as the child ids (a target with no valid child, one with a single
valid slot, one with a repeated id; d4 in {1, 2, 3, 16, 64, 65, 128}; k across
the batch of 8 and up to 70; p in {0, 0.3, 0.5}; three seeds, one above 2^63;
the smallest shapes (1, 1, 64) and (1, 25, 8)), self ids random with
self_ids[0] = -1, and one case where a -1 self row has valid children.
tests/test_lightsage_host.py holds that coverage.
"""
import functools

import numpy as np
import pytest
import torch

from tests import dropout_common as dc
from tests import lightsage_common as lc

pytestmark = pytest.mark.gpu

CANARY = 0x7FC5A5A5
PAD = 13
ERR_ARG = 1
CASES = lc.kernel_cases()


def _cid(c):
    return f"t{c['n_t']}k{c['k']}d{c['dim']}p{c['p']}r{c['n_rows']}s{len(c['neg_self'])}"


IDS = [_cid(c) for c in CASES]


def _api():
    from furusato_recommend_amd import _lib
    return _lib.lib, _lib.stream_handle()


def _canary_f32(n):
    return torch.full((n + PAD,), CANARY, dtype=torch.int32, device="cuda").view(torch.float32)


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _split(buf, n, shape):
    a = _np(buf)
    return a[:n].reshape(shape), bool(np.all(_bits(a[n:]) == CANARY))


def _all_canary(buf):
    return bool(np.all(_bits(_np(buf)) == CANARY))


def _check_bound(tag, got, ref, bound):
    got = np.asarray(got)
    assert np.isfinite(got).all(), (tag, np.argwhere(~np.isfinite(got))[:5].tolist())
    err = np.abs(got.astype(np.float64) - ref)
    bound = np.broadcast_to(bound, err.shape)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print(f"[lightsage] {tag}: max err / bound = {ratio:.4f}")
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0 and np.isfinite(ratio), (tag, bad[:5].tolist(), float(err.max()), ratio)


@functools.lru_cache(maxsize=None)
def _data(i):
    """Host inputs and float64 references of a case, computed once."""
    c = CASES[i]
    n_t, k, dim, n_rows = c["n_t"], c["k"], c["dim"], c["n_rows"]
    rng = np.random.default_rng([n_t, k, dim, n_rows, 41, i])
    ids, sid = dc.fanout_ids(c), lc.self_ids(c)
    table = rng.standard_normal((n_rows, dim)).astype(np.float32)
    g = (rng.uniform(0.5, 1.5, (n_t, dim)) * rng.choice([-1.0, 1.0], (n_t, dim))).astype(np.float32)
    x_all = rng.standard_normal((n_t * k, dim)).astype(np.float32)    # valid = NULL children
    mask, scale = dc.fanout_mask(c["p"], c["seed"], n_t * k, dim)
    zero = np.float32(0)
    rows_c = np.where((ids >= 0)[:, None], table[np.maximum(ids, 0)], zero)
    rows_s = np.where((sid >= 0)[:, None], table[np.maximum(sid, 0)], zero)
    for a in (ids, sid, table, g, x_all, mask, rows_c, rows_s):
        a.setflags(write=False)
    return dict(c=c, ids=ids, sid=sid, table=table, g=g, x_all=x_all, mask=mask, scale=scale,
                rows_c=rows_c, rows_s=rows_s)


# ------------------------------------------------------------------- forward
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_resmean_forward(i):
    """Both forward forms against the float64 loop with the host mask; the
    gather form equals the plain form on table[ids] bit for bit; a target
    without a valid child gets its self row; valid = NULL is all-valid."""
    lib, st = _api()
    d = _data(i)
    c, ids, sid = d["c"], d["ids"], d["sid"]
    n_t, k, dim, p, seed = c["n_t"], c["k"], c["dim"], c["p"], c["seed"]
    n_out = n_t * dim
    table_d, ids_d, sid_d = _dev(d["table"], np.float32), _dev(ids, np.int32), _dev(sid, np.int32)
    rows_c_d, rows_s_d = _dev(d["rows_c"], np.float32), _dev(d["rows_s"], np.float32)
    ref, A, cnt = lc.hop_loop(d["rows_s"], d["rows_c"], ids, k, d["mask"], d["scale"])
    bound = lc.fwd_bound(A, cnt)
    runs = []
    for _ in range(2):
        fus, unf = _canary_f32(n_out), _canary_f32(n_out)
        assert lib.mirec_fanout_resmean_gather(table_d.data_ptr(), sid_d.data_ptr(),
                                               ids_d.data_ptr(), n_t, k, dim, p, seed,
                                               fus.data_ptr(), st) == 0
        assert lib.mirec_fanout_resmean(rows_s_d.data_ptr(), rows_c_d.data_ptr(), ids_d.data_ptr(),
                                        n_t, k, dim, p, seed, unf.data_ptr(), st) == 0
        f, cf = _split(fus, n_out, (n_t, dim))
        u, cu = _split(unf, n_out, (n_t, dim))
        assert cf and cu
        runs.append((f, u))
    (f, u), (f2, u2) = runs
    assert np.array_equal(_bits(f), _bits(f2)) and np.array_equal(_bits(u), _bits(u2))
    assert np.array_equal(_bits(f), _bits(u))             # the same sums in the same order
    _check_bound(f"fwd gather {_cid(c)}", f, ref, bound)
    _check_bound(f"fwd rows {_cid(c)}", u, ref, bound)
    none = cnt == 0
    assert np.array_equal(_bits(f[none]), _bits(d["rows_s"][none]))
    neg = np.flatnonzero((sid < 0) & ~none)               # no self row: the mean alone
    if neg.size:
        mean_only, _, _ = lc.hop_loop(np.zeros_like(d["rows_s"]), d["rows_c"], ids, k, d["mask"],
                                      d["scale"])
        _check_bound(f"fwd -1 self {_cid(c)}", f[neg], mean_only[neg], bound[neg])
    assert len(c["neg_self"]) < 2 or neg.size >= 1

    # valid = NULL equals all-valid flags, and the float64 loop over every slot
    x_d = _dev(d["x_all"], np.float32)
    ones_d = _dev(np.zeros(n_t * k), np.int32)
    ref0, A0, cnt0 = lc.hop_loop(d["rows_s"], d["x_all"], None, k, d["mask"], d["scale"])
    outs = []
    for vptr in (None, ones_d.data_ptr(), None):
        o = _canary_f32(n_out)
        assert lib.mirec_fanout_resmean(rows_s_d.data_ptr(), x_d.data_ptr(), vptr, n_t, k, dim, p,
                                        seed, o.data_ptr(), st) == 0
        a, clean = _split(o, n_out, (n_t, dim))
        assert clean
        outs.append(a)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    assert np.array_equal(_bits(outs[0]), _bits(outs[2]))
    _check_bound(f"fwd null {_cid(c)}", outs[0], ref0, lc.fwd_bound(A0, cnt0))


# ------------------------------------------------------------------ backward
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_resmean_bwd(i):
    """grad_self is grad_out bit for bit; grad_child's zero pattern is the
    host mask (|g| >= 0.5), invalid slots and dropped elements are +0, kept
    elements within gamma(4) |ref|; valid = ids and valid = NULL."""
    lib, st = _api()
    d = _data(i)
    c, ids = d["c"], d["ids"]
    n_t, k, dim, p, seed = c["n_t"], c["k"], c["dim"], c["p"], c["seed"]
    n_s, n_c = n_t * dim, n_t * k * dim
    g_d, ids_d = _dev(d["g"], np.float32), _dev(ids, np.int32)
    for tag, valid, vptr in (("ids", ids, ids_d.data_ptr()), ("null", None, None)):
        ref_s, ref_c = lc.backward_closed(d["g"], valid, k, d["mask"], d["scale"])
        ok = np.ones(n_t * k, bool) if valid is None else valid >= 0
        live = ok[:, None] & d["mask"]
        assert np.array_equal(ref_c != 0, live)
        outs = []
        for _ in range(2):
            gs, gc_ = _canary_f32(n_s), _canary_f32(n_c)
            assert lib.mirec_fanout_resmean_bwd(g_d.data_ptr(), vptr, n_t, k, dim, p, seed,
                                                gs.data_ptr(), gc_.data_ptr(), st) == 0
            a, ca = _split(gs, n_s, (n_t, dim))
            b, cb = _split(gc_, n_c, (n_t * k, dim))
            assert ca and cb
            outs.append((a, b))
        (a, b), (a2, b2) = outs
        assert np.array_equal(_bits(a), _bits(a2)) and np.array_equal(_bits(b), _bits(b2))
        assert np.array_equal(_bits(a), _bits(d["g"]))
        assert np.array_equal(b != 0, live), (tag, int(((b != 0) != live).sum()))
        assert np.all(_bits(b)[~live] == 0)
        _check_bound(f"bwd {tag} {_cid(c)}", b, ref_c, lc.bwd_bound(ref_c))


# ------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_alone():
    """dim = 6, k = 0, p = 1, p = NaN, p < 0 and a NULL output -> MIREC_ERR_ARG
    from all three entry points; n_targets = 0 -> OK; nothing written."""
    lib, st = _api()
    n_t, k, dim = 3, 4, 8
    src = _dev(np.ones((64, 8)), np.float32)
    ids = _dev(np.zeros(64), np.int32)
    out, out2 = _canary_f32(64 * 8), _canary_f32(64 * 8)
    s, v, o, o2 = src.data_ptr(), ids.data_ptr(), out.data_ptr(), out2.data_ptr()

    def every(n_t, k, dim, p, o=o, o2=o2):
        return {
            "gather": lib.mirec_fanout_resmean_gather(s, v, v, n_t, k, dim, p, 5, o, st),
            "rows": lib.mirec_fanout_resmean(s, s, v, n_t, k, dim, p, 5, o, st),
            "rows_null": lib.mirec_fanout_resmean(s, s, None, n_t, k, dim, p, 5, o, st),
            "bwd": lib.mirec_fanout_resmean_bwd(s, v, n_t, k, dim, p, 5, o, o2, st),
        }

    for bad in ((n_t, k, 6, 0.3), (n_t, 0, dim, 0.3), (n_t, -1, dim, 0.3), (n_t, k, dim, 1.0),
                (n_t, k, dim, float("nan")), (n_t, k, dim, -0.1), (0, k, dim, 1.0),
                (-1, k, dim, 0.3), (n_t, k, 0, 0.3)):
        rcs = every(*bad)
        assert all(rc == ERR_ARG for rc in rcs.values()), (bad, rcs)
    rcs = every(n_t, k, dim, 0.3, o=None)
    assert all(rc == ERR_ARG for rc in rcs.values()), rcs
    assert lib.mirec_fanout_resmean_bwd(s, v, n_t, k, dim, 0.3, 5, o, None, st) == ERR_ARG
    assert lib.mirec_fanout_resmean_gather(None, v, v, n_t, k, dim, 0.3, 5, o, st) == ERR_ARG
    assert lib.mirec_fanout_resmean_gather(s, None, v, n_t, k, dim, 0.3, 5, o, st) == ERR_ARG
    rcs = every(0, k, dim, 0.3)
    assert all(rc == 0 for rc in rcs.values()), rcs
    assert _all_canary(out) and _all_canary(out2)
