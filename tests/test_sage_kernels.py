"""csrc/sage.hip called directly through the C ABI against float64 numpy with
the host-made dropout mask of tests/dropout_common.py: mirec_fanout_mean and
its backward, mirec_fanout_mean_gather and both its backwards (float atomics
and the sorted form), mirec_gather_rows, mirec_scatter_add_rows,
mirec_pack_seed_nodes and mirec_sample_fanout (with replacement).

Conventions (tests/test_ssm_shared_kernels.py's).  Every output buffer starts
as one quiet-NaN bit pattern and is longer than what the kernel should write;
the excess is compared bitwise.  Every call runs twice into fresh buffers and
must repeat bitwise, except the float-atomic kernels, whose two runs are both
held to the bound.  Integer outputs are compared exactly.

Tolerance: none is measured.  The mask is an integer function of (seed,
element index) restated on the host, so which elements are dropped is compared
exactly, and a value that is a sum of m terms is held to gamma(m + 4) * A
(dropout_common's docstring: u = 2^-24, A the sum of the absolute terms, any
summation order).  A kept element of the unfused backward is one term:
gamma(4) * |ref|.

Shapes: dropout_common.fanout_cases / sorted_cases (the dispatch edges of the
unfused backward's count, the batch of 8 of the forward, the 64-child limit of
the atomic backward, the 64-entry chunks and 256-column passes of the sorted
sum); tests/test_dropout_host.py holds their coverage.

Measured on an MI355X, the largest err / bound over all cases of a kernel
(how much room the derived bound leaves; it does not set the bound):

    mirec_fanout_mean (valid = NULL / ids)        0.28 / 0.27
    mirec_fanout_mean_gather                      0.27
    mirec_fanout_mean_bwd (kept elements)         0.41
    mirec_fanout_mean_gather_bwd (atomic)         0.48
    mirec_fanout_mean_gather_bwd_sorted           0.48
    mirec_scatter_add_rows                        0.19
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import dropout_common as dc

pytestmark = pytest.mark.gpu

CANARY = 0x7FC5A5A5
PAD = 13
ERR_ARG, ERR_WORKSPACE = 1, 4
CASES = dc.fanout_cases()
SORTED = dc.sorted_cases()


def _cid(c):
    return f"{c.get('name', 'f')}-t{c['n_t']}k{c['k']}d{c['dim']}p{c['p']}r{c['n_rows']}"


# ------------------------------------------------------------------ plumbing
def _api():
    from furusato_recommend_amd import _lib
    return _lib.lib, _lib.stream_handle()


def _canary_f32(n):
    return torch.full((n + PAD,), CANARY, dtype=torch.int32, device="cuda").view(torch.float32)


def _canary_i32(n):
    return torch.full((n + PAD,), CANARY, dtype=torch.int32, device="cuda")


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _split(buf, n, shape):
    """(written part reshaped, True iff the excess is still the canary)."""
    a = _np(buf)
    return a[:n].reshape(shape), bool(np.all(_bits(a[n:]) == CANARY))


def _all_canary(buf):
    return bool(np.all(_bits(_np(buf)) == CANARY))


def _with_base(base):
    """A device table holding base, then PAD canary floats."""
    t = _canary_f32(base.size)
    t[:base.size] = _dev(base.reshape(-1), np.float32)
    return t


def _check_bound(tag, got, ref, bound):
    """Every element written (no NaN canary left, nothing non-finite) and
    within its bound; NaN fails both assertions."""
    got = np.asarray(got)
    assert np.isfinite(got).all(), (tag, np.argwhere(~np.isfinite(got))[:5].tolist())
    err = np.abs(got.astype(np.float64) - ref)
    bound = np.broadcast_to(bound, err.shape)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print(f"[sage] {tag}: max err / bound = {ratio:.4f}")
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0 and np.isfinite(ratio), (tag, bad[:5].tolist(), float(err.max()), ratio)


# ---------------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def _data(i, sorted_list=False):
    """Host inputs and float64 references of a case, computed once."""
    c = (SORTED if sorted_list else CASES)[i]
    n_t, k, dim, n_rows = c["n_t"], c["k"], c["dim"], c["n_rows"]
    rng = np.random.default_rng([n_t, k, dim, n_rows, 5, int(sorted_list), i])
    ids = c["ids"] if sorted_list else dc.fanout_ids(c)
    table = rng.standard_normal((n_rows, dim)).astype(np.float32)
    base = rng.standard_normal((n_rows, dim)).astype(np.float32)
    g = (rng.uniform(0.5, 1.5, (n_t, dim)) * rng.choice([-1.0, 1.0], (n_t, dim))).astype(np.float32)
    x_all = rng.standard_normal((n_t * k, dim)).astype(np.float32)   # valid = NULL input
    mask, scale = dc.fanout_mask(c["p"], c["seed"], n_t * k, dim)
    for a in (ids, table, base, g, x_all, mask):
        a.setflags(write=False)
    return dict(c=c, ids=ids, table=table, base=base, g=g, x_all=x_all, mask=mask, scale=scale,
                valid=ids >= 0)


@functools.lru_cache(maxsize=None)
def _gather_ref(i, sorted_list):
    d = _data(i, sorted_list)
    return dc.gather_bwd_ref(d["g"], d["ids"], d["c"]["k"], d["mask"], d["scale"], d["base"])


def _gather_rows(lib, st, table, ids, n, dim):
    out = _canary_f32(n * dim)
    assert lib.mirec_gather_rows(table.data_ptr(), ids.data_ptr(), n, dim, out.data_ptr(), st) == 0
    return out


# ------------------------------------------------------------------- forward
@pytest.mark.parametrize("i", range(len(CASES)), ids=[_cid(c) for c in CASES])
def test_fanout_mean_forward(i):
    """mirec_fanout_mean (valid = NULL and valid = ids) and
    mirec_fanout_mean_gather against the float64 mean with the host mask;
    fused == gather_rows + unfused bit for bit; no valid child -> zeros."""
    lib, st = _api()
    d = _data(i)
    c, ids, valid = d["c"], d["ids"], d["valid"]
    n_t, k, dim, p, seed = c["n_t"], c["k"], c["dim"], c["p"], c["seed"]
    n_out = n_t * dim
    table_d, ids_d = _dev(d["table"], np.float32), _dev(ids, np.int32)

    # gather: bitwise table[ids], zeros for -1
    rows_d = _gather_rows(lib, st, table_d, ids_d, n_t * k, dim)
    rows, clean = _split(rows_d, n_t * k * dim, (n_t * k, dim))
    want_rows = np.where(valid[:, None], d["table"][np.maximum(ids, 0)], np.float32(0))
    assert clean and np.array_equal(_bits(rows), _bits(want_rows))

    ref, A, m = dc.fanout_mean_ref(want_rows, valid, k, d["mask"], d["scale"])
    bound = dc.sum_bound(A, m)
    runs = []
    for _ in range(2):
        unf, fus = _canary_f32(n_out), _canary_f32(n_out)
        assert lib.mirec_fanout_mean(rows_d.data_ptr(), ids_d.data_ptr(), n_t, k, dim, p, seed,
                                     unf.data_ptr(), st) == 0
        assert lib.mirec_fanout_mean_gather(table_d.data_ptr(), ids_d.data_ptr(), n_t, k, dim, p,
                                            seed, fus.data_ptr(), st) == 0
        u, cu = _split(unf, n_out, (n_t, dim))
        f, cf = _split(fus, n_out, (n_t, dim))
        assert cu and cf
        runs.append((u, f))
    (u, f), (u2, f2) = runs
    assert np.array_equal(_bits(u), _bits(u2)) and np.array_equal(_bits(f), _bits(f2))
    assert np.array_equal(_bits(u), _bits(f))            # mirec.h: the same mask, one pass
    _check_bound(f"fwd ids {_cid(c)}", u, ref, bound)
    _check_bound(f"fwd gather {_cid(c)}", f, ref, bound)
    none = valid.reshape(n_t, k).sum(1) == 0
    assert np.all(_bits(f[none]) == 0) and np.all(_bits(u[none]) == 0)

    # valid = NULL: every child counts
    x_d = _dev(d["x_all"], np.float32)
    ref0, A0, m0 = dc.fanout_mean_ref(d["x_all"], np.ones(n_t * k, bool), k, d["mask"], d["scale"])
    assert np.all(m0 == k)
    outs = []
    for _ in range(2):
        o = _canary_f32(n_out)
        assert lib.mirec_fanout_mean(x_d.data_ptr(), None, n_t, k, dim, p, seed, o.data_ptr(),
                                     st) == 0
        a, clean = _split(o, n_out, (n_t, dim))
        assert clean
        outs.append(a)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    _check_bound(f"fwd null {_cid(c)}", outs[0], ref0, dc.sum_bound(A0, m0))


# ---------------------------------------------------------- unfused backward
@pytest.mark.parametrize("i", range(len(CASES)), ids=[_cid(c) for c in CASES])
def test_fanout_mean_bwd(i):
    """mirec_fanout_mean_bwd: the zero pattern of grad_x is the host mask
    (|g| >= 0.5), rows of invalid children and dropped elements are +0, kept
    elements within gamma(4) |ref|; valid = ids and valid = NULL."""
    lib, st = _api()
    d = _data(i)
    c, ids = d["c"], d["ids"]
    n_t, k, dim, p, seed = c["n_t"], c["k"], c["dim"], c["p"], c["seed"]
    n_out = n_t * k * dim
    g_d, ids_d = _dev(d["g"], np.float32), _dev(ids, np.int32)
    for tag, valid, vptr in (("ids", d["valid"], ids_d.data_ptr()),
                             ("null", np.ones(n_t * k, bool), None)):
        ref = dc.fanout_mean_bwd_ref(d["g"], valid, k, d["mask"], d["scale"])
        live = valid[:, None] & d["mask"]
        assert np.array_equal(ref != 0, live)
        outs = []
        for _ in range(2):
            o = _canary_f32(n_out)
            assert lib.mirec_fanout_mean_bwd(g_d.data_ptr(), vptr, n_t, k, dim, p, seed,
                                             o.data_ptr(), st) == 0
            a, clean = _split(o, n_out, (n_t * k, dim))
            assert clean
            outs.append(a)
        got = outs[0]
        assert np.array_equal(_bits(got), _bits(outs[1]))
        assert np.array_equal(got != 0, live), (tag, int(((got != 0) != live).sum()))
        assert np.all(_bits(got)[~live] == 0)
        _check_bound(f"bwd {tag} {_cid(c)}", got, ref, dc.gamma(4) * np.abs(ref))


# ----------------------------------------------------------- atomic backward
ATOMIC = [i for i, c in enumerate(CASES) if c["k"] <= 64]


@pytest.mark.parametrize("i", ATOMIC, ids=[_cid(CASES[i]) for i in ATOMIC])
def test_fanout_mean_gather_bwd_atomic(i):
    """mirec_fanout_mean_gather_bwd onto a random base: every row within
    gamma(m + 4) A in both runs; rows no entry names stay base bit for bit."""
    lib, st = _api()
    d = _data(i)
    c, ids = d["c"], d["ids"]
    n_t, k, dim, n_rows = c["n_t"], c["k"], c["dim"], c["n_rows"]
    ref, A, m = _gather_ref(i, False)
    g_d, ids_d = _dev(d["g"], np.float32), _dev(ids, np.int32)
    for run in range(2):
        tg = _with_base(d["base"])
        assert lib.mirec_fanout_mean_gather_bwd(g_d.data_ptr(), ids_d.data_ptr(), n_t, k, dim,
                                                c["p"], c["seed"], tg.data_ptr(), st) == 0
        got, clean = _split(tg, n_rows * dim, (n_rows, dim))
        assert clean
        _check_bound(f"atomic {_cid(c)} run {run}", got, ref, dc.sum_bound(A, m))
        assert np.array_equal(_bits(got[m == 0]), _bits(d["base"][m == 0]))


# ----------------------------------------------------------- sorted backward
def _sorted_ws(lib, c):
    need = ctypes.c_size_t(0)
    assert lib.mirec_fanout_mean_gather_bwd_sorted_workspace(c["n_t"], c["k"], c["n_rows"],
                                                             ctypes.byref(need)) == 0
    return int(need.value)


@pytest.mark.parametrize("i", range(len(SORTED)), ids=[_cid(c) for c in SORTED])
def test_fanout_mean_gather_bwd_sorted(i):
    """mirec_fanout_mean_gather_bwd_sorted: the atomic form's reference and
    bound, bitwise repeatable, untouched rows bitwise base, nothing past the
    workspace; one byte short -> MIREC_ERR_WORKSPACE and nothing written."""
    lib, st = _api()
    d = _data(i, True)
    c, ids = d["c"], d["ids"]
    n_t, k, dim, n_rows = c["n_t"], c["k"], c["dim"], c["n_rows"]
    ref, A, m = _gather_ref(i, True)
    g_d, ids_d = _dev(d["g"], np.float32), _dev(ids, np.int32)
    need = _sorted_ws(lib, c)
    assert need > 0

    def call(ws_bytes):
        tg = _with_base(d["base"])
        ws = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        rc = lib.mirec_fanout_mean_gather_bwd_sorted(
            g_d.data_ptr(), ids_d.data_ptr(), n_t, k, dim, c["p"], c["seed"], n_rows,
            tg.data_ptr(), ws.data_ptr(), ws_bytes, st)
        got, clean = _split(tg, n_rows * dim, (n_rows, dim))
        return rc, got, clean, _np(ws)

    rc, got, clean, ws = call(need)
    rc2, got2, clean2, ws2 = call(need)
    assert rc == rc2 == 0 and clean and clean2
    assert np.all(ws[need:] == 0xA5) and np.all(ws2[need:] == 0xA5)
    assert np.array_equal(_bits(got), _bits(got2))
    _check_bound(f"sorted {_cid(c)}", got, ref, dc.sum_bound(A, m))
    assert np.array_equal(_bits(got[m == 0]), _bits(d["base"][m == 0]))
    if not d["valid"].any():
        assert np.array_equal(_bits(got), _bits(d["base"]))
    rc, got, clean, ws = call(need - 1)
    assert rc == ERR_WORKSPACE and clean and np.all(ws == 0xA5)
    assert np.array_equal(_bits(got), _bits(d["base"]))


# ------------------------------------------------------------- the row movers
@pytest.mark.parametrize("dim", [4, 12, 64, 260, 1024])
@pytest.mark.parametrize("n", [1, 185])
def test_gather_rows(n, dim):
    lib, st = _api()
    rng = np.random.default_rng([n, dim])
    n_rows = 23
    table = rng.standard_normal((n_rows, dim)).astype(np.float32)
    ids = rng.integers(0, n_rows, n).astype(np.int32)
    if n > 3:
        ids[::7] = -1
        ids[3], ids[-1] = ids[1], ids[1]
        assert ids[1] >= 0
    want = np.where((ids >= 0)[:, None], table[np.maximum(ids, 0)], np.float32(0))
    table_d, ids_d = _dev(table, np.float32), _dev(ids, np.int32)
    outs = []
    for _ in range(2):
        a, clean = _split(_gather_rows(lib, st, table_d, ids_d, n, dim), n * dim, (n, dim))
        assert clean
        outs.append(a)
    assert np.array_equal(_bits(outs[0]), _bits(want)) and np.array_equal(_bits(outs[1]), _bits(want))


@pytest.mark.parametrize("dim", [1, 5, 64])
@pytest.mark.parametrize("n", [1, 301])
def test_scatter_add_rows(n, dim):
    """No % 4 rule here.  Held to gamma(m + 4) (|base| + sum |grad|), m the
    repeats of the row; rows no id names stay base bit for bit."""
    lib, st = _api()
    rng = np.random.default_rng([n, dim, 3])
    n_rows = 19
    base = rng.standard_normal((n_rows, dim)).astype(np.float32)
    grad = rng.standard_normal((n, dim)).astype(np.float32)
    ids = rng.integers(0, n_rows - 2, n).astype(np.int32)      # the last two rows: untouched
    if n > 1:
        ids[::5] = -1
        ids[1:40:2] = 4                                          # a row with many repeats
    ref, A, m = dc.scatter_add_ref(grad, ids, base)
    assert m[-1] == 0 and (n == 1 or m[4] >= 20)
    grad_d, ids_d = _dev(grad, np.float32), _dev(ids, np.int32)
    for run in range(2):
        tg = _with_base(base)
        assert lib.mirec_scatter_add_rows(grad_d.data_ptr(), ids_d.data_ptr(), n, dim,
                                          tg.data_ptr(), st) == 0
        got, clean = _split(tg, n_rows * dim, (n_rows, dim))
        assert clean
        _check_bound(f"scatter n{n} d{dim} run {run}", got, ref, dc.sum_bound(A, m))
        assert np.array_equal(_bits(got[m == 0]), _bits(base[m == 0]))


@pytest.mark.parametrize("B", [1, 257])
def test_pack_seed_nodes(B):
    lib, st = _api()
    rng = np.random.default_rng(B)
    n_users = 1000
    u, p, n = (rng.integers(0, 900, B).astype(np.int32) for _ in range(3))
    want = np.concatenate([u, n_users + p, n_users + n]).astype(np.int32)
    u_d, p_d, n_d = (_dev(a, np.int32) for a in (u, p, n))
    outs = []
    for _ in range(2):
        o = _canary_i32(3 * B)
        assert lib.mirec_pack_seed_nodes(u_d.data_ptr(), p_d.data_ptr(), n_d.data_ptr(), B,
                                         n_users, o.data_ptr(), st) == 0
        a, clean = _split(o, 3 * B, (3 * B,))
        assert clean
        outs.append(a)
    assert np.array_equal(outs[0], want) and np.array_equal(outs[1], want)
    o = _canary_i32(4)
    assert lib.mirec_pack_seed_nodes(None, None, None, 0, n_users, o.data_ptr(), st) == 0
    assert _all_canary(o)


# ------------------------------------------------ the sampler with replacement
@pytest.mark.parametrize("k", [1, 25])
def test_sample_fanout_exact_draws(k):
    """children[i] = col[beg + ((mix64(mix64(seed) ^ (offset + i)) * deg) >>
    64)] for a node inside the graph with deg > 0, else -1: an empty row, a
    row of one entry, node ids < 0 and >= n_rows, offset + i across 2^32."""
    from furusato_recommend_amd import _lib
    lib, st = _api()
    rng = np.random.default_rng(k)
    deg = np.array([0, 1, 7, 300, 0, 2, 64])
    n_rows = len(deg)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.integers(0, 10_000, int(rowptr[-1])).astype(np.int32)
    nodes = np.array([0, 1, 2, 3, -1, n_rows, 4, 5, 6, -7, n_rows + 3, 3, 1, 2], np.int32)
    n = len(nodes)
    rowptr_d, col_d, nodes_d = _dev(rowptr, np.int64), _dev(col, np.int32), _dev(nodes, np.int32)
    csr = _lib.CSR(rowptr=rowptr_d.data_ptr(), col=col_d.data_ptr(), n_rows=n_rows,
                   nnz=int(rowptr[-1]))
    for seed, offset in ((123, (1 << 32) - 5), (dc.SEED_BIG, 0), (0, (1 << 64) - 3)):
        want = np.full(n * k, -1, np.int32)
        s = dc.mix64(seed)
        for i in range(n * k):
            v = int(nodes[i // k])
            if 0 <= v < n_rows and deg[v] > 0:
                r = dc.mix64(s ^ ((offset + i) & dc.M64))
                want[i] = col[int(rowptr[v]) + ((r * int(deg[v])) >> 64)]
        assert offset == 0 or (offset + n * k - 1 >= 1 << 32)
        outs = []
        for _ in range(2):
            o = _canary_i32(n * k)
            assert lib.mirec_sample_fanout(ctypes.byref(csr), nodes_d.data_ptr(), n, k, seed,
                                           offset, o.data_ptr(), st) == 0
            a, clean = _split(o, n * k, (n * k,))
            assert clean
            outs.append(a)
        assert np.array_equal(outs[0], want) and np.array_equal(outs[1], want)
        w2 = want.reshape(n, k)
        assert (w2[[0, 4, 5, 6, 9, 10]] == -1).all() and (w2[[1, 12]] == col[0]).all()


# ------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_alone():
    """dim = 6, k = 0, p = 1, p = NaN -> MIREC_ERR_ARG from every hop mean;
    k = 65 from the atomic backward; n_targets = 0 -> OK; nothing written."""
    lib, st = _api()
    n_t, k, dim, n_rows = 3, 4, 8, 16
    src = _dev(np.ones((n_rows * 70, 8)), np.float32)
    ids = _dev(np.zeros(n_t * 70), np.int32)
    need = ctypes.c_size_t(0)
    assert lib.mirec_fanout_mean_gather_bwd_sorted_workspace(n_t, 70, n_rows,
                                                             ctypes.byref(need)) == 0
    out = _canary_f32(n_rows * 70 * 8)
    ws = torch.full((int(need.value),), 0xA5, dtype=torch.uint8, device="cuda")
    s, v, o = src.data_ptr(), ids.data_ptr(), out.data_ptr()

    def every(n_t, k, dim, p):
        return {
            "mean": lib.mirec_fanout_mean(s, v, n_t, k, dim, p, 5, o, st),
            "mean_null": lib.mirec_fanout_mean(s, None, n_t, k, dim, p, 5, o, st),
            "bwd": lib.mirec_fanout_mean_bwd(s, v, n_t, k, dim, p, 5, o, st),
            "gather": lib.mirec_fanout_mean_gather(s, v, n_t, k, dim, p, 5, o, st),
            "gather_bwd": lib.mirec_fanout_mean_gather_bwd(s, v, n_t, k, dim, p, 5, o, st),
            "sorted": lib.mirec_fanout_mean_gather_bwd_sorted(s, v, n_t, k, dim, p, 5, n_rows, o,
                                                              ws.data_ptr(), ws.numel(), st),
        }

    for bad in ((n_t, k, 6, 0.3), (n_t, 0, dim, 0.3), (n_t, k, dim, 1.0),
                (n_t, k, dim, float("nan")), (n_t, k, dim, -0.1), (0, k, dim, 1.0)):
        rcs = every(*bad)
        assert all(rc == ERR_ARG for rc in rcs.values()), (bad, rcs)
    assert lib.mirec_fanout_mean_gather_bwd(s, v, n_t, 65, dim, 0.3, 5, o, st) == ERR_ARG
    assert lib.mirec_gather_rows(s, v, n_t, 6, o, st) == ERR_ARG
    assert lib.mirec_gather_rows(s, v, n_t, 1028, o, st) == ERR_ARG
    assert lib.mirec_scatter_add_rows(s, v, n_t, 0, o, st) == ERR_ARG
    rcs = every(0, k, dim, 0.3)
    assert all(rc == 0 for rc in rcs.values()), rcs
    assert _all_canary(out) and bool(np.all(_np(ws) == 0xA5))
