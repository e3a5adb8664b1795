"""Host restatement of the counter-hash dropout of csrc/common.h (the rule is
written out in include/mirec.h), float64 references of the GraphSAGE hop ops
that use it, the rounding bound the GPU tests hold the kernels to, and the
case lists of tests/test_sage_kernels.py and
tests/test_rowtail_dropout_kernels.py.  numpy only; nothing from the package.

The mask is a pure integer function of (seed, element index), so this file is
an exact oracle for it: tests/test_dropout_host.py checks the restatement
(published splitmix64 vectors, the other restatements in the suite, torch
float64 autograd) and that the case lists contain the edges they claim.

The bound.  u = 2^-24, gamma(n) = n u / (1 - n u).  An output that is a sum of
m float32 terms, each a product of up to three factors (1 / cnt or a division,
g, scale) and possibly added onto a base value, satisfies
|got - ref| <= gamma(m + 4) * A, with A the sum of the absolute terms (|base|
included), whatever the summation order; fused multiply-adds only lower the
error.  References use the float32 `scale` widened to float64, so its own
rounding is not counted.
"""
import math
import sys

import numpy as np

M64 = (1 << 64) - 1
U = 2.0 ** -24
KEY_CONST = 0xA24BAED4963EE407
SEED_BIG = (1 << 63) + 0x1234_5678_9ABC
SEEDS = (0, 123, SEED_BIG)


def gamma(n):
    """gamma_n of the standard rounding analysis (scalar or array n)."""
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------ mask rule
def mix64(x):
    """The splitmix64 finaliser on a Python int, mod 2^64."""
    x = (int(x) + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def mix64_v(x):
    """mix64 over a uint64 array (wrapping arithmetic)."""
    x = np.asarray(x, np.uint64).copy()
    with np.errstate(over="ignore"):
        x += np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def dropout_params(p, seed):
    """(key, thresh, scale) of a launch; scale is a numpy float32.  p is taken
    as float32; p outside [0, 1) (NaN included) raises ValueError."""
    p32 = np.float32(p)
    if not (p32 >= np.float32(0) and p32 < np.float32(1)):
        raise ValueError(f"dropout p = {p!r} outside [0, 1)")
    key = mix64((int(seed) & M64) ^ KEY_CONST)
    thresh = int(math.floor(float(p32) * 65536.0 + 0.5))
    if p32 > 0 and thresh == 0:
        thresh = 1
    thresh = min(thresh, 65535)
    scale = np.float32(1) / (np.float32(1) - p32) if p32 > 0 else np.float32(1)
    assert scale.dtype == np.float32
    return key, thresh, scale


def keep(key, thresh, idx):
    """Whether element idx survives (scalar form)."""
    h = mix64((int(key) + (int(idx) >> 2)) & M64)
    return ((h >> (16 * (int(idx) & 3))) & 0xFFFF) >= thresh


def keep_v(key, thresh, idx):
    """keep over an array of element indices (any shape) -> bool array."""
    idx = np.asarray(idx, np.uint64)
    with np.errstate(over="ignore"):
        h = mix64_v(idx // np.uint64(4) + np.uint64(key))
    sl = (h >> (np.uint64(16) * (idx & np.uint64(3)))) & np.uint64(0xFFFF)
    return sl >= np.uint64(thresh)


def keep_rows(key, thresh, n, width):
    """keep over the n * width consecutive elements 0 .. n*width - 1 as [n,
    width] (width % 4 == 0): one hash per aligned quad, its four 16-bit slices
    read as the little-endian uint16 view — keep_v's result, a quarter of the
    hashing (the table-gradient references mask 5e7 elements)."""
    assert width % 4 == 0 and sys.byteorder == "little"
    with np.errstate(over="ignore"):
        h = mix64_v(np.arange(n * (width // 4), dtype=np.uint64) + np.uint64(key))
    return (h.view(np.uint16) >= np.uint16(thresh)).reshape(n, width)


def run_key(key, base):
    """The key of a row-tail launch that was given *seed_base = base."""
    return mix64(int(key) ^ (int(base) & M64))


# ------------------------------------------------------------ element indices
def fanout_index(n_entries, dim):
    """(t*k + c)*dim + col for every entry e = t*k + c: [n_entries, dim]."""
    e = np.arange(n_entries, dtype=np.uint64)[:, None]
    return e * np.uint64(dim) + np.arange(dim, dtype=np.uint64)[None, :]


def rowtail_index(n, d):
    """row*d + col: [n, d]."""
    return fanout_index(n, d)


def fanout_mask(p, seed, n_entries, dim):
    """(keep [n_entries, dim] bool, scale float32) of a fanout launch."""
    key, thresh, scale = dropout_params(p, seed)
    if dim % 4 == 0:
        return keep_rows(key, thresh, n_entries, dim), scale
    return keep_v(key, thresh, fanout_index(n_entries, dim)), scale


def rowtail_mask(p, seed, n, d, base=None):
    """(keep [n, d] bool, scale float32) of a row-tail launch; base = None is
    seed_base = NULL (the key itself, which differs from base = 0)."""
    key, thresh, scale = dropout_params(p, seed)
    if base is not None:
        key = run_key(key, base)
    return keep_rows(key, thresh, n, d), scale


# ---------------------------------------------------------- float64 references
def _counts(valid, k):
    v = np.asarray(valid, bool).reshape(-1, k)
    return v, v.sum(1)


def fanout_mean_ref(rows, valid, k, mask, scale):
    """out[t] = sum over valid c of keep * scale * rows[t*k + c] / cnt_t (0 if
    cnt_t = 0).  rows [n_t*k, dim] are the child rows (x, or table[ids] — the
    rows of invalid children are ignored); valid [n_t*k] bool.
    Returns (out, A, m): float64 [n_t, dim] twice and the term count [n_t]."""
    v, cnt = _counts(valid, k)
    n_t, dim = v.shape[0], rows.shape[1]
    w = (mask.reshape(n_t, k, dim) & v[:, :, None]) * float(scale)
    terms = np.where(v[:, :, None], w * rows.astype(np.float64).reshape(n_t, k, dim), 0.0)
    den = np.maximum(cnt, 1)[:, None].astype(np.float64)
    return terms.sum(1) / den, np.abs(terms).sum(1) / den, cnt


def fanout_mean_bwd_ref(g, valid, k, mask, scale):
    """grad_x[t*k + c] = keep * scale * g[t] / cnt_t for a valid child, 0 for
    an invalid one: float64 [n_t*k, dim]."""
    v, cnt = _counts(valid, k)
    n_t, dim = g.shape
    per = g.astype(np.float64) / np.maximum(cnt, 1)[:, None]
    out = np.where(v[:, :, None] & mask.reshape(n_t, k, dim), float(scale) * per[:, None, :], 0.0)
    return out.reshape(n_t * k, dim)


def entry_contributions(g, ids, k, mask, scale):
    """Per-entry rows of the gather backward, keep * scale * g[t] / cnt_t
    (zero rows for ids < 0): float64 [n_t*k, dim]."""
    return fanout_mean_bwd_ref(g, np.asarray(ids) >= 0, k, mask, scale)


def scatter_add_ref(rows, ids, base):
    """table[r] = base[r] + sum of rows[e] over the entries with ids[e] = r.
    Returns (table, A, m): float64 [n_rows, dim] twice (A: the absolute terms,
    |base| included) and the entry count per row [n_rows]."""
    ids = np.asarray(ids, np.int64)
    ok = ids >= 0
    out = base.astype(np.float64).copy()
    A = np.abs(out)
    r64 = np.asarray(rows, np.float64)
    np.add.at(out, ids[ok], r64[ok])
    np.add.at(A, ids[ok], np.abs(r64[ok]))
    return out, A, np.bincount(ids[ok], minlength=base.shape[0])


def gather_bwd_ref(g, ids, k, mask, scale, base):
    """table_grad[r] = base[r] + sum over entries e with ids[e] = r of keep *
    scale * g[t_e] / cnt_{t_e}: (table_grad, A, m) as scatter_add_ref."""
    return scatter_add_ref(entry_contributions(g, ids, k, mask, scale), ids, base)


def sum_bound(A, m):
    """gamma(m + 4) * A with m per row ([rows] against A [rows, dim])."""
    return gamma(np.asarray(m, np.float64) + 4.0)[:, None] * A


# ----------------------------------------------------------------- fanout cases
def _case_rng(*key):
    return np.random.default_rng([int(x) & 0xFFFFFFFF for x in key])


def fanout_cases():
    """The (n_targets, k, dim, p, seed, n_rows) list of the hop-mean tests.
    d4 = dim / 4 decides the unfused backward's count: a ballot over groups of
    d4 lanes for a power of two <= 64 (ceil(k / d4) rounds), else a loop."""
    S0, S1, S2 = SEEDS
    rows = [
        # n_t  k  dim    p  seed n_rows
        (37, 5, 4, 0.3, S0, 1000),     # d4 = 1: five ballot rounds; 185 work items
        (37, 8, 8, 0.5, S1, 64),       # d4 = 2
        (37, 9, 12, 0.3, S2, 1000),    # d4 = 3: loop count; one past the batch of 8
        (37, 25, 64, 0.5, S0, 64),     # d4 = 16 < k: two rounds
        (37, 5, 64, 0.3, S1, 1000),    # d4 = 16 > k: one round
        (37, 64, 256, 0.3, S2, 1000),  # d4 = 64 = k: a whole wave per child
        (37, 70, 256, 0.5, S0, 64),    # d4 = 64 < k (past the atomic form's limit)
        (37, 1, 260, 0.3, S1, 1000),   # d4 = 65: loop count
        (37, 9, 512, 0.5, S2, 1000),   # d4 = 128: loop count, two column passes
        (37, 64, 12, 0.5, S1, 64),     # loop count with k at the atomic limit
        (37, 25, 260, 0.0, S2, 1000),  # p = 0 at a loop-count width
        (37, 8, 64, 0.0, S0, 1),       # p = 0; a one-row table
        (1, 25, 8, 0.3, S0, 64),
        (1, 70, 512, 0.3, S1, 1000),
        (1, 1, 64, 0.0, S1, 1000),
    ]
    return [dict(n_t=a, k=b, dim=c, p=d, seed=e, n_rows=f) for a, b, c, d, e, f in rows]


def fanout_ids(case):
    """Child ids [n_t*k] int32 of a case, -1 = invalid.  With n_t >= 4: target
    0 has no valid child, target 1 exactly one, in the last slot, target 2 all
    valid, target 3 all valid with its first id repeated in its last slot (k >=
    2); the rest are random with about a quarter invalid."""
    n_t, k, n_rows = case["n_t"], case["k"], case["n_rows"]
    rng = _case_rng(n_t, k, case["dim"], n_rows, 17)
    ids = rng.integers(0, n_rows, (n_t, k)).astype(np.int32)
    ids[rng.random((n_t, k)) < 0.25] = -1
    if n_t >= 4:
        ids[0] = -1
        ids[1, :-1] = -1
        ids[1, -1] = n_rows - 1
        ids[2] = rng.integers(0, n_rows, k)
        ids[3] = rng.integers(0, n_rows, k)
        ids[3, -1] = ids[3, 0]
    else:
        ids[0, -1] = n_rows - 1
    return ids.reshape(-1)


# ----------------------------------------------------------------- sorted cases
def _layout_ids(n, runs, n_invalid, n_rows, rng):
    """n entries: runs = [(id, length)], n_invalid invalid ones, the rest
    distinct ids above every run id; shuffled (the sort restores the runs)."""
    ids = [np.full(ln, r, np.int64) for r, ln in runs]
    used = sum(ln for _, ln in runs) + n_invalid
    top = max([r for r, _ in runs], default=-1) + 1
    rest = n - used
    assert rest >= 0 and top + rest <= n_rows
    ids += [np.full(n_invalid, -1, np.int64), top + np.arange(rest)]
    return rng.permutation(np.concatenate(ids)).astype(np.int32)


def sorted_cases():
    """Cases of the sorted backward: every fanout case, then layouts built for
    the 64-entry chunk grid of the sorted sum (each dict carries its ids)."""
    out = []
    for c in fanout_cases():
        out.append(dict(c, ids=fanout_ids(c), name="fanout"))
    S0, S1, S2 = SEEDS
    rng = _case_rng(64, 9)
    # 333 entries; sorted: id 0 fills chunk 0, id 1 (150 entries) starts on
    # entry 64 and holds chunks 1 and 2 whole, id 3 (40) crosses entry 256
    c = dict(n_t=37, k=9, dim=512, p=0.3, seed=S2, n_rows=1000, name="runs")
    c["ids"] = _layout_ids(333, [(0, 64), (1, 150), (2, 10), (3, 40)], 30, 1000, rng)
    out.append(c)
    # the same layout at one column pass and p = 0.5
    c = dict(n_t=37, k=9, dim=64, p=0.5, seed=S0, n_rows=1000, name="runs")
    c["ids"] = _layout_ids(333, [(5, 64), (6, 150), (7, 10), (8, 40)], 0, 1000, rng)
    out.append(c)
    # one row: a single run over all 185 entries, no invalid tail
    c = dict(n_t=37, k=5, dim=260, p=0.5, seed=S1, n_rows=1, name="one_row")
    c["ids"] = np.zeros(185, np.int32)
    out.append(c)
    # nothing valid
    c = dict(n_t=37, k=8, dim=8, p=0.3, seed=S0, n_rows=64, name="all_invalid")
    c["ids"] = np.full(296, -1, np.int32)
    out.append(c)
    return out


def sorted_runs(ids, n_rows):
    """(keys sorted, [(key, start, end)] of the valid runs) after the stable
    sort by key (invalid entries take the key n_rows)."""
    keys = np.where(np.asarray(ids) >= 0, ids, n_rows).astype(np.int64)
    ks = keys[np.argsort(keys, kind="stable")]
    cut = np.flatnonzero(np.diff(ks)) + 1
    starts, ends = np.r_[0, cut], np.r_[cut, len(ks)]
    return ks, [(int(ks[s]), int(s), int(e)) for s, e in zip(starts, ends) if ks[s] < n_rows]


# --------------------------------------------------------------- row-tail cases
def rowtail_cases():
    """(n, d, p, seed, base) of the row-tail tests; base None = seed_base NULL.
    d picks the lanes-per-row / columns-per-lane shape of the dispatch: 4 ->
    (1, 1), 12 -> (4, 1), 36 -> (16, 1), 128 -> (32, 1), 520 -> (64, 4: 130
    float4 over 64 lanes round up to 4), 1024 -> (64, 4); 8 -> (2, 1), 32 ->
    (8, 1), 256 -> (64, 1) and 384 -> (64, 2) are the remaining shapes
    (rowtail_shape restates the choice; the host test asserts all nine)."""
    S0, S1, S2 = SEEDS
    B2 = (1 << 63) + 5
    rows = [
        (67, 4, 0.3, S0, None), (67, 12, 0.5, S1, 0), (67, 36, 0.3, S2, 1),
        (67, 128, 0.5, S0, B2), (67, 128, 0.3, S1, None), (1, 128, 0.3, S2, 0),
        (67, 520, 0.3, S1, B2), (1, 520, 0.5, S0, None), (67, 1024, 0.5, S2, 1),
        (1, 1024, 0.3, S1, None), (67, 256, 0.3, S0, 1), (67, 384, 0.5, S2, None),
        (67, 8, 0.3, S2, B2), (67, 32, 0.5, S1, 0),
    ]
    return [dict(n=a, d=b, p=c, seed=d, base=e) for a, b, c, d, e in rows]


def rowtail_shape(d):
    """(lanes per row, float4 columns per lane) the row tail runs d with:
    the smallest power of two >= d / 4 up to 64 lanes, then 1, 2 or 4."""
    d4, lpr = d // 4, 1
    while lpr < d4 and lpr < 64:
        lpr *= 2
    nc = -(-d4 // lpr)
    return lpr, 1 if nc <= 1 else (2 if nc <= 2 else 4)


def fused_rowtail_cases():
    """The same for the forms with the Linear inside (d = 128, Kr = 32)."""
    return [c for c in rowtail_cases() if c["d"] == 128]
