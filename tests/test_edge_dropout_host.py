"""Edge dropout, host side: mirec_edge_keep_mask (the keep function the
propagation kernel evaluates, restated over a host CSR) — determinism, the
transpose identity, multi-edges, keep_prob = 1, the kept fraction and the
independence of the two directions, argument checks, and the ABI.  No GPU.

All seeds are fixed; the statistical bounds are conditions on those seeds
(5 sigma of the binomial), not measurements."""
import ctypes

import numpy as np
import pytest

SEEDS = (1, 2, 3)


def keep_mask(rowptr, col, n_rows, seed, keep_prob, transposed=False):
    from furusato_recommend_amd._lib import lib
    rowptr = np.ascontiguousarray(rowptr, np.int64)
    col = np.ascontiguousarray(col, np.int32)
    keep = np.full(len(col), 255, np.uint8)
    rc = lib.mirec_edge_keep_mask(rowptr.ctypes.data, col.ctypes.data, n_rows, seed,
                                  keep_prob, int(transposed), keep.ctypes.data)
    return rc, keep


def mix64(x):
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def edge_keep(seed, i, j, keep_prob):
    """include/mirec.h's formula, restated."""
    key = mix64(seed ^ 0xD6E8FEB86659FD93)
    t = min(max(int(float(np.float32(keep_prob)) * 2.0 ** 32), 1), 1 << 32)
    return (mix64(key ^ ((i << 32) | j)) >> 32) < t


@pytest.fixture(scope="module")
def sym():
    """A symmetric CSR without duplicates: 30 000 distinct unordered pairs
    {i, j}, i != j, over 600 nodes, both directions stored (60 000 entries)."""
    rng = np.random.default_rng(5)
    n = 600
    code = rng.choice(n * (n - 1) // 2, 30_000, replace=False)
    iu, ju = np.triu_indices(n, 1)
    a, b = iu[code], ju[code]
    src, dst = np.concatenate([a, b]), np.concatenate([b, a])
    order = np.lexsort((src, dst))
    src, dst = src[order], dst[order]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))]).astype(np.int64)
    return n, rowptr, src.astype(np.int32), dst.astype(np.int64)


def twin(n, col, dst):
    """twin[e] = the entry (i -> j) of entry e = (j -> i), by explicit lookup."""
    pos = {(int(d), int(c)): e for e, (d, c) in enumerate(zip(dst, col))}
    return np.array([pos[(int(c), int(d))] for d, c in zip(dst, col)])


def test_deterministic_and_seeded(sym):
    n, rowptr, col, _ = sym
    rc, a = keep_mask(rowptr, col, n, 11, 0.6)
    rc2, b = keep_mask(rowptr, col, n, 11, 0.6)
    rc3, c = keep_mask(rowptr, col, n, 12, 0.6)
    assert rc == rc2 == rc3 == 0
    assert set(np.unique(a)) == {0, 1}
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c)
    # the seed is a full 64-bit value
    _, d = keep_mask(rowptr, col, n, 11 + (1 << 63), 0.6)
    assert not np.array_equal(a, d)


def test_matches_the_documented_formula(sym):
    n, rowptr, col, dst = sym
    for seed, p, tr in ((7, 0.6, False), ((1 << 64) - 3, 0.25, True), (0, 1.0, False)):
        rc, got = keep_mask(rowptr, col, n, seed, p, tr)
        assert rc == 0
        es = np.arange(0, len(col), 97)
        want = [edge_keep(seed, int(col[e]), int(dst[e]), p) if tr
                else edge_keep(seed, int(dst[e]), int(col[e]), p) for e in es]
        assert np.array_equal(got[es].astype(bool), np.array(want))


def test_transposed_mask_is_the_plain_mask_of_the_twin_entry(sym):
    n, rowptr, col, dst = sym
    tw = twin(n, col, dst)
    for seed in SEEDS:
        _, plain = keep_mask(rowptr, col, n, seed, 0.6, False)
        _, trans = keep_mask(rowptr, col, n, seed, 0.6, True)
        assert np.array_equal(trans, plain[tw])      # entry (j -> i) transposed = (i -> j) plain
        assert not np.array_equal(trans, plain)      # ... and it is a different mask


def test_duplicates_share_one_draw():
    rng = np.random.default_rng(9)
    n, nnz = 50, 4000                                # 2 500 cells: many multi-edges
    src, dst = rng.integers(0, n, nnz), np.sort(rng.integers(0, n, nnz))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))])
    for tr in (False, True):
        _, k = keep_mask(rowptr, src, n, 4, 0.5, tr)
        cell = dst * n + src
        first = {}
        n_dup = 0
        for e, c in enumerate(cell):
            if c in first:
                n_dup += 1
                assert k[e] == k[first[c]]
            first.setdefault(c, e)
        assert n_dup > 1000 and 0 < k.sum() < nnz


def test_keep_prob_one_keeps_everything(sym):
    n, rowptr, col, _ = sym
    for tr in (False, True):
        rc, k = keep_mask(rowptr, col, n, 123, 1.0, tr)
        assert rc == 0 and np.all(k == 1)


@pytest.mark.parametrize("p", [0.3, 0.6, 0.9])
def test_kept_fraction(sym, p):
    n, rowptr, col, _ = sym
    m = len(col)                                     # 60 000 distinct (i, j)
    assert m >= 20_000
    for seed in SEEDS:
        _, k = keep_mask(rowptr, col, n, seed, p)
        frac = k.mean()
        print(f"keep_prob {p} seed {seed}: kept {frac:.5f}")
        assert abs(frac - p) <= 5 * np.sqrt(p * (1 - p) / m)


@pytest.mark.parametrize("p", [0.3, 0.6, 0.9])
def test_the_two_directions_are_independent(sym, p):
    n, rowptr, col, dst = sym
    tw = twin(n, col, dst)
    one = col < dst                                  # each unordered pair once
    pairs = int(one.sum())
    assert pairs == 30_000
    q = 2 * p * (1 - p)
    for seed in SEEDS:
        _, k = keep_mask(rowptr, col, n, seed, p)
        share = float((k[one] != k[tw][one]).mean())
        print(f"keep_prob {p} seed {seed}: directions disagree on {share:.5f} (2p(1-p) = {q:.5f})")
        assert abs(share - q) <= 5 * np.sqrt(q * (1 - q) / pairs)


@pytest.mark.parametrize("bad", [0.0, -0.25, 1.0001, 2.0, float("nan"), float("inf")])
def test_keep_prob_outside_the_interval_is_rejected(sym, bad):
    n, rowptr, col, _ = sym
    rc, k = keep_mask(rowptr, col, n, 1, bad)
    assert rc == 1                                   # MIREC_ERR_ARG
    assert np.all(k == 255)                          # nothing written


def test_empty_and_null():
    from furusato_recommend_amd._lib import lib
    rp = np.zeros(4, np.int64)
    assert lib.mirec_edge_keep_mask(rp.ctypes.data, None, 3, 1, 0.5, 0, None) == 0
    assert lib.mirec_edge_keep_mask(None, None, 3, 1, 0.5, 0, None) == 1


def test_abi_mirror_and_version():
    from furusato_recommend_amd import _lib
    sz = [ctypes.c_size_t() for _ in range(3)]
    assert _lib.lib.mirec_struct_sizes(*(ctypes.byref(x) for x in sz)) == 0
    assert [x.value for x in sz] == [ctypes.sizeof(_lib.CSR), ctypes.sizeof(_lib.Prop),
                                     ctypes.sizeof(_lib.AdamH)]
    assert _lib.lib.mirec_abi_version() == 1
    # the dropout of a launch is a struct of its own: mirec_prop_t is untouched
    assert _lib.lib.mirec_drop_sizeof() == ctypes.sizeof(_lib.Drop) == 16
    d = _lib.Drop()                                  # all zero = off
    assert (d.keep_prob, d.transposed, d.seed) == (0.0, 0, 0)
    assert [f[0] for f in _lib.Drop._fields_] == ["keep_prob", "transposed", "seed"]
    assert [f[0] for f in _lib.Prop._fields_][-1] == "scale_next"


def test_step_seed_is_the_documented_function():
    from furusato_recommend_amd.engine import PropagationEngine
    f = PropagationEngine.dropout_seed
    assert f(0, 0) == 0 and f(0, 5) == 5
    assert f(2020, 7) == (2020 << 32) | 7
    assert f(-1, 1) == (0xFFFFFFFF << 32) | 1
    assert len({f(s, t) for s in range(4) for t in range(4)}) == 16
