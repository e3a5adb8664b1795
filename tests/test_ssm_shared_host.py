"""mirec_cpu_shared_sample, the host twin of the shared-negative-set sampler
(DESIGN.md §19): values in range, independence of the thread count, counter
addressing (set b of a call does not depend on n_sets), (seed, offset)
sensitivity, argument checks and one uniformity check.  No GPU.

All seeds are fixed; the statistical bound is a condition on those seeds
(5 sigma of the binomial), not a measurement."""
import ctypes

import numpy as np
import pytest

SENTINEL = -7


def shared_sample(m_items, n_sets, m, seed, offset, n_threads=1, alloc=None, null=False):
    """(rc, out [alloc] int32): the call into a sentinel-filled buffer."""
    from furusato_recommend_amd import _lib
    out = np.full(alloc if alloc is not None else max(n_sets * m, 1), SENTINEL, np.int32)
    rc = _lib.lib.mirec_cpu_shared_sample(m_items, n_sets, m, ctypes.c_uint64(seed),
                                          ctypes.c_uint64(offset),
                                          None if null else out.ctypes.data, n_threads)
    return rc, out


def test_values_lie_in_range_and_repeat():
    for m_items in (1, 2, 50, 2 ** 31 - 2):
        rc, a = shared_sample(m_items, 5, 300, 11, 3)
        rc2, b = shared_sample(m_items, 5, 300, 11, 3)
        assert rc == rc2 == 0 and np.array_equal(a, b)
        assert a.min() >= 0 and a.max() < m_items
    assert len(np.unique(shared_sample(50, 5, 300, 11, 3)[1])) == 50


def test_independent_of_the_thread_count():
    # 40 x 2048 elements: up to 20 worker threads take contiguous blocks
    rc, base = shared_sample(1000, 40, 2048, 5, 9, n_threads=1)
    assert rc == 0
    for nt in (3, 16):
        rc, got = shared_sample(1000, 40, 2048, 5, 9, n_threads=nt)
        assert rc == 0 and np.array_equal(base, got)


def test_set_b_does_not_depend_on_the_number_of_sets():
    m = 257
    _, a = shared_sample(1000, 4, m, 8, 21)
    _, b = shared_sample(1000, 7, m, 8, 21)
    assert np.array_equal(a, b[: 4 * m])
    assert not np.array_equal(b[: m], b[m: 2 * m])     # the sets differ among themselves


def test_offset_and_seed_change_the_output():
    _, a = shared_sample(1000, 4, 256, 8, 21)
    _, b = shared_sample(1000, 4, 256, 8, 22)
    _, c = shared_sample(1000, 4, 256, 9, 21)
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)
    # another offset is another stream, not a window of the same one: no long
    # common run at any shift (a sliding window would share all but one entry)
    assert not np.array_equal(a[1:], b[:-1]) and not np.array_equal(a[:-1], b[1:])
    assert np.mean(a == b) < 0.02


@pytest.mark.parametrize("what", ["m_items0", "m_items-1", "sets0", "sets-1", "m0", "m-2", "null",
                                  "too_many"])
def test_bad_arguments_are_refused_with_the_buffer_untouched(what):
    m_items, n_sets, m, null = 50, 3, 16, False
    if what.startswith("m_items"):
        m_items = int(what[7:])
    elif what.startswith("sets"):
        n_sets = int(what[4:])
    elif what == "too_many":
        n_sets, m = 2 ** 16, 2 ** 15                   # n_sets * m = 2^31
    elif what.startswith("m"):
        m = int(what[1:])
    else:
        null = True
    rc, out = shared_sample(m_items, n_sets, m, 1, 0, alloc=64, null=null)
    assert rc == 1                                     # MIREC_ERR_ARG
    assert np.all(out == SENTINEL)


def test_draws_are_uniform():
    """m_items = 50, three fixed seeds x 60 000 draws: every item's count lies
    within 5 sigma of the binomial, per seed (expected 1 200 per item; 150
    comparisons at 5 sigma: a false alarm about 1e-4) and pooled over the
    seeds (expected 3 600 per item; the normal approximation is good for
    both) — a condition on these seeds."""
    q, worst, pooled = 1.0 / 50, 0.0, np.zeros(50, np.int64)
    for seed in (101, 102, 103):
        rc, a = shared_sample(50, 30, 2000, seed, 0)
        assert rc == 0 and len(a) == 60_000
        c = np.bincount(a, minlength=50)
        pooled += c
        z = np.abs(c - len(a) * q) / np.sqrt(len(a) * q * (1 - q))
        worst = max(worst, float(z.max()))
    tot = int(pooled.sum())
    zp = float((np.abs(pooled - tot * q) / np.sqrt(tot * q * (1 - q))).max())
    print(f"largest deviation: {worst:.2f} sigma per seed, {zp:.2f} sigma pooled")
    assert worst <= 5.0 and zp <= 5.0
