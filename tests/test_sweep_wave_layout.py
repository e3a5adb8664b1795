"""The per-wave column-sweep layout (mirec_sweep_wave_build, include/mirec.h)
built through the C ABI on small numpy graphs, no GPU.  Guarantees checked:

1. the real slots of the streams are a permutation of exactly the block's
   entries;
2. per row the columns ascend, duplicate edges in CSR order (the per-row
   summation order of the group form);
3. every step of 4 slots names 4 different rows (or padding);
4. no real slot sits MIREC_SWEEP_LOOKAHEAD (16) or more away from its place in
   the wave's merged (column, CSR position) order, counted in real slots;
5. padding appears only where no pending entry inside the lookahead window is
   conflict-free, or after the stream's last real slot.

Slot k*16 + u*4 + g of a stream is step u, lane group g of batch k; a pad
slot has local row -1 and the column of the slot before it."""
import ctypes

import numpy as np
import pytest

W, LOOK, BATCH = 8, 16, 16


def _csr(u, i, nu, mi):
    from furusato_recommend_amd._lib import lib
    u = np.ascontiguousarray(u, np.int64)
    i = np.ascontiguousarray(i, np.int64)
    n = nu + mi
    rowptr = np.empty(n + 1, np.int64)
    col = np.empty(max(2 * len(u), 1), np.int32)
    dinv = np.empty(n, np.float32)
    assert lib.mirec_csr_bipartite(u.ctypes.data, i.ctypes.data, len(u), nu, mi,
                                   rowptr.ctypes.data, col.ctypes.data, dinv.ctypes.data) == 0
    return rowptr, col


def _build(rowptr, col, row0, n_rows, src0, n_src, tile_rows):
    """Size query, then the fill: (rc, wptr, lrow [n_slots], col [n_slots])."""
    from furusato_recommend_amd._lib import lib
    n_tiles = -(-n_rows // tile_rows)
    wptr = np.full(n_tiles * W + 1, -1, np.int64)
    n_slots = ctypes.c_int64(-1)
    rc = lib.mirec_sweep_wave_build(rowptr.ctypes.data, col.ctypes.data, row0, n_rows, src0,
                                    n_src, tile_rows, wptr.ctypes.data, None, 0,
                                    ctypes.byref(n_slots))
    if rc not in (0, 4):
        return rc, wptr, None, None
    assert (rc == 4) == (n_slots.value > 0) and wptr[-1] == n_slots.value
    slot = np.full(max(n_slots.value, 1), 0x7777777777777777, np.int64)
    wptr2 = np.full_like(wptr, -1)
    rc = lib.mirec_sweep_wave_build(rowptr.ctypes.data, col.ctypes.data, row0, n_rows, src0,
                                    n_src, tile_rows, wptr2.ctypes.data, slot.ctypes.data,
                                    n_slots.value, ctypes.byref(n_slots))
    assert np.array_equal(wptr, wptr2)
    slot = slot[:n_slots.value]
    return rc, wptr, (slot >> 32).astype(np.int64), (slot & 0xffffffff).astype(np.int64)


def _wave_rows(t, w, tile_rows, n_rows):
    wave_rows = -(-tile_rows // W)
    tile_end = min((t + 1) * tile_rows, n_rows)
    r0 = min(t * tile_rows + w * wave_rows, tile_end)
    return r0, min(r0 + wave_rows, tile_end)


def _check(rowptr, col, row0, n_rows, src0, n_src, tile_rows):
    """Asserts the five guarantees; returns (slots, pad slots, streams)."""
    rc, wptr, lrow, scol = _build(rowptr, col, row0, n_rows, src0, n_src, tile_rows)
    assert rc == 0
    n_tiles = -(-n_rows // tile_rows)
    assert wptr[0] == 0 and np.all(np.diff(wptr) >= 0) and np.all(np.diff(wptr) % BATCH == 0)
    seen = np.zeros(n_rows, np.int64)
    n_real = 0
    for t in range(n_tiles):
        for w in range(W):
            r0, r1 = _wave_rows(t, w, tile_rows, n_rows)
            seen[r0:r1] += 1
            # the wave's merged order: (column, CSR position)
            e0, e1 = rowptr[row0 + r0], rowptr[row0 + r1]
            order = np.lexsort((np.arange(e0, e1), col[e0:e1]))
            m_col = col[e0:e1][order].astype(np.int64)
            m_row = (np.repeat(np.arange(r0, r1), np.diff(rowptr[row0 + r0:row0 + r1 + 1]))[order]
                     - t * tile_rows)
            n = len(order)
            lr, sc = lrow[wptr[t * W + w]:wptr[t * W + w + 1]], scol[wptr[t * W + w]:
                                                                  wptr[t * W + w + 1]]
            real = lr >= 0
            assert np.all(lr[~real] == -1) and real.sum() == n
            n_real += n
            if n == 0:
                assert len(lr) == 0
                continue
            # 1 + 2: per row the stream holds the row's merged entries in merged order
            # (equal columns are equal terms; their CSR order is the tagged test below)
            pos_of = np.full(len(lr), -1, np.int64)  # merged position of each real slot
            for r in np.unique(m_row):
                mine = np.flatnonzero(real & (lr == r))
                want = np.flatnonzero(m_row == r)
                assert np.array_equal(sc[mine], m_col[want])
                assert np.all(np.diff(sc[mine]) >= 0)
                pos_of[mine] = want
            assert set(np.unique(lr[real])) == set(np.unique(m_row))
            assert sorted(pos_of[real].tolist()) == list(range(n))  # a permutation
            # 4: bounded displacement, counted in real slots
            rank = np.cumsum(real) - 1
            assert np.all(np.abs(rank[real] - pos_of[real]) < LOOK)
            # pad columns: the slot before; a stream never starts with padding
            assert real[0]
            assert np.all(sc[1:][~real[1:]] == sc[:-1][~real[1:]])
            # 3 + 5, step by step
            pending = np.ones(n, bool)
            for s0 in range(0, len(lr), 4):
                rows = lr[s0:s0 + 4][real[s0:s0 + 4]]
                assert len(set(rows.tolist())) == len(rows)
                pending[pos_of[s0:s0 + 4][real[s0:s0 + 4]]] = False
                if len(rows) < 4 and pending.any():
                    head = int(np.flatnonzero(pending)[0])
                    # (the head before this step was <= this one, so this window
                    # contains what was left of that step's)
                    cand = np.flatnonzero(pending[:head + LOOK])
                    cand = cand[cand < int(np.min(pos_of[s0:s0 + 4][real[s0:s0 + 4]])) + LOOK]
                    assert all(int(m_row[c]) in rows.tolist() for c in cand)
                if not pending.any():
                    assert not real[s0 + 4:].any()  # only padding after the last entry
                    break
    assert np.all(seen == 1)
    assert n_real == rowptr[row0 + n_rows] - rowptr[row0]
    return len(lrow), int((lrow < 0).sum()), (wptr, lrow, scol)


def _replay(rowptr, col, row0, n_rows, tile_rows, streams, x):
    """float32 accumulators, one add per real slot in slot order (what the
    kernel does) against the per-row sequential float32 sum in ascending
    column order: bitwise."""
    wptr, lrow, scol = streams
    out = np.zeros((n_rows, x.shape[1]), np.float32)
    for s in range(len(wptr) - 1):
        t = s // W
        for lr, c in zip(lrow[wptr[s]:wptr[s + 1]], scol[wptr[s]:wptr[s + 1]]):
            if lr >= 0:
                out[t * tile_rows + lr] = out[t * tile_rows + lr] + x[c]
    ref = np.zeros_like(out)
    for r in range(n_rows):
        for c in np.sort(col[rowptr[row0 + r]:rowptr[row0 + r + 1]], kind="stable"):
            ref[r] = ref[r] + x[c]
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), ref.view(np.uint32))


def _random_graph():
    rng = np.random.default_rng(5)
    nu, mi, ne = 300, 61, 2500  # 61: no multiple of any tile size used
    u = rng.integers(0, nu, ne)
    i = rng.integers(0, mi - 3, ne)  # the last three items have no edges
    i[:40] = 7                       # a heavy item; duplicate (user, item) edges below
    u[:10] = 5
    return nu, mi, _csr(u, i, nu, mi)


# 16: ragged last tile (61 = 3 * 16 + 13) whose last waves own 1 and 0 rows;
# 20: wave_rows 3, the last wave of a full tile owns 2 rows; 5 and 7:
# tile_rows < 8, waves without a row; 64: one ragged tile
@pytest.mark.parametrize("tile_rows", [16, 20, 5, 7, 64])
def test_item_block_random_graph(tile_rows):
    nu, mi, (rowptr, col) = _random_graph()
    total, pads, streams = _check(rowptr, col, nu, mi, 0, nu, tile_rows)
    print(f"tile_rows {tile_rows}: {pads} pad slots of {total}")
    x = np.random.default_rng(1).standard_normal((nu + mi, 3)).astype(np.float32)
    _replay(rowptr, col, nu, mi, tile_rows, streams, x)


@pytest.mark.parametrize("tile_rows", [24, 50, 6])
def test_user_block_source_offset(tile_rows):
    """The user rows gather from the item block: src0 = n_users."""
    nu, mi, (rowptr, col) = _random_graph()
    _, _, streams = _check(rowptr, col, 0, nu, nu, mi, tile_rows)
    assert np.all(streams[2] >= nu)  # columns as in the CSR, pad slots included
    x = np.random.default_rng(2).standard_normal((nu + mi, 3)).astype(np.float32)
    _replay(rowptr, col, 0, nu, tile_rows, streams, x)


def _hand_graph():
    """40 users x 9 items: item 0 has no edges, item 1 user 5 three times,
    item 2 only users of [8, 16) (one band of 8), the others random."""
    rng = np.random.default_rng(3)
    u = [5, 30, 5, 2, 5] + [9, 12, 8, 15, 12] + rng.integers(0, 40, 50).tolist()
    i = [1] * 5 + [2] * 5 + rng.integers(3, 9, 50).tolist()
    return 40, 9, _csr(np.array(u), np.array(i), 40, 9)


def test_hand_built_graph():
    nu, mi, (rowptr, col) = _hand_graph()
    # tile_rows 8: every wave owns ONE row, so every step is one real slot and
    # three pads; the second tile has a single row
    total, pads, (wptr, lrow, scol) = _check(rowptr, col, nu, mi, 0, nu, 8)
    real = lrow >= 0
    assert np.all(real.reshape(-1, 4).sum(1) <= 1)
    assert wptr[1] == 0                                   # item 0: an empty stream
    s1 = slice(wptr[1], wptr[2])                          # item 1
    assert scol[s1][real[s1]].tolist() == [2, 5, 5, 5, 30]
    assert lrow[s1][:20:4].tolist() == [1] * 5 and wptr[2] - wptr[1] == 32
    s2 = slice(wptr[2], wptr[3])                          # item 2: one band, pads included
    assert np.all((scol[s2] >= 8) & (scol[s2] < 16))
    assert np.all(np.diff(wptr[W + 1:]) == 0)             # waves 1..7 of the last tile
    x = np.random.default_rng(4).standard_normal((nu + mi, 3)).astype(np.float32)
    _replay(rowptr, col, nu, mi, 8, (wptr, lrow, scol), x)
    # the same rows in one tile of two-row waves
    _check(rowptr, col, nu, mi, 0, nu, 16)


def test_duplicates_keep_csr_order():
    """Equal columns are told apart only by position: a row whose CSR order is
    descending comes out ascending, so the key is (column, CSR position) and
    equal columns keep their CSR order (a stable sort by column)."""
    nu, mi = 6, 2
    rowptr, col = _csr(np.array([5, 4, 3, 2, 1, 0]), np.zeros(6, np.int64), nu, mi)
    rc, wptr, lrow, scol = _build(rowptr, col, nu, mi, 0, nu, 2)
    assert rc == 0 and scol[lrow >= 0].tolist() == [0, 1, 2, 3, 4, 5]


def test_padding_cap_uniform_graph():
    """A condition, not a measurement: with at least 8 rows per non-empty wave
    the greedy lookahead-16 schedule rarely fails to fill a step (a CPU
    simulation on Poisson-degree rows gave 0.05 % to 2.0 %), and the tail of
    a stream is under one batch: 15 of about 800 slots here."""
    rng = np.random.default_rng(7)
    nu, mi, ne = 3000, 128, 12800   # 2 tiles of 64 rows, 8 rows per wave, degree ~100
    rowptr, col = _csr(rng.integers(0, nu, ne), rng.integers(0, mi, ne), nu, mi)
    total, pads, _ = _check(rowptr, col, nu, mi, 0, nu, 64)
    print(f"pad slots: {pads} of {total} = {100 * pads / total:.2f} %")
    assert pads <= 0.05 * total


def test_empty_and_errors():
    from furusato_recommend_amd._lib import lib
    nu, mi = 4, 3
    rowptr, col = _csr(np.zeros(0, np.int64), np.zeros(0, np.int64), nu, mi)
    rc, wptr, lrow, _ = _build(rowptr, col, nu, mi, 0, nu, 2)
    assert rc == 0 and np.all(wptr == 0) and len(lrow) == 0
    # a column outside the source block: MIREC_ERR_RANGE, as mirec_sweep_build
    rowptr, col = _csr([0, 3], [0, 1], nu, mi)
    assert _build(rowptr, col, nu, mi, 0, 3, 2)[0] == 5
    assert _build(rowptr, col, nu, mi, 1, nu - 1, 2)[0] == 5   # below src0
    assert _build(rowptr, col, 0, nu, nu, mi, 2)[0] == 0       # the user rows are fine
    # null arrays and bad sizes: MIREC_ERR_ARG
    n = ctypes.c_int64(0)
    wptr = np.zeros(2 * W + 1, np.int64)
    args = (nu, mi, 0, nu, 2)
    assert lib.mirec_sweep_wave_build(None, col.ctypes.data, *args, wptr.ctypes.data, None, 0,
                                      ctypes.byref(n)) == 1
    assert lib.mirec_sweep_wave_build(rowptr.ctypes.data, col.ctypes.data, *args, None, None, 0,
                                      ctypes.byref(n)) == 1
    assert lib.mirec_sweep_wave_build(rowptr.ctypes.data, None, *args, wptr.ctypes.data, None, 0,
                                      ctypes.byref(n)) == 1
    assert lib.mirec_sweep_wave_build(rowptr.ctypes.data, col.ctypes.data, *args,
                                      wptr.ctypes.data, None, 64, ctypes.byref(n)) == 1
    assert lib.mirec_sweep_wave_build(rowptr.ctypes.data, col.ctypes.data, nu, mi, 0, nu, 0,
                                      wptr.ctypes.data, None, 0, ctypes.byref(n)) == 1
    # too little room: MIREC_ERR_WORKSPACE with the size filled in
    slot = np.zeros(8, np.int64)
    assert lib.mirec_sweep_wave_build(rowptr.ctypes.data, col.ctypes.data, *args,
                                      wptr.ctypes.data, slot.ctypes.data, 8,
                                      ctypes.byref(n)) == 4 and n.value == 32
