"""mirec_sweep_wave_pack (csrc/graph.cpp): the 4-byte form of the per-wave
sweep layout's slots, derived from mirec_sweep_wave_build's 8-byte output.

Host only.  For the items and the users layout of the 3 000 x 700 graph of
tests/test_prop_sweep_wave.py at several tile sizes, the packed slots unpacked
in numpy equal the 8-byte slots, padding included (row -1, the column of the
slot before).  Tile sizes: 8 (one row per wave, mostly padding), 196, 255 and
256 (the last tile with an 8-bit row field and the first with 9), 280."""
import ctypes

import numpy as np
import pytest

from furusato_recommend_amd import SyntheticBipartite, _lib

lib = _lib.lib
W = 8  # MIREC_SWEEP_WAVES
ERR_RANGE = 5


@pytest.fixture(scope="module")
def csr():
    ds = SyntheticBipartite(3000, 700, 40000, seed=1, test_frac=0)
    nu, mi = ds.n_users, ds.m_items
    u, i = np.asarray(ds.trainUser, np.int64), np.asarray(ds.trainItem, np.int64)
    src = np.concatenate([u, nu + i])
    dst = np.concatenate([nu + i, u])
    order = np.lexsort((dst, src))
    rowptr = np.zeros(nu + mi + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=nu + mi), out=rowptr[1:])
    return rowptr, dst[order].astype(np.int32), nu, mi


def build(rowptr, col, row0, n_rows, src0, n_src, tile_rows):
    n_tiles = -(-n_rows // tile_rows)
    wptr = np.empty(n_tiles * W + 1, np.int64)
    n_slots = ctypes.c_int64(0)
    rc = lib.mirec_sweep_wave_build(rowptr.ctypes.data, col.ctypes.data, row0, n_rows, src0,
                                    n_src, tile_rows, wptr.ctypes.data, None, 0,
                                    ctypes.byref(n_slots))
    assert rc == _lib.ERR_WORKSPACE and n_slots.value > 0
    slot = np.empty(n_slots.value, np.int64)
    rc = lib.mirec_sweep_wave_build(rowptr.ctypes.data, col.ctypes.data, row0, n_rows, src0,
                                    n_src, tile_rows, wptr.ctypes.data, slot.ctypes.data,
                                    slot.shape[0], ctypes.byref(n_slots))
    assert rc == 0
    return slot


def pack(slot8, src0, n_src, tile_rows):
    slot4 = np.full(slot8.shape[0], 0xDEADBEEF, np.uint32)
    bits = ctypes.c_int32(-7)
    rc = lib.mirec_sweep_wave_pack(slot8.ctypes.data, slot8.shape[0], src0, n_src, tile_rows,
                                   slot4.ctypes.data, ctypes.byref(bits))
    return rc, slot4, bits.value


def unpack(slot4, bits, src0):
    col_bits = 32 - bits
    row = (slot4 >> np.uint32(col_bits)).astype(np.int64)
    row[row == (1 << bits) - 1] = -1
    col = (slot4 & np.uint32((1 << col_bits) - 1)).astype(np.int64) + src0
    return row, col


def check_roundtrip(slot8, src0, n_src, tile_rows):
    rc, slot4, bits = pack(slot8, src0, n_src, tile_rows)
    assert rc == 0
    assert (1 << (bits - 1)) <= tile_rows < (1 << bits)  # the smallest width that fits
    row, col = unpack(slot4, bits, src0)
    assert np.array_equal(row, slot8 >> 32)
    assert np.array_equal(col, slot8 & 0xFFFFFFFF)
    return row, col


@pytest.mark.parametrize("tile_rows", [8, 196, 255, 256, 280])
@pytest.mark.parametrize("block", ["items", "users"])
def test_packed_slots_unpack_to_the_8_byte_slots(csr, block, tile_rows):
    rowptr, col, nu, mi = csr
    row0, n_rows, src0, n_src = (nu, mi, 0, nu) if block == "items" else (0, nu, nu, mi)
    slot8 = build(rowptr, col, row0, n_rows, src0, n_src, tile_rows)
    row, scol = check_roundtrip(slot8, src0, n_src, tile_rows)
    pads = row == -1
    assert pads.any() and (~pads).any()
    # a padding slot carries the column of the slot before it
    idx = np.flatnonzero(pads)
    assert idx.min() > 0 and np.array_equal(scol[idx], scol[idx - 1])
    assert row.max() == min(tile_rows, n_rows) - 1
    if tile_rows == 8:
        assert pads.mean() > 0.5  # one row per wave: a step is one real slot


def test_row_field_width_at_the_edge(csr):
    rowptr, col, nu, mi = csr
    for tile_rows, want in ((255, 8), (256, 9), (1, 1), (3, 2), (4, 3)):
        slot8 = np.array([(tile_rows - 1) << 32 | 5, (0xFFFFFFFF << 32) | 5], np.uint64)
        rc, slot4, bits = pack(slot8.view(np.int64), 0, 100, tile_rows)
        assert rc == 0 and bits == want
        row, c = unpack(slot4, bits, 0)
        assert row.tolist() == [tile_rows - 1, -1] and c.tolist() == [5, 5]


def test_source_block_too_large_is_refused_before_any_write():
    slot8 = np.array([7], np.int64)  # row 0, column 7
    src0 = 3
    for n_src, ok in (((1 << 23) + 1, False), (1 << 23, True)):
        rc, slot4, bits = pack(slot8, src0, n_src, 256)
        if ok:
            assert rc == 0 and bits == 9 and slot4[0] == 4
        else:
            assert rc == ERR_RANGE
            assert slot4[0] == 0xDEADBEEF and bits == -7  # nothing was touched


def test_slot_outside_the_block_is_refused():
    for bad in (np.array([2], np.int64),                 # column below src0
                np.array([3 + 10], np.int64),            # column past the block
                np.array([(9 << 32) | 4], np.int64)):    # row past the tile
        rc, _, _ = pack(bad, 3, 10, 9)
        assert rc == ERR_RANGE


def test_length_not_a_multiple_of_64(csr):
    """The kernel loads a chunk of 64 slots clamped to the last slot; the host
    counterpart: a layout whose length is no multiple of 64 (streams are whole
    batches of 16) packs every slot, the last one included, and touches
    nothing past it."""
    rowptr, col, nu, mi = csr
    slot8 = build(rowptr, col, nu, mi, 0, nu, 196)
    n = slot8.shape[0]
    assert n % 16 == 0
    if n % 64 == 0:
        n -= 16
    slot8 = slot8[:n]
    guard = np.full(n + 4, 0xDEADBEEF, np.uint32)
    bits = ctypes.c_int32(0)
    rc = lib.mirec_sweep_wave_pack(slot8.ctypes.data, n, 0, nu, 196, guard.ctypes.data,
                                   ctypes.byref(bits))
    assert rc == 0 and bits.value == 8
    assert (guard[n:] == 0xDEADBEEF).all()
    row, c = unpack(guard[:n], bits.value, 0)
    assert np.array_equal(row, slot8 >> 32) and np.array_equal(c, slot8 & 0xFFFFFFFF)


def test_user_tile_rule():
    """Graph's default tile of a block swept in passes: at C2 (1 M user rows,
    512 workgroups, 320-row cap) 280 rows, 3 572 tiles, 6.98 passes."""
    from furusato_recommend_amd.graph import sweep_user_tile_rows
    t = sweep_user_tile_rows(1_000_000, 512, 320)
    assert t == 280 and -(-1_000_000 // t) == 3572
    assert sweep_user_tile_rows(1_000_000, 512, 256) == 256  # 8 passes, none of them even
    assert sweep_user_tile_rows(1000, 512, 320) == 320       # fewer tiles than workgroups
    assert sweep_user_tile_rows(512 * 3 * 64, 512, 100) == 96  # 1 024 tiles: 2 full passes
