"""The column-sweep layout of the item rows (mirec_sweep_build, include/mirec.h)
built through the C ABI on small numpy graphs, no GPU: it is a permutation of
exactly the item rows' entries, every row's entries ascend in column with
duplicate edges in CSR order, and the tile / group bounds cover every item row
exactly once (empty rows, ragged last tile and group included)."""
import ctypes

import numpy as np
import pytest


def _csr(u, i, nu, mi):
    from furusato_recommend_amd._lib import lib
    u = np.ascontiguousarray(u, np.int64)
    i = np.ascontiguousarray(i, np.int64)
    n = nu + mi
    rowptr = np.empty(n + 1, np.int64)
    col = np.empty(2 * len(u), np.int32)
    dinv = np.empty(n, np.float32)
    assert lib.mirec_csr_bipartite(u.ctypes.data, i.ctypes.data, len(u), nu, mi,
                                   rowptr.ctypes.data, col.ctypes.data, dinv.ctypes.data) == 0
    return rowptr, col


def _build(rowptr, col, nu, mi, tile_rows, group_rows, n_src=None):
    from furusato_recommend_amd._lib import lib
    nt, ng = ctypes.c_int32(0), ctypes.c_int32(0)
    assert lib.mirec_sweep_shape(mi, tile_rows, group_rows, ctypes.byref(nt),
                                 ctypes.byref(ng)) == 0
    assert nt.value == -(-mi // tile_rows) and ng.value == -(-tile_rows // group_rows)
    n_ent = int(rowptr[nu + mi] - rowptr[nu])
    gptr = np.full(nt.value * ng.value + 1, -1, np.int64)
    ent = np.full(2 * max(n_ent, 1), -7, np.int32)
    rc = lib.mirec_sweep_build(rowptr.ctypes.data, col.ctypes.data, nu, mi,
                               nu if n_src is None else n_src, tile_rows, group_rows,
                               gptr.ctypes.data, ent.ctypes.data)
    return rc, nt.value, ng.value, gptr, ent[:2 * n_ent].reshape(-1, 2)


def _check(rowptr, col, nu, mi, tile_rows, group_rows):
    rc, nt, ng, gptr, ent = _build(rowptr, col, nu, mi, tile_rows, group_rows)
    assert rc == 0
    base = rowptr[nu]
    n_ent = int(rowptr[nu + mi] - base)
    assert gptr[0] == 0 and gptr[-1] == n_ent and np.all(np.diff(gptr) >= 0)
    seen_rows = np.zeros(mi, np.int64)
    got = {}  # item row -> its columns in stream order
    for t in range(nt):
        tile_len = min(tile_rows, mi - t * tile_rows)
        for g in range(ng):
            lo = min(g * group_rows, tile_len)
            hi = min(lo + group_rows, tile_len)
            seen_rows[t * tile_rows + lo:t * tile_rows + hi] += 1
            e = ent[gptr[t * ng + g]:gptr[t * ng + g + 1]]
            # the stream holds exactly its rows' entries ...
            assert len(e) == rowptr[nu + t * tile_rows + hi] - rowptr[nu + t * tile_rows + lo]
            assert np.all((e[:, 1] >= lo) & (e[:, 1] < hi))
            # ... sorted by column (the kernel walks the bands in this order)
            assert np.all(np.diff(e[:, 0]) >= 0)
            for c, lr in e:
                got.setdefault(t * tile_rows + int(lr), []).append(int(c))
    assert np.all(seen_rows == 1)  # every item row in exactly one (tile, group)
    total = 0
    for r in range(mi):
        cols = col[rowptr[nu + r]:rowptr[nu + r + 1]]
        # per row: the CSR entries stably sorted by column == ascending column,
        # duplicates kept (a permutation of the row's entries, nothing else)
        assert got.get(r, []) == np.sort(cols, kind="stable").tolist()
        total += len(cols)
    assert total == n_ent == sum(len(v) for v in got.values())


@pytest.mark.parametrize("tile_rows,group_rows", [(16, 3), (7, 7), (5, 1), (64, 2), (100, 4)])
def test_layout_random_graph(tile_rows, group_rows):
    rng = np.random.default_rng(5)
    nu, mi, ne = 300, 61, 2500  # 61: no multiple of any tile or group size used
    u = rng.integers(0, nu, ne)
    i = rng.integers(0, mi - 3, ne)  # the last three items have no edges
    i[:40] = 7                       # a heavy item; duplicate (user, item) edges below
    u[:10] = 5
    rowptr, col = _csr(u, i, nu, mi)
    assert rowptr[nu + mi] - rowptr[nu + mi - 3] == 0
    _check(rowptr, col, nu, mi, tile_rows, group_rows)


def test_layout_duplicates_keep_csr_order():
    """Duplicate edges are distinguishable only by position: tag them through
    a second graph whose columns encode the edge order."""
    nu, mi = 6, 2
    u = np.array([4, 1, 4, 0, 4, 1, 3])
    i = np.array([0, 0, 0, 1, 0, 0, 1])
    rowptr, col = _csr(u, i, nu, mi)
    rc, nt, ng, gptr, ent = _build(rowptr, col, nu, mi, 2, 1)
    assert rc == 0 and nt == 1 and ng == 2
    assert ent[gptr[0]:gptr[1]].tolist() == [[1, 0], [1, 0], [4, 0], [4, 0], [4, 0]]
    assert ent[gptr[1]:gptr[2]].tolist() == [[0, 1], [3, 1]]
    # the sort key is (column, CSR position): equal columns stay in CSR order,
    # checked on the builder's index arithmetic with distinct columns in a
    # row whose CSR order is descending
    u2 = np.array([5, 4, 3, 2, 1, 0])
    rowptr2, col2 = _csr(u2, np.zeros(6, np.int64), nu, mi)
    rc, _, _, gptr2, ent2 = _build(rowptr2, col2, nu, mi, 2, 2)
    assert rc == 0 and ent2[:, 0].tolist() == [0, 1, 2, 3, 4, 5]


def test_layout_empty_and_errors():
    from furusato_recommend_amd._lib import lib
    nu, mi = 4, 3
    rowptr, col = _csr(np.zeros(0, np.int64), np.zeros(0, np.int64), nu, mi)
    rc, nt, ng, gptr, ent = _build(rowptr, np.zeros(1, np.int32), nu, mi, 2, 1)
    assert rc == 0 and np.all(gptr == 0) and len(ent) == 0
    # a column outside the source block: MIREC_ERR_RANGE
    rowptr, col = _csr([0, 3], [0, 1], nu, mi)
    rc, *_ = _build(rowptr, col, nu, mi, 2, 1, n_src=3)
    assert rc == 5
    n = ctypes.c_int32(0)
    assert lib.mirec_sweep_shape(5, 0, 1, ctypes.byref(n), ctypes.byref(n)) == 1
    assert lib.mirec_sweep_groups(64) == 32
    assert lib.mirec_sweep_groups(32) == 0
