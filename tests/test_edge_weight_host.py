"""Edge weights, host side: the CSR entry order (mirec_csr_entry_order), the
values and weighted dinv of a Graph built with weights, the bipartite form,
validation, and symmetry of a weighted edge multiset.  No GPU."""
import numpy as np
import pytest
import torch


def _entry_order(dst, n):
    from furusato_recommend_amd._lib import lib
    dst = np.ascontiguousarray(dst, np.int64)
    perm = np.full(len(dst), -1, np.int64)
    rc = lib.mirec_csr_entry_order(dst.ctypes.data, len(dst), n, perm.ctypes.data)
    return rc, perm


def _graph(n=40, nnz=500, seed=0, **kw):
    from furusato_recommend_amd.graph import Graph
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, nnz)
    dst = rng.integers(0, n - 3, nnz)          # the last rows stay empty
    dst[:70] = 5                               # a row longer than a 64-entry chunk
    w = rng.uniform(0.25, 4.0, nnz).astype(np.float32)
    g = Graph.from_edge_index(np.stack([src, dst]), n, "cpu", edge_weight=w, **kw)
    return g, src, dst, w


def test_entry_order_is_the_stable_destination_sort():
    rng = np.random.default_rng(1)
    n, nnz = 50, 700
    dst = np.concatenate([np.zeros(100, np.int64), rng.integers(0, n, nnz - 100)])
    rc, perm = _entry_order(dst, n)
    assert rc == 0
    assert np.array_equal(perm, np.argsort(dst, kind="stable"))
    # the order mirec_csr_from_coo writes its columns in
    from furusato_recommend_amd._lib import lib
    src = rng.integers(0, n, nnz).astype(np.int64)
    rowptr, col = np.empty(n + 1, np.int64), np.empty(nnz, np.int32)
    assert lib.mirec_csr_from_coo(src.ctypes.data, dst.ctypes.data, nnz, n, rowptr.ctypes.data,
                                  col.ctypes.data, None) == 0
    assert np.array_equal(col, src[perm])


def test_entry_order_empty_and_out_of_range():
    rc, perm = _entry_order(np.zeros(0, np.int64), 4)
    assert rc == 0 and perm.size == 0
    assert _entry_order([0, 4, 1], 4)[0] == 5   # MIREC_ERR_RANGE
    assert _entry_order([0, -1, 1], 4)[0] == 5


def test_graph_values_are_the_weights_in_entry_order():
    g, src, dst, w = _graph()
    perm = np.argsort(dst, kind="stable")
    assert np.array_equal(g.perm.numpy(), perm)
    assert np.array_equal(g.val.numpy(), w[perm])
    assert np.array_equal(g.col.numpy(), src[perm])
    assert g.csr.val == g.val.data_ptr()
    assert g.sweep_layout(64) is None
    from furusato_recommend_amd.graph import Graph
    plain = Graph.from_edge_index(np.stack([src, dst]), g.n_nodes, "cpu")
    assert plain.val is None and not plain.csr.val
    assert g.bytes_per_layer(64) == plain.bytes_per_layer(64) + 4 * g.nnz


def test_weighted_dinv_matches_float64():
    g, src, dst, w = _graph()
    deg = np.bincount(dst, weights=w.astype(np.float64), minlength=g.n_nodes)
    ref = np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)
    got = g.dinv.numpy().astype(np.float64)
    assert np.all(got[deg == 0] == 0.0) and (deg == 0).any()
    assert np.max(np.abs(got - ref) / np.maximum(ref, 1e-30)) < 1e-6
    g1, *_ = _graph(normalize=False)
    assert np.all(g1.dinv.numpy() == 1.0)


def test_bipartite_both_directions_carry_the_interaction_weight():
    from furusato_recommend_amd.graph import Graph
    rng = np.random.default_rng(2)
    nu, mi, ne = 9, 6, 80
    u, i = rng.integers(0, nu, ne), rng.integers(0, mi - 1, ne)   # last item isolated
    w = rng.uniform(0.25, 4.0, ne).astype(np.float32)
    g = Graph.from_interactions(u, i, nu, mi, "cpu", weight=w)
    rp, col, val, perm = g.rowptr_host, g.col_host, g.val.numpy(), g.perm.numpy()
    assert np.array_equal(val, w[perm]) and g.symmetric
    # row u lists its items in interaction order, row nu + i its users
    for r in range(nu + mi):
        es = np.nonzero(u == r)[0] if r < nu else np.nonzero(i == r - nu)[0]
        k = slice(rp[r], rp[r + 1])
        assert np.array_equal(perm[k], es)
        assert np.array_equal(col[k], (nu + i[es]) if r < nu else u[es])
        assert np.array_equal(val[k], w[es])
    deg = np.bincount(np.concatenate([u, nu + i]), weights=np.concatenate([w, w]).astype(np.float64),
                      minlength=nu + mi)
    ref = np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)
    assert np.max(np.abs(g.dinv.numpy() - ref) / np.maximum(ref, 1e-30)) < 1e-6
    assert g.dinv.numpy()[-1] == 0.0


@pytest.mark.parametrize("bad,normalize", [
    (np.array([1.0, np.nan, 1.0, 1.0]), True),
    (np.array([1.0, np.inf, 1.0, 1.0]), False),
    (np.array([1.0, -0.5, 1.0, 1.0]), True),
    (np.ones(3), True),
    (np.ones((4, 1)), False),
])
def test_invalid_weights_raise(bad, normalize):
    from furusato_recommend_amd.graph import Graph
    ei = np.array([[0, 1, 2, 1], [1, 0, 1, 2]])
    with pytest.raises(ValueError):
        Graph.from_edge_index(ei, 3, "cpu", edge_weight=bad, normalize=normalize)
    if bad.shape == (4,):
        with pytest.raises(ValueError):
            Graph.from_interactions(ei[0], ei[1], 3, 3, "cpu", weight=bad)


def test_negative_weights_allowed_without_normalisation_and_refresh():
    from furusato_recommend_amd.graph import Graph
    ei = np.array([[0, 1, 2, 1], [1, 0, 1, 2]])
    g = Graph.from_edge_index(ei, 3, "cpu", edge_weight=np.array([1.0, -2.0, 3.0, -4.0]),
                              normalize=False)
    assert np.array_equal(g.val.numpy(), np.float32([-2.0, 1.0, 3.0, -4.0]))
    # set_edge_weight: values (and the transpose's) follow a new tensor
    g.set_edge_weight(torch.tensor([5.0, 6.0, 7.0, 8.0]))
    assert np.array_equal(g.val.numpy(), np.float32([6.0, 5.0, 7.0, 8.0]))
    assert not g.symmetric
    assert np.array_equal(g.transpose.val.numpy(), np.float32([5.0, 6.0, 8.0, 7.0]))
    with pytest.raises(ValueError):
        g.set_edge_weight(torch.ones(5))
    gn = Graph.from_edge_index(ei, 3, "cpu", edge_weight=np.ones(4))
    with pytest.raises(ValueError):
        gn.set_edge_weight(torch.ones(4))      # dinv depends on the weights
    with pytest.raises(ValueError):
        Graph.from_edge_index(ei, 3, "cpu").set_edge_weight(torch.ones(4))


def test_symmetry_is_decided_on_weighted_triples():
    from furusato_recommend_amd.graph import Graph
    # 0 <-> 1 and 1 <-> 2, the second pair duplicated: a symmetric structure
    src = np.array([0, 1, 2, 1, 1, 2])
    dst = np.array([1, 0, 1, 2, 2, 1])
    ei = np.stack([src, dst])
    sym = Graph.from_edge_index(ei, 3, "cpu", edge_weight=np.array([1.5, 1.5, 2.0, 2.0, 3.0, 3.0]))
    assert sym.symmetric and sym.transpose is None
    # the duplicates' weights matched crosswise still form the same triples
    cross = Graph.from_edge_index(ei, 3, "cpu", edge_weight=np.array([1.5, 1.5, 2.0, 3.0, 2.0, 3.0]))
    assert cross.symmetric
    w = np.array([1.5, 0.5, 2.0, 2.0, 3.0, 3.0], np.float32)      # w_01 != w_10
    asym = Graph.from_edge_index(ei, 3, "cpu", edge_weight=w)
    assert not asym.symmetric
    t = asym.transpose
    pt = np.argsort(src, kind="stable")
    assert np.array_equal(t.col.numpy(), dst[pt])
    assert np.array_equal(t.val.numpy(), w[pt])
    assert np.array_equal(t.dinv.numpy(), asym.dinv.numpy())
    # dense check: the transpose CSR is the transposed weighted matrix
    def dense(g):
        a = np.zeros((3, 3))
        rp, c, v = g.rowptr_host, g.col.numpy(), g.val.numpy()
        for r in range(3):
            for k in range(rp[r], rp[r + 1]):
                a[r, c[k]] += v[k]
        return a
    assert np.array_equal(dense(t), dense(asym).T)
