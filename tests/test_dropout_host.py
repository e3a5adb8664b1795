"""tests/dropout_common.py checked on the host: the restated mask rule of
csrc/common.h (published splitmix64 vectors, the suite's other restatements,
the documented values of dropout_params, vectorised == scalar, the kept
fraction), the float64 references against torch float64 autograd, and the
coverage the case lists of tests/test_sage_kernels.py and
tests/test_rowtail_dropout_kernels.py claim.  No GPU.

Every seed is fixed; the kept-fraction bound is a condition on those seeds
(0.002 is 4 sigma of the binomial over 2^20 draws at p = 0.5), not a
measurement."""
import numpy as np
import pytest
import torch

from tests import dropout_common as dc

P_VALUES = (0.3, 0.5, 1e-6, 0.999995, 0.0)


# ------------------------------------------------------------------- the rule
def test_mix64_published_splitmix64_vectors():
    g = 0x9E3779B97F4A7C15
    assert dc.mix64(0) == 0xE220A8397B1DCDAF
    assert dc.mix64(g) == 0x6E789E6AA1B965F4
    assert dc.mix64((2 * g) & dc.M64) == 0x06C45D188009454F
    got = dc.mix64_v(np.array([0, g, (2 * g) & dc.M64], np.uint64))
    assert [int(x) for x in got] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def test_mix64_agrees_with_the_other_restatements():
    from tests.test_edge_dropout_host import mix64 as mix_edge
    from tests.test_gpu_parity import _mix64 as mix_parity
    rng = np.random.default_rng(1)
    xs = [0, 1, dc.M64, 1 << 63] + [int(x) for x in rng.integers(0, 1 << 63, 200)] \
        + [int(x) + (1 << 63) for x in rng.integers(0, 1 << 63, 200)]
    vec = dc.mix64_v(np.array(xs, np.uint64))
    for x, v in zip(xs, vec):
        assert dc.mix64(x) == mix_parity(x) == int(mix_edge(x)) == int(v)


def test_dropout_params_values():
    assert dc.dropout_params(0.3, 0)[1] == 19661
    key, thresh, scale = dc.dropout_params(0.5, 7)
    assert thresh == 32768 and scale == np.float32(2) and scale.dtype == np.float32
    assert key == dc.mix64(7 ^ 0xA24BAED4963EE407)
    assert dc.dropout_params(1e-6, 0)[1] == 1
    assert dc.dropout_params(0.999995, 0)[1] == 65535
    assert dc.dropout_params(0.0, 0)[1:] == (0, np.float32(1))
    s = dc.dropout_params(0.3, 0)[2]
    assert s == np.float32(1) / (np.float32(1) - np.float32(0.3)) and s.dtype == np.float32
    # a seed >= 2^63 is a plain uint64
    assert dc.dropout_params(0.3, dc.SEED_BIG)[0] == dc.mix64(dc.SEED_BIG ^ 0xA24BAED4963EE407)
    for bad in (1.0, -0.1, float("nan"), 1.5):
        with pytest.raises(ValueError):
            dc.dropout_params(bad, 0)


def test_vectorised_keep_equals_scalar_keep():
    rng = np.random.default_rng(2)
    idx = np.concatenate([np.arange(64), rng.integers(0, 1 << 40, 500),
                          (1 << 33) + np.arange(9)]).astype(np.uint64)
    keys = [dc.dropout_params(0.3, s)[0] for s in dc.SEEDS] + [dc.M64, dc.M64 - 5, 0]
    for key in keys:          # the last keys make key + (idx >> 2) wrap
        for thresh in (1, 19661, 32768, 65535):
            vec = dc.keep_v(key, thresh, idx)
            assert [bool(v) for v in vec] == [dc.keep(key, thresh, int(i)) for i in idx]
    assert dc.keep_v(keys[0], 0, idx).all()
    # the four elements of a quad are the four 16-bit slices of one hash
    h = dc.mix64((dc.M64 - 5 + 3) & dc.M64)
    for j in range(4):
        assert dc.keep(dc.M64 - 5, 30000, 12 + j) == (((h >> (16 * j)) & 0xFFFF) >= 30000)


def test_quad_form_equals_the_element_form():
    for key in (dc.dropout_params(0.3, dc.SEED_BIG)[0], dc.M64 - 2, 0):
        for thresh in (0, 1, 19661, 32768, 65535):
            for n, w in ((7, 4), (5, 12), (3, 260)):
                assert np.array_equal(dc.keep_rows(key, thresh, n, w),
                                      dc.keep_v(key, thresh, dc.fanout_index(n, w)))
    m, _ = dc.fanout_mask(0.5, 7, 6, 8)
    key, thresh, _ = dc.dropout_params(0.5, 7)
    assert m.shape == (6, 8) and bool(m[4, 3]) == dc.keep(key, thresh, 4 * 8 + 3)


@pytest.mark.parametrize("p", P_VALUES)
def test_kept_fraction(p):
    key, thresh, _ = dc.dropout_params(p, 123)
    frac = float(dc.keep_v(key, thresh, np.arange(1 << 20, dtype=np.uint64)).mean())
    assert abs(frac - (1 - thresh / 65536)) < 0.002, frac


def test_run_key_and_null_base_differ():
    key = dc.dropout_params(0.3, 5)[0]
    assert dc.run_key(key, 0) == dc.mix64(key) != key
    assert dc.run_key(key, (1 << 63) + 5) == dc.mix64(key ^ ((1 << 63) + 5))
    a, _ = dc.rowtail_mask(0.3, 5, 16, 8, None)
    b, _ = dc.rowtail_mask(0.3, 5, 16, 8, 0)
    assert not np.array_equal(a, b)


def test_element_indices():
    idx = dc.fanout_index(6, 12)
    assert idx.dtype == np.uint64 and int(idx[5, 7]) == 5 * 12 + 7
    # (t*k + c)*dim + col with t = 1, k = 3, c = 2
    assert int(idx[1 * 3 + 2, 0]) == (1 * 3 + 2) * 12


# -------------------------------------------------- references against autograd
@pytest.mark.parametrize("p", [0.0, 0.3, 0.5])
def test_references_equal_torch_float64_autograd(p):
    n_t, k, dim, n_rows = 9, 5, 8, 11
    rng = np.random.default_rng(int(p * 10))
    ids = rng.integers(0, n_rows, n_t * k).astype(np.int32)
    ids[rng.random(n_t * k) < 0.3] = -1
    ids[:k] = -1
    valid = ids >= 0
    mask, scale = dc.fanout_mask(p, 123, n_t * k, dim)
    table = rng.standard_normal((n_rows, dim)).astype(np.float32)
    g = rng.standard_normal((n_t, dim)).astype(np.float32)
    base = rng.standard_normal((n_rows, dim)).astype(np.float32)

    tt = torch.from_numpy(table).double().requires_grad_(True)
    x = tt[torch.from_numpy(np.maximum(ids, 0)).long()]
    x.retain_grad()
    m = torch.from_numpy(mask & valid[:, None]).double()
    cnt = torch.from_numpy(valid.reshape(n_t, k).sum(1)).double().clamp(min=1)
    out = (x * m * float(scale)).view(n_t, k, dim).sum(1) / cnt[:, None]
    out.backward(torch.from_numpy(g).double())

    rows = table[np.maximum(ids, 0)]
    ref, A, cnt_ref = dc.fanout_mean_ref(rows, valid, k, mask, scale)
    assert np.abs(ref - out.detach().numpy()).max() < 1e-12
    assert (ref[0] == 0).all() and (A >= np.abs(ref) - 1e-15).all()
    assert np.array_equal(cnt_ref, valid.reshape(n_t, k).sum(1))
    gx = dc.fanout_mean_bwd_ref(g, valid, k, mask, scale)
    assert np.abs(gx - x.grad.numpy()).max() < 1e-12
    tg, A2, mm = dc.gather_bwd_ref(g, ids, k, mask, scale, base)
    assert np.abs(tg - (base.astype(np.float64) + tt.grad.numpy())).max() < 1e-12
    assert np.array_equal(mm, np.bincount(ids[valid], minlength=n_rows))
    assert (A2 >= np.abs(tg) - 1e-12).all() and (A2 >= np.abs(base)).all()
    # the adjoint identity <g, fwd(x)> == <bwd(g), x>
    lhs = float((g.astype(np.float64) * ref).sum())
    rhs = float((gx * rows.astype(np.float64)).sum())
    assert abs(lhs - rhs) < 1e-12 * max(1.0, abs(lhs))


def test_gamma_is_the_standard_constant():
    assert dc.gamma(1) == dc.U / (1 - dc.U)
    assert np.allclose(dc.gamma(np.array([4, 68])), [4 * dc.U / (1 - 4 * dc.U),
                                                     68 * dc.U / (1 - 68 * dc.U)], rtol=0, atol=0)
    b = dc.sum_bound(np.ones((2, 3)), np.array([0, 64]))
    assert b.shape == (2, 3) and b[0, 0] == dc.gamma(4) and b[1, 2] == dc.gamma(68)


# ------------------------------------------------------------ coverage conditions
def _d4_pow2(dim):
    d4 = dim // 4
    return d4 <= 64 and d4 & (d4 - 1) == 0


def test_fanout_case_list_covers_every_dispatch_edge():
    cases = dc.fanout_cases()
    assert {c["dim"] for c in cases} >= {4, 8, 12, 64, 256, 260, 512}
    assert {c["k"] for c in cases} >= {1, 5, 8, 9, 25, 64, 70}
    assert {c["n_t"] for c in cases} == {1, 37}
    assert {c["p"] for c in cases} == {0.0, 0.3, 0.5}
    assert {c["seed"] for c in cases} == set(dc.SEEDS) and max(dc.SEEDS) >= 1 << 63
    assert {c["n_rows"] for c in cases} == {1, 64, 1000}
    pow2 = [c for c in cases if _d4_pow2(c["dim"]) and c["n_t"] == 37]
    assert any(c["k"] < c["dim"] // 4 for c in pow2)           # one ballot round
    assert any(c["k"] > c["dim"] // 4 > 1 for c in pow2)       # several
    assert any(c["dim"] == 256 and c["k"] > 64 for c in pow2)  # several whole-wave rounds
    # the loop count (d4 not a power of two, or above 64) with p > 0 and p = 0
    loop = [c for c in cases if not _d4_pow2(c["dim"]) and c["n_t"] == 37 and c["k"] > 1]
    assert {c["dim"] for c in loop} >= {12, 260, 512}
    assert any(c["p"] == 0 for c in loop) and any(c["p"] > 0 for c in loop)
    # partial last wave of the unfused backward, partial last block of the atomic one
    assert any(c["n_t"] * c["k"] * (c["dim"] // 4) == 185 for c in cases) and 37 % 4
    assert all(c["k"] <= 64 or c["dim"] % 4 == 0 for c in cases)


@pytest.mark.parametrize("case", dc.fanout_cases(), ids=lambda c: f"t{c['n_t']}k{c['k']}d{c['dim']}")
def test_fanout_case_holds_the_named_targets(case):
    n_t, k, dim, n_rows = case["n_t"], case["k"], case["dim"], case["n_rows"]
    ids = dc.fanout_ids(case)
    assert ids.shape == (n_t * k,) and ids.dtype == np.int32
    assert ids.min() >= -1 and ids.max() < n_rows
    v = (ids >= 0).reshape(n_t, k)
    assert v.any()
    if n_t >= 4:
        cnt = v.sum(1)
        assert (cnt == 0).any()
        assert any(cnt[t] == 1 and v[t, -1] for t in range(n_t))
        assert (cnt == k).any()
        if k >= 2:   # (a single child cannot repeat)
            r = ids.reshape(n_t, k)
            assert any(len(np.unique(r[t][v[t]])) < v[t].sum() for t in range(n_t))
        if k >= 4:
            assert ((cnt > 0) & (cnt < k)).sum() >= 2    # mixed validity
    if case["p"] > 0:
        mask, _ = dc.fanout_mask(case["p"], case["seed"], n_t * k, dim)
        sel = mask[ids >= 0]
        assert sel.any() and not sel.all()
        # and not the same mask for every child of a target or every target
        if n_t >= 4 and k >= 2:
            m3 = mask.reshape(n_t, k, dim)
            assert not np.array_equal(m3[2, 0], m3[2, 1]) or dim == 4
            assert not np.array_equal(m3[2], m3[3])


def test_sorted_case_list_holds_the_run_layouts():
    cases = dc.sorted_cases()
    assert len(cases) == len(dc.fanout_cases()) + 4
    assert {c["n_rows"] for c in cases} == {1, 64, 1000}
    on_grid = crossing = two_chunks = no_tail = all_invalid = wide_two = 0
    for c in cases:
        ids, n = c["ids"], c["n_t"] * c["k"]
        assert ids.shape == (n,) and ids.dtype == np.int32
        assert ids.min() >= -1 and ids.max() < c["n_rows"]
        ks, runs = dc.sorted_runs(ids, c["n_rows"])
        assert sum(e - s for _, s, e in runs) == int((ids >= 0).sum())
        no_tail += bool((ids >= 0).all())
        all_invalid += bool((ids < 0).all())
        for _, s, e in runs:
            on_grid += s > 0 and s % 64 == 0
            crossing += s % 64 != 0 and (e - 1) // 64 == s // 64 + 1
            two = (e // 64) - ((s + 63) // 64) >= 2
            two_chunks += two
            wide_two += two and c["dim"] > 256
        if c["p"] > 0 and (ids >= 0).any():
            mask, _ = dc.fanout_mask(c["p"], c["seed"], n, c["dim"])
            sel = mask[ids >= 0]
            assert sel.any() and not sel.all()
    assert on_grid and crossing and two_chunks and no_tail and all_invalid
    assert wide_two      # a run over whole chunks at dim > 256 (two column passes)
    # the layout case as it was built: the second run starts on entry 64 and
    # holds chunks 1 and 2, the fourth crosses entry 256
    runs = dc.sorted_runs(cases[len(dc.fanout_cases())]["ids"], 1000)[1]
    assert [(s, e) for _, s, e in runs[:4]] == [(0, 64), (64, 214), (214, 224), (224, 264)]


def test_rowtail_case_list():
    cases = dc.rowtail_cases()
    assert {c["d"] for c in cases} >= {4, 12, 36, 128, 520, 1024}
    assert {dc.rowtail_shape(c["d"]) for c in cases} == \
        {(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4)}
    assert dc.rowtail_shape(520) == (64, 4) and dc.rowtail_shape(128) == (32, 1)
    assert {c["n"] for c in cases} == {1, 67}
    assert {c["p"] for c in cases} == {0.3, 0.5}
    assert {c["base"] for c in cases} == {None, 0, 1, (1 << 63) + 5}
    fused = dc.fused_rowtail_cases()
    assert {c["base"] for c in fused} >= {None, 0, (1 << 63) + 5} and {c["n"] for c in fused} == {1, 67}
    for c in cases:
        mask, scale = dc.rowtail_mask(c["p"], c["seed"], c["n"], c["d"], c["base"])
        assert mask.shape == (c["n"], c["d"]) and mask.any() and not mask.all()
        other, _ = dc.rowtail_mask(c["p"], c["seed"], c["n"], c["d"],
                                   0 if c["base"] is None else None)
        assert not np.array_equal(mask, other)      # the base decides the mask
