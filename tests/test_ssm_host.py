"""mirec_cpu_ssm_sample, the host twin of the sampled-softmax sampler (the
streams the device kernel runs, restated on CPU threads): equality with
mirec_cpu_bpr_sample at K = 1, the shared (u, p, first negative) columns,
thread-count independence, validity, (seed, offset + t) addressing, the
exhausted-retry flag, argument checks and one uniformity check.  No GPU.

All seeds are fixed; the statistical bound is a condition on those seeds
(5 sigma of the binomial), not a measurement."""
import ctypes

import numpy as np
import pytest
import torch

from tests.ssm_common import cpu_bpr_sample, cpu_ssm_sample, host_graph, sampler_interactions

NU, MI = 300, 50


@pytest.fixture(scope="module")
def data():
    u, i = sampler_interactions(NU, MI)
    return u, i


@pytest.fixture(scope="module", params=[False, True], ids=["uniform", "pos_cdf"])
def graph(request, data):
    g = host_graph(data[0], data[1], NU, MI, probs=request.param)
    deg = np.diff(g.rowptr_host[: NU + 1])
    assert deg[7] == 0                                # no positives
    assert len(np.unique(_positives(g, 11))) == MI - 2  # all items but two
    cell = data[0] * MI + data[1]
    assert len(np.unique(cell)) < len(cell)           # multi-edges
    return g


def _positives(g, u):
    rp, col = g.rowptr_host, g.col_host
    return col[rp[u]:rp[u + 1]] - g.n_users


def test_k1_equals_the_bpr_sampler_bit_for_bit(graph):
    for shard, n_shards in ((0, 1), (1, 3)):
        rc, u, p, n, err = cpu_ssm_sample(graph, 5000, 1, 9, 77, shard, n_shards)
        rc2, u2, p2, n2, err2 = cpu_bpr_sample(graph, 5000, 9, 77, shard, n_shards)
        assert rc == rc2 == 0 and err == err2 == 0
        assert np.array_equal(u, u2) and np.array_equal(p, p2) and np.array_equal(n[:, 0], n2)
        assert np.all(u % n_shards == shard)


def test_first_columns_at_k8_equal_the_k1_call(graph):
    _, u1, p1, n1, _ = cpu_ssm_sample(graph, 4000, 1, 3, 1000)
    rc, u8, p8, n8, err = cpu_ssm_sample(graph, 4000, 8, 3, 1000)
    assert rc == 0 and err == 0 and n8.shape == (4000, 8)
    assert np.array_equal(u1, u8) and np.array_equal(p1, p8) and np.array_equal(n1[:, 0], n8[:, 0])
    assert len(np.unique(n8[:, 1:])) > MI // 2        # the other columns are drawn too


def test_independent_of_the_thread_count(graph):
    # 9 000 pairs: up to three worker threads take contiguous blocks
    base = cpu_ssm_sample(graph, 9000, 4, 5, 0, n_threads=1)
    for nt in (2, 3, 16):
        got = cpu_ssm_sample(graph, 9000, 4, 5, 0, n_threads=nt)
        assert all(np.array_equal(a, b) for a, b in zip(base[1:4], got[1:4])) and got[4] == 0


def test_negatives_are_valid(graph):
    rc, u, p, n, err = cpu_ssm_sample(graph, 3000, 8, 21, 5)
    assert rc == 0 and err == 0
    assert u.min() >= 0 and u.max() < NU and 7 not in u
    assert p.min() >= 0 and p.max() < MI and n.min() >= 0 and n.max() < MI
    for t in range(len(u)):
        row = _positives(graph, u[t])
        assert p[t] in row and not np.isin(n[t], row).any()
    assert 11 in u                                    # the user with two candidates only
    assert set(n[u == 11].reshape(-1).tolist()) == {MI - 2, MI - 1}


def test_reproducible_with_offset_addressing(graph):
    a = cpu_ssm_sample(graph, 600, 5, 4, 100)
    b = cpu_ssm_sample(graph, 600, 5, 4, 100)
    assert all(np.array_equal(x, y) for x, y in zip(a[1:4], b[1:4]))
    # pair t of a call is stream (seed, offset + t)
    c = cpu_ssm_sample(graph, 400, 5, 4, 300)
    assert all(np.array_equal(x[200:], y) for x, y in zip(a[1:4], c[1:4]))
    d = cpu_ssm_sample(graph, 600, 5, 5, 100)         # another seed: another batch
    assert not np.array_equal(a[3], d[3])


def test_err_is_set_when_a_user_holds_every_item():
    g = host_graph(np.array([0, 0, 0, 1]), np.array([0, 1, 2, 0]), 2, 3)
    rc, u, p, n, err = cpu_ssm_sample(g, 64, 3, 1, 0)
    assert rc == 0 and err == 1 and 0 in u
    ok = u == 1
    assert not np.isin(n[ok], [0]).any()              # user 1's pairs are still drawn
    g2 = host_graph(np.array([0, 1]), np.array([0, 1]), 2, 3)
    assert cpu_ssm_sample(g2, 64, 3, 1, 0)[4] == 0


def test_bad_arguments_are_refused(graph):
    from furusato_recommend_amd import _lib
    rc, u, p, n, err = cpu_ssm_sample(graph, 16, 0, 1, 0)
    assert rc == 1 and np.all(u == -7) and np.all(n == -7)            # MIREC_ERR_ARG
    assert cpu_ssm_sample(graph, 16, -3, 1, 0)[0] == 1
    bufs = [torch.zeros(16, dtype=torch.int32) for _ in range(4)]
    base = [graph.rowptr_host.ctypes.data, graph.col_host.ctypes.data, None, None]
    for null in (0, 1, 4, 5, 6, 7):
        args = base + [b.data_ptr() for b in bufs]
        args[null] = None
        rc = _lib.lib.mirec_cpu_ssm_sample(args[0], args[1], args[2], args[3], NU, MI, 4, 4,
                                           ctypes.c_uint64(1), ctypes.c_uint64(0), 0, 1,
                                           args[4], args[5], args[6], args[7], 1)
        assert rc == 1, null


def test_negatives_are_uniform_over_the_non_positives(data):
    """For five users, every non-positive item's share of the user's negatives
    (all K columns) over the fixed seeds below stays within 5 sigma of the
    binomial — a condition on these seeds."""
    g = host_graph(data[0], data[1], NU, MI)
    users = (0, 1, 2, 3, 11)
    counts = {u: np.zeros(MI, np.int64) for u in users}
    for seed in (101, 102, 103):
        _, u, p, n, err = cpu_ssm_sample(g, 60_000, 8, seed, 0)
        assert err == 0
        for w in users:
            counts[w] += np.bincount(n[u == w].reshape(-1), minlength=MI)
    worst = 0.0
    for w in users:
        cand = np.setdiff1d(np.arange(MI), _positives(g, w))
        c, tot = counts[w], counts[w].sum()
        assert tot > 2000 and c[np.setdiff1d(np.arange(MI), cand)].sum() == 0
        q = 1.0 / len(cand)
        z = np.abs(c[cand] - tot * q) / np.sqrt(tot * q * (1 - q))
        worst = max(worst, float(z.max()))
    print(f"largest deviation: {worst:.2f} sigma")
    assert worst <= 5.0
