"""Shared by tests/test_ssm_host.py, tests/test_ssm_kernels.py and
tests/test_ssm.py: the sampler's host graph, the float64 restatement of the
sampled-softmax loss (per-pair quantities, seed tables, the dense training
step) and its float32 twin for the kernel tolerance protocol.  Nothing here
is collected by pytest.

The loss.  Pair t = (u, p) with negatives n_0 .. n_{K-1},
temperature tau, out = the layer mean, E = the table:
    s+ = <out_u, out_p> / tau,  s_k = <out_u, out_nk> / tau
    l_t = logsumexp(s+, s_.) - s+
    reg_t = 1/2 (|E_u|^2 + |E_p|^2 + sum_k |E_nk|^2)
    loss = mean_t l_t + decay * sum_t reg_t / B
"""
import ctypes

import numpy as np
import torch

F32 = np.float32
U24 = 2.0 ** -24


def rel(a, b):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


# ------------------------------------------------------------------- sampler
def sampler_interactions(n_users=300, m_items=50, seed=5):
    """A few hundred users x 50 items: user 7 has no positives, user 11 holds
    every item but two, 60 interactions appear twice (multi-edges)."""
    rng = np.random.default_rng(seed)
    us, its = [], []
    for u in range(n_users):
        if u == 7:
            continue
        if u == 11:
            row = np.arange(m_items - 2)
        else:
            row = rng.choice(m_items, int(rng.integers(1, 12)), replace=False)
        us.append(np.full(len(row), u))
        its.append(row)
    u, i = np.concatenate(us), np.concatenate(its)
    dup = rng.choice(len(u), 60, replace=False)
    u, i = np.concatenate([u, u[dup]]), np.concatenate([i, i[dup]])
    order = rng.permutation(len(u))
    return u[order].astype(np.int64), i[order].astype(np.int64)


def host_graph(u, i, n_users, m_items, probs=False):
    from furusato_recommend_amd.graph import Graph
    g = Graph.from_interactions(u, i, n_users, m_items, "cpu")
    if probs:
        rng = np.random.default_rng(1)
        g.set_positive_probs([rng.random(int(d)) + 0.01
                              for d in np.diff(g.rowptr_host[: n_users + 1])])
    return g


def cpu_ssm_sample(g, batch, k, seed, offset, shard=0, n_shards=1, n_threads=1):
    """mirec_cpu_ssm_sample on a host graph: (rc, users, pos, neg [batch, k], err)."""
    from furusato_recommend_amd import _lib
    u = torch.full((max(batch, 1),), -7, dtype=torch.int32)
    p = torch.full((max(batch, 1),), -7, dtype=torch.int32)
    n = torch.full((max(batch, 1), max(k, 1)), -7, dtype=torch.int32)
    err = torch.zeros(1, dtype=torch.int32)
    rc = _lib.lib.mirec_cpu_ssm_sample(
        g.rowptr_host.ctypes.data, g.col_host.ctypes.data, _lib.ptr(g.col_sorted),
        _lib.ptr(getattr(g, "pos_cdf", None)), g.n_users, g.m_items, batch, k,
        ctypes.c_uint64(seed), ctypes.c_uint64(offset), shard, n_shards, u.data_ptr(),
        p.data_ptr(), n.data_ptr(), err.data_ptr(), n_threads)
    return rc, u.numpy(), p.numpy(), n.numpy(), int(err.item())


def cpu_bpr_sample(g, batch, seed, offset, shard=0, n_shards=1, n_threads=1):
    from furusato_recommend_amd import _lib
    u, p, n = (torch.full((max(batch, 1),), -7, dtype=torch.int32) for _ in range(3))
    err = torch.zeros(1, dtype=torch.int32)
    rc = _lib.lib.mirec_cpu_bpr_sample(
        g.rowptr_host.ctypes.data, g.col_host.ctypes.data, _lib.ptr(g.col_sorted),
        _lib.ptr(getattr(g, "pos_cdf", None)), g.n_users, g.m_items, batch,
        ctypes.c_uint64(seed), ctypes.c_uint64(offset), shard, n_shards, u.data_ptr(),
        p.data_ptr(), n.data_ptr(), err.data_ptr(), n_threads)
    return rc, u.numpy(), p.numpy(), n.numpy(), int(err.item())


# ------------------------------------------- per-pair quantities, float64 / 32
def occurrence_keys(users, pos, neg, n_users):
    """The (2 + K) B node keys in occurrence order: users, positives, then
    the negatives row-major."""
    return np.concatenate([users, n_users + pos, n_users + neg.reshape(-1)]).astype(np.int64)


def reference(out, emb, users, pos, neg, n_users, decay, temp, grad_scale, n_layers):
    """float64 autograd with out and emb as independent leaves.  Returns the
    per-pair terms / reg / coef [B, K] / coef_pos / g_u, the loss, the seed
    tables gp (= d loss / d out * grad_scale / (L+1)) and ge (= d loss /
    d emb * grad_scale) over all nodes, the seed_p normaliser S per node, the
    g_u normaliser Su per pair and A = (|<u,p>| + max_k |<u,n_k>|) / temp,
    the sums of absolute products behind a pair's scalars."""
    o = torch.tensor(np.asarray(out, np.float64), requires_grad=True)
    e = torch.tensor(np.asarray(emb, np.float64), requires_grad=True)
    u = torch.as_tensor(np.array(users)).long()
    p = torch.as_tensor(np.array(pos)).long() + n_users
    n = torch.as_tensor(np.array(neg)).long() + n_users
    B, K = n.shape
    sp = (o[u] * o[p]).sum(1) / temp
    sn = torch.einsum("bd,bkd->bk", o[u], o[n]) / temp
    sp.retain_grad()
    sn.retain_grad()
    terms = torch.logsumexp(torch.cat([sp[:, None], sn], 1), 1) - sp
    reg = 0.5 * ((e[u] ** 2).sum(1) + (e[p] ** 2).sum(1) + (e[n] ** 2).sum((1, 2)))
    loss = terms.mean() + decay * reg.sum() / B
    loss.backward()
    coef = sn.grad.numpy() * grad_scale / temp          # = grad_scale w / (B temp)
    cpos = coef.sum(1)
    od = o.detach().numpy()
    un, pn, nn_ = u.numpy(), p.numpy(), n.numpy()
    g_u = np.einsum("bk,bkd->bd", coef, od[nn_]) - cpos[:, None] * od[pn]
    Su = (np.einsum("bk,bkd->bd", np.abs(coef), np.abs(od[nn_]))
          + np.abs(cpos)[:, None] * np.abs(od[pn]))
    S = np.zeros_like(od)
    np.add.at(S, un, Su)
    np.add.at(S, pn, np.abs(cpos)[:, None] * np.abs(od[un]))
    np.add.at(S, nn_.reshape(-1), (np.abs(coef)[:, :, None] * np.abs(od[un])[:, None, :])
              .reshape(B * K, -1))
    A = (np.abs(od[un] * od[pn]).sum(1)
         + np.abs(od[un][:, None, :] * od[nn_]).sum(2).max(1)) / temp
    return dict(terms=terms.detach().numpy(), reg=reg.detach().numpy(), coef=coef, coef_pos=cpos,
                g_u=g_u, loss=float(loss.detach()), x=(sn - sp[:, None]).detach().numpy(),
                gp=o.grad.numpy() * grad_scale / (n_layers + 1), ge=e.grad.numpy() * grad_scale,
                S=S.max(1) / (n_layers + 1), Su=Su.max(1), A=A)


def forward_f32(out, emb, users, pos, neg, n_users, decay, temp, grad_scale):
    """The same per-pair quantities and the loss in float32 with plain numpy
    and the same max-subtracted algorithm (the measure of what float32 can
    give, not the kernel)."""
    u, p, n = np.asarray(users), np.asarray(pos) + n_users, np.asarray(neg) + n_users
    B, K = n.shape
    fb, ft = F32(B), F32(temp)
    ou, op, on = out[u], out[p], out[n]
    ps = (ou * op).sum(1, dtype=F32) / ft
    s = (ou[:, None, :] * on).sum(2, dtype=F32) / ft
    m = np.maximum(ps, s.max(1))
    with np.errstate(over="ignore", under="ignore"):
        e_pos = np.exp(ps - m)
        e = np.exp(s - m[:, None])
        s_neg = np.zeros(B, F32)
        acc = np.zeros(ou.shape, F32)
        for k in range(K):
            s_neg = s_neg + e[:, k]
            acc = acc + e[:, k, None] * on[:, k]
        z = e_pos + s_neg
        terms = np.where(m == ps, np.log1p(s_neg), (m - ps) + np.log(z)).astype(F32)
    scale = F32(grad_scale) * (F32(1) / (z * fb * ft))
    coef = scale[:, None] * e
    cpos = scale * s_neg
    g_u = scale[:, None] * acc - cpos[:, None] * op
    eu, ep, en = emb[u], emb[p], emb[n]
    reg = F32(0.5) * ((eu * eu).sum(1, dtype=F32) + (ep * ep).sum(1, dtype=F32)
                      + (en * en).sum((1, 2), dtype=F32))
    loss = terms.sum(dtype=F32) / fb + F32(decay) * (reg.sum(dtype=F32) / fb)
    for a in (terms, coef, cpos, g_u, reg):
        assert a.dtype == F32
    assert loss.dtype == F32
    return dict(terms=terms, coef=coef, coef_pos=cpos, g_u=g_u, reg=reg, loss=loss)


def seeds_f32(out, emb, users, f32, keys, n_neg, decay, grad_scale, n_layers):
    """seed_p / seed_e of every head in float32: each run accumulated one
    entry at a time, in stable sorted order, from forward_f32's coefficients.
    Returns {head q: (row_p, row_e)}."""
    B, K = len(users), n_neg
    n = (2 + K) * B
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    re1 = F32(F32(decay) / F32(B) * F32(grad_scale))
    div = F32(n_layers + 1)
    coef = f32["coef"].reshape(-1)
    res, q = {}, 0
    while q < n:
        node, gp, ge = ks[q], np.zeros(out.shape[1], F32), np.zeros(out.shape[1], F32)
        q2 = q
        while q2 < n and ks[q2] == node:
            occ = int(order[q2])
            if occ < B:
                gp = gp + f32["g_u"][occ]
            elif occ < 2 * B:
                gp = gp - f32["coef_pos"][occ - B] * out[users[occ - B]]
            else:
                j = occ - 2 * B
                gp = gp + coef[j] * out[users[j // K]]
            ge = ge + re1 * emb[node]
            q2 += 1
        assert gp.dtype == F32 and ge.dtype == F32
        res[q] = (gp / div, ge)
        q = q2
    return res


# ------------------------------------------------- the dense training step
NU, MI = 300, 40
N = NU + MI


def interactions():
    """tests/test_edge_dropout.py's kind of graph: 300 users, 40 items, about
    3 000 interactions: item 0 is a hub (every user once, some twice: beyond
    narrow_max), 200 users have degree <= 8, item 39 is isolated, 80
    interactions appear twice."""
    rng = np.random.default_rng(21)
    us, its = [np.arange(NU)], [np.zeros(NU, np.int64)]
    for u in range(NU):
        k = int(rng.integers(0, 7)) if u < 200 else int(rng.integers(12, 30))
        us.append(np.full(k, u))
        its.append(rng.integers(1, MI - 1, k))
    u, i = np.concatenate(us), np.concatenate(its)
    dup = rng.choice(len(u), 80, replace=False)
    u, i = np.concatenate([u, u[dup]]), np.concatenate([i, i[dup]])
    order = rng.permutation(len(u))
    return u[order].astype(np.int64), i[order].astype(np.int64)


class DS:
    def __init__(self):
        self.trainUser, self.trainItem = interactions()
        self.n_users, self.m_items = NU, MI
        self.trainDataSize = len(self.trainUser)
        self.testDict = {}


class Ref:
    """The float64 side of tests/test_ssm.py, shared by every test and never
    modified: dense propagation matrices (plain, edge-weighted, r-adjusted,
    edge-dropped), fixed batches and the training step in torch autograd +
    torch.optim.Adam."""

    KMAX = 8

    def __init__(self):
        from furusato_recommend_amd.graph import Graph
        self.ds = DS()
        g = Graph.from_interactions(self.ds.trainUser, self.ds.trainItem, NU, MI, "cpu")
        self.rowptr, self.col = g.rowptr_host.copy(), g.col_host.copy()
        self.deg = np.diff(self.rowptr).astype(np.float64)
        self.rows = np.repeat(np.arange(N), np.diff(self.rowptr))
        self._dense = {}
        rng = np.random.default_rng(23)
        # two batches of 64 pairs and a short third one (150 pairs in all)
        self.batches = []
        for b in (64, 64, 22):
            u, p = rng.integers(0, NU, b), rng.integers(0, MI, b)
            n = rng.integers(0, MI, (b, self.KMAX))
            n[0, 1] = n[0, 0]            # a negative repeated within its pair
            n[1, 0] = p[1]               # a negative equal to the positive
            self.batches.append((u, p, n))
        self.weight = (0.25 + rng.random(len(self.ds.trainUser)) * 2).astype(np.float32)

    def batch(self, t, k):
        u, p, n = self.batches[t]
        return u, p, n[:, :k].copy()

    def dense(self, weight=None, r=0.5, drop=None):
        """M with M[i, j] the weight of entry (j -> i): counts (or summed edge
        weights) over deg_j^r deg_i^(1-r), deg the (weighted) row sums; or
        (``drop`` = (seed, keep_prob)) the kept entries of the r = 0.5 matrix
        over keep_prob, with the degrees of the full graph."""
        key = (None if weight is None else "w", r, drop)
        if key in self._dense:
            return self._dense[key]
        a = np.zeros((N, N))
        if drop is not None:
            from furusato_recommend_amd._lib import lib
            k = np.empty(len(self.col), np.uint8)
            assert lib.mirec_edge_keep_mask(self.rowptr.ctypes.data, self.col.ctypes.data, N,
                                            drop[0], drop[1], 0, k.ctypes.data) == 0
            np.add.at(a, (self.rows, self.col), k / float(np.float32(drop[1])))
            deg = self.deg
        else:
            w = np.ones(len(self.ds.trainUser)) if weight is None else weight.astype(np.float64)
            u, i = self.ds.trainUser, self.ds.trainItem + NU
            np.add.at(a, (u, i), w)
            np.add.at(a, (i, u), w)
            deg = a.sum(1)
        safe = np.where(deg > 0, deg, 1.0)
        left = np.where(deg > 0, safe ** -(1.0 - r), 0.0)
        right = np.where(deg > 0, safe ** -r, 0.0)
        self._dense[key] = left[:, None] * a * right[None, :]
        return self._dense[key]

    def emb(self, d, seed=0):
        return 0.1 * torch.randn(N, d, generator=torch.Generator().manual_seed(100 + d + seed))

    @staticmethod
    def out(E, L, M):
        x, acc = E, E
        for _ in range(L):
            x = M @ x
            acc = acc + x
        return acc / (L + 1)

    @classmethod
    def ssm_loss(cls, E, L, M, batch, decay, temp):
        out = cls.out(E, L, M)
        u, p, n = (torch.from_numpy(np.asarray(a)).long() for a in batch)
        p, n = p + NU, n + NU
        sp = (out[u] * out[p]).sum(1) / temp
        sn = torch.einsum("bd,bkd->bk", out[u], out[n]) / temp
        terms = torch.logsumexp(torch.cat([sp[:, None], sn], 1), 1) - sp
        reg = 0.5 * (E[u].pow(2).sum() + E[p].pow(2).sum() + E[n].pow(2).sum()) / len(u)
        return terms.mean() + decay * reg

    @classmethod
    def bpr_loss(cls, E, L, M, batch, decay):
        out = cls.out(E, L, M)
        u, p, n = (torch.from_numpy(np.asarray(a)).long() for a in batch)
        p, n = p + NU, n.reshape(-1) + NU
        z = (out[u] * out[n]).sum(1) - (out[u] * out[p]).sum(1)
        reg = 0.5 * (E[u].pow(2).sum() + E[p].pow(2).sum() + E[n].pow(2).sum()) / len(u)
        return torch.nn.functional.softplus(z).mean() + decay * reg

    def steps(self, E0, L, mats, batches, lr, decay, temp):
        """Step t on matrix mats[t] with batches[t]; returns (tables, losses)."""
        E = E0.double().clone().requires_grad_(True)
        opt = torch.optim.Adam([E], lr=lr)
        tabs, losses = [], []
        for M, b in zip(mats, batches):
            opt.zero_grad()
            loss = self.ssm_loss(E, L, torch.from_numpy(M), b, decay, temp)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            tabs.append(E.detach().clone())
        return tabs, losses
