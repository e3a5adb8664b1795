"""Float64 restatement of the LightSAGE hop (model/lightsage.py:274-290: no
weights, no ReLU), the whole tree forward, the dense full-graph form, the
closed-form backward, the rounding bounds the GPU tests hold
csrc/lightsage.hip to, and the case lists of tests/test_lightsage_kernels.py.
numpy / torch on the host only; nothing from the package.

The arithmetic, for target t with the k child slots t*k .. t*k + k - 1 (a slot
is valid iff its flag / id is >= 0; a repeated id is two slots):

    out[t] = self[t] + (1 / cnt_t) sum over valid c of keep * scale * child[t*k + c]
    cnt_t  = number of valid slots; the mean is 0 when cnt_t = 0

keep / scale are the counter-hash dropout of tests/dropout_common.py at element
index (t*k + c)*dim + col.  Two forms of the hop:
  * ``hop_loop``: a per-target Python loop (numpy);
  * ``hop_edges``: the reference's own order (:281-286) — gather the source
    rows along gat_common.tree_edges, mask them, scatter-mean onto the target
    rows, add the target rows (torch, differentiable).
``tree_forward`` is the whole tree in the second form with the model's seeds:
layer i, target group g draws seed dropout_seed * 1_000_003 + g * 131 + i,
except layer 0, which is ONE launch over its concatenated targets with the
seed of (g, i) = (0, 0).  ``dense_full`` is the recurrence on the full graph,
x(l+1) = x(l) + mean over every CSR entry, out = sum_l x(l) / (L + 1).

The bounds are derived with dropout_common's rule, not measured (u = 2^-24,
gamma(n) = n u / (1 - n u)).  An output is a base (the self row) plus cnt
terms of three factors (1 / cnt, the row element, scale), so
    |got - ref| <= gamma(cnt + 5) * (|self| + sum |term|)
(dropout_common: gamma(m + 4) * A for m terms onto a base; the add of the base
after the division is one more rounding).  A kept element of the backward is
one term of three factors: gamma(4) * |term|; grad_self is a copy and is
compared bitwise.  References use the float32 ``scale`` widened to float64.
"""
import numpy as np
import torch

from tests import dropout_common as dc
from tests import gat_common as gc

M64 = dc.M64


def seed_of(dropout_seed, g, i):
    """The model's seed of layer i, target group g (GraphSAGE's seed_of)."""
    return (int(dropout_seed) * 1_000_003 + g * 131 + i) & M64


# --------------------------------------------------------------------- the hop
def hop_loop(x_self, x_child, valid, k, mask, scale):
    """Per-target loop in numpy float64.  mask [n_t*k, dim] bool.  Returns
    (out, A, cnt): [n_t, dim] twice (A = |self| + sum |term|) and [n_t]."""
    x_self, x_child = np.asarray(x_self, np.float64), np.asarray(x_child, np.float64)
    n_t, dim = x_self.shape
    ok = gc.valid_mask(valid, n_t, k)
    out, A, cnt = x_self.copy(), np.abs(x_self), np.zeros(n_t, np.int64)
    for t in range(n_t):
        slots = [t * k + c for c in range(k) if ok[t, c]]
        cnt[t] = len(slots)
        for e in slots:
            term = np.where(mask[e], float(scale) * x_child[e], 0.0) / len(slots)
            out[t] += term
            A[t] += np.abs(term)
    return out, A, cnt


def scatter_mean(src_rows, dst, n_rows):
    """Mean of the rows per destination (0 without an edge), torch float64."""
    s = torch.zeros(n_rows, src_rows.shape[1], dtype=src_rows.dtype).index_add(0, dst, src_rows)
    cnt = torch.zeros(n_rows, dtype=src_rows.dtype).index_add(
        0, dst, torch.ones_like(dst, dtype=src_rows.dtype))
    return s / cnt.clamp(min=1.0)[:, None]


def hop_edges(x_self, x_child, valid, k, mask=None, scale=1.0):
    """The reference's order on rows x = [children ; targets] (torch float64,
    differentiable in both row tensors): source rows along the edge list,
    masked, scatter-mean, plus the target rows."""
    n_t = x_self.shape[0]
    x = torch.cat([x_child, x_self])
    ei = gc.tree_edges(valid, n_t, k)
    src = x[ei[0]]
    if mask is not None:
        m = torch.from_numpy(np.ascontiguousarray(mask)).to(x.dtype) * float(scale)
        src = src * m[ei[0]]
    aggr = scatter_mean(src, ei[1], x.shape[0])
    return (x + aggr)[n_t * k:]


def backward_closed(g, valid, k, mask, scale):
    """(grad_self, grad_child) in float64: grad_self = g; grad_child[t*k + c] =
    keep * scale * g[t] / cnt_t, a zero row for an invalid slot."""
    g = np.asarray(g, np.float64)
    n_t, dim = g.shape
    ok = gc.valid_mask(valid, n_t, k)
    cnt = np.maximum(ok.sum(1), 1)
    per = (g / cnt[:, None])[:, None, :] * float(scale)
    live = ok[:, :, None] & np.asarray(mask, bool).reshape(n_t, k, dim)
    return g.copy(), np.where(live, per, 0.0).reshape(n_t * k, dim)


def fwd_bound(A, cnt):
    return dc.gamma(np.asarray(cnt, np.float64) + 5.0)[:, None] * A


def bwd_bound(ref):
    return dc.gamma(4) * np.abs(ref)


# -------------------------------------------------------------------- the tree
def _rows(table, ids):
    ids = torch.as_tensor(np.asarray(ids)).long()
    return table[ids.clamp(min=0)] * (ids >= 0).to(table.dtype)[:, None]


def tree_forward(table, groups, depths, children, L, sizes, p=0.0, dropout_seed=0):
    """Seed embeddings of a SampleTree given as (ids per group, depth per
    group, children dict) in torch float64, differentiable in ``table``."""
    d = table.shape[1]
    h = [_rows(table, g) for g in groups]
    out = h[0]
    for i in range(L):
        hop = L - i
        k = sizes[hop - 1]
        tg = [gi for gi, dep in enumerate(depths) if dep <= hop - 1]
        new = list(h)
        if i == 0:
            # one launch: t runs over the concatenated targets
            n_all = sum(len(groups[gi]) for gi in tg)
            mask, scale = (dc.fanout_mask(p, seed_of(dropout_seed, 0, 0), n_all * k, d)
                           if p > 0 else (None, 1.0))
            row = 0
        for gi in tg:
            ci = children[(gi, hop)]
            n_t = len(groups[gi])
            if p == 0:
                m, sc = None, 1.0
            elif i == 0:
                m, sc = mask[row * k:(row + n_t) * k], scale
                row += n_t
            else:
                m, sc = dc.fanout_mask(p, seed_of(dropout_seed, gi, i), n_t * k, d)
            new[gi] = hop_edges(h[gi], h[ci], np.asarray(groups[ci]), k, m, sc)
        h = new
        out = out + h[0]
    return out / (L + 1)


def dense_full(x, rowptr, col, L):
    """out = sum_l x(l) / (L + 1), x(l+1) = x(l) + mean over every CSR entry
    col[rowptr[r] : rowptr[r + 1]] of x(l) (each entry once; 0 for an empty
    row).  torch float64."""
    dst = torch.from_numpy(np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)))
    src = torch.from_numpy(np.asarray(col, np.int64))
    out = x
    for _ in range(L):
        x = x + scatter_mean(x[src], dst, x.shape[0])
        out = out + x
    return out / (L + 1)


# ------------------------------------------------------------------- the cases
def kernel_cases():
    """dropout_common.fanout_cases (with ``fanout_ids`` as the child ids) and
    one more whose target 2 — every slot valid — has a -1 self row."""
    cases = [dict(c, neg_self=(0,)) for c in dc.fanout_cases()]
    cases.append(dict(n_t=37, k=5, dim=64, p=0.3, seed=dc.SEEDS[1], n_rows=1000, neg_self=(0, 2)))
    return cases


def self_ids(case):
    """Self ids [n_t] int32: random rows, -1 for the targets of ``neg_self``."""
    rng = np.random.default_rng([case["n_t"], case["k"], case["dim"], case["n_rows"], 29])
    ids = rng.integers(0, case["n_rows"], case["n_t"]).astype(np.int32)
    for t in case["neg_self"]:
        ids[t] = -1
    return ids
