"""Float64 restatement of the graph-attention hop (PyG ``GATConv`` semantics:
concat=True, add_self_loops=True, negative_slope 0.2, no attention dropout;
the arithmetic is restated from PyG's documentation, torch_geometric is not
used), the rounding bounds the GPU tests hold csrc/gat.hip to, and the case
lists of tests/test_gat_kernels.py.  numpy / torch on the host only; nothing
from the package.

Two independent forms of the forward:
  * ``tree_loop``: a per-target Python loop over the tree layout (child rows
    t*k .. t*k + k - 1, a validity flag per slot, the self slot last);
  * ``edge_softmax``: PyG's edge-list form — logits per edge, a scatter
    softmax over the destination, a scatter sum — with the self loops
    appended, in torch float64 (differentiable: the autograd yardstick of the
    closed-form backward and of the model tests).
``tree_edges`` turns a tree level into that edge list, ``tree_layers`` a whole
SampleTree into the per-layer lists; ``dense_full`` is the full-graph form
the CSR kernel is held to (every CSR entry once, multi-edges included).

The bounds.  u = 2^-24, gamma(n) = n u / (1 - n u).  References are float64
on the float32-rounded inputs.
  logit      s_j is a C-term dot plus a C-term dot, one add and the leaky
             multiply: |ds_j| <= gamma(C + 3) * sum |z a| =: delta_j, doubled
             (a logit whose sign differs between the two precisions moves
             e_j by at most 0.8 |s_j| <= 0.8 delta_j more).
  exp        EXP_ULP = 2^-22 relative for one hardware exp2 (v_exp_f32: 1 ulp
             = 2^-23, doubled), the one explicit constant; its argument (e_j -
             max) * log2(e) carries three roundings, 3 u |x_j| absolute.  A
             weight passes through its own exp2 and at most NB = ceil(k / 8)
             rescales (one exp2 and one multiply each), the arguments summing
             to x_j: rel_w_j = 3 u |x_j| + (NB + 1) (EXP_ULP + u).
  softmax    alpha_j's relative error: expm1(2 max delta) from the logits
             (first order: d alpha_j = alpha_j (d e_j - sum alpha_m d e_m)),
             rel_w_j, the denominator's sum alpha_m rel_w_m + gamma(k + NB +
             4); weights below 2^-126 flush to 0: + 2^-120 absolute.
  out        sum_j |d alpha_j| |z_j| + gamma(k + NB + 5) * A, A = sum_j
             alpha_j |z_j| (+ |bias|): the gamma(m) * A forward error of the
             weighted sum in any order.
The backward's bounds follow the same way from its formulas (``bwd_bounds``:
every stage's error is carried into the next one's absolute terms, each
stage taken as one float32 rounding per operation — the kernel keeps the
per-head scalars in double, which only lowers its error; a logit within
delta_j of 0 may take either slope; TINY = 2^-100 absolute for products that
leave the normal float32 range).  Every bound is then capped at CAP * max
|reference| of its tensor (1e-4, the project's fp32 bar; never below TINY).
The backward takes alpha as an input: its reference is the closed form on the
float32-rounded alpha, so it is a test of the backward alone.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
EXP_ULP = 2.0 ** -22
CAP = 1e-4
TINY = 2.0 ** -100
SLOPE = 0.2
BATCH = 8           # children per rescale of the kernels' online softmax
MAX_BLOCKS = 1024   # partial-sum blocks of the backward (csrc/gat.hip)

# (n_t, k, H, C)
CASES = [(1, 1, 1, 4), (3, 5, 4, 4), (33, 10, 4, 16), (65, 25, 4, 32), (7, 64, 8, 32),
         (257, 3, 4, 8)]
# more targets than MAX_BLOCKS blocks take in one round: the backward's
# grid-stride loop runs twice for the first blocks
STRIDE_CASE = (4101, 2, 8, 32)
VALID_MODES = ("null", "all", "none", "some")
SCALES = (1.0, 30.0)   # variance of the inputs and attention vectors


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def lanes(H, C):
    """(float4 columns of a row, lanes per target, targets per 256-thread
    block) of the kernels' layout."""
    d4 = H * C // 4
    lpt = 1
    while lpt < d4:
        lpt *= 2
    return d4, lpt, 256 // lpt


def bwd_blocks(n_t, H, C):
    per = lanes(H, C)[2]
    return min(-(-n_t // per), MAX_BLOCKS)


# ------------------------------------------------------------------- inputs
def make_inputs(case, mode, scale, seed=0):
    """float32 inputs of a case: dict(zc [n_t*k, D], zs [n_t, D], valid (int32
    [n_t*k] or None), a_src, a_dst [D], bias [D], g [n_t, D])."""
    n_t, k, H, C = case
    D = H * C
    rng = np.random.default_rng([n_t, k, H, C, VALID_MODES.index(mode), int(scale), seed])
    sd = np.sqrt(scale)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    d = dict(zc=f32(rng.standard_normal((n_t * k, D)) * sd),
             zs=f32(rng.standard_normal((n_t, D)) * sd),
             a_src=f32(rng.standard_normal(D) * sd), a_dst=f32(rng.standard_normal(D) * sd),
             bias=f32(rng.standard_normal(D)),
             g=f32(rng.uniform(0.5, 1.5, (n_t, D)) * rng.choice([-1.0, 1.0], (n_t, D))))
    if mode == "null":
        d["valid"] = None
    elif mode == "all":
        d["valid"] = rng.integers(0, 1000, n_t * k).astype(np.int32)
    elif mode == "none":
        d["valid"] = np.full(n_t * k, -1, np.int32)
    else:  # about 30 % invalid; the last target without a valid child
        v = rng.integers(0, 1000, (n_t, k)).astype(np.int32)
        v[rng.random((n_t, k)) < 0.3] = -1
        v[-1] = -1
        d["valid"] = v.reshape(-1)
    return d


def valid_mask(valid, n_t, k):
    if valid is None:
        return np.ones((n_t, k), bool)
    return (np.asarray(valid) >= 0).reshape(n_t, k)


# ---------------------------------------------------- form 1: per-target loop
def tree_loop(zc, zs, valid, a_src, a_dst, bias, k, H, slope=SLOPE):
    """(out [n_t, D], alpha [n_t, k + 1, H], s [n_t, k + 1, H]) in float64;
    alpha and s are 0 in the invalid slots, slot k is the self slot."""
    zc, zs = np.asarray(zc, np.float64), np.asarray(zs, np.float64)
    a_src, a_dst = np.asarray(a_src, np.float64), np.asarray(a_dst, np.float64)
    n_t, D = zs.shape
    C = D // H
    ok = valid_mask(valid, n_t, k)
    out = np.zeros((n_t, D))
    alpha = np.zeros((n_t, k + 1, H))
    s_all = np.zeros((n_t, k + 1, H))
    for t in range(n_t):
        slots = [c for c in range(k) if ok[t, c]] + [k]
        rows = [zc[t * k + c] if c < k else zs[t] for c in slots]
        for h in range(H):
            cs = slice(h * C, (h + 1) * C)
            dst = float(zs[t, cs] @ a_dst[cs])
            s = np.array([float(r[cs] @ a_src[cs]) + dst for r in rows])
            e = np.where(s > 0, s, slope * s)
            p = np.exp(e - e.max())
            a = p / p.sum()
            for j, c in enumerate(slots):
                alpha[t, c, h] = a[j]
                s_all[t, c, h] = s[j]
                out[t, cs] += a[j] * rows[j][cs]
    if bias is not None:
        out = out + np.asarray(bias, np.float64)
    return out, alpha, s_all


# ------------------------------------------------ form 2: edge-list (PyG style)
def edge_softmax(z, edge_index, a_src, a_dst, bias, H, slope=SLOPE):
    """GATConv's message passing on projected rows z [N, D] (torch float64):
    edge_index [2, E] = (source, destination) rows, a self loop appended for
    every node.  Returns (out [N, D], alpha [E + N, H], s [E + N, H])."""
    N, D = z.shape
    C = D // H
    loops = torch.arange(N, dtype=torch.long)
    src = torch.cat([edge_index[0].long(), loops])
    dst = torch.cat([edge_index[1].long(), loops])
    zh = z.view(N, H, C)
    l_src = (zh * a_src.reshape(1, H, C)).sum(-1)
    l_dst = (zh * a_dst.reshape(1, H, C)).sum(-1)
    s = l_src[src] + l_dst[dst]
    e = F.leaky_relu(s, slope)
    idx = dst[:, None].expand(-1, H)
    mx = torch.full((N, H), -float("inf"), dtype=z.dtype).scatter_reduce(
        0, idx, e.detach(), "amax", include_self=True)
    p = torch.exp(e - mx[dst])
    den = torch.zeros(N, H, dtype=z.dtype).index_add(0, dst, p)
    alpha = p / den[dst]
    out = torch.zeros(N, H, C, dtype=z.dtype).index_add(0, dst, alpha[..., None] * zh[src])
    out = out.reshape(N, D)
    if bias is not None:
        out = out + bias
    return out, alpha, s


def tree_edges(valid, n_t, k):
    """Edge list of one tree level over the rows [children ; targets]: child
    row t*k + c -> target row n_t*k + t for every valid slot (a repeated id
    is two slots, hence two edges)."""
    ok = valid_mask(valid, n_t, k)
    t, c = np.nonzero(ok)
    return torch.from_numpy(np.stack([t * k + c, n_t * k + t]).astype(np.int64))


def tree_level(zc, zs, valid, a_src, a_dst, bias, k, H, slope=SLOPE):
    """The hop of one level through the edge-list form: out [n_t, D] (torch
    float64, differentiable in every tensor argument)."""
    n_t = zs.shape[0]
    out, _, _ = edge_softmax(torch.cat([zc, zs]), tree_edges(valid, n_t, k), a_src, a_dst, bias,
                             H, slope)
    return out[n_t * k:]


def tree_layers(groups, depths, children, L, sizes):
    """[(target group, child group, k, edge list)] per layer i of a
    SampleTree given as (ids per group, depth per group, children dict)."""
    layers = []
    for i in range(L):
        hop = L - i
        lay = []
        for gi, dep in enumerate(depths):
            if dep > hop - 1:
                continue
            ci = children[(gi, hop)]
            k = sizes[hop - 1]
            lay.append((gi, ci, k, tree_edges(np.asarray(groups[ci]), len(groups[gi]), k)))
        layers.append(lay)
    return layers


def model_forward(table, convs, groups, depths, children, L, sizes, H, slope=SLOPE):
    """The 'gnn' forward without dropout in torch float64: table [N, d],
    convs = [(W [d, d], a_src [d], a_dst [d], bias [d])] per layer.  Rows of
    ids < 0 are zero rows.  Returns the seed rows h^(L)."""
    h = []
    for g in groups:
        g = torch.as_tensor(np.asarray(g)).long()
        rows = table[g.clamp(min=0)] * (g >= 0).to(table.dtype)[:, None]
        h.append(rows)
    for i, lay in enumerate(tree_layers(groups, depths, children, L, sizes)):
        W, a_s, a_d, b = convs[i]
        new = list(h)
        for gi, ci, k, ei in lay:
            n_t = h[gi].shape[0]
            z = torch.cat([h[ci] @ W.t(), h[gi] @ W.t()])
            out = edge_softmax(z, ei, a_s, a_d, b, H, slope)[0][n_t * k:]
            new[gi] = out.relu() if i != L - 1 else out
        h = new
    return h[0]


def dense_full(z, rowptr, col, a_src, a_dst, bias, H, slope=SLOPE):
    """Full-graph layer in float64: row r attends over every CSR entry
    col[rowptr[r] : rowptr[r + 1]] (each entry once) and itself.  Returns
    (out, bound): the forward bound of ``fwd_bounds`` per row."""
    z = np.asarray(z, np.float64)
    n = len(rowptr) - 1
    out, bound = np.zeros_like(z), np.zeros_like(z)
    for r in range(n):
        nb = np.asarray(col[rowptr[r]:rowptr[r + 1]], np.int64)
        k = max(len(nb), 1)
        zc = np.zeros((k, z.shape[1]))
        zc[:len(nb)] = z[nb]
        valid = np.where(np.arange(k) < len(nb), 0, -1).astype(np.int32)
        o, al, s = tree_loop(zc, z[r:r + 1], valid, a_src, a_dst, bias, k, H, slope)
        out[r] = o[0]
        bound[r] = fwd_bounds(zc, z[r:r + 1], valid, a_src, a_dst, bias, k, H, al, s, o,
                              slope, cap=False)[0][0]
    return out, bound


# --------------------------------------------------------- closed-form backward
def _stack(zc, zs, k):
    n_t, D = zs.shape
    return np.concatenate([zc.reshape(n_t, k, D), zs[:, None, :]], axis=1)  # [n_t, k+1, D]


def backward_closed(g, zc, zs, valid, a_src, a_dst, alpha, s, k, H, slope=SLOPE):
    """The issue's closed form, float64: (grad_z_child, grad_z_self,
    grad_att_src, grad_att_dst) from alpha [n_t, k+1, H] (0 in invalid slots)
    and the logits s."""
    g, zc, zs = (np.asarray(x, np.float64) for x in (g, zc, zs))
    a_src, a_dst = np.asarray(a_src, np.float64), np.asarray(a_dst, np.float64)
    alpha = np.asarray(alpha, np.float64)
    n_t, D = zs.shape
    C = D // H
    za = _stack(zc, zs, k).reshape(n_t, k + 1, H, C)
    g4 = g.reshape(n_t, 1, H, C)
    da = (g4 * za).sum(-1)                                    # [n_t, k+1, H]
    S = (alpha * da).sum(1, keepdims=True)
    de = alpha * (da - S)
    ds = de * np.where(s > 0, 1.0, slope)
    gz = alpha[..., None] * g4 + ds[..., None] * a_src.reshape(1, 1, H, C)
    sum_ds = ds.sum(1)                                        # [n_t, H]
    gzs = gz[:, k] + sum_ds[..., None] * a_dst.reshape(1, H, C)
    g_src = (ds[..., None] * za).sum((0, 1)).reshape(D)
    g_dst = (sum_ds[..., None] * za[:, k]).sum(0).reshape(D)
    return gz[:, :k].reshape(n_t * k, D), gzs.reshape(n_t, D), g_src, g_dst


# ---------------------------------------------------------------------- bounds
def _cap(bound, ref, cap=True):
    if not cap:
        return bound
    return np.minimum(bound, max(CAP * float(np.abs(ref).max()), TINY) if ref.size else 0.0)


def _logit_delta(za, zs, a_src, a_dst, H, C):
    """delta [n_t, k+1, H]: the logit error bound (doubled, see above)."""
    n_t, k1 = za.shape[:2]
    absdot = np.abs(za * a_src.reshape(1, 1, H, C)).sum(-1) + \
        np.abs(zs.reshape(n_t, 1, H, C) * a_dst.reshape(1, 1, H, C)).sum(-1)
    return 2.0 * gamma(C + 3) * absdot


def fwd_bounds(zc, zs, valid, a_src, a_dst, bias, k, H, alpha, s, out, slope=SLOPE, cap=True):
    """(bound_out [n_t, D], bound_alpha [n_t, k+1, H]) for float64 references
    alpha, s, out of the same float32-rounded inputs."""
    zc, zs = np.asarray(zc, np.float64), np.asarray(zs, np.float64)
    a_src, a_dst = np.asarray(a_src, np.float64), np.asarray(a_dst, np.float64)
    n_t, D = zs.shape
    C = D // H
    nb = -(-k // BATCH)
    ok = np.concatenate([valid_mask(valid, n_t, k), np.ones((n_t, 1), bool)], 1)[..., None]
    za = _stack(zc, zs, k).reshape(n_t, k + 1, H, C)
    delta = np.where(ok, _logit_delta(za, zs, a_src, a_dst, H, C), 0.0)
    e = np.where(s > 0, s, slope * s)
    emax = np.where(ok, e, -np.inf).max(1, keepdims=True)
    x = np.where(ok, np.abs(e - emax), 0.0)
    rel_w = 3 * U * x + (nb + 1) * (EXP_ULP + U)
    rel_a = np.expm1(2 * delta.max(1, keepdims=True)) + rel_w + \
        (alpha * rel_w).sum(1, keepdims=True) + gamma(k + nb + 4)
    d_alpha = np.where(ok, alpha * rel_a + 2.0 ** -120, 0.0)
    A = (alpha[..., None] * np.abs(za)).sum(1).reshape(n_t, D)
    b = (d_alpha[..., None] * np.abs(za)).sum(1).reshape(n_t, D)
    if bias is not None:
        A = A + np.abs(np.asarray(bias, np.float64))
    b_out = b + gamma(k + nb + 5) * A
    return _cap(b_out, out, cap), _cap(d_alpha, alpha, cap)


def bwd_bounds(g, zc, zs, valid, a_src, a_dst, alpha, s, k, H, refs, slope=SLOPE):
    """Bounds of (grad_z_child, grad_z_self, grad_att_src, grad_att_dst)
    against backward_closed on the same inputs (alpha an input)."""
    g, zc, zs = (np.asarray(x, np.float64) for x in (g, zc, zs))
    a_src, a_dst = np.asarray(a_src, np.float64), np.asarray(a_dst, np.float64)
    alpha = np.asarray(alpha, np.float64)
    n_t, D = zs.shape
    C = D // H
    za = _stack(zc, zs, k).reshape(n_t, k + 1, H, C)
    g4 = g.reshape(n_t, 1, H, C)
    A_s, A_d = np.abs(a_src).reshape(1, 1, H, C), np.abs(a_dst).reshape(1, H, C)
    da = (g4 * za).sum(-1)
    E_da = gamma(C + 1) * np.abs(g4 * za).sum(-1)
    S = (alpha * da).sum(1, keepdims=True)
    E_S = (alpha * E_da).sum(1, keepdims=True) + gamma(k + 3) * (alpha * np.abs(da)).sum(
        1, keepdims=True)
    de = alpha * (da - S)
    E_de = alpha * (E_da + E_S) + 3 * U * alpha * (np.abs(da) + np.abs(S))
    ds = de * np.where(s > 0, 1.0, slope)
    flip = np.abs(s) <= _logit_delta(za, zs, a_src, a_dst, H, C)
    E_ds = E_de + U * np.abs(ds) + np.where(flip, (1.0 - slope) * np.abs(de), 0.0)
    t_a, t_s = np.abs(alpha[..., None] * g4), np.abs(ds)[..., None] * A_s
    ok = np.concatenate([valid_mask(valid, n_t, k), np.ones((n_t, 1), bool)], 1)
    E_gz = np.where(ok[..., None, None], E_ds[..., None] * A_s + gamma(3) * (t_a + t_s) + TINY, 0.0)
    sum_ds = ds.sum(1)
    E_sum = E_ds.sum(1) + gamma(k + 2) * np.abs(ds).sum(1)
    E_gzs = E_ds[:, k][..., None] * A_s[0] + E_sum[..., None] * A_d + \
        gamma(5) * (t_a[:, k] + t_s[:, k] + np.abs(sum_ds)[..., None] * A_d) + TINY
    E_src = (E_ds[..., None] * np.abs(za)).sum((0, 1)) + \
        gamma(n_t * (k + 1) + 8) * (np.abs(ds)[..., None] * np.abs(za)).sum((0, 1)) + TINY
    E_dst = (E_sum[..., None] * np.abs(za[:, k])).sum(0) + \
        gamma(n_t + 8) * (np.abs(sum_ds)[..., None] * np.abs(za[:, k])).sum(0) + TINY
    bounds = (E_gz[:, :k].reshape(n_t * k, D), E_gzs.reshape(n_t, D), E_src.reshape(D),
              E_dst.reshape(D))
    return tuple(_cap(b, r) for b, r in zip(bounds, refs))


# ------------------------------------------------------------- the CSR graphs
def csr_graph_edges():
    """(users, items, n_users, m_items) of the mirec_csr_gat test graph: 37 x
    11 bipartite with duplicate edges, item 10 isolated, user 36 of degree 1,
    item 0 a hub of degree >= 300 (every user of 0..35, nine times over)."""
    rng = np.random.default_rng(37)
    u = [np.repeat(np.arange(36), 9)]          # the hub: 324 entries
    i = [np.zeros(324, np.int64)]
    uu = rng.integers(0, 36, 90)
    ii = rng.integers(1, 10, 90)
    u += [uu, uu[:12], np.array([36])]         # 12 duplicates, the degree-1 user
    i += [ii, ii[:12], np.array([3])]
    return np.concatenate(u).astype(np.int64), np.concatenate(i).astype(np.int64), 37, 11


def small_graph_edges():
    """A second bipartite graph whose largest degree is below the fanout
    limit of 64, for the tree / CSR cross-check: 20 x 7, duplicates, item 6
    isolated."""
    rng = np.random.default_rng(20)
    u = rng.integers(0, 20, 70)
    i = rng.integers(0, 6, 70)
    return (np.concatenate([u, u[:8]]).astype(np.int64),
            np.concatenate([i, i[:8]]).astype(np.int64), 20, 7)


def host_csr(u, i, n_users, m_items):
    """(rowptr int64 [n + 1], col int32 [2 E]) of the symmetric bipartite
    graph, rows in edge order, multi-edges kept (numpy, no library)."""
    src = np.concatenate([i + n_users, u])
    dst = np.concatenate([u, i + n_users])
    order = np.argsort(dst, kind="stable")
    n = n_users + m_items
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(dst, minlength=n), out=rowptr[1:])
    return rowptr, src[order].astype(np.int32)
