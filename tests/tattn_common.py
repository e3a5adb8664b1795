"""Float64 restatement of the dot-product attention hop (PyG ``TransformerConv``
semantics: concat=True, beta=False, no edge features, no attention dropout,
root_weight=True; the arithmetic is restated from PyG's documentation,
torch_geometric is not used), the rounding bounds the GPU tests hold
csrc/tattn.hip to, and the case lists of tests/test_tattn_kernels.py.  numpy /
torch on the host only; nothing from the package.

The hop takes PROJECTED rows: q and skip per target, key and value per child
slot.  For target t and head h over the valid slots j (no self slot):
    s_j = <q_t,h, key_j,h> * scale,  alpha_j = softmax_j s_j,
    out_t,h = sum_j alpha_j value_j,h + skip_t,h
``scale`` is the float32 the kernel is given, float32(1 / sqrt(C)): an input.

Two independent forms of the forward:
  * ``tree_loop``: a per-target Python loop over the tree layout (child rows
    t*k .. t*k + k - 1, a validity flag per slot);
  * ``edge_attention``: PyG's edge-list form — a logit per edge from the
    destination's query and the source's key, a scatter softmax over the
    destination, a scatter sum of the sources' values, the skip row added —
    with NO self loops appended, in torch float64 (differentiable: the
    autograd yardstick of the closed-form backward and of the model tests).
``tree_edges`` turns a tree level into that edge list, ``tree_layers`` a whole
SampleTree into the per-layer lists; ``dense_full`` is the full-graph form
the CSR kernel is held to (every CSR entry once, multi-edges included).

The bounds.  u = 2^-24, gamma(n) = n u / (1 - n u).  References are float64
on the float32-rounded inputs.
  logit      s_j is a C-term dot (C products, C - 1 adds, in any order) and
             one multiply by scale: |ds_j| <= gamma(C + 1) * scale * sum |q k|
             =: delta_j.
  exp        EXP_ULP = 2^-22 relative for one hardware exp2 (v_exp_f32: 1 ulp
             = 2^-23, doubled), the one explicit constant; its argument (s_j -
             max) * log2(e) carries three roundings, 3 u |x_j| absolute.  A
             weight passes through its own exp2 and at most NB = ceil(k / 8)
             rescales (one exp2 and one multiply each), the arguments summing
             to x_j: rel_w_j = 3 u |x_j| + (NB + 1) (EXP_ULP + u).
  softmax    alpha_j's relative error: expm1(2 max delta) from the logits
             (first order: d alpha_j = alpha_j (d s_j - sum alpha_m d s_m)),
             rel_w_j, the denominator's sum alpha_m rel_w_m + gamma(k + NB +
             4); weights below 2^-126 flush to 0: + 2^-120 absolute.
  out        sum_j |d alpha_j| |v_j| + gamma(k + NB + 5) * A, A = sum_j
             alpha_j |v_j| + |skip|: the gamma(m) * A forward error of the
             weighted sum in any order (the skip add is one of the m).
The backward's bounds follow the same way from its formulas (``bwd_bounds``:
every stage's error is carried into the next one's absolute terms, each stage
taken as one float32 rounding per operation — the kernel keeps the per-head
scalars in double, which only lowers its error; TINY = 2^-100 absolute for
products that leave the normal float32 range):
  dalpha_j   a C-term dot: E_da = gamma(C + 1) sum |g v_j|
  S          sum alpha dalpha: E_S = sum alpha E_da + gamma(k + 3) sum alpha |da|
  ds_j       alpha_j (da_j - S) scale: scale (alpha_j (E_da_j + E_S) + 3 u
             alpha_j (|da_j| + |S|)) + 2 u |ds_j|
  grad_v_j   alpha_j g: u |alpha_j g|
  grad_k_j   ds_j q: E_ds_j |q| + u |ds_j q|
  grad_q     sum_j ds_j k_j: sum E_ds_j |k_j| + gamma(k + 2) sum |ds_j k_j|
grad_skip is grad_out bit for bit.  Every bound is then capped at CAP * max
|reference| of its tensor (1e-4, the project's fp32 bar; never below TINY).
The backward takes alpha as an input: its reference is the closed form on the
float32-rounded alpha, so it is a test of the backward alone.  Nothing
measured goes into a bound.
"""
import numpy as np
import torch

U = 2.0 ** -24
EXP_ULP = 2.0 ** -22
CAP = 1e-4
TINY = 2.0 ** -100
BATCH = 8           # children per rescale of the kernels' online softmax
OVERFLOW = 88.73    # exp(88.73) > float32 max: a logit above it needs the max subtraction

# (n_t, k, H, C)
CASES = [(1, 1, 1, 4), (3, 5, 8, 4), (33, 10, 8, 8), (65, 25, 8, 16), (7, 64, 8, 32),
         (257, 3, 4, 8), (5, 7, 2, 12), (9, 9, 5, 20)]
# input seed per case: at variance 60 the largest logit of every case but
# (1,1,1,4) must exceed OVERFLOW (tests/test_tattn_host.py); a case that falls
# short gets another seed here, the threshold stays
SEEDS = {(5, 7, 2, 12): 1}   # seed 0: the 'some' mode's largest logit is 67.2
VALID_MODES = ("null", "all", "none", "some")
SCALES = (1.0, 60.0)   # variance of the projected rows


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


def kernel_scale(C):
    """The logit scale the kernels are given: float32(1 / sqrt(C))."""
    return np.float32(1.0 / np.sqrt(C))


# ------------------------------------------------------------------- inputs
def make_inputs(case, mode, scale, seed=None):
    """float32 inputs of a case: dict(q, skip [n_t, D], key, val [n_t*k, D],
    valid (int32 [n_t*k] or None), g [n_t, D])."""
    n_t, k, H, C = case
    D = H * C
    seed = SEEDS.get(case, 0) if seed is None else seed
    rng = np.random.default_rng([n_t, k, H, C, VALID_MODES.index(mode), int(scale), seed])
    sd = np.sqrt(scale)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    d = dict(q=f32(rng.standard_normal((n_t, D)) * sd),
             skip=f32(rng.standard_normal((n_t, D)) * sd),
             key=f32(rng.standard_normal((n_t * k, D)) * sd),
             val=f32(rng.standard_normal((n_t * k, D)) * sd),
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
def tree_loop(q, skip, key, val, valid, k, H, scale=None):
    """(out [n_t, D], alpha [n_t, k, H], s [n_t, k, H]) in float64; alpha and
    s are 0 in the invalid slots.  skip may be None."""
    q, key, val = (np.asarray(x, np.float64) for x in (q, key, val))
    n_t, D = q.shape
    C = D // H
    scale = float(kernel_scale(C)) if scale is None else float(scale)
    ok = valid_mask(valid, n_t, k)
    out = np.zeros((n_t, D))
    alpha = np.zeros((n_t, k, H))
    s_all = np.zeros((n_t, k, H))
    for t in range(n_t):
        slots = [c for c in range(k) if ok[t, c]]
        if not slots:
            continue
        for h in range(H):
            cs = slice(h * C, (h + 1) * C)
            s = np.array([float(q[t, cs] @ key[t * k + c, cs]) * scale for c in slots])
            p = np.exp(s - s.max())
            a = p / p.sum()
            for j, c in enumerate(slots):
                alpha[t, c, h] = a[j]
                s_all[t, c, h] = s[j]
                out[t, cs] += a[j] * val[t * k + c, cs]
    if skip is not None:
        out = out + np.asarray(skip, np.float64)
    return out, alpha, s_all


# ------------------------------------------------ form 2: edge-list (PyG style)
def edge_attention(q, key, val, skip, edge_index, H, scale=None):
    """TransformerConv's message passing on projected rows [N, D] (torch
    float64): edge_index [2, E] = (source, destination) rows; no self loops.
    Returns (out [N, D], alpha [E, H]).  A node without an incoming edge gets
    its skip row."""
    N, D = q.shape
    C = D // H
    scale = float(kernel_scale(C)) if scale is None else float(scale)
    src, dst = edge_index[0].long(), edge_index[1].long()
    qh, kh, vh = q.view(N, H, C), key.view(N, H, C), val.view(N, H, C)
    s = (qh[dst] * kh[src]).sum(-1) * scale
    idx = dst[:, None].expand(-1, H)
    mx = torch.full((N, H), -float("inf"), dtype=q.dtype).scatter_reduce(
        0, idx, s.detach(), "amax", include_self=True)
    p = torch.exp(s - mx[dst])
    den = torch.zeros(N, H, dtype=q.dtype).index_add(0, dst, p)
    alpha = p / den[dst]
    out = torch.zeros(N, H, C, dtype=q.dtype).index_add(0, dst, alpha[..., None] * vh[src])
    out = out.reshape(N, D)
    if skip is not None:
        out = out + skip
    return out, alpha


def tree_edges(valid, n_t, k):
    """Edge list of one tree level over the rows [children ; targets]: child
    row t*k + c -> target row n_t*k + t for every valid slot (a repeated id
    is two slots, hence two edges)."""
    ok = valid_mask(valid, n_t, k)
    t, c = np.nonzero(ok)
    return torch.from_numpy(np.stack([t * k + c, n_t * k + t]).astype(np.int64))


def tree_level(q, skip, key, val, valid, k, H, scale=None):
    """The hop of one level through the edge-list form: out [n_t, D] (torch
    float64, differentiable in every tensor argument)."""
    n_t, D = q.shape
    zc, zt = torch.zeros(n_t * k, D, dtype=q.dtype), torch.zeros(n_t, D, dtype=q.dtype)
    out, _ = edge_attention(torch.cat([zc, q]), torch.cat([key, zt]), torch.cat([val, zt]),
                            torch.cat([zc, skip]), tree_edges(valid, n_t, k), H, scale)
    return out[n_t * k:]


def tree_layers(groups, depths, children, L, sizes):
    """[(target group, child group, k)] per layer i of a SampleTree given as
    (ids per group, depth per group, children dict)."""
    layers = []
    for i in range(L):
        hop = L - i
        layers.append([(gi, children[(gi, hop)], sizes[hop - 1])
                       for gi, dep in enumerate(depths) if dep <= hop - 1])
    return layers


def model_forward(table, convs, groups, depths, children, L, sizes, H, taps=None):
    """The 'tgrec' forward without dropout in torch float64: table [N, d],
    convs = [dict(lin_key=(W, b), lin_query=..., lin_value=..., lin_skip=...)]
    per layer.  Rows of ids < 0 are zero rows.  Returns the seed rows h^(L).
    ``taps`` (a list) receives (layer, projected key rows) of every launch:
    the gradient of lin_key.bias is the column sum of their gradients, a sum
    that is identically 0 (a shift of every key by one vector moves all
    logits of a target alike), so its scale is the sum of their absolute
    values."""
    h = []
    for g in groups:
        g = torch.as_tensor(np.asarray(g)).long()
        h.append(table[g.clamp(min=0)] * (g >= 0).to(table.dtype)[:, None])
    lin = lambda x, wb: x @ wb[0].t() + wb[1]  # noqa: E731
    for i, lay in enumerate(tree_layers(groups, depths, children, L, sizes)):
        c = convs[i]
        new = [None] * len(h)
        for gi, ci, k in lay:
            keys = lin(h[ci], c["lin_key"])
            if taps is not None:
                taps.append((i, keys))
            out = tree_level(lin(h[gi], c["lin_query"]), lin(h[gi], c["lin_skip"]), keys,
                             lin(h[ci], c["lin_value"]), np.asarray(groups[ci]), k, H)
            new[gi] = out.relu() if i != L - 1 else out
        h = new
    return h[0]


def dense_full(q, skip, key, val, rowptr, col, H):
    """Full-graph layer in float64: row r attends with q[r] over every CSR
    entry col[rowptr[r] : rowptr[r + 1]] (each entry once, no self loop).
    Returns (out, bound): the forward bound of ``fwd_bounds`` per row."""
    q, skip, key, val = (np.asarray(x, np.float64) for x in (q, skip, key, val))
    n = len(rowptr) - 1
    out, bound = np.zeros_like(q), np.zeros_like(q)
    for r in range(n):
        nb = np.asarray(col[rowptr[r]:rowptr[r + 1]], np.int64)
        k = max(len(nb), 1)
        kc, vc = np.zeros((k, q.shape[1])), np.zeros((k, q.shape[1]))
        kc[:len(nb)], vc[:len(nb)] = key[nb], val[nb]
        valid = np.where(np.arange(k) < len(nb), 0, -1).astype(np.int32)
        o, al, s = tree_loop(q[r:r + 1], skip[r:r + 1], kc, vc, valid, k, H)
        out[r] = o[0]
        bound[r] = fwd_bounds(q[r:r + 1], skip[r:r + 1], kc, vc, valid, k, H, al, s, o,
                              cap=False)[0][0]
    return out, bound


# --------------------------------------------------------- closed-form backward
def backward_closed(g, q, key, val, valid, alpha, k, H, scale=None):
    """The issue's closed form, float64: (grad_q [n_t, D], grad_key, grad_val
    [n_t*k, D]) from alpha [n_t, k, H] (0 in invalid slots); grad_skip = g."""
    g, q, key, val = (np.asarray(x, np.float64) for x in (g, q, key, val))
    alpha = np.asarray(alpha, np.float64)
    n_t, D = q.shape
    C = D // H
    scale = float(kernel_scale(C)) if scale is None else float(scale)
    k4, v4 = key.reshape(n_t, k, H, C), val.reshape(n_t, k, H, C)
    g4, q4 = g.reshape(n_t, 1, H, C), q.reshape(n_t, 1, H, C)
    da = (g4 * v4).sum(-1)                                    # [n_t, k, H]
    S = (alpha * da).sum(1, keepdims=True)
    ds = alpha * (da - S) * scale
    gv = alpha[..., None] * g4
    gk = ds[..., None] * q4
    gq = (ds[..., None] * k4).sum(1)
    return gq.reshape(n_t, D), gk.reshape(n_t * k, D), gv.reshape(n_t * k, D)


# ---------------------------------------------------------------------- bounds
def _cap(bound, ref, cap=True):
    if not cap:
        return bound
    return np.minimum(bound, max(CAP * float(np.abs(ref).max()), TINY) if ref.size else 0.0)


def fwd_bounds(q, skip, key, val, valid, k, H, alpha, s, out, scale=None, cap=True):
    """(bound_out [n_t, D], bound_alpha [n_t, k, H]) for float64 references
    alpha, s, out of the same float32-rounded inputs."""
    q, key, val = (np.asarray(x, np.float64) for x in (q, key, val))
    n_t, D = q.shape
    C = D // H
    scale = float(kernel_scale(C)) if scale is None else float(scale)
    nb = -(-k // BATCH)
    ok = valid_mask(valid, n_t, k)[..., None]
    k4, v4 = key.reshape(n_t, k, H, C), val.reshape(n_t, k, H, C)
    q4 = q.reshape(n_t, 1, H, C)
    delta = np.where(ok, gamma(C + 1) * scale * np.abs(q4 * k4).sum(-1), 0.0)
    smax = np.where(ok, s, -np.inf).max(1, keepdims=True)
    x = np.where(ok, np.abs(s - np.where(np.isfinite(smax), smax, 0.0)), 0.0)
    rel_w = 3 * U * x + (nb + 1) * (EXP_ULP + U)
    rel_a = np.expm1(2 * delta.max(1, keepdims=True)) + rel_w + \
        (alpha * rel_w).sum(1, keepdims=True) + gamma(k + nb + 4)
    d_alpha = np.where(ok, alpha * rel_a + 2.0 ** -120, 0.0)
    A = (alpha[..., None] * np.abs(v4)).sum(1).reshape(n_t, D)
    b = (d_alpha[..., None] * np.abs(v4)).sum(1).reshape(n_t, D)
    if skip is not None:
        A = A + np.abs(np.asarray(skip, np.float64))
    b_out = b + gamma(k + nb + 5) * A
    return _cap(b_out, out, cap), _cap(d_alpha, alpha, cap)


def bwd_bounds(g, q, key, val, valid, alpha, k, H, refs, scale=None):
    """Bounds of (grad_q, grad_key, grad_val) against backward_closed on the
    same inputs (alpha an input)."""
    g, q, key, val = (np.asarray(x, np.float64) for x in (g, q, key, val))
    alpha = np.asarray(alpha, np.float64)
    n_t, D = q.shape
    C = D // H
    scale = float(kernel_scale(C)) if scale is None else float(scale)
    ok = valid_mask(valid, n_t, k)[..., None, None]
    k4, v4 = key.reshape(n_t, k, H, C), val.reshape(n_t, k, H, C)
    g4, q4 = g.reshape(n_t, 1, H, C), q.reshape(n_t, 1, H, C)
    da = (g4 * v4).sum(-1)
    E_da = gamma(C + 1) * np.abs(g4 * v4).sum(-1)
    S = (alpha * da).sum(1, keepdims=True)
    E_S = (alpha * E_da).sum(1, keepdims=True) + \
        gamma(k + 3) * (alpha * np.abs(da)).sum(1, keepdims=True)
    ds = alpha * (da - S) * scale
    E_ds = scale * (alpha * (E_da + E_S) + 3 * U * alpha * (np.abs(da) + np.abs(S))) + \
        2 * U * np.abs(ds)
    E_gv = np.where(ok, U * np.abs(alpha[..., None] * g4) + TINY, 0.0)
    E_gk = np.where(ok, E_ds[..., None] * np.abs(q4) + U * np.abs(ds[..., None] * q4) + TINY, 0.0)
    E_gq = (E_ds[..., None] * np.abs(k4)).sum(1) + \
        gamma(k + 2) * np.abs(ds[..., None] * k4).sum(1) + TINY
    bounds = (E_gq.reshape(n_t, D), E_gk.reshape(n_t * k, D), E_gv.reshape(n_t * k, D))
    return tuple(_cap(b, r) for b, r in zip(bounds, refs))
