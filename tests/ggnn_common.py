"""Float64 restatement of the gated graph hop (PyG ``GatedGraphConv(d,
num_layers=1, aggr='mean')`` semantics, restated from PyG's documentation;
torch_geometric is not used), the rounding bounds the GPU tests hold
csrc/ggnn.hip to, and the case lists of tests/test_ggnn_kernels.py.  numpy /
torch on the host only; nothing from the package.

The arithmetic, per node i with children j and input rows x:
    m_j = x_j W          a_i = mean_j m_j (0 without a valid child)
    gi = a_i W_ihᵀ + b_ih    gh = x_i W_hhᵀ + b_hh      thirds r, z, n
    r = σ(gi_r + gh_r)  z = σ(gi_z + gh_z)  n = tanh(gi_n + r gh_n)
    h' = (1 - z) n + z x_i

Two independent forms of the gate:
  * ``gate_np``: the formulas in numpy, σ(x) = 0.5 (1 + tanh(x / 2));
  * ``cell_torch``: torch.nn.GRUCell in float64 with the same weights
    (differentiable: the autograd yardstick of the closed-form backward
    ``backward_closed`` and of the model tests).
Two forms of the hop:
  * ``hop_loop``: a per-target Python loop over the tree layout (child rows
    t*k .. t*k + k - 1, a slot is valid iff its flag is >= 0): mean first,
    then the projection, then the gate;
  * ``hop_edges``: PyG's order — project every row, scatter-mean over the
    edge list of gat_common.tree_edges, then the cell.
``model_forward`` is the whole tree in the second form, ``dense_full`` the
full-graph layer (every CSR entry once, multi-edges included).

The bounds.  u = 2^-24, gamma(n) = n u / (1 - n u).  References are float64
on the float32-rounded inputs; every float32 operation of the kernel is one
rounding (relative u) unless said otherwise.
  exp        EXP_ULP = 2^-22 relative for one hardware exp2 (v_exp_f32: 1 ulp
             = 2^-23, doubled), as in gat_common; its argument c * x with c =
             fl(log2 e) carries the constant's rounding and the product's, 3
             u |x| absolute with room: rho(x) = EXP_ULP + 3 u |x|.
  rcp        RCP_ULP = 2^-22 relative for one hardware reciprocal (v_rcp_f32:
             1 ulp = 2^-23, doubled).  The doubling of the two constants
             covers every product of two error terms left out below.
  sigmoid    s = 1 / (1 + e), e = exp(-x): a log-perturbation eps of e moves
             s by at most s (1 - s) eps exp(eps) (d s / d ln e = -s (1 - s),
             which itself changes by at most exp(eps) along the way); eps =
             dx + rho(x), dx the pre-activation's absolute error.  The sum 1 +
             e and the reciprocal: s (u + RCP_ULP).  An exponential or a
             reciprocal below 2^-126 flushes to 0: TINY absolute.
  tanh       n = 1 - 2 w, w = sigmoid(-2 x): 2 dw + u |n| (the final fma).
  reference  its own float64 error is absolute where it cancels — 1 + tanh in
             the stable sigmoid, 1 - z, 1 - n^2 — and a gate of 1e-12 times a
             gradient would be held to less than that: REF = 2^-50 absolute
             on each of r, z, n covers it.
  gates      x_r = gi_r + gh_r: dx = u |x_r| (z alike); x_n = fma(r, gh_n,
             gi_n): dx = |gh_n| dr + u |x_n|.
  out        fma(z, h - n, n) with q = h - n: (1 - z) dn + |q| dz + dz dn +
             z u |q| + u |out| (both uses of n carry the same error, so it
             enters through d out / d n = 1 - z); max(., 0) does not raise it.
The backward's bounds carry dr, dz, dn the same way through its formulas
(``bwd_bounds``: every product E(a b) = E_a |b| + |a| E_b + E_a E_b + u |a
b|).  Every bound is then capped at CAP * max |reference| of its tensor
(1e-4, the project's fp32 bar; never below TINY = 2^-100).  The backward's
reference takes its ReLU mask from the float32 forward's ``out``, so it is a
test of the backward alone.  A bias gradient is a column sum over n rows in
some fixed order: the rows' bounds summed plus gamma(n + 8) * sum |term|.
"""
import numpy as np
import torch

from tests import gat_common as gc

U = 2.0 ** -24
EXP_ULP = 2.0 ** -22
RCP_ULP = 2.0 ** -22
CAP = 1e-4
TINY = 2.0 ** -100
REF = 2.0 ** -50
MAX_BLOCKS = 2048   # grid cap of both kernels (csrc/ggnn.hip: kGruMaxBlocks)

# (n, d)
CASES = [(1, 4), (3, 12), (33, 64), (257, 128), (65, 256)]
SCALES = (1.0, 30.0)   # variance of the pre-activations and of h
SATURATED = (90.0, 1e4)


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def rows_per_block(d):
    """Rows a 256-thread block takes per round: 256 / (lanes per row), the
    lanes per row the next power of two >= d / 4."""
    lanes = 1
    while lanes < d // 4:
        lanes *= 2
    return 256 // lanes


# more rows than MAX_BLOCKS blocks take in one round: the grid-stride loop
# runs a second time for the first block
STRIDE_CASE = (MAX_BLOCKS * rows_per_block(4) + 3, 4)


# ------------------------------------------------------------------- inputs
def make_inputs(case, scale, seed=0):
    """float32 inputs of a case: dict(gi, gh [n, 3d], h [n, d], g [n, d])."""
    n, d = case
    rng = np.random.default_rng([n, d, int(scale), seed])
    sd = np.sqrt(scale)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    return dict(gi=f32(rng.standard_normal((n, 3 * d)) * sd),
                gh=f32(rng.standard_normal((n, 3 * d)) * sd),
                h=f32(rng.standard_normal((n, d)) * sd),
                g=f32(rng.uniform(0.5, 1.5, (n, d)) * rng.choice([-1.0, 1.0], (n, d))))


def make_saturated(case, seed=0):
    """Pre-activations drawn from {+-90, +-1e4}: gi from the set everywhere,
    gh zero in the r and z thirds (so x_r, x_z are in the set) and from the
    set in the n third (x_n = gi_n + r gh_n, r in {0, 1} up to rounding: sums
    of two members, 0 included — the tanh both saturated and not)."""
    n, d = case
    rng = np.random.default_rng([n, d, 90, seed])
    vals = np.array([s * v for v in SATURATED for s in (1.0, -1.0)])
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    gi = rng.choice(vals, (n, 3 * d))
    gh = np.zeros((n, 3 * d))
    gh[:, 2 * d:] = rng.choice(vals, (n, d))
    return dict(gi=f32(gi), gh=f32(gh), h=f32(rng.standard_normal((n, d))),
                g=f32(rng.uniform(0.5, 1.5, (n, d)) * rng.choice([-1.0, 1.0], (n, d))))


# ----------------------------------------------------------- the gate, form 1
def sigmoid(x):
    return 0.5 * (1.0 + np.tanh(0.5 * np.asarray(x, np.float64)))


def gates_np(gi, gh):
    """(r, z, n, x_r, x_z, x_n) in float64."""
    gi, gh = np.asarray(gi, np.float64), np.asarray(gh, np.float64)
    d = gi.shape[1] // 3
    x_r, x_z = gi[:, :d] + gh[:, :d], gi[:, d:2 * d] + gh[:, d:2 * d]
    r, z = sigmoid(x_r), sigmoid(x_z)
    x_n = gi[:, 2 * d:] + r * gh[:, 2 * d:]
    return r, z, np.tanh(x_n), x_r, x_z, x_n


def gate_np(gi, gh, h, relu=False):
    r, z, n, *_ = gates_np(gi, gh)
    out = (1.0 - z) * n + z * np.asarray(h, np.float64)
    return np.maximum(out, 0.0) if relu else out


def backward_closed(g, gi, gh, h, mask=None):
    """The issue's closed form in float64: (d_gi, d_gh, d_h) for g = dL/dh'
    (``mask``: where the fused ReLU passed the gradient; None = no ReLU).
    d_h is the direct path only."""
    g, h = np.asarray(g, np.float64), np.asarray(h, np.float64)
    if mask is not None:
        g = np.where(mask, g, 0.0)
    r, z, n, *_ = gates_np(gi, gh)
    d = h.shape[1]
    gh_n = np.asarray(gh, np.float64)[:, 2 * d:]
    dh = g * z
    dn = g * (1.0 - z)
    dz = g * (h - n)
    pn = dn * (1.0 - n * n)
    dr = pn * gh_n
    pr = dr * r * (1.0 - r)
    pz = dz * z * (1.0 - z)
    return (np.concatenate([pr, pz, pn], 1), np.concatenate([pr, pz, pn * r], 1), dh)


# ----------------------------------------------------------- the gate, form 2
def cell_torch(a, h, w_ih, w_hh, b_ih, b_hh):
    """torch.nn.GRUCell(d, d) in float64 on the given weights (differentiable
    in every argument)."""
    d = h.shape[1]
    cell = torch.nn.GRUCell(d, d).double()
    return torch.func.functional_call(
        cell, dict(weight_ih=w_ih, weight_hh=w_hh, bias_ih=b_ih, bias_hh=b_hh), (a, h))


def make_conv(d, seed=0, scale=1.0):
    """float32-representable float64 torch parameters (W [d, d], W_ih, W_hh
    [3d, d], b_ih, b_hh [3d]) drawn like the hop's reset."""
    rng = np.random.default_rng([d, seed, 77])
    b = scale / np.sqrt(d)
    mk = lambda *s: torch.from_numpy(  # noqa: E731
        rng.uniform(-b, b, s).astype(np.float32).astype(np.float64))
    return mk(d, d), mk(3 * d, d), mk(3 * d, d), mk(3 * d), mk(3 * d)


# ------------------------------------------------------------------- the hop
def hop_loop(x_child, x_self, valid, k, conv, relu=False):
    """Per-target loop, mean first (numpy float64): out [n_t, d]."""
    W, w_ih, w_hh, b_ih, b_hh = (np.asarray(p, np.float64) for p in conv)
    x_child, x_self = np.asarray(x_child, np.float64), np.asarray(x_self, np.float64)
    n_t, d = x_self.shape
    ok = gc.valid_mask(valid, n_t, k)
    out = np.zeros((n_t, d))
    for t in range(n_t):
        rows = [x_child[t * k + c] for c in range(k) if ok[t, c]]
        mean = np.mean(rows, axis=0) if rows else np.zeros(d)
        a = mean @ W
        gi = (a @ w_ih.T + b_ih)[None]
        gh = (x_self[t] @ w_hh.T + b_hh)[None]
        out[t] = gate_np(gi, gh, x_self[t:t + 1], relu)[0]
    return out


def scatter_mean(m, edge_index, n_rows):
    """Mean of the source rows per destination row (0 without an edge)."""
    src, dst = edge_index[0].long(), edge_index[1].long()
    s = torch.zeros(n_rows, m.shape[1], dtype=m.dtype).index_add(0, dst, m[src])
    cnt = torch.zeros(n_rows, dtype=m.dtype).index_add(0, dst, torch.ones_like(dst, dtype=m.dtype))
    return s / cnt.clamp(min=1.0)[:, None]


def hop_edges(x, edge_index, conv):
    """GatedGraphConv's order on rows x [N, d] (torch float64): project every
    row, scatter-mean over the edges (source, destination), then the cell on
    every row.  Differentiable."""
    W, w_ih, w_hh, b_ih, b_hh = conv
    a = scatter_mean(x @ W, edge_index, x.shape[0])
    return cell_torch(a, x, w_ih, w_hh, b_ih, b_hh)


def tree_level(x_child, x_self, valid, k, conv):
    n_t = x_self.shape[0]
    out = hop_edges(torch.cat([x_child, x_self]), gc.tree_edges(valid, n_t, k), conv)
    return out[n_t * k:]


def model_forward(table, convs, groups, depths, children, L, sizes):
    """The 'gnn' forward with conv = 'ggnn' and no dropout in torch float64:
    table [N, d], convs = [(W, W_ih, W_hh, b_ih, b_hh)] per layer.  Rows of
    ids < 0 are zero rows and are left out of their parent's mean.  Returns
    the seed rows h^(L)."""
    h = []
    for g in groups:
        g = torch.as_tensor(np.asarray(g)).long()
        h.append(table[g.clamp(min=0)] * (g >= 0).to(table.dtype)[:, None])
    for i, lay in enumerate(gc.tree_layers(groups, depths, children, L, sizes)):
        new = list(h)
        for gi, ci, k, ei in lay:
            n_t = h[gi].shape[0]
            out = hop_edges(torch.cat([h[ci], h[gi]]), ei, convs[i])[n_t * k:]
            new[gi] = out.relu() if i != L - 1 else out
        h = new
    return h[0]


def dense_full(x, rowptr, col, conv):
    """Full-graph layer (torch float64): row r takes the mean over every CSR
    entry col[rowptr[r] : rowptr[r + 1]], each entry once."""
    dst = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    ei = torch.from_numpy(np.stack([np.asarray(col, np.int64), dst]))
    return hop_edges(x, ei, conv)


# ---------------------------------------------------------------------- bounds
def _cap(bound, ref):
    return np.minimum(bound, max(CAP * float(np.abs(ref).max()), TINY) if ref.size else 0.0)


def _rho(x):
    return EXP_ULP + 3.0 * U * np.abs(x)


def _sig_err(s, eps):
    """Error of a hardware sigmoid whose exact value is s, its exponential
    off by the log-perturbation eps."""
    return s * (1.0 - s) * eps * np.exp(eps) + s * (U + RCP_ULP) + TINY


def gate_errors(gi, gh):
    """(dr, dz, dn): absolute error bounds of the kernel's gates."""
    r, z, n, x_r, x_z, x_n = gates_np(gi, gh)
    d = r.shape[1]
    gh_n = np.abs(np.asarray(gh, np.float64)[:, 2 * d:])
    dr = _sig_err(r, U * np.abs(x_r) + _rho(x_r)) + REF
    dz = _sig_err(z, U * np.abs(x_z) + _rho(x_z)) + REF
    dx_n = gh_n * dr + U * np.abs(x_n)
    w = 0.5 * (1.0 - n)                      # sigmoid(-2 x_n)
    dn = 2.0 * _sig_err(w, 2.0 * dx_n + _rho(2.0 * x_n)) + U * np.abs(n) + REF
    return dr, dz, dn


def fwd_bounds(gi, gh, h, ref):
    """Bound of out (with or without the ReLU) against ``ref`` = gate_np."""
    r, z, n, *_ = gates_np(gi, gh)
    dr, dz, dn = gate_errors(gi, gh)
    q = np.abs(np.asarray(h, np.float64) - n)
    pre = (1.0 - z) * n + z * np.asarray(h, np.float64)
    b = (1.0 - z) * dn + q * dz + dz * dn + z * U * q + U * np.abs(pre) + TINY
    return _cap(b, ref)


def _mul(a, ea, b, eb):
    """(|a b|, bound) of fl(a_hat * b_hat)."""
    p = np.abs(a * b)
    return p, ea * np.abs(b) + np.abs(a) * eb + ea * eb + U * p


def bwd_bounds(g, gi, gh, h, mask, refs):
    """Bounds of (d_gi, d_gh, d_h) against backward_closed on the same inputs
    (the mask an input), and their uncapped forms for the bias sums."""
    g, h = np.asarray(g, np.float64), np.asarray(h, np.float64)
    if mask is not None:
        g = np.where(mask, g, 0.0)
    r, z, n, *_ = gates_np(gi, gh)
    dr, dz, dn = gate_errors(gi, gh)
    d = h.shape[1]
    gh_n = np.asarray(gh, np.float64)[:, 2 * d:]
    zero = np.zeros_like(g)
    _, e_dh = _mul(g, zero, z, dz)
    omz, e_omz = 1.0 - z, dz + U * (1.0 - z)
    dn_, e_dn_ = g * omz, _mul(g, zero, omz, e_omz)[1]
    q, e_q = h - n, dn + U * np.abs(h - n)
    dz_, e_dz_ = g * q, _mul(g, zero, q, e_q)[1]
    t, e_t = 1.0 - n * n, 2.0 * np.abs(n) * dn + dn * dn + U * np.abs(1.0 - n * n)
    pn, e_pn = dn_ * t, _mul(dn_, e_dn_, t, e_t)[1]
    e_hn = _mul(pn, e_pn, r, dr)[1]
    dr_, e_dr_ = pn * gh_n, _mul(pn, e_pn, gh_n, zero)[1]
    rr, e_rr = r * (1.0 - r), np.abs(1.0 - 2.0 * r) * dr + dr * dr + 2.0 * U * r * (1.0 - r)
    zz, e_zz = z * (1.0 - z), np.abs(1.0 - 2.0 * z) * dz + dz * dz + 2.0 * U * z * (1.0 - z)
    e_pr = _mul(dr_, e_dr_, rr, e_rr)[1]
    e_pz = _mul(dz_, e_dz_, zz, e_zz)[1]
    raw = (np.concatenate([e_pr, e_pz, e_pn], 1) + TINY,
           np.concatenate([e_pr, e_pz, e_hn], 1) + TINY, e_dh + TINY)
    return tuple(_cap(b, ref) for b, ref in zip(raw, refs)), raw


def bias_bounds(raw, ref_rows):
    """Bound of the column sums of a gradient [n, m] taken in float32 in any
    fixed order, against the float64 column sums of its reference rows."""
    n = ref_rows.shape[0]
    b = raw.sum(0) + gamma(n + 8) * np.abs(ref_rows).sum(0) + TINY
    return _cap(b, ref_rows.sum(0))
