"""Gated graph hop (PyG ``GatedGraphConv(d, num_layers=1, aggr='mean')``;
model/gnn.py:185-232, conv = 'ggnn') on the HIP kernels of csrc/ggnn.hip.

Per node i with sampled (or all) children j and input rows x:

    m_j = x_j · W                    W = weight[0] [d, d], not transposed
    a_i = mean_j m_j                 (0 without a valid child)
    h'_i = GRUCell(a_i, x_i)         torch.nn.GRUCell's arithmetic

The mean commutes with the linear map, so the hop takes the children's mean
first (mirec_fanout_mean on a tree, the CSR propagation kernel on the full
graph: one pass over the child rows) and projects only the n_t target rows:
a = (mean_j x_j) · W, gi = a · W_ihᵀ + b_ih, gh = x · W_hhᵀ + b_hh — three
GEMMs over n_t rows (linear.py's MFMA GEMMs, the two biases added in the
GEMM epilogue) and no GEMM over the n_t · k child rows.  ``gru_gate`` is the
cell's element-wise part (autograd over mirec_gru_gate / mirec_gru_gate_bwd;
the backward recomputes the gates, only the output is kept, for the fused
ReLU's mask).  The bias gradients are the column sums of the gate's ∂gi and
∂gh, taken by the GEMM backward in a fixed order (mirec_gemm_tn's column sums
or linear.col_sums): no float atomics, a step repeats bitwise.

``GGNNHop`` carries PyG's parameter names — ``weight`` [1, d, d],
``rnn.weight_ih`` / ``rnn.weight_hh`` [3d, d], ``rnn.bias_ih`` /
``rnn.bias_hh`` [3d] — so reference checkpoints load.
"""
from __future__ import annotations

import math
import weakref

import torch
import torch.nn as nn

from . import _lib
from ._lib import check, lib
from .graph import Graph
from .graphsage import _FanoutMean, csr_mean
from .linear import gemm_nn, gemm_nt, gemm_tn, linear

MAX_DIM = 1024  # csrc/ggnn.hip: kGruMaxDim


class _GRUGate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gi, gh, h, relu: bool):
        gi, gh, h = gi.contiguous(), gh.contiguous(), h.contiguous()
        n, d = h.shape
        out = torch.empty_like(h)
        check(lib.mirec_gru_gate(gi.data_ptr(), gh.data_ptr(), h.data_ptr(), n, d, int(relu),
                                 out.data_ptr(), _lib.stream_handle()), "gru_gate")
        ctx.save_for_backward(gi, gh, h, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, grad):
        gi, gh, h, out = ctx.saved_tensors
        n, d = h.shape
        grad = grad.contiguous()
        d_gi, d_gh, d_h = torch.empty_like(gi), torch.empty_like(gh), torch.empty_like(h)
        check(lib.mirec_gru_gate_bwd(grad.data_ptr(), gi.data_ptr(), gh.data_ptr(), h.data_ptr(),
                                     _lib.ptr(out), n, d, d_gi.data_ptr(), d_gh.data_ptr(),
                                     d_h.data_ptr(), _lib.stream_handle()), "gru_gate_bwd")
        return d_gi, d_gh, d_h, None


def gru_gate(gi: torch.Tensor, gh: torch.Tensor, h: torch.Tensor, relu: bool = False):
    """The GRU cell's gate on finished pre-activations: gi = a W_ihᵀ + b_ih,
    gh = h W_hhᵀ + b_hh [n, 3d] (thirds r, z, n), h [n, d]; returns (1 - z) n
    + z h [n, d], under a ReLU if ``relu``.  Differentiable in gi, gh and h
    (the direct path of h only: the one through gh belongs to its GEMM)."""
    if h.dim() != 2 or gi.dim() != 2 or gi.shape != gh.shape \
            or gi.shape != (h.shape[0], 3 * h.shape[1]):
        raise ValueError("gru_gate: gi and gh [n, 3d], h [n, d]")
    d = h.shape[1]
    if d % 4 or not 4 <= d <= MAX_DIM:
        raise ValueError(f"gru_gate: the row width must be a multiple of 4 in [4, {MAX_DIM}]")
    if not (h.is_cuda and gi.device == h.device and gh.device == h.device
            and gi.dtype == gh.dtype == h.dtype == torch.float32):
        raise ValueError("gru_gate: float32 rows on one HIP device")
    return _GRUGate.apply(gi, gh, h, bool(relu))


class _MatmulNN(torch.autograd.Function):
    """a · w with w [K, N] read as stored (GatedGraphConv's ``weight[0]``):
    the MFMA GEMMs when the shapes are theirs, torch's otherwise."""

    @staticmethod
    def forward(ctx, a, w):
        a = a.contiguous()
        ctx.save_for_backward(a, w)
        y = gemm_nn(a, w)
        return a @ w if y is None else y

    @staticmethod
    def backward(ctx, dy):
        a, w = ctx.saved_tensors
        dy = dy.contiguous()
        da = dw = None
        if ctx.needs_input_grad[0]:
            da = gemm_nt(dy, w)
            if da is None:
                da = dy @ w.t()
        if ctx.needs_input_grad[1]:
            r = gemm_tn(a, dy, False)
            dw = a.t() @ dy if r is None else r[0]
        return da, dw


def fanout_mean(x_child: torch.Tensor, valid: torch.Tensor, k: int) -> torch.Tensor:
    """Mean of every target's valid child rows (valid[t*k + c] >= 0; 0 for a
    target without one): mirec_fanout_mean without dropout."""
    if x_child.dim() != 2 or valid.numel() != x_child.shape[0] or valid.numel() % k:
        raise ValueError("ggnn: x_child [n_t*k, d] and one valid flag per child row")
    if not (x_child.is_cuda and x_child.dtype == torch.float32) or x_child.shape[1] % 4:
        raise ValueError("ggnn: float32 rows of a multiple of 4 floats on a HIP device")
    return _FanoutMean.apply(x_child, valid.to(torch.int32).contiguous(), int(k), 0.0, 0)


_MEAN_DINV = weakref.WeakKeyDictionary()  # Graph -> 1 / deg (0 for isolated rows)


def mean_dinv(graph: Graph) -> torch.Tensor:
    v = _MEAN_DINV.get(graph)
    if v is None:
        deg = torch.from_numpy(graph.degree()).to(graph.device).float()
        v = torch.where(deg > 0, 1.0 / deg.clamp(min=1), torch.zeros_like(deg))
        _MEAN_DINV[graph] = v
    return v


class _GRUParams(nn.Module):
    """The parameters of torch.nn.GRUCell(d, d) under its names."""

    def __init__(self, d: int, device=None):
        super().__init__()
        self.weight_ih = nn.Parameter(torch.empty(3 * d, d, device=device))
        self.weight_hh = nn.Parameter(torch.empty(3 * d, d, device=device))
        self.bias_ih = nn.Parameter(torch.empty(3 * d, device=device))
        self.bias_hh = nn.Parameter(torch.empty(3 * d, device=device))


class GGNNHop(nn.Module):
    """GatedGraphConv(d, num_layers=1, aggr='mean') on sampled trees
    (``forward``) and on the full graph (``full``)."""

    def __init__(self, d: int, device=None):
        super().__init__()
        if d % 4 or not 4 <= d <= MAX_DIM:
            raise ValueError(f"GGNN hop: d must be a multiple of 4 in [4, {MAX_DIM}]")
        self.d = int(d)
        self.weight = nn.Parameter(torch.empty(1, d, d, device=device))
        self.rnn = _GRUParams(d, device=device)
        self.reset_parameters()

    def reset_parameters(self):
        # PyG's uniform(out_channels, weight) and GRUCell's reset: U(-1/√d, 1/√d)
        bound = 1.0 / math.sqrt(self.d)
        with torch.no_grad():
            for p in self.parameters():
                nn.init.uniform_(p, -bound, bound)

    def aggregate(self, x_child, valid, k: int) -> torch.Tensor:
        return fanout_mean(x_child, valid, k)

    def update(self, a: torch.Tensor, h: torch.Tensor, relu: bool = False) -> torch.Tensor:
        """GRUCell(a · W, h): the three GEMMs and the gate."""
        m = _MatmulNN.apply(a, self.weight.view(self.d, self.d))
        gi = linear(m, self.rnn.weight_ih, self.rnn.bias_ih)
        gh = linear(h, self.rnn.weight_hh, self.rnn.bias_hh)
        return gru_gate(gi, gh, h, relu)

    def forward(self, x_child, x_self, valid, k: int) -> torch.Tensor:
        return self.update(self.aggregate(x_child, valid, k), x_self)

    @torch.no_grad()
    def full(self, graph: Graph, x: torch.Tensor) -> torch.Tensor:
        """The layer over the whole graph: every row takes the mean over all
        its CSR entries (a multi-edge once per entry; 0 for an isolated row)."""
        if x.dim() != 2 or x.shape != (graph.n_nodes, self.d):
            raise ValueError("GGNN hop: x holds one row of d floats per node")
        x = x.contiguous()
        agg = torch.empty_like(x)
        csr_mean(graph, mean_dinv(graph), x, agg)
        return self.update(agg, x)
