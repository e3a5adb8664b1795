"""Graph-attention hop (PyG ``GATConv``, concat=True, add_self_loops=True, no
attention dropout; model/gnn.py:196-206) on the HIP kernels of csrc/gat.hip.

``fanout_gat`` is the hop on a fixed-fanout sampled tree (autograd over
mirec_fanout_gat / mirec_fanout_gat_bwd; the softmax weights are kept for the
backward), ``csr_gat`` the forward over every row of a CSR graph (full-graph
inference), ``GATHop`` the layer with PyG's (>= 2.4) parameter names:
``lin.weight`` [H·C, d_in] without bias, ``att_src`` / ``att_dst`` [1, H, C],
``bias`` [H·C].  The projection z = x · lin.weightᵀ runs through
linear.linear (the MFMA GEMMs).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from ._lib import check, lib
from .graph import Graph
from .headrow import check_shape
from .linear import col_sums, linear


class _FanoutGAT(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z_child, z_self, valid, k, att_src, att_dst, bias, heads, slope):
        n_t, D = z_self.shape
        ch = D // heads
        z_child, z_self = z_child.contiguous(), z_self.contiguous()
        a_s, a_d = att_src.reshape(-1).contiguous(), att_dst.reshape(-1).contiguous()
        out = torch.empty_like(z_self)
        need = any(ctx.needs_input_grad)
        alpha = torch.empty(n_t, k + 1, heads, dtype=z_self.dtype, device=z_self.device) \
            if need else None
        check(lib.mirec_fanout_gat(z_child.data_ptr(), z_self.data_ptr(), _lib.ptr(valid),
                                   a_s.data_ptr(), a_d.data_ptr(), _lib.ptr(bias), n_t, k, heads,
                                   ch, slope, out.data_ptr(), _lib.ptr(alpha),
                                   _lib.stream_handle()), "fanout_gat")
        if need:
            saved = [z_child, z_self, a_s, a_d, alpha] + ([valid] if valid is not None else [])
            ctx.save_for_backward(*saved)
        ctx.cfg = (n_t, k, heads, ch, slope, valid is not None, bias is not None)
        ctx.shapes = (att_src.shape, att_dst.shape)
        return out

    @staticmethod
    def backward(ctx, grad):
        n_t, k, heads, ch, slope, has_valid, has_bias = ctx.cfg
        z_child, z_self, a_s, a_d, alpha, *rest = ctx.saved_tensors
        valid = rest[0] if has_valid else None
        grad = grad.contiguous()
        gzc, gzs = torch.empty_like(z_child), torch.empty_like(z_self)
        gs, gd = torch.empty_like(a_s), torch.empty_like(a_d)
        nw = int(lib.mirec_fanout_gat_bwd_work_floats(n_t, k, heads, ch))
        work = torch.empty(max(nw, 1), dtype=grad.dtype, device=grad.device)
        check(lib.mirec_fanout_gat_bwd(grad.data_ptr(), z_child.data_ptr(), z_self.data_ptr(),
                                       _lib.ptr(valid), a_s.data_ptr(), a_d.data_ptr(),
                                       alpha.data_ptr(), n_t, k, heads, ch, slope,
                                       gzc.data_ptr(), gzs.data_ptr(), gs.data_ptr(),
                                       gd.data_ptr(), work.data_ptr(), _lib.stream_handle()),
              "fanout_gat_bwd")
        gb = col_sums(grad) if has_bias and ctx.needs_input_grad[6] else None
        return (gzc, gzs, None, None, gs.view(ctx.shapes[0]), gd.view(ctx.shapes[1]), gb, None,
                None)


def fanout_gat(z_child: torch.Tensor, z_self: torch.Tensor, valid: torch.Tensor | None, k: int,
               att_src: torch.Tensor, att_dst: torch.Tensor, bias: torch.Tensor | None,
               heads: int, slope: float = 0.2) -> torch.Tensor:
    """The attention hop over a tree level: target t attends over its k child
    rows z_child[t*k : (t+1)*k] with valid[t*k + c] >= 0 (all if ``valid`` is
    None; int32, e.g. the sampled child ids) and over its own row z_self[t].
    z_child [n_t*k, H·C], z_self [n_t, H·C] are projected rows; att_src /
    att_dst hold H·C floats (any shape); returns [n_t, H·C].  Differentiable
    in z_child, z_self, att_src, att_dst and bias."""
    if z_self.dim() != 2 or z_child.dim() != 2 or z_child.shape[1] != z_self.shape[1] \
            or z_child.shape[0] != z_self.shape[0] * k:
        raise ValueError("fanout_gat: z_child [n_t*k, D] and z_self [n_t, D]")
    D = z_self.shape[1]
    if D % heads:
        raise ValueError("fanout_gat: the row width must be heads * channels")
    check_shape("GAT hop", int(k), int(heads), D // heads)
    if not (z_self.is_cuda and z_self.dtype == torch.float32 and z_child.dtype == torch.float32):
        raise ValueError("fanout_gat: float32 rows on a HIP device")
    if att_src.numel() != D or att_dst.numel() != D or (bias is not None and bias.numel() != D):
        raise ValueError("fanout_gat: att_src, att_dst and bias hold heads * channels floats")
    if valid is not None:
        if valid.numel() != z_child.shape[0]:
            raise ValueError("fanout_gat: one valid flag per child row")
        valid = valid.to(torch.int32).contiguous()
    return _FanoutGAT.apply(z_child, z_self, valid, int(k), att_src, att_dst, bias, int(heads),
                            float(slope))


@torch.no_grad()
def csr_gat(graph: Graph, z: torch.Tensor, att_src: torch.Tensor, att_dst: torch.Tensor,
            bias: torch.Tensor | None, heads: int, slope: float = 0.2) -> torch.Tensor:
    """The attention layer over the whole graph: row r attends over every
    entry of its CSR row and its self loop (forward only)."""
    n, D = z.shape
    if n != graph.n_nodes or D % heads:
        raise ValueError("csr_gat: z holds one row of heads * channels floats per node")
    check_shape("GAT hop", 1, int(heads), D // heads)
    z = z.contiguous()
    out = torch.empty_like(z)
    logits = torch.empty(n, 2 * heads, dtype=z.dtype, device=z.device)
    check(lib.mirec_csr_gat(graph.csr_ptr(), z.data_ptr(), att_src.reshape(-1).contiguous().data_ptr(),
                            att_dst.reshape(-1).contiguous().data_ptr(), _lib.ptr(bias), heads,
                            D // heads, float(slope), out.data_ptr(), logits.data_ptr(),
                            _lib.stream_handle()), "csr_gat")
    return out


class _Projection(nn.Module):
    """``lin``: a weight [out, in] without bias (PyG's Linear(bias=False))."""

    def __init__(self, d_in: int, d_out: int, device=None):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(d_out, d_in, device=device))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return linear(x, self.weight, None)


class GATHop(nn.Module):
    """GATConv(d_in, ch, heads=heads, add_self_loops=True) on sampled trees
    (``forward``) and on the full graph (``full``)."""

    def __init__(self, d_in: int, heads: int, ch: int, slope: float = 0.2, device=None):
        super().__init__()
        check_shape("GAT hop", 1, heads, ch)
        self.d_in, self.heads, self.ch, self.slope = int(d_in), int(heads), int(ch), float(slope)
        self.lin = _Projection(d_in, heads * ch, device=device)
        self.att_src = nn.Parameter(torch.empty(1, heads, ch, device=device))
        self.att_dst = nn.Parameter(torch.empty(1, heads, ch, device=device))
        self.bias = nn.Parameter(torch.empty(heads * ch, device=device))
        self.reset_parameters()

    def reset_parameters(self):
        # PyG: glorot on lin.weight and both attention vectors, zeros on bias
        with torch.no_grad():
            nn.init.xavier_uniform_(self.lin.weight)
            nn.init.xavier_uniform_(self.att_src)
            nn.init.xavier_uniform_(self.att_dst)
            nn.init.zeros_(self.bias)

    def project(self, x: torch.Tensor) -> torch.Tensor:
        return self.lin(x)

    def attend(self, z_child, z_self, valid, k: int) -> torch.Tensor:
        return fanout_gat(z_child, z_self, valid, k, self.att_src, self.att_dst, self.bias,
                          self.heads, self.slope)

    def forward(self, x_child, x_self, valid, k: int) -> torch.Tensor:
        return self.attend(self.project(x_child), self.project(x_self), valid, k)

    @torch.no_grad()
    def full(self, graph: Graph, x: torch.Tensor) -> torch.Tensor:
        return csr_gat(graph, self.project(x), self.att_src, self.att_dst, self.bias, self.heads,
                       self.slope)
