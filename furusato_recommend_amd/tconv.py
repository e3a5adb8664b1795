"""Dot-product attention hop (PyG ``TransformerConv``, concat=True, beta=False,
no edge features, no attention dropout, root_weight=True; model/tgrec.py:
161-171) on the HIP kernels of csrc/tattn.hip.

``fanout_tattn`` is the hop on a fixed-fanout sampled tree (autograd over
mirec_fanout_tattn / mirec_fanout_tattn_bwd; the softmax weights are kept for
the backward), ``csr_tattn`` the forward over every row of a CSR graph
(full-graph inference), ``TransformerHop`` the layer with PyG's parameter
names: ``lin_key``, ``lin_query``, ``lin_value``, ``lin_skip``, each a weight
[H·C, d_in] and a bias [H·C].

The kernels address rows through a stride, so the projections run as two
stacked GEMMs through linear.linear (the MFMA GEMMs): [lin_key ; lin_value]
over the children gives ``kv`` [n, 2 H·C] = (key | value) and [lin_query ;
lin_skip] over the targets gives ``qs`` [n, 2 H·C] = (query | skip); the
kernels read the halves in place and the backward writes its four gradients
straight into the two [·, 2 H·C] buffers those GEMMs' backward consumes.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import _lib
from ._lib import check, lib
from .graph import Graph
from .headrow import check_shape
from .linear import Linear, linear


def _check_rows(name: str, kv: torch.Tensor, qs: torch.Tensor, heads: int) -> int:
    """Validates the fused row buffers; returns D = heads * channels."""
    if kv.dim() != 2 or qs.dim() != 2 or kv.shape[1] != qs.shape[1] or qs.shape[1] % 2:
        raise ValueError(f"{name}: kv [n, 2 D] = (key | value) and qs [n, 2 D] = (query | skip)")
    D = qs.shape[1] // 2
    if heads < 1 or D % heads:
        raise ValueError(f"{name}: the row width must be 2 * heads * channels")
    if not (qs.is_cuda and kv.device == qs.device and qs.dtype == torch.float32
            and kv.dtype == torch.float32):
        raise ValueError(f"{name}: float32 rows on a HIP device")
    return D


class _FanoutTAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kv, qs, valid, k, heads):
        n_t, D2 = qs.shape
        D = D2 // 2
        ch = D // heads
        scale = 1.0 / math.sqrt(ch)
        kv, qs = kv.contiguous(), qs.contiguous()
        out = torch.empty(n_t, D, dtype=qs.dtype, device=qs.device)
        need = any(ctx.needs_input_grad)
        alpha = torch.empty(n_t, k, heads, dtype=qs.dtype, device=qs.device) if need else None
        check(lib.mirec_fanout_tattn(qs.data_ptr(), qs.data_ptr() + 4 * D, D2, kv.data_ptr(),
                                     kv.data_ptr() + 4 * D, D2, _lib.ptr(valid), n_t, k, heads,
                                     ch, scale, out.data_ptr(), _lib.ptr(alpha),
                                     _lib.stream_handle()), "fanout_tattn")
        if need:
            ctx.save_for_backward(kv, qs, alpha, *([valid] if valid is not None else []))
        ctx.cfg = (n_t, k, heads, ch, scale, valid is not None)
        return out

    @staticmethod
    def backward(ctx, grad):
        n_t, k, heads, ch, scale, has_valid = ctx.cfg
        kv, qs, alpha, *rest = ctx.saved_tensors
        valid = rest[0] if has_valid else None
        D = heads * ch
        grad = grad.contiguous()
        gkv, gqs = torch.empty_like(kv), torch.empty_like(qs)
        check(lib.mirec_fanout_tattn_bwd(grad.data_ptr(), qs.data_ptr(), 2 * D, kv.data_ptr(),
                                         kv.data_ptr() + 4 * D, 2 * D, _lib.ptr(valid),
                                         alpha.data_ptr(), n_t, k, heads, ch, scale,
                                         gqs.data_ptr(), gqs.data_ptr() + 4 * D, 2 * D,
                                         gkv.data_ptr(), gkv.data_ptr() + 4 * D, 2 * D,
                                         _lib.stream_handle()), "fanout_tattn_bwd")
        return gkv, gqs, None, None, None


def fanout_tattn(kv: torch.Tensor, qs: torch.Tensor, valid: torch.Tensor | None, k: int,
                 heads: int) -> torch.Tensor:
    """The attention hop over a tree level: target t attends with its query
    over its k child rows kv[t*k : (t+1)*k] with valid[t*k + c] >= 0 (all if
    ``valid`` is None; int32, e.g. the sampled child ids) and adds its skip
    row; there is no self slot.  kv [n_t*k, 2 D] = (key | value), qs [n_t,
    2 D] = (query | skip), D = heads * channels, the logits scaled by
    1 / sqrt(channels); returns [n_t, D].  Differentiable in kv and qs."""
    D = _check_rows("fanout_tattn", kv, qs, int(heads))
    if kv.shape[0] != qs.shape[0] * k:
        raise ValueError("fanout_tattn: kv holds k child rows per row of qs")
    check_shape("transformer hop", int(k), int(heads), D // heads)
    if valid is not None:
        if valid.numel() != kv.shape[0]:
            raise ValueError("fanout_tattn: one valid flag per child row")
        if valid.device != kv.device:
            raise ValueError("fanout_tattn: valid lies on the rows' HIP device")
        valid = valid.to(torch.int32).contiguous()
    return _FanoutTAttn.apply(kv, qs, valid, int(k), int(heads))


@torch.no_grad()
def csr_tattn(graph: Graph, kv: torch.Tensor, qs: torch.Tensor, heads: int) -> torch.Tensor:
    """The attention layer over the whole graph: row r attends with its query
    over every entry of its CSR row (no self loop) and adds its skip row
    (forward only).  kv, qs [n_nodes, 2 D] as in fanout_tattn."""
    D = _check_rows("csr_tattn", kv, qs, int(heads))
    if kv.shape[0] != graph.n_nodes or qs.shape[0] != graph.n_nodes:
        raise ValueError("csr_tattn: kv and qs hold one row per node")
    ch = D // heads
    check_shape("transformer hop", 1, int(heads), ch)
    kv, qs = kv.contiguous(), qs.contiguous()
    out = torch.empty(qs.shape[0], D, dtype=qs.dtype, device=qs.device)
    check(lib.mirec_csr_tattn(graph.csr_ptr(), qs.data_ptr(), qs.data_ptr() + 4 * D, 2 * D,
                              kv.data_ptr(), kv.data_ptr() + 4 * D, 2 * D, heads, ch,
                              1.0 / math.sqrt(ch), out.data_ptr(), _lib.stream_handle()),
          "csr_tattn")
    return out


class TransformerHop(nn.Module):
    """TransformerConv(d_in, ch, heads=heads, root_weight=True) on sampled
    trees (``forward``) and on the full graph (``full``)."""

    def __init__(self, d_in: int, heads: int, ch: int, device=None):
        super().__init__()
        check_shape("transformer hop", 1, heads, ch)
        self.d_in, self.heads, self.ch = int(d_in), int(heads), int(ch)
        for name in ("lin_key", "lin_query", "lin_value", "lin_skip"):
            setattr(self, name, Linear(d_in, heads * ch, device=device))
        self.reset_parameters()

    def reset_parameters(self):
        # PyG's Linear.reset_parameters with its default initialisers:
        # Kaiming-uniform(a = sqrt 5) on the weight, U(-1/sqrt fan_in, 1/sqrt
        # fan_in) on the bias
        bound = 1.0 / math.sqrt(self.d_in)
        with torch.no_grad():
            for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_skip):
                nn.init.kaiming_uniform_(lin.weight, a=math.sqrt(5))
                nn.init.uniform_(lin.bias, -bound, bound)

    @staticmethod
    def _stacked(a: Linear, b: Linear, x: torch.Tensor) -> torch.Tensor:
        """x through the stacked weight [a ; b] in one GEMM.  The four Linears
        stay separate parameters (PyG's state_dict keys, one Adam state
        each), so the stacked weight and bias are concatenated per call — two
        small copies of 2 H·C (d_in + 1) floats, split again by autograd in
        the backward — beside a GEMM over every row of the group."""
        return linear(x, torch.cat([a.weight, b.weight]), torch.cat([a.bias, b.bias]))

    def project_kv(self, x: torch.Tensor) -> torch.Tensor:
        """(lin_key(x) | lin_value(x)) [n, 2 H·C] in one GEMM."""
        return self._stacked(self.lin_key, self.lin_value, x)

    def project_qs(self, x: torch.Tensor) -> torch.Tensor:
        """(lin_query(x) | lin_skip(x)) [n, 2 H·C] in one GEMM."""
        return self._stacked(self.lin_query, self.lin_skip, x)

    def attend(self, kv, qs, valid, k: int) -> torch.Tensor:
        return fanout_tattn(kv, qs, valid, k, self.heads)

    def forward(self, x_child, x_self, valid, k: int) -> torch.Tensor:
        return self.attend(self.project_kv(x_child), self.project_qs(x_self), valid, k)

    @torch.no_grad()
    def full(self, graph: Graph, x: torch.Tensor) -> torch.Tensor:
        return csr_tattn(graph, self.project_kv(x), self.project_qs(x), self.heads)
