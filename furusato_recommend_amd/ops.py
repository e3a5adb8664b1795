"""``torch.ops.mirec.*`` — the propagation hot path registered as PyTorch
operators (``torch.ops.mirec.lgcn_propagate(x, csr) -> y``
wrapped with its autograd formula), on top of the same C ABI
(``mirec_propagate``) the modules call.

Operator arguments must be tensors and scalars, so a graph (its CSR, the
normalisation and the hub-row split of ``graph.Graph``) is passed as an
integer handle: ``handle(graph)`` registers it (weakly: the entry goes when
the Graph object does) and returns the id.  The autograd node of a call keeps
the Graph object itself alive until the backward has run (a temporary
``LGConv()``, or one module called on a second edge_index before the first
call's backward, would otherwise drop the only other reference).

    h = ops.handle(graph)
    y = torch.ops.mirec.lgcn_propagate(x, h)          # y = Â x
    y.backward(g)                                      # x.grad = Âᵀ g

``lgcn_propagate_t`` is Âᵀ x (the same CSR for a symmetric edge multiset,
the transposed one otherwise).  ``lgcn_propagate_w(x, edge_weight, graph)`` is
the edge-weighted y = Â x on a graph built with weights
(``Graph.from_edge_index(..., edge_weight=)``): its backward gives Âᵀ ȳ for
``x`` and, on a ``normalize=False`` graph, the per-edge dots
ȳ[dst_e] · x[src_e] (mirec_edge_dot) for ``edge_weight``.  ``lgcn_propagate_drop(x, graph, keep_prob, seed)`` is y = Â x
with edge dropout (PyG's ``dropout_edge`` followed by ``LGConv``; the mask is
a hash of (seed, destination, source) evaluated inside the kernel, restated
by ``mirec_edge_keep_mask``); its backward is ``lgcn_propagate_drop_t``, the
transposed mask on the same CSR.  All have fake
(meta) implementations, so they trace under torch.compile / torch.export
without running a kernel.
Reference call sites: model/lgcn.py:66,82 (``LGConv()(x, edge_index)``).
"""
from __future__ import annotations

import itertools
import weakref

import torch

_graphs: "weakref.WeakValueDictionary[int, object]" = weakref.WeakValueDictionary()
_ids = itertools.count(1)


def handle(graph) -> int:
    """The operator handle of a graph.Graph (registered on first use).  The
    operators are PyG's LGConv, which has no r: an r-adjusted graph
    (``from_interactions(r != 0.5)``) is refused, its transpose is not its
    own CSR."""
    if getattr(graph, "scale_src", None) is not None:
        raise ValueError("mirec operators: the graph carries r-adjusted scales "
                         f"(r = {graph.r}); torch.ops.mirec.* propagate with deg^-1/2 only")
    h = getattr(graph, "_op_handle", None)
    if h is None or _graphs.get(h) is not graph:
        h = next(_ids)
        _graphs[h] = graph
        graph._op_handle = h
    return h


def _graph(h: int):
    g = _graphs.get(int(h))
    if g is None:
        raise ValueError(f"mirec: no graph registered under handle {h}")
    return g


def _apply(g, x: torch.Tensor, **drop) -> torch.Tensor:
    from .lgconv import _spmm  # width padding / column blocks for any D
    if x.device.type != "cuda" or x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError("mirec.lgcn_propagate: float32 [N, D] tensor on the HIP device")
    if x.shape[0] != g.n_nodes:
        raise ValueError(f"mirec.lgcn_propagate: x has {x.shape[0]} rows, graph {g.n_nodes}")
    return _spmm(g, x, **drop)


@torch.library.custom_op("mirec::lgcn_propagate", mutates_args=())
def lgcn_propagate(x: torch.Tensor, graph: int) -> torch.Tensor:
    """y = Â x on graph ``graph`` (csrc/prop.hip prop_kernel)."""
    return _apply(_graph(graph), x)


@torch.library.custom_op("mirec::lgcn_propagate_t", mutates_args=())
def lgcn_propagate_t(x: torch.Tensor, graph: int) -> torch.Tensor:
    """y = Âᵀ x (the backward of lgcn_propagate)."""
    g = _graph(graph)
    return _apply(g if g.symmetric else g.transpose, x)


@lgcn_propagate.register_fake
def _(x, graph):
    return torch.empty_like(x)


@lgcn_propagate_t.register_fake
def _(x, graph):
    return torch.empty_like(x)


# ---- edge dropout ---------------------------------------------------------------
def _check_drop(g, keep_prob: float) -> None:
    if not (0.0 < float(keep_prob) <= 1.0):
        raise ValueError(f"mirec.lgcn_propagate_drop: keep_prob must lie in (0, 1], "
                         f"got {keep_prob!r}")
    if g.val is not None:
        raise ValueError("mirec.lgcn_propagate_drop: edge dropout and edge weights are not "
                         "combined")


@torch.library.custom_op("mirec::lgcn_propagate_drop", mutates_args=())
def lgcn_propagate_drop(x: torch.Tensor, graph: int, keep_prob: float, seed: int) -> torch.Tensor:
    """y = Â_drop x: PyG's ``dropout_edge`` followed by ``LGConv`` in one
    launch, with dinv of the full graph (the reference's __dropout_x drops
    entries of the normalised matrix).  Entry (j → i) is kept iff
    mirec_edge_keep(seed, i, j) (include/mirec.h; multi-edges share the draw)
    and kept entries are divided by ``keep_prob``.  ``seed`` is taken modulo
    2^64."""
    g = _graph(graph)
    _check_drop(g, keep_prob)
    return _apply(g, x, dropout=(keep_prob, seed))


@torch.library.custom_op("mirec::lgcn_propagate_drop_t", mutates_args=())
def lgcn_propagate_drop_t(x: torch.Tensor, graph: int, keep_prob: float,
                          seed: int) -> torch.Tensor:
    """y = Â_dropᵀ x (the backward of lgcn_propagate_drop): the transposed
    mask keep(seed, j, i) on the same CSR (the transposed one for an
    asymmetric edge multiset)."""
    g = _graph(graph)
    _check_drop(g, keep_prob)
    return _apply(g if g.symmetric else g.transpose, x, dropout=(keep_prob, seed),
                  transposed=True)


@lgcn_propagate_drop.register_fake
def _(x, graph, keep_prob, seed):
    return torch.empty_like(x)


@lgcn_propagate_drop_t.register_fake
def _(x, graph, keep_prob, seed):
    return torch.empty_like(x)


def _setup_drop(ctx, inputs, output):
    ctx.graph_obj = _graph(inputs[1])
    ctx.drop = (float(inputs[2]), int(inputs[3]))


def _bwd_drop(ctx, grad):
    return (torch.ops.mirec.lgcn_propagate_drop_t(grad.contiguous(), handle(ctx.graph_obj),
                                                  *ctx.drop), None, None, None)


def _bwd_drop_t(ctx, grad):
    return (torch.ops.mirec.lgcn_propagate_drop(grad.contiguous(), handle(ctx.graph_obj),
                                                *ctx.drop), None, None, None)


lgcn_propagate_drop.register_autograd(_bwd_drop, setup_context=_setup_drop)
lgcn_propagate_drop_t.register_autograd(_bwd_drop_t, setup_context=_setup_drop)


# ---- edge-weighted propagation ------------------------------------------------
def _install(g, w: torch.Tensor) -> None:
    """Make the normalize=False graph ``g`` hold the weights ``w``.  The graph
    keeps the tensor it was last refreshed from (so its storage cannot be
    reused by another tensor) and its version: the same tensor, unchanged,
    costs nothing."""
    tok = g._w_token
    if (tok is not None and tok[0].data_ptr() == w.data_ptr() and tok[1] == w._version
            and tok[0].shape == w.shape):
        return
    g.set_edge_weight(w)
    g._w_token = (w.detach(), w._version)


def _check_w(g, w: torch.Tensor) -> None:
    if g.val is None:
        raise ValueError("mirec.lgcn_propagate_w: the graph was built without edge weights")
    n_edges = g.nnz // 2 if g._coo is None else g.nnz
    if w.dim() != 1 or w.shape[0] != n_edges or not w.is_floating_point():
        raise ValueError(f"mirec.lgcn_propagate_w: edge_weight must be a float [{n_edges}] "
                         f"tensor, got {w.dtype} {tuple(w.shape)}")


@torch.library.custom_op("mirec::lgcn_propagate_w", mutates_args=())
def lgcn_propagate_w(x: torch.Tensor, edge_weight: torch.Tensor, graph: int) -> torch.Tensor:
    """y = Â x with per-edge weights (csrc/prop.hip, the weighted prop_kernel instantiations).  On a
    ``normalize=False`` graph ``edge_weight`` is installed into the graph's
    CSR values first (a device gather, skipped when it already holds them); a
    ``normalize=True`` graph is static: it holds the weights it was built
    with (its dinv depends on them) and ``edge_weight`` must be those."""
    g = _graph(graph)
    _check_w(g, edge_weight)
    if not g.normalize:
        _install(g, edge_weight)
    return _apply(g, x)


@lgcn_propagate_w.register_fake
def _(x, edge_weight, graph):
    return torch.empty_like(x)


def _edge_dot(g, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Per-entry dots in CSR order for any width (padding / 256-column blocks
    like lgconv._spmm; the blocks' dots are added in column order)."""
    import torch.nn.functional as F

    from . import _lib
    from .engine import edge_dot
    from .lgconv import _width
    out = torch.empty(max(g.nnz, 1), dtype=torch.float32, device=a.device)
    d = a.shape[1]
    if d in _lib.SUPPORTED_DIMS:
        edge_dot(g, a.contiguous(), b.contiguous(), out)
        return out[: g.nnz]
    total = None
    for c0 in range(0, d, 256):
        ab, bb = a[:, c0:c0 + 256], b[:, c0:c0 + 256]
        pad = _width(ab.shape[1]) - ab.shape[1]
        edge_dot(g, F.pad(ab, (0, pad)).contiguous(), F.pad(bb, (0, pad)).contiguous(), out)
        total = out.clone() if total is None else total.add_(out)
    return total[: g.nnz]


def _setup_w(ctx, inputs, output):
    x, w, h = inputs
    g = _graph(h)
    ctx.graph_obj = g
    ctx.w_grad = bool(ctx.needs_input_grad[1])
    if ctx.w_grad and g.normalize:
        raise NotImplementedError(
            "mirec.lgcn_propagate_w: the gradient with respect to edge_weight is not "
            "implemented for normalize=True (dinv depends on the weights); use "
            "normalize=False or detach the weights")
    ctx.save_for_backward(x if ctx.w_grad else None, None if g.normalize else w)


def _bwd_w(ctx, grad):
    g = ctx.graph_obj
    x, w = ctx.saved_tensors
    grad = grad.contiguous()
    if w is not None:
        _install(g, w)  # this call's weights, if the graph holds others by now
    gx = _apply(g if g.symmetric else g.transpose, grad) if ctx.needs_input_grad[0] else None
    gw = None
    if ctx.w_grad:
        dots = _edge_dot(g, grad, x)  # CSR order
        if g._coo is not None:        # perm is a permutation of the edges
            gw = torch.empty_like(dots).index_copy_(0, g.perm, dots)
        else:                         # bipartite: both directions of interaction e
            gw = torch.zeros(g.nnz // 2, dtype=dots.dtype, device=dots.device)
            gw.index_add_(0, g.perm, dots)
        gw = gw.to(w.dtype)
    return gx, gw, None


lgcn_propagate_w.register_autograd(_bwd_w, setup_context=_setup_w)


def _setup(ctx, inputs, output):
    ctx.graph_obj = _graph(inputs[1])  # strong reference for the node's lifetime


def _bwd(ctx, grad):
    return torch.ops.mirec.lgcn_propagate_t(grad.contiguous(), handle(ctx.graph_obj)), None


def _bwd_t(ctx, grad):
    return torch.ops.mirec.lgcn_propagate(grad.contiguous(), handle(ctx.graph_obj)), None


lgcn_propagate.register_autograd(_bwd, setup_context=_setup)
lgcn_propagate_t.register_autograd(_bwd_t, setup_context=_setup)

__all__ = ["handle", "lgcn_propagate", "lgcn_propagate_t", "lgcn_propagate_w",
           "lgcn_propagate_drop", "lgcn_propagate_drop_t"]
