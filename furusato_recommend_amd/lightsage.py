"""LightSAGE (model/lightsage.py) on the HIP engine: LightGCN's idea on
GraphSAGE's sampled trees.  No weight matrices, no ReLU; the only parameter is
the [N, d] id table.

In scope: the sampled-tree forward (lightsage.py:274-290), the BPR loss with
the reference's doubling norm term (:292-303), OneEpoch / the step, and a
full-graph inference.  Out of scope, as for the other tree models: the
proprietary feature and text towers (the initial embedding is the id table
alone), data parallelism and HIP-graph capture.

Forward, on graphsage.SampleTree.  Layer i has hop h = L - i; its targets are
the groups of depth <= h - 1, the children of target group g are group
children[(g, h)] (depth h, fanout k = sizes[h - 1]):

    x0_g         = table[ids_g]                     (a row of id < 0 is 0)
    x(i+1)_g[t]  = xi_g[t] + (1 / cnt_t) sum over valid c of drop(xi_child[t k + c])
    cnt_t        = the slots c with id >= 0; the mean is 0 when cnt_t = 0
    emb          = (x0_0 + x1_0 + ... + xL_0) / (L + 1)     (group 0: the 3B seeds)

``drop`` is the counter-hash element dropout of include/mirec.h at element
index (t k + c) d + col (the reference drops the gathered source rows per
edge: one mask element per slot and column), seed dropout_seed * 1_000_003 +
g * 131 + i for layer i >= 1, target group g (GraphSAGE's ``seed_of``).  Layer
0 is ONE launch over all its targets — every hop-L child group has the same
fanout, so the target groups' ids and their leaf groups' ids concatenate —
with seed_of(0, 0) and t running over the concatenated targets.
``dropout_p`` defaults to 0.2 (lightsage.py:58), training only.

Loss: all_param += all_param + |p| over the parameters in registration order;
the item slice stands for item_feature_embeddings (registered first, :100)
and the user slice for user_feature_embeddings, so all_param = 2 |I| + |U|
(HEAVY_SLICE = 1, as for TGRec).

Leaf-gather form (FUSED_HOP = True): layer 0 reads self and child rows
straight from the table (mirec_fanout_resmean_gather), layers >= 1 are one
mirec_fanout_resmean per (target group, child group) pair on slices of the
previous layer's buffer; nothing of the tree is materialised but one
[targets, d] buffer per layer and the 3B seed rows.  The whole forward is one
autograd node with a hand-written backward: per layer >= 1 one
mirec_fanout_resmean_bwd per pair (every row of a layer's input is one
target's self row or one slot's child row, exactly once: plain stores, no
atomics), then layer 0 as three row groups of the sorted table gradient
(graphsage.TableGrad) and the fused Adam on top.  A step repeats bitwise.
FUSED_HOP = False runs the same model on the kernels GraphSAGE has
(_TableTerms with its leaf mean, _FanoutMean, torch adds), with the same
hash, seeds and element indices: the cross-check and the benchmark's
baseline.

Inference — a deliberate deviation.  ``propagated`` applies the training
recurrence on the full graph: x(l+1) = x(l) + mean over every CSR entry of row
i of x(l) (a multi-edge counts once per entry, an isolated row's mean is 0),
out = sum_l x(l) / (L + 1), no dropout.  The reference's getUsersRating
(:363-392) resets its accumulators inside the layer loop and so returns (2
x(L) - x(L-1)) / (L + 1), which is not the quantity the loss trains.  It runs
on graphsage.csr_mean (the CSR propagation kernel) plus torch adds: no new
kernel there.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from . import engine as _engine
from ._lib import check, lib
from .graphsage import SampleTree, TreeModel, _FanoutMean, _TableTerms, csr_mean
from .rows import slice_norms2

# The leaf-gather form on csrc/lightsage.hip (True) or the composition of the
# kernels GraphSAGE has (False).  Measured at the C3 shape:
# the fused form is the faster one.
FUSED_HOP = True


class _Plan:
    """The launches of one tree: layer 0's concatenated ids and, per layer i
    >= 1, (target group, rows, self offset, child offset, child ids, k) with
    the offsets into the previous layer's buffer, whose groups lie in group
    order."""

    def __init__(self, tree: SampleTree, L: int, sizes):
        groups = tree.groups
        for (gi, hop), ci in tree.children.items():
            if groups[ci][0].numel() != groups[gi][0].numel() * int(sizes[hop - 1]):
                raise ValueError("LightSAGE: a child group is not fanout x its parent group")
        self.L = L
        self.targets = []   # per layer: its target groups, ascending
        self.offset = []    # per layer: {group: first row in the layer's output}
        self.rows = []      # per layer: rows of the output
        for i in range(L):
            tg = [gi for gi, (_, dep) in enumerate(groups) if dep <= L - 1 - i]
            off, n = {}, 0
            for gi in tg:
                off[gi] = n
                n += groups[gi][0].numel()
            self.targets.append(tg)
            self.offset.append(off)
            self.rows.append(n)
        t0 = self.targets[0]
        self.k0 = int(sizes[L - 1])
        self.self_ids = _cat([groups[gi][0] for gi in t0])
        self.child_ids = _cat([groups[tree.children[(gi, L)]][0] for gi in t0])
        self.seed_ids = groups[0][0]
        self.pairs = [None]
        for i in range(1, L):
            hop = L - i
            prev = self.offset[i - 1]
            self.pairs.append([(gi, groups[gi][0].numel(), prev[gi],
                                prev[tree.children[(gi, hop)]],
                                groups[tree.children[(gi, hop)]][0], int(sizes[hop - 1]))
                               for gi in self.targets[i]])


def _cat(parts):
    return parts[0] if len(parts) == 1 else torch.cat(parts)


class _TreeForward(torch.autograd.Function):
    """emb and the two slice norms from the table, the leaf-gather form."""

    @staticmethod
    def forward(ctx, table, plan: _Plan, p: float, seed_of, sink, norms, n_user: int):
        d = table.shape[1]
        L = plan.L
        st = _lib.stream_handle()
        dev = table.device
        n_seed = plan.seed_ids.numel()
        acc = torch.empty(n_seed, d, dtype=table.dtype, device=dev)
        check(lib.mirec_gather_rows(table.data_ptr(), plan.seed_ids.data_ptr(), n_seed, d,
                                    acc.data_ptr(), st), "gather_rows")
        x = torch.empty(plan.rows[0], d, dtype=table.dtype, device=dev)
        check(lib.mirec_fanout_resmean_gather(table.data_ptr(), plan.self_ids.data_ptr(),
                                              plan.child_ids.data_ptr(), plan.rows[0], plan.k0, d,
                                              float(p), ctypes.c_uint64(seed_of(0, 0)),
                                              x.data_ptr(), st), "fanout_resmean_gather")
        acc += x[:n_seed]          # group 0 is the first target group of every layer
        for i in range(1, L):
            new = torch.empty(plan.rows[i], d, dtype=table.dtype, device=dev)
            off = plan.offset[i]
            for gi, n_t, so, co, valid, k in plan.pairs[i]:
                check(lib.mirec_fanout_resmean(x[so:].data_ptr(), x[co:].data_ptr(),
                                               valid.data_ptr(), n_t, k, d, float(p),
                                               ctypes.c_uint64(seed_of(gi, i)),
                                               new[off[gi]:].data_ptr(), st), "fanout_resmean")
            x = new
            acc += x[:n_seed]
        acc *= 1.0 / (L + 1)
        norms2 = slice_norms2(table, n_user) if norms is None else norms.view(2)
        ctx.save_for_backward(table, norms2)
        ctx.cfg = (plan, float(p), seed_of, sink)
        ctx.set_materialize_grads(False)
        return acc, norms2

    @staticmethod
    def backward(ctx, g_emb, g_norms):
        table, norms2 = ctx.saved_tensors
        plan, p, seed_of, sink = ctx.cfg
        L, d = plan.L, table.shape[1]
        st = _lib.stream_handle()
        if g_norms is None:
            sink.coef.zero_()
        else:
            check(lib.mirec_norm_coef(g_norms.contiguous().data_ptr(), 1, norms2.data_ptr(), 1, 2,
                                      sink.coef.data_ptr(), st), "norm_coef")
        if g_emb is None:
            sink.skip()
            return (sink.materialize(table) if sink.dense else None), None, None, None, None, \
                None, None
        ge = g_emb * (1.0 / (L + 1))       # the gradient of every x(i)_0 through the mean
        n_seed = ge.shape[0]
        g = ge                             # gradient of layer L - 1's output (group 0 alone)
        for i in range(L - 1, 0, -1):
            off = plan.offset[i]
            gin = torch.empty(plan.rows[i - 1], d, dtype=ge.dtype, device=ge.device)
            for gi, n_t, so, co, valid, k in plan.pairs[i]:
                check(lib.mirec_fanout_resmean_bwd(g[off[gi]:].data_ptr(), valid.data_ptr(), n_t,
                                                   k, d, p, ctypes.c_uint64(seed_of(gi, i)),
                                                   gin[so:].data_ptr(), gin[co:].data_ptr(), st),
                      "fanout_resmean_bwd")
            gin[:n_seed] += ge             # x(i)_0's own term of the layer mean
            g = gin
        sink.accumulate([(plan.self_ids, g, 1, 0, 0.0, 0),
                         (plan.child_ids, g, plan.k0, 1, p, seed_of(0, 0)),
                         (plan.seed_ids, ge, 1, 0, 0.0, 0)])
        return (sink.materialize(table) if sink.dense else None), None, None, None, None, None, \
            None


class LightSAGE(TreeModel):
    HEAVY_SLICE = 1  # all_param = 2 |I| + |U| (lightsage.py:292-303)

    def __init__(self, config: dict, dataset):
        super().__init__(config, dataset)
        deg = torch.from_numpy(self.graph.degree()).to(self.device).float()
        self._mean_dinv = torch.where(deg > 0, 1.0 / deg.clamp(min=1), torch.zeros_like(deg))
        # the table steps through the fused kernel from the pending sorted
        # gradient (TableGrad.adam), which leaves the slice norms for the next
        # forward, as GraphSAGE's
        self._table_state = self.optims.states[0]
        self._tg.dense = False
        self._norm_cache = None

    def build_layers(self):
        """No layer holds a parameter."""
        if self.latent_dim % 4 != 0:
            raise ValueError("LightSAGE: recdim must be a multiple of 4")
        if any(k < 1 for k in self.sizes):
            raise ValueError("LightSAGE: every fanout must be at least 1")

    # ------------------------------------------------------------- forward
    def forward(self, tree: SampleTree, dropout_seed: int | None = None) -> torch.Tensor:
        """Seed embeddings: the mean of the seeds' rows over layers 0..L."""
        L = self.num_layers
        if len(tree.groups) != len(SampleTree.canonical_layout(L)[0]):
            raise ValueError("LightSAGE: the tree does not have the model's depth")
        p = self.dropout_p if (self.training and dropout_seed is not None) else 0.0

        def seed_of(gi, i):
            return 0 if p == 0.0 else (dropout_seed * 1_000_003 + gi * 131 + i) & ((1 << 64) - 1)

        plan = _Plan(tree, L, self.sizes)
        if FUSED_HOP:
            emb, norms2 = _TreeForward.apply(self._table, plan, p, seed_of, self._tg,
                                             self._cached_norms(), self.n_user)
            self._slice_norms2 = norms2
            return emb
        return self._forward_composed(tree, plan, p, seed_of)

    def _forward_composed(self, tree, plan, p, seed_of):
        """The same forward on GraphSAGE's kernels: the table node gathers the
        layer-0 targets' rows and takes the leaf mean (one leaf group: the
        concatenated children, layer 0's single seed), then per pair
        _FanoutMean and a torch add."""
        L = self.num_layers
        groups = tree.groups
        t0 = plan.targets[0]
        leaves = ((plan.child_ids, plan.k0, p, seed_of(0, 0)),)
        # the seeds' rows twice: as layer 0's self rows and as x0_0 of the mean
        ids = torch.cat([plan.self_ids, plan.seed_ids])
        rows, x0, norms2, aggr = _TableTerms.apply(
            self._table, ids, self.n_user, leaves, self._tg, self._cached_norms(),
            [plan.self_ids.numel(), plan.seed_ids.numel()])
        self._slice_norms2 = norms2
        x = rows + aggr
        h = dict(zip(t0, x.split([groups[gi][0].numel() for gi in t0])))
        acc = x0 + h[0]
        for i in range(1, L):
            hop = L - i
            new = {}
            for gi in plan.targets[i]:
                ci = tree.children[(gi, hop)]
                new[gi] = h[gi] + _FanoutMean.apply(h[ci], groups[ci][0], self.sizes[hop - 1], p,
                                                    seed_of(gi, i))
            h = new
            acc = acc + h[0]
        return acc * (1.0 / (L + 1))

    # ------------------------------------------------------------ training
    def table_grad_dense(self) -> torch.Tensor:
        """The id table's gradient after a backward (before the step)."""
        if self._table.grad is not None:
            return self._table.grad
        if not self._tg.pending:
            raise RuntimeError("no pending table gradient")
        return self._tg.materialize(self._table.detach())

    def _norm_token(self):
        return (self._table._version, _engine._raw_writes)

    def _cached_norms(self):
        c = self._norm_cache
        if c is not None and c[1] == self._norm_token():
            return c[0]
        self._norm_cache = None
        return None

    @torch.no_grad()
    def optimizer_step(self):
        """Adam of the table through the fused kernel from the pending sorted
        gradient (the non-dense form; it leaves the updated slices' norms for
        the next forward), or torch-side when the gradient was materialised."""
        if self._table.grad is not None or not self._tg.pending:
            self.optims.step()
            self._tg.pending = False
            return
        norms = torch.empty(2, device=self.device)
        self._tg.adam(self._table_state, norms)
        _engine._note_raw_write()
        self._norm_cache = (norms, self._norm_token())

    # ----------------------------------------------------------- inference
    @torch.no_grad()
    def propagated(self) -> torch.Tensor:
        """sum_l x(l) / (L + 1) with x(l+1) = x(l) + mean over every neighbour
        of x(l) (see the module docstring: not the reference's accumulator)."""
        x = self._table.detach().contiguous()
        out = x.clone()
        for _ in range(self.num_layers):
            agg = torch.empty_like(x)
            csr_mean(self.graph, self._mean_dinv, x, agg)
            x = agg.add_(x)
            out += x
        return out.mul_(1.0 / (self.num_layers + 1))
