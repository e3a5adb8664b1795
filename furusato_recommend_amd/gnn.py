"""The reference's 'gnn' model (model/gnn.py) with conv = 'gat' (the default)
or 'ggnn' on the HIP engine: the trainer surface and sampler of the
sampled-tree base class (graphsage.TreeModel), the hop a graph-attention
layer — GATConv(d, d // heads, heads=heads, add_self_loops=True), gnn.py:
196-206 — or a gated one — GatedGraphConv(d, num_layers=1, aggr='mean'): a
GRU cell on (mean of the projected children, the node's row), ggnn.py —
instead of GraphSAGE's mean.

In scope: the sampled-tree forward (gnn.py:394-406: per layer dropout on the
layer's input rows, the conv, ReLU except after the last layer, the target
rows kept), the BPR loss with the reference's parameter-norm term
(:408-420), OneEpoch, and the full-graph inference of getUsersRating
(:480-495).  Out of scope, as in graphsage.py: the proprietary feature and
text towers — the initial node embedding is the id embedding alone, one
[N, d] table — and conv in {transformer, gcn, sage} ('transformer' hops are
the 'tgrec' model's), attention dropout, data parallelism and HIP-graph
capture.

Tree layout: graphsage.SampleTree.  Layer i (hop L - i) updates every group
of depth <= L-1-i from its hop-(L-i) child group, so the groups of depth <=
L-i are live; they are projected once per layer, all in one GEMM (at layer 0
that is the whole gathered tree), and every (target group, child group) pair
is one mirec_fanout_gat launch (gat.fanout_gat).  With conv = 'ggnn' the live
rows are not projected: every pair is one mirec_fanout_mean over the dropped
child rows, and all the layer's targets go through ONE GGNNHop.update on
their concatenation (three GEMMs over the target rows and the GRU gate, the
ReLU fused into it) — no GEMM touches a child row.

Loss: mean softplus(<u,n> - <u,p>) + decay * all_param / B.  The reference
accumulates all_param = 2 * all_param + |p| over the parameters whose name
contains "embedding"; in scope those are user_id_embedding, then
item_id_embedding, so all_param = 2 |U|_2 + |I|_2 — the attention layers'
parameters, and the GRU's, carry no norm term.

The table's rows come from one gather and its gradient from the sorted row
sums of graphsage.TableGrad in its dense form (a fixed summation order, so a
step repeats bitwise; Adam then runs over every parameter with AdamGroup).
All of that — the sampler, the step, the loss, the inference loop over
``GATHop.full`` (mirec_csr_gat: every neighbour and the self loop, gnn.py:
480-495) or ``GGNNHop.full`` (the mean over every neighbour, then the cell) —
is graphsage.TreeModel's; this module adds the hop and the forward.
"""
from __future__ import annotations

import torch

from .gat import GATHop
from .ggnn import GGNNHop
from .graphsage import SampleTree, TreeModel, _TableTerms

CONVS = ("gat", "ggnn")


class GNN(TreeModel):
    HOP, HEADS = GATHop, 4
    HEAVY_SLICE = 0  # all_param = 2 |U| + |I| (gnn.py:408-420)

    def __init__(self, config: dict, dataset):
        conv = config.get("conv", "gat")
        if conv not in CONVS:
            raise ValueError(f"GNN: conv={conv!r} is not supported (supported: "
                             f"{', '.join(CONVS)})")
        super().__init__(config, dataset)

    def build_layers(self):
        self.conv = self.config.get("conv", "gat")
        if self.conv != "ggnn":
            return super().build_layers()
        # no heads; the fanout limits are the mean kernel's (k >= 1)
        d = self.latent_dim
        if d % 4 != 0:
            raise ValueError("GNN: recdim must be a multiple of 4")
        if any(k < 1 for k in self.sizes):
            raise ValueError("GNN: every fanout must be at least 1")
        self.convs = torch.nn.ModuleList([GGNNHop(d, device=self.device)
                                          for _ in range(self.num_layers)])

    def forward(self, tree: SampleTree, dropout_seed: int | None = None) -> torch.Tensor:
        """Seed embeddings h^(L) for a sampled tree (gnn.py:394-406)."""
        if self.conv == "ggnn":
            return self._forward_ggnn(tree, dropout_seed)
        L = self.num_layers
        p = self.dropout_p if (self.training and dropout_seed is not None) else 0.0
        groups = tree.groups
        ids = torch.cat([g for g, _ in groups])
        rows, norms2 = _TableTerms.apply(self._table, ids, self.n_user, (), self._tg, None,
                                         [ids.numel()])
        self._slice_norms2 = norms2  # consumed by loss_fused()
        h = list(rows.split([g.numel() for g, _ in groups]))
        for i, conv in enumerate(self.convs):
            hop = L - i
            live = [gi for gi, (_, depth) in enumerate(groups) if depth <= hop]
            # every live group projected once, in one GEMM (layer 0: the
            # gathered rows as they lie)
            x = rows if i == 0 else torch.cat([h[gi] for gi in live])
            x = self._dropout(x, p, 0 if dropout_seed is None else dropout_seed * 1_000_003 + i)
            z = dict(zip(live, conv.project(x).split([h[gi].shape[0] for gi in live])))
            new = list(h)
            for gi in live:
                if groups[gi][1] > hop - 1:
                    continue
                ci = tree.children[(gi, hop)]
                out = conv.attend(z[ci], z[gi], groups[ci][0], self.sizes[hop - 1])
                new[gi] = out.relu() if i != L - 1 else out
            h = new
        return h[0]

    def _forward_ggnn(self, tree: SampleTree, dropout_seed: int | None) -> torch.Tensor:
        """The same walk with gated hops: per layer the dropout mask over the
        concatenated live rows (children and hidden rows both come from the
        dropped rows), one mean per (target group, child group) pair, and ONE
        update — three GEMMs and the gate, ReLU fused except after the last
        layer — over the layer's target groups together."""
        L = self.num_layers
        p = self.dropout_p if (self.training and dropout_seed is not None) else 0.0
        groups = tree.groups
        ids = torch.cat([g for g, _ in groups])
        rows, norms2 = _TableTerms.apply(self._table, ids, self.n_user, (), self._tg, None,
                                         [ids.numel()])
        self._slice_norms2 = norms2  # consumed by loss_fused()
        h = list(rows.split([g.numel() for g, _ in groups]))
        for i, conv in enumerate(self.convs):
            hop = L - i
            live = [gi for gi, (_, depth) in enumerate(groups) if depth <= hop]
            x = rows if i == 0 else torch.cat([h[gi] for gi in live])
            x = self._dropout(x, p, 0 if dropout_seed is None else dropout_seed * 1_000_003 + i)
            sizes = [h[gi].shape[0] for gi in live]
            xd = dict(zip(live, x.split(sizes)))
            tgts = [gi for gi in live if groups[gi][1] <= hop - 1]
            aggr = [conv.aggregate(xd[tree.children[(gi, hop)]],
                                   groups[tree.children[(gi, hop)]][0], self.sizes[hop - 1])
                    for gi in tgts]
            if tgts == live[:len(tgts)]:  # the targets lie together at the front of x
                x_self = x[:sum(sizes[:len(tgts)])]
            else:
                x_self = torch.cat([xd[gi] for gi in tgts])
            a = aggr[0] if len(aggr) == 1 else torch.cat(aggr)
            out = conv.update(a, x_self, relu=i != L - 1)
            new = list(h)
            for gi, o in zip(tgts, out.split([xd[gi].shape[0] for gi in tgts])):
                new[gi] = o
            h = new
        return h[0]
