"""The reference's 'tgrec' model (model/tgrec.py) on the HIP engine:
the trainer surface and sampler of the sampled-tree base class
(graphsage.TreeModel), the hop a dot-product attention layer — TransformerConv(d, d // heads, heads=heads, root_weight=True),
tgrec.py:161-171 (heads = 8 there).

In scope: the sampled-tree forward (tgrec.py:280-292: per layer the conv, ReLU
except after the last layer, the target rows kept, then dropout on the kept
rows — after the last layer too, so in training the seed embeddings are
dropped out), the BPR loss with the reference's parameter-norm term
(:294-306), OneEpoch, and the full-graph inference of getUsersRating
(:366-382: every neighbour, ReLU between layers, no dropout).  Out of scope,
as in graphsage.py and gnn.py: the proprietary feature and text towers — the
initial node embedding is the id embedding alone, one [N, d] table — and
'tgrec2' / 'tgsrec' (time encodings), beta gating, edge features, attention
dropout, data parallelism and HIP-graph capture.

Tree layout: graphsage.SampleTree.  Layer i (hop L - i) updates every group
of depth <= L-1-i (the targets) from its hop-(L-i) child group, the groups of
depth == L-i (the children); the two sets are disjoint (a group of depth ==
hop is nobody's target at that hop, SampleTree.canonical_layout).  Per layer
the children go through ONE stacked GEMM [lin_key ; lin_value], the targets
through ONE stacked GEMM [lin_query ; lin_skip], and every (target group,
child group) pair is one mirec_fanout_tattn launch (tconv.fanout_tattn) that
reads the halves of the two GEMM outputs in place.

Loss: mean softplus(<u,n> - <u,p>) + decay * all_param / B.  The reference
accumulates all_param = 2 * all_param + |p| over the parameters whose name
contains "embedding", in registration order item_feature_embeddings,
user_feature_embeddings, word_embedding; in scope the item and user slices of
the id table stand in for the first two, so all_param = 2 |I|_2 + |U|_2 — the
opposite order to 'gnn' — and the attention parameters carry no norm term.

The table's rows come from one gather and its gradient from the sorted row
sums of graphsage.TableGrad in its dense form (a fixed summation order; the
attention backward is plain stores, so a step repeats bitwise; Adam then runs
over every parameter with AdamGroup).  All of that — the sampler, the step,
the loss, the inference loop over ``TransformerHop.full`` (mirec_csr_tattn:
every neighbour plus the skip row, tgrec.py:366-382) — is
graphsage.TreeModel's; this module adds the hop, the gather and the forward.
"""
from __future__ import annotations

import torch

from .graphsage import SampleTree, TreeModel, _TableTerms
from .tconv import TransformerHop

MAX_TABLE_OUTPUTS = 8  # MIREC_TABLE_GRAD_MAX_GROUPS: row groups of one table gradient


def _cat(parts):
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def _split(x, sizes):
    return [x] if len(sizes) == 1 else list(x.split(sizes))


class TGRec(TreeModel):
    HOP, HEADS = TransformerHop, 8  # tgrec.py:162
    HEAVY_SLICE = 1  # all_param = 2 |I| + |U| (tgrec.py:294-306)

    def _gather(self, tree: SampleTree):
        """The tree's table rows: (rows per group, rows of the leaf groups as
        they lie, rows of the other groups as they lie).  Consecutive groups
        on the same side of layer 0 (leaves: its children; the rest: its
        targets) form one output of the table node, so layer 0's two GEMMs
        read the gathered rows without a copy and the rows' gradients arrive
        per run, not as slices of one tensor."""
        groups = tree.groups
        L = self.num_layers
        sizes = [g.numel() for g, _ in groups]
        leaf = [depth == L for _, depth in groups]
        runs = [[0]]
        for gi in range(1, len(groups)):
            if leaf[gi] == leaf[gi - 1]:
                runs[-1].append(gi)
            else:
                runs.append([gi])
        if len(runs) > MAX_TABLE_OUTPUTS:  # deep trees: one output, layer 0 concatenates
            runs = [list(range(len(groups)))]
        ids = torch.cat([g for g, _ in groups])
        splits = [sum(sizes[gi] for gi in run) for run in runs]
        *parts, norms2 = _TableTerms.apply(self._table, ids, self.n_user, (), self._tg, None,
                                           splits)
        self._slice_norms2 = norms2  # (|U|, |I|), consumed by loss() / loss_fused()
        h = [None] * len(groups)
        for run, part in zip(runs, parts):
            for gi, rows in zip(run, _split(part, [sizes[gi] for gi in run])):
                h[gi] = rows
        if len(runs) == 1 and len(groups) > 1:
            return h, None, None
        return (h, _cat([p for run, p in zip(runs, parts) if leaf[run[0]]]),
                _cat([p for run, p in zip(runs, parts) if not leaf[run[0]]]))

    def forward(self, tree: SampleTree, dropout_seed: int | None = None) -> torch.Tensor:
        """Seed embeddings h^(L) for a sampled tree (tgrec.py:280-292)."""
        L = self.num_layers
        p = self.dropout_p if (self.training and dropout_seed is not None) else 0.0
        groups = tree.groups
        h, x_leaf, x_rest = self._gather(tree)
        for i, conv in enumerate(self.convs):
            hop = L - i
            kids = [gi for gi, (_, depth) in enumerate(groups) if depth == hop]
            tgts = [gi for gi, (_, depth) in enumerate(groups) if depth <= hop - 1]
            if i == 0 and x_leaf is not None:
                x_kv, x_qs = x_leaf, x_rest
            else:
                x_kv, x_qs = _cat([h[gi] for gi in kids]), _cat([h[gi] for gi in tgts])
            kv = dict(zip(kids, _split(conv.project_kv(x_kv), [h[gi].shape[0] for gi in kids])))
            qs = dict(zip(tgts, _split(conv.project_qs(x_qs), [h[gi].shape[0] for gi in tgts])))
            outs = []
            for gi in tgts:
                ci = tree.children[(gi, hop)]
                out = conv.attend(kv[ci], qs[gi], groups[ci][0], self.sizes[hop - 1])
                outs.append(out.relu() if i != L - 1 else out)
            if p > 0.0:
                # after the layer, on the kept rows: one mask per (step, layer)
                # over the layer's target groups in group order
                outs = _split(self._dropout(_cat(outs), p, dropout_seed * 1_000_003 + i),
                              [o.shape[0] for o in outs])
            new = [None] * len(groups)  # the children are consumed: only targets stay
            for gi, out in zip(tgts, outs):
                new[gi] = out
            h = new
        return h[0]
