"""The reference's 'tgrec' model (model/tgrec.py) on the HIP engine:
GraphSAGE's trainer surface and sampler, the hop a dot-product attention
layer — TransformerConv(d, d // heads, heads=heads, root_weight=True),
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
over every parameter with AdamGroup).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .engine import AdamGroup, AdamState
from .gnn import GNN
from .graph import DEFAULT_SPLIT, Graph, positive_probs
from .graphsage import GraphSAGE, SampleTree, TableGrad, _BWD_ON_CALLER, _SageLoss, _TableTerms
from .tconv import TransformerHop

MAX_TABLE_OUTPUTS = 8  # MIREC_TABLE_GRAD_MAX_GROUPS: row groups of one table gradient


def _cat(parts):
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def _split(x, sizes):
    return [x] if len(sizes) == 1 else list(x.split(sizes))


class TGRec(nn.Module):
    def __init__(self, config: dict, dataset):
        super().__init__()
        self.config = config
        self.n_user = self.num_users = int(dataset.n_users)
        self.m_item = self.num_items = int(dataset.m_items)
        self.latent_dim = d = int(config.get("recdim", 128))
        self.num_layers = L = int(config.get("layer", 2))
        self.heads = H = int(config.get("heads", 8))  # tgrec.py:162
        k = int(config.get("num_neighbors", 5))
        self.sizes = [int(s) for s in config.get("fanouts", [k] * L)]
        if len(self.sizes) != L:
            raise ValueError("fanouts must have one size per layer")
        if H < 1 or d % (4 * H) != 0:
            raise ValueError("recdim must be a multiple of 4 * heads")
        if H > 8 or d > 256 or not all(1 <= s <= 64 for s in self.sizes):
            raise ValueError("TGRec: heads <= 8, recdim <= 256, fanouts in 1..64")
        self.dropout_p = float(config.get("dropout_p", 0.2))  # tgrec.py: nn.Dropout(0.2)
        if not 0.0 <= self.dropout_p < 1.0:
            raise ValueError("dropout_p must lie in [0, 1)")
        self.fanout_replace = bool(config.get("fanout_replace", False))
        self.device = torch.device(config.get("device", "cuda:0"))
        if self.device.type != "cuda":
            raise RuntimeError("TGRec (furusato_recommend_amd) runs on a HIP device only")
        n = self.n_user + self.m_item
        # one [N, d] table; the reference's two id tables are views into it
        self._table = nn.Parameter(torch.empty(n, d, device=self.device))
        self.convs = nn.ModuleList([TransformerHop(d, H, d // H, device=self.device)
                                    for _ in range(L)])
        with torch.no_grad():
            nn.init.normal_(self._table, std=0.1)  # GraphSAGE's id-table init
        self.graph = Graph.from_interactions(dataset.trainUser, dataset.trainItem,
                                             self.n_user, self.m_item, self.device,
                                             split=int(config.get("csr_split", DEFAULT_SPLIT)))
        self.graph.set_positive_probs(positive_probs(config))
        self.optims = AdamGroup([AdamState(p, lr=config["lr"]) for p in self.parameters()])
        self._tg = TableGrad(n, self.n_user, d, self.device)
        self._tg.dense = True  # the gradient is materialised as the table's .grad
        self._step_seed = int(config.get("seed", 2020))
        self._calls = 0
        self._slice_norms2 = None

    @property
    def user_id_embeddings(self):
        return self._table[: self.n_user]

    @property
    def item_id_embeddings(self):
        return self._table[self.n_user:]

    # the sampler and the trainer's helpers are GraphSAGE's own, the seeded
    # dropout mask is GNN's
    sample_tree = GraphSAGE.sample_tree
    sample = GraphSAGE.sample
    OneEpoch = GraphSAGE.OneEpoch
    _seed_nodes = GraphSAGE._seed_nodes
    eval_ratings = GraphSAGE.eval_ratings
    getUsersRating = GraphSAGE.getUsersRating
    _dropout = GNN._dropout

    # ------------------------------------------------------------- forward
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

    # ---------------------------------------------------------------- loss
    def loss(self, user_emb, pos_emb, neg_emb):
        """tgrec.py:294-306: mean softplus(neg - pos) + decay * (2 |I| + |U|) / B
        (see the module docstring for the norm term)."""
        pos_scores = torch.sum(user_emb * pos_emb, dim=1)
        neg_scores = torch.sum(user_emb * neg_emb, dim=1)
        n2 = self._slice_norms2
        self._slice_norms2 = None
        if n2 is None:
            nu, ni = self._table[: self.n_user].norm(2), self._table[self.n_user:].norm(2)
        else:
            nu, ni = n2[0], n2[1]
        all_param = (ni + ni + nu) / user_emb.size(0)
        return torch.mean(F.softplus(neg_scores - pos_scores)) + all_param * self.config["decay"]

    def loss_fused(self, emb: torch.Tensor) -> torch.Tensor:
        """loss() on the forward's seed embeddings [u ; p ; n] in two launches
        (graphsage._SageLoss with no small parameters weighs its two norms 2
        and 1: it is fed (|I|, |U|), the slice norms swapped)."""
        n2 = self._slice_norms2
        if n2 is None or not emb.is_contiguous() or emb.shape[1] % 4:
            B = emb.shape[0] // 3
            return self.loss(emb[:B], emb[B:2 * B], emb[2 * B:])
        self._slice_norms2 = None
        return _SageLoss.apply(emb, n2.flip(0), float(self.config["decay"]))

    # ------------------------------------------------------------ training
    @torch.no_grad()
    def optimizer_step(self):
        self.optims.step()
        self._tg.pending = False

    def stageOne(self, users, pos, neg, tree: SampleTree | None = None):
        """One BPR step: sample the tree over [users ; pos ; neg] (or take
        ``tree``), forward, loss, backward, Adam over every parameter."""
        seed = self._step_seed * 7919 + self._calls
        self._calls += 1
        for p in self.parameters():
            p.grad = None
        if tree is None:
            tree = self.sample_tree(self._seed_nodes(users, pos, neg), seed)
        emb = self.forward(tree, dropout_seed=seed if self.training else None)
        loss = self.loss_fused(emb)
        with _BWD_ON_CALLER():
            loss.backward()
        self.optimizer_step()
        return loss.detach()

    # ----------------------------------------------------------- inference
    @torch.no_grad()
    def propagated(self) -> torch.Tensor:
        """Full-graph inference (tgrec.py:366-382): per layer the four
        projections (two stacked GEMMs), the attention of every node over ALL
        its neighbours plus its skip row (mirec_csr_tattn), ReLU except after
        the last layer; no dropout."""
        x = self._table.detach()
        for i, conv in enumerate(self.convs):
            x = conv.full(self.graph, x)
            if i != self.num_layers - 1:
                x = x.relu_()
        return x

    @torch.no_grad()
    def eval_embeddings(self):
        """(user rows, item rows) of one full-graph propagation: the operands
        of the streamed evaluation (evaluate.score_topk / evaluate_ranked)."""
        out = self.propagated()
        return out[: self.n_user], out[self.n_user:]
