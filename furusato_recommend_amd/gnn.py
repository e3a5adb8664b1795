"""The reference's 'gnn' model (model/gnn.py) with conv = 'gat' on the HIP
engine: GraphSAGE's trainer surface and sampler, the hop a graph-attention
layer — GATConv(d, d // heads, heads=heads, add_self_loops=True),
gnn.py:196-206 — instead of a mean.

In scope: the sampled-tree forward (gnn.py:394-406: per layer dropout on the
layer's input rows, the conv, ReLU except after the last layer, the target
rows kept), the BPR loss with the reference's parameter-norm term
(:408-420), OneEpoch, and the full-graph inference of getUsersRating
(:480-495).  Out of scope, as in graphsage.py: the proprietary feature and
text towers — the initial node embedding is the id embedding alone, one
[N, d] table — and conv in {transformer, ggnn, gcn, sage}, attention dropout,
data parallelism and HIP-graph capture.

Tree layout: graphsage.SampleTree.  Layer i (hop L - i) updates every group
of depth <= L-1-i from its hop-(L-i) child group, so the groups of depth <=
L-i are live; they are projected once per layer, all in one GEMM (at layer 0
that is the whole gathered tree), and every (target group, child group) pair
is one mirec_fanout_gat launch (gat.fanout_gat).

Loss: mean softplus(<u,n> - <u,p>) + decay * all_param / B.  The reference
accumulates all_param = 2 * all_param + |p| over the parameters whose name
contains "embedding"; in scope those are user_id_embedding, then
item_id_embedding, so all_param = 2 |U|_2 + |I|_2 — the attention layers'
parameters carry no norm term.

The table's rows come from one gather and its gradient from the sorted row
sums of graphsage.TableGrad in its dense form (a fixed summation order, so a
step repeats bitwise; Adam then runs over every parameter with AdamGroup).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import check, lib
from .engine import AdamGroup, AdamState
from .gat import GATHop
from .graph import DEFAULT_SPLIT, Graph, positive_probs
from .graphsage import GraphSAGE, SampleTree, TableGrad, _BWD_ON_CALLER, _SageLoss, _TableTerms

CONVS = ("gat",)


class GNN(nn.Module):
    def __init__(self, config: dict, dataset):
        super().__init__()
        self.config = config
        conv = config.get("conv", "gat")
        if conv not in CONVS:
            raise ValueError(f"GNN: conv={conv!r} is not supported (supported: "
                             f"{', '.join(CONVS)})")
        self.n_user = self.num_users = int(dataset.n_users)
        self.m_item = self.num_items = int(dataset.m_items)
        self.latent_dim = d = int(config.get("recdim", 128))
        self.num_layers = L = int(config.get("layer", 2))
        self.heads = H = int(config.get("heads", 4))
        k = int(config.get("num_neighbors", 5))
        self.sizes = [int(s) for s in config.get("fanouts", [k] * L)]
        if len(self.sizes) != L:
            raise ValueError("fanouts must have one size per layer")
        if H < 1 or d % (4 * H) != 0:
            raise ValueError("recdim must be a multiple of 4 * heads")
        if H > 8 or d > 256 or not all(1 <= s <= 64 for s in self.sizes):
            raise ValueError("GNN (gat): heads <= 8, recdim <= 256, fanouts in 1..64")
        self.dropout_p = float(config.get("dropout_p", 0.2))  # gnn.py:59
        if not 0.0 <= self.dropout_p < 1.0:
            raise ValueError("dropout_p must lie in [0, 1)")
        self.fanout_replace = bool(config.get("fanout_replace", False))
        self.device = torch.device(config.get("device", "cuda:0"))
        if self.device.type != "cuda":
            raise RuntimeError("GNN (furusato_recommend_amd) runs on a HIP device only")
        n = self.n_user + self.m_item
        # one [N, d] table; the reference's two id tables are views into it
        self._table = nn.Parameter(torch.empty(n, d, device=self.device))
        self.convs = nn.ModuleList([GATHop(d, H, d // H, device=self.device) for _ in range(L)])
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

    # the sampler and the trainer's helpers are GraphSAGE's own
    sample_tree = GraphSAGE.sample_tree
    sample = GraphSAGE.sample
    OneEpoch = GraphSAGE.OneEpoch
    _seed_nodes = GraphSAGE._seed_nodes
    eval_ratings = GraphSAGE.eval_ratings
    getUsersRating = GraphSAGE.getUsersRating

    # ------------------------------------------------------------- forward
    def _dropout(self, x: torch.Tensor, p: float, seed: int) -> torch.Tensor:
        if p == 0.0:
            return x
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed & ((1 << 62) - 1))
        keep = torch.rand(x.shape, generator=gen, device=x.device) >= p
        return x * keep.to(x.dtype).mul_(1.0 / (1.0 - p))

    def forward(self, tree: SampleTree, dropout_seed: int | None = None) -> torch.Tensor:
        """Seed embeddings h^(L) for a sampled tree (gnn.py:394-406)."""
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

    # ---------------------------------------------------------------- loss
    def loss(self, user_emb, pos_emb, neg_emb):
        """gnn.py:408-420: mean softplus(neg - pos) + decay * (2 |U| + |I|) / B
        (see the module docstring for the norm term)."""
        pos_scores = torch.sum(user_emb * pos_emb, dim=1)
        neg_scores = torch.sum(user_emb * neg_emb, dim=1)
        n2 = self._slice_norms2
        self._slice_norms2 = None
        if n2 is None:
            nu, ni = self._table[: self.n_user].norm(2), self._table[self.n_user:].norm(2)
        else:
            nu, ni = n2[0], n2[1]
        all_param = (nu + nu + ni) / user_emb.size(0)
        return torch.mean(F.softplus(neg_scores - pos_scores)) + all_param * self.config["decay"]

    def loss_fused(self, emb: torch.Tensor) -> torch.Tensor:
        """loss() on the forward's seed embeddings [u ; p ; n] in two launches
        (graphsage._SageLoss with no small parameters: weights 2 and 1)."""
        n2 = self._slice_norms2
        if n2 is None or not emb.is_contiguous() or emb.shape[1] % 4:
            B = emb.shape[0] // 3
            return self.loss(emb[:B], emb[B:2 * B], emb[2 * B:])
        self._slice_norms2 = None
        return _SageLoss.apply(emb, n2, float(self.config["decay"]))

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
        """Full-graph inference (gnn.py:480-495): per layer the projection,
        the attention over ALL neighbours of every node and its self loop
        (mirec_csr_gat), ReLU except after the last layer; no dropout."""
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
