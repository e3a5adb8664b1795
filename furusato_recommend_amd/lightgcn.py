"""LightGCN with the reference's model-class surface, on the HIP engine.

Drop-in for ``model.lgcn.LightGCN`` (model/lgcn.py:44-151): same constructor
``(config, dataset)``, same methods (``forward``, ``getEmbedding``,
``bpr_loss``, ``getUsersRating``, ``stageOne``, ``OneEpoch``) and the same
``state_dict`` key ``all_embedding.weight`` [(n_users + m_items), recdim], so
reference checkpoints load unchanged.

Two execution paths, both on libmirec:
  * ``stageOne`` / ``OneEpoch`` — the training hot path: the fused engine
    step (engine.PropagationEngine.train_step), no autograd graph, Adam fused
    into the last backward layer.
  * ``forward`` / ``bpr_loss`` — differentiable: propagation is an
    autograd.Function whose backward is the same HIP SpMM (Â is symmetric),
    for callers that build their own loss.

``config["loss"] = "ssm"`` trains with the sampled-softmax loss instead of
BPR: ``config["neg_size"]`` negatives per positive and the temperature
``config["ssm_temp"]`` (engine.PropagationEngine.train_step_ssm, DESIGN.md
§18); ``stageOne`` / ``OneEpoch`` / ``sample`` then carry ``neg`` of shape
[n, neg_size], and ``softmax_loss`` is the differentiable form.
``LightGCNSSM`` (lgcnssm.py, 'lgnssm') is this class with that default.
``config["neg_shared"] = M`` (with the "ssm" loss) draws one set of M
negatives per batch instead, shared by all its pairs (train_step_ssm_shared,
DESIGN.md §19): ``stageOne`` takes ``neg`` [M], ``OneEpoch`` and ``sample``
one set per batch, [ceil(n / bpr_batch_size), M].

``rAdjGCN`` (radj.py) is this class on a graph with the r-adjusted
normalisation; ``LightGCN`` itself ignores ``config["r"]``, as the
reference's 'lgn' does (model/lgcn.py never reads it).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .engine import (AdamState, PropagationEngine, check, sample_pairs, sample_shared,
                     sample_triples)
from .graph import DEFAULT_SPLIT, Graph, positive_probs


class _Propagate(torch.autograd.Function):
    """out = (Σ_{l=0..L} Â^l E)/(L+1) with a HIP backward (Horner, dense seed)."""

    @staticmethod
    def forward(ctx, emb, engine: PropagationEngine, dropout=None):
        ctx.engine = engine
        ctx.dropout = dropout  # (keep_prob, seed) of THIS forward, or None
        if dropout is None:
            return engine.forward(emb.contiguous()).clone()
        engine.set_dropout(*dropout)
        try:
            return engine.forward(emb.contiguous()).clone()
        finally:
            engine.set_dropout(None)

    @staticmethod
    def backward(ctx, grad_out):
        eng = ctx.engine
        L = eng.L
        d = (grad_out.contiguous() / float(L + 1))
        if L == 0:
            return d, None, None
        g = d
        # the transposed mask of this node's own forward, whatever the engine
        # has run since
        if ctx.dropout is not None:
            eng.set_dropout(*ctx.dropout)
        try:
            for _ in range(L):
                nxt = torch.empty_like(d)
                eng.propagate_accumulate(g, d, nxt, transposed=True)
                g = nxt
        finally:
            eng.set_dropout(None)
        return g, None, None


def _config_get(config, *keys, default=None):
    for k in keys:
        if k in config:
            return config[k]
    return default


class LightGCN(nn.Module):
    """model/lgcn.py:44-151 on MI355X.  ``config["r"]`` is ignored here (the
    reference's 'lgn' ignores it too): the normalisation is deg^-1/2 on both
    sides; ``rAdjGCN`` is the model that reads it."""

    edge_dropout_supported = True  # config["dropout"]; rAdjGCN refuses it
    default_loss = "bpr"           # config["loss"] when absent; LightGCNSSM: "ssm"

    def _graph_r(self, config) -> float:
        """The r of the graph's normalisation 1 / (deg_j^r · deg_i^(1−r))."""
        return 0.5

    def __init__(self, config: dict, dataset):
        super().__init__()
        self.dataset = dataset
        self.config = config
        self.num_users = int(dataset.n_users)
        self.num_items = int(dataset.m_items)
        self.latent_dim = int(_config_get(config, "recdim", "latent_dim_rec", default=64))
        self.num_layers = int(_config_get(config, "layer", "lightGCN_n_layers", default=3))
        self.device = torch.device(config.get("device", "cuda:0"))
        if self.device.type != "cuda":
            raise RuntimeError("LightGCN (furusato_recommend_amd) runs on a HIP device only")
        # config["edge_weight"]: one non-negative weight per training
        # interaction, aligned with dataset.trainUser / trainItem (counts,
        # recency decay, confidence); None = the plain 0/1 graph.  Every path
        # below (stageOne, OneEpoch, forward, getUsersRating, the streamed
        # evaluation, frontier pruning, the fused Adam) then runs weighted:
        # the weights live in the graph's CSR.
        weight = config.get("edge_weight")
        if weight is not None and len(weight) != len(dataset.trainUser):
            raise ValueError(f"config['edge_weight']: {len(weight)} weights for "
                             f"{len(dataset.trainUser)} training interactions")
        # config["dropout"] / config["keep_prob"] (parse.py:16-18, world.py:
        # 38-39; the flat key "keepprob" is accepted too): the original
        # LightGCN's edge dropout (model/MF.py:158-176, 187-194).  While the
        # module is in training mode every step (stageOne, OneEpoch, forward /
        # bpr_loss) runs on a graph whose entries are kept with probability
        # keep_prob and divided by it, one mask per step shared by all layers
        # and by the backward; eval() restores the full graph.
        self.dropout = bool(int(_config_get(config, "dropout", default=0) or 0))
        self.keep_prob = float(_config_get(config, "keep_prob", "keepprob", default=0.6))
        self._drop_step = 0  # steps taken under dropout: the mask sequence's position
        if self.dropout:
            if not (0.0 < self.keep_prob <= 1.0):
                raise ValueError(f"config['keep_prob'] must lie in (0, 1], got {self.keep_prob!r}")
            if weight is not None:
                raise ValueError("config['dropout'] with config['edge_weight']: edge dropout "
                                 "and edge weights are not combined")
            if not self.edge_dropout_supported:
                raise ValueError(f"config['dropout'] with {type(self).__name__}: edge dropout "
                                 "and the r-adjusted normalisation's scales are not combined")
        # config["loss"]: "bpr" (one negative per positive, model/lgcn.py:98-118)
        # or "ssm", the sampled softmax over config["neg_size"] negatives per
        # positive at temperature config["ssm_temp"] (the intent of
        # model/lgcnssm.py, whose neg_size is undefined and whose loss body is
        # still the BPR softplus; DESIGN.md §18 has the definition).
        self.loss_name = str(_config_get(config, "loss", default=self.default_loss))
        if self.loss_name not in ("bpr", "ssm"):
            raise ValueError(f"config['loss'] must be 'bpr' or 'ssm', got {self.loss_name!r}")
        neg_size = _config_get(config, "neg_size", default=1)
        if int(neg_size) != neg_size or int(neg_size) < 1:
            raise ValueError(f"config['neg_size'] must be an integer >= 1, got {neg_size!r}")
        self.neg_size = int(neg_size)
        self.ssm_temp = float(_config_get(config, "ssm_temp", default=1.0))
        if not (self.ssm_temp > 0.0 and self.ssm_temp < float("inf")):
            raise ValueError(f"config['ssm_temp'] must be positive and finite, "
                             f"got {self.ssm_temp!r}")
        if self.loss_name == "bpr":
            self.neg_size = 1  # the BPR loss takes one negative: the key is not read
        # config["neg_shared"] = M: one set of M negatives per batch, shared
        # by all its pairs, in place of neg_size negatives per pair (DESIGN.md
        # §19); absent or None: per-pair negatives as above
        neg_shared = _config_get(config, "neg_shared", default=None)
        if neg_shared is not None:
            if int(neg_shared) != neg_shared or int(neg_shared) < 1:
                raise ValueError(f"config['neg_shared'] must be an integer >= 1, "
                                 f"got {neg_shared!r}")
            if self.loss_name != "ssm":
                raise ValueError("config['neg_shared'] needs config['loss'] = 'ssm', "
                                 f"got {self.loss_name!r}")
            if self.neg_size > 1:
                raise ValueError("config['neg_shared'] with config['neg_size'] > 1: "
                                 "two ways to ask for negatives")
        self.neg_shared = None if neg_shared is None else int(neg_shared)
        self.graph = Graph.from_interactions(dataset.trainUser, dataset.trainItem,
                                             self.num_users, self.num_items, self.device,
                                             split=int(config.get("csr_split", DEFAULT_SPLIT)),
                                             weight=weight, r=self._graph_r(config))
        self.graph.set_positive_probs(positive_probs(config))
        self.__init_weight()
        self.optim = AdamState(self.all_embedding.weight, lr=config["lr"])
        self.engine = PropagationEngine(self.graph, self.latent_dim, self.num_layers,
                                        int(config.get("bpr_batch_size", 2048)),
                                        prune=bool(config.get("prune", True)),
                                        n_neg=self.neg_size, n_shared=self.neg_shared or 0)
        self.engine.loss_name = self.loss_name
        self.engine.edge_dropout = self.keep_prob if self.dropout else None
        self._loss_accum = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.test_item_emb = None

    def __init_weight(self):
        # model/lgcn.py:70-76: Embedding(n_items + n_users, d), N(0, 0.1)
        self.all_embedding = nn.Embedding(self.num_items + self.num_users, self.latent_dim,
                                          device=self.device)
        nn.init.normal_(self.all_embedding.weight, std=0.1)

    # ---------------------------------------------------------- edge dropout
    def dropout_seed(self, step: int) -> int:
        """The mask seed of the ``step``-th training step under dropout
        (counted from 0 over stageOne / OneEpoch batches / training-mode
        forwards alike): PropagationEngine.dropout_seed(config["seed"], step)
        = (seed mod 2^32) * 2^32 + step mod 2^32, config["seed"] defaulting to
        0.  It does not depend on the rank.  mirec_edge_keep_mask with this
        seed and keep_prob restates the step's mask."""
        return PropagationEngine.dropout_seed(int(self.config.get("seed", 0) or 0), step)

    def _next_dropout(self):
        """(keep_prob, seed) of the step about to run, advancing the counter;
        None when dropout is off or the module is in eval mode."""
        if not (self.dropout and self.training):
            return None
        d = (self.keep_prob, self.dropout_seed(self._drop_step))
        self._drop_step += 1
        return d

    # --------------------------------------------------------- reference API
    def forward(self):
        out = _Propagate.apply(self.all_embedding.weight, self.engine, self._next_dropout())
        return out[: self.num_users], out[self.num_users:]

    def getEmbedding(self, users, pos_items, neg_items):
        all_users, all_items = self.forward()
        users_emb = all_users[users]
        pos_emb = all_items[pos_items]
        neg_emb = all_items[neg_items]
        users_emb_ego = self.all_embedding(users)
        pos_emb_ego = self.all_embedding(pos_items + self.num_users)
        neg_emb_ego = self.all_embedding(neg_items + self.num_users)
        return users_emb, pos_emb, neg_emb, users_emb_ego, pos_emb_ego, neg_emb_ego

    def bpr_loss(self, users, pos, neg):
        (users_emb, pos_emb, neg_emb, userEmb0, posEmb0, negEmb0) = self.getEmbedding(
            users.long(), pos.long(), neg.long())
        reg_loss = (0.5 * (userEmb0.norm(2).pow(2) + posEmb0.norm(2).pow(2)
                           + negEmb0.norm(2).pow(2)) / float(len(users)))
        pos_scores = torch.sum(users_emb * pos_emb, dim=1)
        neg_scores = torch.sum(users_emb * neg_emb, dim=1)
        loss = torch.mean(torch.nn.functional.softplus(neg_scores - pos_scores))
        return loss, reg_loss

    def softmax_loss(self, users, pos, neg):
        """The sampled-softmax loss on ``forward()``, differentiable: ``neg``
        is [n, K]; returns (mean_t logsumexp(s+_t, s_t,.) - s+_t, reg_loss)
        with s = <u, i> / ssm_temp and reg_loss = 1/2 (|E_u|^2 + |E_p|^2 +
        |E_neg|^2) / n over the gathered ego rows (a negative drawn twice
        counts twice), as ``bpr_loss`` returns its pair.  What
        model/lgcnssm.py:98-118 evidently means: its body is still the BPR
        softplus, which this equals for K = 1, ssm_temp = 1.

        Under config["neg_shared"] ``neg`` is the shared list [M]: the
        softmax of pair t runs over s+_t and the candidates that are neither
        a training positive of its user nor its ``pos`` (the mask of
        mirec_ssm_shared_mask), and reg_loss counts each shared slot once."""
        if self.neg_shared is not None:
            return self._softmax_loss_shared(users, pos, neg)
        users, pos, neg = users.long(), pos.long(), self._neg2d(neg, len(users)).long()
        all_users, all_items = self.forward()
        ue, pe, ne = all_users[users], all_items[pos], all_items[neg]
        u0 = self.all_embedding(users)
        p0 = self.all_embedding(pos + self.num_users)
        n0 = self.all_embedding(neg + self.num_users)
        reg_loss = (0.5 * (u0.norm(2).pow(2) + p0.norm(2).pow(2) + n0.norm(2).pow(2))
                    / float(len(users)))
        sp = torch.sum(ue * pe, dim=1) / self.ssm_temp
        sn = torch.einsum("bd,bkd->bk", ue, ne) / self.ssm_temp
        lse = torch.logsumexp(torch.cat([sp[:, None], sn], dim=1), dim=1)
        return torch.mean(lse - sp), reg_loss

    def _softmax_loss_shared(self, users, pos, shared):
        shared = self._shared1d(shared)
        u32, p32, s32 = self._as_i32(users), self._as_i32(pos), self._as_i32(shared)
        B, M = len(u32), len(s32)
        mask = torch.empty(B, M, dtype=torch.uint8, device=self.device)
        from . import _lib
        check(_lib.lib.mirec_ssm_shared_mask(self.graph.csr_ptr(), u32.data_ptr(), B,
                                             p32.data_ptr(), s32.data_ptr(), M, self.num_users,
                                             mask.data_ptr(), _lib.stream_handle()),
              "ssm_shared_mask")
        users, pos, shared = u32.long(), p32.long(), s32.long()
        all_users, all_items = self.forward()
        ue, pe, ne = all_users[users], all_items[pos], all_items[shared]
        u0 = self.all_embedding(users)
        p0 = self.all_embedding(pos + self.num_users)
        n0 = self.all_embedding(shared + self.num_users)
        reg_loss = (0.5 * (u0.norm(2).pow(2) + p0.norm(2).pow(2) + n0.norm(2).pow(2))
                    / float(B))
        sp = torch.sum(ue * pe, dim=1) / self.ssm_temp
        sn = (ue @ ne.t()) / self.ssm_temp
        sn = sn.masked_fill(mask.bool(), float("-inf"))
        lse = torch.logsumexp(torch.cat([sp[:, None], sn], dim=1), dim=1)
        return torch.mean(lse - sp), reg_loss

    def _shared1d(self, neg):
        """``neg`` as the shared list [neg_shared] of one batch."""
        if not torch.is_tensor(neg):
            neg = torch.as_tensor(neg)
        if neg.dim() != 1 or int(neg.shape[0]) != self.neg_shared:
            raise ValueError(f"neg must have shape [{self.neg_shared}] with "
                             f"config['neg_shared'], got {tuple(neg.shape)}")
        return neg

    def _neg2d(self, neg, n: int):
        """``neg`` as the [n, K] tensor of the sampled-softmax paths
        (K = neg_size; a flat [n] tensor is accepted for K = 1)."""
        if not torch.is_tensor(neg):
            neg = torch.as_tensor(neg)
        if neg.dim() == 1 and self.neg_size == 1:
            neg = neg[:, None]
        if neg.dim() != 2 or tuple(neg.shape) != (n, self.neg_size):
            raise ValueError(f"neg must have shape [{n}, {self.neg_size}] with "
                             f"config['loss'] = 'ssm', got {tuple(neg.shape)}")
        return neg

    @torch.no_grad()
    def propagated(self) -> torch.Tensor:
        """Full layer-mean embeddings [N, D] (no autograd; the engine's
        buffer, valid until the next engine call).  Propagates only when the
        table changed since the last full propagation."""
        return self.engine.forward_cached(self.all_embedding.weight)

    @torch.no_grad()
    def getUsersRating(self, users):
        """model/lgcn.py:120-125.  The reference re-propagates the whole graph
        on every call — once per 10 000-user batch of Trainer.test
        (trainer.py:130); here the propagation is reused while the table is
        unchanged, so an unchanged reference Trainer.test propagates once
        per evaluation."""
        out = self.propagated()
        users_emb = out[users.long()]
        items_emb = out[self.num_users:]
        return torch.matmul(users_emb, items_emb.t())

    @torch.no_grad()
    def eval_ratings(self):
        """users -> rating rows [len(users), m_items] with ONE propagation for
        the whole evaluation (getUsersRating semantics, model/lgcn.py:120-125)."""
        out = self.propagated()
        items = out[self.num_users:]
        return lambda users: out[users.long()] @ items.t()

    def eval_embeddings(self):
        """(user rows [n_users, D], item rows [m_items, D]) of one propagation:
        the operands of the streaming evaluation (evaluate.score_topk)."""
        out = self.propagated()
        return out[: self.num_users], out[self.num_users:]

    def _as_i32(self, t):
        if not torch.is_tensor(t):
            t = torch.as_tensor(t)
        return t.to(device=self.device, dtype=torch.int32, non_blocking=True).contiguous()

    @torch.no_grad()
    def stageOne(self, user, pos, neg, loss_accum=None):
        """One fused BPR step (model/lgcn.py:127-133); returns the loss tensor.
        With config["loss"] = "ssm": one sampled-softmax step, ``neg`` [n, K];
        with config["neg_shared"]: ``neg`` is the batch's shared list [M]."""
        w = self.all_embedding.weight
        if self.neg_shared is not None:
            return self.engine.train_step_ssm_shared(
                w, self.optim, self._as_i32(user), self._as_i32(pos),
                self._as_i32(self._shared1d(neg)), float(self.config["decay"]), self.ssm_temp,
                loss_accum, dropout=self._next_dropout()).clone()
        if self.loss_name == "ssm":
            neg = self._as_i32(self._neg2d(neg, len(user)))
            return self.engine.train_step_ssm(w, self.optim, self._as_i32(user),
                                              self._as_i32(pos), neg,
                                              float(self.config["decay"]), self.ssm_temp,
                                              loss_accum, dropout=self._next_dropout()).clone()
        return self.engine.train_step(w, self.optim, self._as_i32(user), self._as_i32(pos),
                                      self._as_i32(neg), float(self.config["decay"]),
                                      loss_accum, dropout=self._next_dropout()).clone()

    @torch.no_grad()
    def OneEpoch(self, user, pos, neg):
        """model/lgcn.py:135-151: minibatch loop; mean loss over len//B + 1.

        With config["loss"] = "ssm" a batch is ``bpr_batch_size`` pairs, each
        with its K negatives (``neg`` [n, K]).  model/lgcnssm.py:135-151
        slices ``neg_size * bpr_batch_size`` rows of flat triples instead,
        which cannot be followed: its own sampler never produces such
        triples (and ``neg_size`` is undefined there)."""
        B = int(self.config["bpr_batch_size"])
        n = len(user)
        total_batch = n // B + 1
        if self.neg_shared is not None:
            # one shared set per batch: neg [ceil(n / B), M]
            if not torch.is_tensor(neg):
                neg = torch.as_tensor(neg)
            n_sets = (n + B - 1) // B
            if neg.dim() != 2 or tuple(neg.shape) != (n_sets, self.neg_shared):
                raise ValueError(f"neg must have shape [{n_sets}, {self.neg_shared}] with "
                                 f"config['neg_shared'], got {tuple(neg.shape)}")
            user, pos, neg = self._as_i32(user), self._as_i32(pos), self._as_i32(neg)
            self._loss_accum.zero_()
            for b, i in enumerate(range(0, n, B)):
                self.engine.train_step_ssm_shared(self.all_embedding.weight, self.optim,
                                                  user[i:i + B], pos[i:i + B], neg[b],
                                                  float(self.config["decay"]), self.ssm_temp,
                                                  self._loss_accum,
                                                  dropout=self._next_dropout())
            return self._loss_accum[0] / total_batch
        if self.loss_name == "ssm":
            user, pos = self._as_i32(user), self._as_i32(pos)
            neg = self._as_i32(self._neg2d(neg, n))
            self._loss_accum.zero_()
            for i in range(0, n, B):
                self.engine.train_step_ssm(self.all_embedding.weight, self.optim, user[i:i + B],
                                           pos[i:i + B], neg[i:i + B],
                                           float(self.config["decay"]), self.ssm_temp,
                                           self._loss_accum, dropout=self._next_dropout())
            return self._loss_accum[0] / total_batch
        user, pos, neg = self._as_i32(user), self._as_i32(pos), self._as_i32(neg)
        self._loss_accum.zero_()
        for i in range(0, n, B):
            self.engine.train_step(self.all_embedding.weight, self.optim, user[i:i + B],
                                   pos[i:i + B], neg[i:i + B], float(self.config["decay"]),
                                   self._loss_accum, dropout=self._next_dropout())
        return self._loss_accum[0] / total_batch

    # ------------------------------------------------------------- sampling
    def sample(self, n_triples: int, seed: int, offset: int = 0, shard: int = 0,
               n_shards: int = 1):
        """On-device UniformSample: int32 (users, pos, neg) device tensors;
        with config["loss"] = "ssm" ``neg`` is [n_triples, neg_size]
        (mirec_ssm_sample: the same users, positives and first negatives);
        with config["neg_shared"] = M it is [ceil(n_triples / bpr_batch_size),
        M], one shared set per batch (mirec_shared_sample of the same seed and
        offset), beside mirec_bpr_sample_ex's users and positives."""
        dev = self.device
        u = torch.empty(n_triples, dtype=torch.int32, device=dev)
        p = torch.empty_like(u)
        if self.neg_shared is not None:
            # the BPR sampler's users and positives (its negative is dropped)
            # and one shared set per batch of bpr_batch_size pairs
            n = torch.empty_like(u)
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            sample_triples(self.graph, n_triples, seed, offset, u, p, n, err, shard, n_shards)
            self._sample_err = err
            B = int(self.config.get("bpr_batch_size", 2048))
            n_sets = max(1, (n_triples + B - 1) // B)
            sets = torch.empty(n_sets, self.neg_shared, dtype=torch.int32, device=dev)
            sample_shared(self.num_items, n_sets, self.neg_shared, seed, offset, sets)
            return u, p, sets
        if self.loss_name == "ssm":
            n = torch.empty(n_triples, self.neg_size, dtype=torch.int32, device=dev)
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            sample_pairs(self.graph, n_triples, self.neg_size, seed, offset, u, p, n, err,
                         shard, n_shards)
            self._sample_err = err
            return u, p, n
        n = torch.empty_like(u)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        sample_triples(self.graph, n_triples, seed, offset, u, p, n, err, shard, n_shards)
        self._sample_err = err
        return u, p, n

    def optimizer_state_dict(self):
        """torch.optim.Adam's state_dict of the table, plus (with dropout on)
        ``edge_dropout_step``, the position in the mask sequence."""
        sd = self.optim.state_dict()
        if self.dropout:
            sd["edge_dropout_step"] = int(self._drop_step)
        return sd

    def load_optimizer_state_dict(self, sd: dict) -> None:
        """Restore optimizer_state_dict(): a resumed run continues the Adam
        moments and the mask sequence where the saved one stopped."""
        self.optim.load_state_dict(sd)
        self._drop_step = int(sd.get("edge_dropout_step", 0))
