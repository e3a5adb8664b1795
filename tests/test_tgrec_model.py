"""The 'tgrec' model (TransformerConv hops) against a float64 torch-autograd
restatement (tests/tattn_common.py: the PyG-style edge-list form over the
tree's per-layer edge lists) on the tiny dataset of tests/test_gnn_model.py,
restated here: 40 users x 15 items, 120 interactions with duplicates, item 14
without interactions, user 39 with a single item; d = 32, H = 8, L = 2,
fanouts [3, 2], B = 8, dropout_p = 0 unless stated.

Tolerance: 1e-4 relative by max-norm per tensor, the project's fp32 bar.
One gradient has no max-norm of its own: lin_key.bias.  Shifting every key of
a target by one vector moves all its logits alike, the softmax does not
change, so that gradient — the column sum of the key rows' gradients — is
identically 0.  It is held to 1e-4 of the largest column sum of the ABSOLUTE
key-row gradients of its layer (the scale of the terms that cancel), taken
from the float64 restatement; the Adam check leaves it out of the sign
comparison, since the sign of a rounding residue is not settled.

The Adam check compares the first step's update D = -lr g / (|g| + eps): for
an element whose |g| is above 1e-3 max |g| (ten times the gradient check's
own absolute tolerance, so its sign is settled) the two updates agree to
1e-3 lr; every update is at most lr in size.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gat_common as gc
from tests import tattn_common as tc

pytestmark = pytest.mark.gpu

NU, MI, D, H, L, FAN, B = 40, 15, 32, 8, 2, [3, 2], 8
LR, DECAY = 1e-2, 0.5
TOL = 1e-4
LINS = ("lin_key", "lin_query", "lin_value", "lin_skip")
PNAMES = ["table"] + [f"convs.{i}.{n}.{w}" for i in range(L) for n in LINS
                      for w in ("weight", "bias")]


class DS:
    def __init__(self):
        rng = np.random.default_rng(40)
        u = rng.integers(0, 39, 107)
        i = rng.integers(0, 14, 107)
        self.trainUser = np.concatenate([u, u[:12], [39]]).astype(np.int64)   # 12 duplicates
        self.trainItem = np.concatenate([i, i[:12], [5]]).astype(np.int64)
        self.n_users, self.m_items = NU, MI


def _cfg(**kw):
    cfg = {"recdim": D, "layer": L, "heads": H, "fanouts": FAN, "lr": LR, "decay": DECAY,
           "dropout_p": 0.0, "device": "cuda:0", "bpr_batch_size": B, "seed": 11}
    cfg.update(kw)
    return cfg


def _model(seed=0, **kw):
    from furusato_recommend_amd.register import MODELS
    torch.manual_seed(seed)
    return MODELS["tgrec"](_cfg(**kw), DS())


def test_dataset_is_what_it_claims():
    ds = DS()
    assert len(ds.trainUser) == 120
    pairs = set(zip(ds.trainUser.tolist(), ds.trainItem.tolist()))
    assert len(pairs) < 120 and 14 not in ds.trainItem and (ds.trainUser == 39).sum() == 1


def _host_tree(ds, seeds, rng, L=L, FAN=FAN):
    """Explicit groups in SampleTree's canonical order: every slot draws its
    own children, without replacement (all neighbours and -1 when the degree
    is below the fanout); a -1 parent has no children."""
    from furusato_recommend_amd.graphsage import SampleTree
    rowptr, col = gc.host_csr(ds.trainUser, ds.trainItem, NU, MI)
    depths, children = SampleTree.canonical_layout(L)

    def draw(parents, k):
        out = np.full((len(parents), k), -1, np.int32)
        for r, p in enumerate(parents):
            if p < 0:
                continue
            nb = col[rowptr[p]:rowptr[p + 1]]
            pick = nb if len(nb) <= k else nb[rng.choice(len(nb), k, replace=False)]
            out[r, :len(pick)] = pick
        return out.reshape(-1)

    groups = [None] * len(depths)
    groups[0] = np.asarray(seeds, np.int32)
    order = sorted(children.items(), key=lambda kv: kv[1])   # child index ascending
    for (gi, hop), ci in order:
        groups[ci] = draw(groups[gi], FAN[hop - 1])
    return groups, depths, children


def _model_params(m):
    return [m._table] + [p for c in m.convs for n in LINS
                         for p in (getattr(c, n).weight, getattr(c, n).bias)]


@pytest.fixture(scope="module")
def setup():
    """One model, one explicit tree, its float64 restatement with gradients."""
    from furusato_recommend_amd.graphsage import SampleTree
    m = _model()
    ds = DS()
    rng = np.random.default_rng(8)
    users = rng.choice(np.unique(ds.trainUser), B)    # users with a positive
    users[0] = 39                                     # the single-item user
    pos = np.array([ds.trainItem[ds.trainUser == u][0] for u in users])
    neg = rng.integers(0, MI, B)
    neg[0] = 14                                       # the item without interactions
    seeds = np.concatenate([users, NU + pos, NU + neg])
    groups, depths, children = _host_tree(ds, seeds, rng)
    assert any((g < 0).any() for g in groups[1:])     # short rows leave empty slots
    k1 = FAN[0]                                       # a seed without any valid child
    assert (groups[children[(0, 1)]].reshape(-1, k1) < 0).all(1).any()
    tree = SampleTree.from_groups([torch.from_numpy(g).cuda() for g in groups], L)
    r = _restate(m, groups, depths, children)
    return dict(r, m=m, ds=ds, tree=tree, triples=(users, pos, neg))


def _restate(m, groups, depths, children, L=L, FAN=FAN):
    """The float64 restatement of a model on an explicit tree: seed rows,
    loss, and the gradient of every parameter (and the scale of the key-row
    gradients per layer, module docstring)."""
    B = len(groups[0]) // 3
    f64 = lambda p: p.detach().double().cpu().requires_grad_(True)  # noqa: E731
    table = f64(m._table)
    convs = [{n: (f64(getattr(c, n).weight), f64(getattr(c, n).bias)) for n in LINS}
             for c in m.convs]
    taps = []
    emb = tc.model_forward(table, convs, groups, depths, children, L, FAN, H, taps=taps)
    u, p, n = emb[:B], emb[B:2 * B], emb[2 * B:]
    soft = F.softplus((u * n).sum(1) - (u * p).sum(1)).mean()
    all_param = 2 * table[NU:].norm(2) + table[:NU].norm(2)       # 2 |I| + |U|
    loss = soft + DECAY * all_param / B
    params = [table] + [t for c in convs for n in LINS for t in c[n]]
    grads = torch.autograd.grad(loss, params + [k for _, k in taps])
    key_scale = [sum(g.abs().sum(0) for (i, _), g in zip(taps, grads[len(params):]) if i == lay)
                 for lay in range(L)]
    return dict(table=table, convs=convs, emb=emb.detach(), loss=float(loss.detach()),
                soft=float(soft.detach()), params=params, grads=grads[:len(params)],
                key_scale=key_scale)


def _rel(got, ref):
    got = got.detach().double().cpu().reshape(-1)
    ref = ref.detach().double().cpu().reshape(-1)
    assert torch.isfinite(got).all()
    return float((got - ref).abs().max() / ref.abs().max())


def _check_grads(m, ref, tag="tgrec"):
    """Every parameter's .grad against the restatement's, 1e-4 by max-norm."""
    names = ["table"] + [f"convs.{i}.{n}.{w}" for i in range(len(m.convs)) for n in LINS
                         for w in ("weight", "bias")]
    for name, p, g in zip(names, _model_params(m), ref["grads"]):
        assert p.grad is not None, name
        if name.endswith("lin_key.bias"):
            # identically 0 (module docstring): held to the scale of its terms
            scale = float(ref["key_scale"][int(name.split(".")[1])].max())
            assert float(g.abs().max()) <= 1e-12 * scale
            r = float(p.grad.detach().double().abs().max()) / scale
        else:
            r = _rel(p.grad, g)
        print(f"[{tag}] grad {name}: rel {r:.2e}")
        assert r <= TOL, (name, r)


def test_forward_loss_and_gradients(setup):
    m = setup["m"]
    m.train()
    for p in m.parameters():
        p.grad = None
    emb = m.forward(setup["tree"], dropout_seed=3)
    assert _rel(emb, setup["emb"]) <= TOL
    loss = m.loss_fused(emb)
    assert abs(float(loss) - setup["loss"]) <= TOL * abs(setup["loss"])
    # the norm term is 2 |I| + |U|: 'gnn''s 2 |U| + |I| would be visibly another loss
    nu, ni = float(setup["table"][:NU].norm(2)), float(setup["table"][NU:].norm(2))
    assert abs(setup["loss"] - (setup["soft"] + DECAY * (2 * ni + nu) / B)) <= 1e-12
    assert abs(DECAY * ((2 * ni + nu) - (2 * nu + ni)) / B) > 100 * TOL * abs(setup["loss"])
    loss.backward()
    assert len(PNAMES) == 1 + 8 * L == len(_model_params(m)) == len(list(m.parameters()))
    _check_grads(m, setup)
    # the unfused loss is the same function
    emb2 = m.forward(setup["tree"], dropout_seed=3)
    l2 = m.loss(emb2[:B], emb2[B:2 * B], emb2[2 * B:])
    assert abs(float(l2) - setup["loss"]) <= TOL * abs(setup["loss"])


def test_three_layers_forward_and_gradients():
    """L = 3: eight groups in four runs (targets, leaves, a target, leaves), so
    layer 0 concatenates two table outputs on each side, and the middle layer
    has two child groups and two target groups."""
    from furusato_recommend_amd.graphsage import SampleTree
    L3, fan, b = 3, [2, 3, 2], 4
    m = _model(seed=2, layer=L3, fanouts=fan, bpr_batch_size=b)
    ds = DS()
    rng = np.random.default_rng(9)
    users = rng.choice(np.unique(ds.trainUser), b)
    pos = np.array([ds.trainItem[ds.trainUser == u][0] for u in users])
    neg = rng.integers(0, MI, b)
    neg[0] = 14
    groups, depths, children = _host_tree(ds, np.concatenate([users, NU + pos, NU + neg]), rng,
                                          L3, fan)
    assert depths == [0, 1, 2, 3, 3, 2, 3, 3] and any((g < 0).any() for g in groups[1:])
    ref = _restate(m, groups, depths, children, L3, fan)
    tree = SampleTree.from_groups([torch.from_numpy(g).cuda() for g in groups], L3)
    m.train()
    emb = m.forward(tree, dropout_seed=3)
    assert _rel(emb, ref["emb"]) <= TOL
    loss = m.loss_fused(emb)
    assert abs(float(loss) - ref["loss"]) <= TOL * abs(ref["loss"])
    loss.backward()
    _check_grads(m, ref, "tgrec L3")


def test_single_table_output_is_the_same_function(setup, monkeypatch):
    """A tree with more runs than the table gradient takes row groups falls
    back to one table output and concatenates at layer 0; forced here by
    lowering the limit."""
    from furusato_recommend_amd import tgrec
    monkeypatch.setattr(tgrec, "MAX_TABLE_OUTPUTS", 1)
    m = _model()
    m.train()
    emb = m.forward(setup["tree"], dropout_seed=3)
    assert _rel(emb, setup["emb"]) <= TOL
    loss = m.loss_fused(emb)
    assert abs(float(loss) - setup["loss"]) <= TOL * abs(setup["loss"])
    loss.backward()
    _check_grads(m, setup, "tgrec one output")


def test_stage_one_is_adam_on_the_restatement(setup):
    m = _model()                                      # same seed: the fixture's parameters
    for a, b in zip(_model_params(m), _model_params(setup["m"])):
        assert torch.equal(a, b)
    before = [p.detach().clone() for p in _model_params(m)]
    users, pos, neg = (torch.from_numpy(x) for x in setup["triples"])
    loss = m.stageOne(users, pos, neg, tree=setup["tree"])
    assert abs(float(loss) - setup["loss"]) <= TOL * abs(setup["loss"])
    ref = [p.detach().clone().requires_grad_(True) for p in setup["params"]]
    opt = torch.optim.Adam(ref, lr=LR)
    for p, g in zip(ref, setup["grads"]):
        p.grad = g.clone()
    opt.step()
    for name, p0, p1, r0, r1, g in zip(PNAMES, before, _model_params(m), setup["params"], ref,
                                       setup["grads"]):
        d_got = (p1.detach() - p0).double().cpu().reshape(-1)
        d_ref = (r1.detach() - r0.detach()).reshape(-1)
        g = g.reshape(-1)
        # p1 - p0 in float32 carries the rounding of p: one ulp of |p| <= 1
        slack = 1e-3 * LR + 2.0 ** -23 * p0.abs().max().item()
        assert d_got.abs().max() <= LR * (1 + 1e-3) + slack, name
        if name.endswith("lin_key.bias"):
            continue                                  # a zero gradient has no settled sign
        settled = g.abs() > 1e-3 * g.abs().max()
        assert settled.any()
        assert (d_got - d_ref)[settled].abs().max() <= slack, name


def test_get_users_rating_is_the_dense_full_graph_form(setup):
    m, ds = setup["m"], setup["ds"]
    rowptr, col = gc.host_csr(ds.trainUser, ds.trainItem, NU, MI)
    dst = np.repeat(np.arange(NU + MI), np.diff(rowptr))
    ei = torch.from_numpy(np.stack([col.astype(np.int64), dst]))
    x = setup["table"].detach()
    for i, c in enumerate(setup["convs"]):
        q, k, v, s = (x @ c[n][0].detach().t() + c[n][1].detach()
                      for n in ("lin_query", "lin_key", "lin_value", "lin_skip"))
        x = tc.edge_attention(q, k, v, s, ei, H)[0]
        if i != L - 1:
            x = x.relu()
    users = np.array([0, 7, 39, 12])
    want = x[users] @ x[NU:].t()
    m.eval()
    got = m.getUsersRating(torch.from_numpy(users))
    assert got.shape == (4, MI) and _rel(got, want) <= TOL
    assert _rel(m.propagated(), x) <= TOL
    m.train()


def test_state_dict_round_trip(setup):
    m = setup["m"]
    sd = m.state_dict()
    want = {"_table"} | {f"convs.{i}.{n}.{w}" for i in range(L) for n in LINS
                         for w in ("weight", "bias")}
    assert set(sd) == want
    for i in range(L):
        for n in LINS:
            assert sd[f"convs.{i}.{n}.weight"].shape == (D, D)
            assert sd[f"convs.{i}.{n}.bias"].shape == (D,)
    assert sd["_table"].shape == (NU + MI, D)
    m2 = _model(seed=123)
    assert not torch.equal(m2._table, m._table)
    m2.load_state_dict(sd)
    assert torch.equal(m2.propagated(), m.propagated())


def test_config_errors():
    with pytest.raises(ValueError):
        _model(recdim=24)                  # not a multiple of 4 * heads
    with pytest.raises(ValueError):
        _model(fanouts=[3])
    with pytest.raises(ValueError):
        _model(heads=16, recdim=64)        # a multiple of 4 * heads, but heads > 8
    assert _model().heads == 8


def test_default_heads_at_d64_runs_a_step():
    cfg = _cfg(recdim=64)
    del cfg["heads"]
    from furusato_recommend_amd import TGRec
    torch.manual_seed(0)
    m = TGRec(cfg, DS())
    assert m.heads == 8 and m.convs[0].ch == 8 and m.dropout_p == 0.0
    u, p, n = m.sample(B, seed=1)
    loss = m.stageOne(u, p, n)
    assert torch.isfinite(loss)
    assert all(torch.isfinite(q).all() for q in m.parameters())
    assert torch.isfinite(m.getUsersRating(torch.arange(5))).all()
    assert TGRec({k: v for k, v in cfg.items() if k != "dropout_p"}, DS()).dropout_p == 0.2


def test_dropout_reaches_the_seed_rows_in_training_only(setup):
    """tgrec.py:280-292 drops out after every layer, the last included."""
    m = _model(dropout_p=0.5)
    for a, b in zip(_model_params(m), _model_params(setup["m"])):
        assert torch.equal(a, b)
    m.train()
    emb = m.forward(setup["tree"], dropout_seed=3)
    zero = (emb == 0)
    assert 0.3 < float(zero.float().mean()) < 0.7
    # the kept entries are scaled by 1 / (1 - p) ... of a forward whose first
    # layer was dropped out too, so only the zero pattern is compared
    assert torch.equal(zero, (m.forward(setup["tree"], dropout_seed=3) == 0))
    assert not torch.equal(zero, (m.forward(setup["tree"], dropout_seed=4) == 0))
    assert not (m.forward(setup["tree"], dropout_seed=None) == 0).any()
    m.eval()
    ev = m.forward(setup["tree"], dropout_seed=3)
    assert not (ev == 0).any() and _rel(ev, setup["emb"]) <= TOL
    m.train()


def test_training_lowers_the_loss():
    m = _model(lr=5e-3, decay=1e-4)
    u, p, n = m.sample(4 * B, seed=2)
    losses = []
    for step in range(30):
        s = slice((step % 4) * B, (step % 4 + 1) * B)
        losses.append(float(m.stageOne(u[s], p[s], n[s])))
    assert np.isfinite(losses).all()
    assert np.mean(losses[-4:]) < np.mean(losses[:4])
    # OneEpoch walks the triples in batches
    assert torch.isfinite(m.OneEpoch(u, p, n))


def test_evaluation_runs_on_it(setup):
    from furusato_recommend_amd.evaluate import evaluate, evaluate_ranked
    m = setup["m"]
    m.eval()
    test = {0: [1, 2], 7: [3], 39: [0, 14], 20: [4, 5, 6]}
    res = evaluate(m, test, topks=(3, 5))
    for k in ("precision", "recall", "ndcg", "hr"):
        assert np.isfinite(res[k]).all() and (res[k] >= 0).all()
    ranked = evaluate_ranked(m, test, topks=(3, 5))
    for k in ("precision", "recall", "ndcg", "hr"):
        assert np.isfinite(ranked[k]).all()
        assert np.allclose(ranked[k], res[k])
    assert np.isfinite(ranked["mrr"]) and np.isfinite(ranked["auc"])
    m.train()


def test_dropout_steps_repeat_bitwise():
    a, b = _model(seed=5, dropout_p=0.3), _model(seed=5, dropout_p=0.3)
    u, p, n = a.sample(B, seed=4)
    for step in range(3):
        la, lb = a.stageOne(u, p, n), b.stageOne(u, p, n)
        assert torch.equal(la, lb), step
    for x, y in zip(a.parameters(), b.parameters()):
        assert torch.equal(x, y)
    # and dropout does something: the same step without it gives another loss
    c = _model(seed=5, dropout_p=0.0)
    assert float(c.stageOne(u, p, n)) != float(_model(seed=5, dropout_p=0.3).stageOne(u, p, n))
