"""The 'gnn' model (conv = 'gat') against a float64 torch-autograd restatement
(tests/gat_common.py: the PyG-style edge-list form over the tree's per-layer
edge lists) on a tiny dataset: 40 users x 15 items, 120 interactions with
duplicates, item 14 without interactions, user 39 with a single item; d = 16,
H = 4, L = 2, fanouts [3, 2], B = 8, dropout_p = 0 unless stated.

Tolerance: 1e-4 relative by max-norm per tensor, the project's fp32 bar.
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

pytestmark = pytest.mark.gpu

NU, MI, D, H, L, FAN, B = 40, 15, 16, 4, 2, [3, 2], 8
LR, DECAY = 1e-2, 1e-2
TOL = 1e-4


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
    return MODELS["gnn"](_cfg(**kw), DS())


def test_dataset_is_what_it_claims():
    ds = DS()
    assert len(ds.trainUser) == 120
    pairs = set(zip(ds.trainUser.tolist(), ds.trainItem.tolist()))
    assert len(pairs) < 120 and 14 not in ds.trainItem and (ds.trainUser == 39).sum() == 1


def _host_tree(ds, seeds, rng):
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
    tree = SampleTree.from_groups([torch.from_numpy(g).cuda() for g in groups], L)
    # float64 restatement
    table = m._table.detach().double().cpu().requires_grad_(True)
    convs = [tuple(p.detach().double().cpu().reshape(-1 if n else p.shape).requires_grad_(True)
                   for n, p in enumerate((c.lin.weight, c.att_src, c.att_dst, c.bias)))
             for c in m.convs]
    emb = gc.model_forward(table, convs, groups, depths, children, L, FAN, H)
    u, p, n = emb[:B], emb[B:2 * B], emb[2 * B:]
    soft = F.softplus((u * n).sum(1) - (u * p).sum(1)).mean()
    all_param = 2 * table[:NU].norm(2) + table[NU:].norm(2)
    loss = soft + DECAY * all_param / B
    params = [table] + [q for c in convs for q in c]
    grads = torch.autograd.grad(loss, params)
    return dict(m=m, ds=ds, tree=tree, triples=(users, pos, neg), table=table, convs=convs,
                emb=emb.detach(), loss=float(loss.detach()), params=params, grads=grads)


def _rel(got, ref):
    got = got.detach().double().cpu().reshape(-1)
    ref = ref.detach().double().cpu().reshape(-1)
    assert torch.isfinite(got).all()
    return float((got - ref).abs().max() / ref.abs().max())


def _model_params(m):
    return [m._table] + [q for c in m.convs for q in (c.lin.weight, c.att_src, c.att_dst, c.bias)]


def test_forward_loss_and_gradients(setup):
    m = setup["m"]
    m.train()
    for p in m.parameters():
        p.grad = None
    emb = m.forward(setup["tree"], dropout_seed=3)
    assert _rel(emb, setup["emb"]) <= TOL
    loss = m.loss_fused(emb)
    assert abs(float(loss) - setup["loss"]) <= TOL * abs(setup["loss"])
    # the norm term is there: the loss without it differs visibly
    all_param = float(2 * setup["table"][:NU].norm(2) + setup["table"][NU:].norm(2))
    assert DECAY * all_param / B > 100 * TOL * abs(setup["loss"])
    loss.backward()
    names = ["table"] + [f"convs.{i}.{n}" for i in range(L)
                         for n in ("lin.weight", "att_src", "att_dst", "bias")]
    for name, p, g in zip(names, _model_params(m), setup["grads"]):
        assert p.grad is not None, name
        r = _rel(p.grad, g)
        print(f"[gnn] grad {name}: rel {r:.2e}")
        assert r <= TOL, (name, r)
    # the unfused loss is the same function
    emb2 = m.forward(setup["tree"], dropout_seed=3)
    l2 = m.loss(emb2[:B], emb2[B:2 * B], emb2[2 * B:])
    assert abs(float(l2) - setup["loss"]) <= TOL * abs(setup["loss"])


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
    for p0, p1, r0, r1, g in zip(before, _model_params(m), setup["params"], ref, setup["grads"]):
        d_got = (p1.detach() - p0).double().cpu().reshape(-1)
        d_ref = (r1.detach() - r0.detach()).reshape(-1)
        g = g.reshape(-1)
        settled = g.abs() > 1e-3 * g.abs().max()
        assert settled.any()
        # p1 - p0 in float32 carries the rounding of p: one ulp of |p| <= 1
        slack = 1e-3 * LR + 2.0 ** -23 * p0.abs().max().item()
        assert (d_got - d_ref)[settled].abs().max() <= slack
        assert d_got.abs().max() <= LR * (1 + 1e-3) + slack


def test_get_users_rating_is_the_dense_full_graph_form(setup):
    m, ds = setup["m"], setup["ds"]
    rowptr, col = gc.host_csr(ds.trainUser, ds.trainItem, NU, MI)
    dst = np.repeat(np.arange(NU + MI), np.diff(rowptr))
    ei = torch.from_numpy(np.stack([col.astype(np.int64), dst]))
    x = setup["table"].detach()
    for i, (W, a_s, a_d, b) in enumerate(setup["convs"]):
        x = gc.edge_softmax(x @ W.detach().t(), ei, a_s.detach(), a_d.detach(), b.detach(), H)[0]
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
    want = {"_table"} | {f"convs.{i}.{n}" for i in range(L)
                         for n in ("lin.weight", "att_src", "att_dst", "bias")}
    assert set(sd) == want
    assert sd["convs.0.lin.weight"].shape == (D, D) and sd["convs.1.att_src"].shape == (1, H, D // H)
    assert sd["convs.0.bias"].shape == (D,)
    m2 = _model(seed=123)
    assert not torch.equal(m2._table, m._table)
    m2.load_state_dict(sd)
    assert torch.equal(m2.propagated(), m.propagated())


def test_config_errors():
    with pytest.raises(ValueError, match="gat"):
        _model(conv="transformer")
    with pytest.raises(ValueError):
        _model(recdim=24)                  # not a multiple of 4 * heads
    with pytest.raises(ValueError):
        _model(fanouts=[3])
    assert _model(conv="gat").heads == 4


def test_default_heads_at_d128_runs_a_step():
    cfg = _cfg(recdim=128)
    del cfg["heads"]
    from furusato_recommend_amd import GNN
    torch.manual_seed(0)
    m = GNN(cfg, DS())
    assert m.heads == 4 and m.convs[0].ch == 32 and m.dropout_p == 0.0
    u, p, n = m.sample(B, seed=1)
    loss = m.stageOne(u, p, n)
    assert torch.isfinite(loss)
    assert all(torch.isfinite(q).all() for q in m.parameters())
    assert torch.isfinite(m.getUsersRating(torch.arange(5))).all()
    assert GNN({k: v for k, v in cfg.items() if k != "dropout_p"}, DS()).dropout_p == 0.2


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
