"""The 'gnn' model with conv = 'ggnn' against a float64 torch-autograd
restatement (tests/ggnn_common.py: PyG's order — project every row, scatter
mean over the tree's per-layer edge lists, torch.nn.GRUCell) on
tests/test_gnn_model.py's tiny dataset: 40 users x 15 items, 120 interactions
with duplicates, item 14 without interactions, user 39 with a single item; d =
16, L = 2, fanouts [3, 2], B = 8, dropout_p = 0 unless stated.

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
from tests import ggnn_common as gg

pytestmark = pytest.mark.gpu

NU, MI, D, L, FAN, B = 40, 15, 16, 2, [3, 2], 8
LR, DECAY = 1e-2, 1e-2
TOL = 1e-4
NAMES = ("weight", "rnn.weight_ih", "rnn.weight_hh", "rnn.bias_ih", "rnn.bias_hh")


class DS:
    def __init__(self):
        rng = np.random.default_rng(40)
        u = rng.integers(0, 39, 107)
        i = rng.integers(0, 14, 107)
        self.trainUser = np.concatenate([u, u[:12], [39]]).astype(np.int64)   # 12 duplicates
        self.trainItem = np.concatenate([i, i[:12], [5]]).astype(np.int64)
        self.n_users, self.m_items = NU, MI


def _cfg(**kw):
    cfg = {"recdim": D, "layer": L, "conv": "ggnn", "fanouts": FAN, "lr": LR, "decay": DECAY,
           "dropout_p": 0.0, "device": "cuda:0", "bpr_batch_size": B, "seed": 11}
    cfg.update(kw)
    return cfg


def _model(seed=0, ds=None, **kw):
    from furusato_recommend_amd.register import MODELS
    torch.manual_seed(seed)
    return MODELS["gnn"](_cfg(**kw), ds or DS())


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


def _hop_params(c):
    return [c.weight, c.rnn.weight_ih, c.rnn.weight_hh, c.rnn.bias_ih, c.rnn.bias_hh]


def _ref_convs(m):
    """Per layer (W [d, d], W_ih, W_hh, b_ih, b_hh) in float64 on the host."""
    return [tuple(p.detach().double().cpu().reshape(p.shape[-2:] if n == 0 else p.shape)
                  .requires_grad_(True) for n, p in enumerate(_hop_params(c))) for c in m.convs]


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
    table = m._table.detach().double().cpu().requires_grad_(True)
    convs = _ref_convs(m)
    emb = gg.model_forward(table, convs, groups, depths, children, L, FAN)
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
    return [m._table] + [q for c in m.convs for q in _hop_params(c)]


def test_forward_loss_and_gradients(setup):
    m = setup["m"]
    m.train()
    for p in m.parameters():
        p.grad = None
    emb = m.forward(setup["tree"], dropout_seed=3)
    r = _rel(emb, setup["emb"])
    print(f"[ggnn] forward: rel {r:.2e}")
    assert r <= TOL
    loss = m.loss_fused(emb)
    assert abs(float(loss) - setup["loss"]) <= TOL * abs(setup["loss"])
    # the norm term is there: the loss without it differs visibly
    all_param = float(2 * setup["table"][:NU].norm(2) + setup["table"][NU:].norm(2))
    assert DECAY * all_param / B > 100 * TOL * abs(setup["loss"])
    loss.backward()
    names = ["table"] + [f"convs.{i}.{n}" for i in range(L) for n in NAMES]
    assert len(names) == len(setup["grads"]) == 1 + 5 * L
    for name, p, g in zip(names, _model_params(m), setup["grads"]):
        assert p.grad is not None, name
        assert float(g.abs().max()) > 0, name
        r = _rel(p.grad, g)
        print(f"[ggnn] grad {name}: rel {r:.2e}")
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
    x = setup["table"].detach()
    for i, conv in enumerate(setup["convs"]):
        x = gg.dense_full(x, rowptr, col, [p.detach() for p in conv])
        if i != L - 1:
            x = x.relu()
    users = np.array([0, 7, 39, 12])
    want = x[users] @ x[NU:].t()
    m.eval()
    got = m.getUsersRating(torch.from_numpy(users))
    assert got.shape == (4, MI) and _rel(got, want) <= TOL
    assert _rel(m.propagated(), x) <= TOL
    m.train()


def test_one_tree_layer_is_the_full_rows_when_the_fanout_covers_every_degree():
    u, i, nu, mi = gc.small_graph_edges()

    class Small:
        trainUser, trainItem, n_users, m_items = u, i, nu, mi

    rowptr, _ = gc.host_csr(u, i, nu, mi)
    k = int(np.diff(rowptr).max())
    assert np.diff(rowptr).min() == 0                 # the isolated item
    m = _model(ds=Small(), layer=1, fanouts=[k])
    m.eval()
    seeds = torch.arange(nu + mi, dtype=torch.int32, device="cuda")
    tree = m.sample_tree(seeds, seed=5)
    kids = tree.groups[tree.children[(0, 1)]][0].cpu().numpy().reshape(nu + mi, k)
    assert np.array_equal((kids >= 0).sum(1), np.diff(rowptr))   # every neighbour, once
    with torch.no_grad():
        emb = m.forward(tree)
    full = m.propagated()
    assert _rel(emb, full) <= TOL
    # and both are the float64 layer
    x = m._table.detach().double().cpu()
    _, col = gc.host_csr(u, i, nu, mi)
    ref = gg.dense_full(x, rowptr, col, [p.detach() for p in _ref_convs(m)[0]])
    assert _rel(full, ref) <= TOL


def test_state_dict_round_trip(setup):
    m = setup["m"]
    sd = m.state_dict()
    want = {"_table"} | {f"convs.{i}.{n}" for i in range(L) for n in NAMES}
    assert set(sd) == want
    assert sd["convs.0.weight"].shape == (1, D, D)
    for i in range(L):
        assert sd[f"convs.{i}.rnn.weight_ih"].shape == (3 * D, D)
        assert sd[f"convs.{i}.rnn.weight_hh"].shape == (3 * D, D)
        assert sd[f"convs.{i}.rnn.bias_ih"].shape == (3 * D,)
        assert sd[f"convs.{i}.rnn.bias_hh"].shape == (3 * D,)
    # the reset: all five inside U(-1/sqrt(d), 1/sqrt(d)) and spread over it
    for n in NAMES:
        w = sd[f"convs.0.{n}"]
        assert float(w.abs().max()) <= 1 / np.sqrt(D) and float(w.abs().max()) > 0.5 / np.sqrt(D)
    m2 = _model(seed=123)
    assert not torch.equal(m2._table, m._table)
    m2.load_state_dict(sd)
    assert torch.equal(m2.propagated(), m.propagated())
    # a reference GRUCell's own state dict loads into the hop's rnn
    cell = torch.nn.GRUCell(D, D)
    m2.convs[0].rnn.load_state_dict(cell.state_dict())
    assert torch.equal(m2.convs[0].rnn.weight_hh.cpu(), cell.weight_hh.detach())


def test_config_errors():
    for conv in ("transformer", "gcn", "sage"):
        with pytest.raises(ValueError, match="gat"):
            _model(conv=conv)
    with pytest.raises(ValueError):
        _model(recdim=18)                  # not a multiple of 4
    with pytest.raises(ValueError):
        _model(fanouts=[3])
    with pytest.raises(ValueError):
        _model(fanouts=[3, 0])
    m = _model(heads=5)                    # heads is ignored: 16 is no multiple of 4 * 5
    assert m.conv == "ggnn" and not hasattr(m, "heads")


@pytest.mark.parametrize("relu", [False, True])
def test_hop_at_d128_on_the_mfma_gemms(relu):
    """The hop where every GEMM shape is the MFMA kernels' (d = 128): forward
    and the gradients of both inputs and all five parameters against float64
    autograd of PyG's order."""
    from furusato_recommend_amd.ggnn import GGNNHop
    n_t, k, d = 37, 5, 128
    rng = np.random.default_rng(128)
    xc = rng.standard_normal((n_t * k, d)).astype(np.float32)
    xs = rng.standard_normal((n_t, d)).astype(np.float32)
    valid = rng.integers(0, 50, (n_t, k)).astype(np.int32)
    valid[rng.random((n_t, k)) < 0.3] = -1
    valid[-1] = -1
    valid = valid.reshape(-1)
    g = rng.standard_normal((n_t, d)).astype(np.float32)
    torch.manual_seed(3)
    hop = GGNNHop(d, device="cuda")
    dev = [torch.from_numpy(a).cuda().requires_grad_(True) for a in (xc, xs)]
    out = hop.update(hop.aggregate(dev[0], torch.from_numpy(valid).cuda(), k), dev[1], relu=relu)
    out.backward(torch.from_numpy(g).cuda())
    ref_in = [torch.from_numpy(a).double().requires_grad_(True) for a in (xc, xs)]
    conv = [p.detach().double().cpu().reshape(p.shape[-2:] if n == 0 else p.shape)
            .requires_grad_(True) for n, p in enumerate(_hop_params(hop))]
    ref = gg.tree_level(ref_in[0], ref_in[1], valid, k, conv)
    if relu:
        ref = ref.relu()
    want = torch.autograd.grad(ref, ref_in + conv, torch.from_numpy(g).double())
    assert _rel(out, ref) <= TOL
    got = [t.grad for t in dev] + [p.grad for p in _hop_params(hop)]
    for name, a, b in zip(("x_child", "x_self") + NAMES, got, want):
        r = _rel(a, b)
        print(f"[ggnn hop d128 relu={relu}] grad {name}: rel {r:.2e}")
        assert r <= TOL, (name, r)
    # rows of an invalid slot get no gradient
    assert not dev[0].grad[torch.from_numpy(valid < 0).cuda()].any()


def test_default_config_at_d128_runs_a_step():
    cfg = _cfg(recdim=128)
    assert "heads" not in cfg
    from furusato_recommend_amd import GNN
    from furusato_recommend_amd.ggnn import GGNNHop
    torch.manual_seed(0)
    m = GNN(cfg, DS())
    assert all(isinstance(c, GGNNHop) for c in m.convs) and m.dropout_p == 0.0
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
