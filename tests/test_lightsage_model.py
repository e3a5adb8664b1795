"""The 'lightsage' model against a float64 torch-autograd restatement
(tests/lightsage_common.py: the reference's order — gather the source rows
along the tree's per-layer edge lists, mask, scatter-mean, add the target
rows) on tests/test_ggnn_model.py's tiny dataset: 40 users x 15 items, 120
interactions with duplicates, item 14 without interactions, user 39 with a
single item; d = 16, L = 2, fanouts [3, 2], B = 8, dropout_p = 0 unless
stated.

Tolerance: 1e-4 relative by max-norm per tensor, the project's fp32 bar.  The
Adam check compares the first step's update D = -lr g / (|g| + eps): for an
element whose |g| is above 1e-3 max |g| (ten times the gradient check's own
absolute tolerance, so its sign is settled) the two updates agree to 1e-3 lr;
every update is at most lr in size.  The two forms of the forward (FUSED_HOP
on / off) take the same hash at the same element indices, so with dropout
they are compared with each other and with the float64 restatement under the
host-made mask, within the same bar.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gat_common as gc
from tests import lightsage_common as lc

pytestmark = pytest.mark.gpu

NU, MI, D, L, FAN, B = 40, 15, 16, 2, [3, 2], 8
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
    cfg = {"recdim": D, "layer": L, "fanouts": FAN, "lr": LR, "decay": DECAY,
           "dropout_p": 0.0, "device": "cuda:0", "bpr_batch_size": B, "seed": 11}
    cfg.update(kw)
    return cfg


def _model(seed=0, ds=None, **kw):
    from furusato_recommend_amd.register import MODELS
    torch.manual_seed(seed)
    return MODELS["lightsage"](_cfg(**kw), ds or DS())


def _host_tree(ds, seeds, rng, L=L, fan=FAN):
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
    for (gi, hop), ci in sorted(children.items(), key=lambda kv: kv[1]):
        groups[ci] = draw(groups[gi], fan[hop - 1])
    return groups, depths, children


def _triples(ds, rng):
    users = rng.choice(np.unique(ds.trainUser), B)    # users with a positive
    users[0] = 39                                     # the single-item user
    pos = np.array([ds.trainItem[ds.trainUser == u][0] for u in users])
    neg = rng.integers(0, MI, B)
    neg[0] = 14                                       # the item without interactions
    return users, pos, neg


def _ref(table, groups, depths, children, L_, fan, p=0.0, dseed=0):
    """(emb, loss, table gradient) of the float64 restatement."""
    emb = lc.tree_forward(table, groups, depths, children, L_, fan, p, dseed)
    u, q, n = emb[:B], emb[B:2 * B], emb[2 * B:]
    soft = F.softplus((u * n).sum(1) - (u * q).sum(1)).mean()
    all_param = 2 * table[NU:].norm(2) + table[:NU].norm(2)       # 2 |I| + |U|
    loss = soft + DECAY * all_param / B
    (grad,) = torch.autograd.grad(loss, [table])
    return emb.detach(), float(loss.detach()), grad


def _dev_tree(groups, L_=L):
    from furusato_recommend_amd.graphsage import SampleTree
    return SampleTree.from_groups([torch.from_numpy(g).cuda() for g in groups], L_)


@pytest.fixture(scope="module")
def setup():
    """One model, one explicit tree, its float64 restatement with gradients."""
    m = _model()
    ds = DS()
    rng = np.random.default_rng(8)
    users, pos, neg = _triples(ds, rng)
    seeds = np.concatenate([users, NU + pos, NU + neg])
    groups, depths, children = _host_tree(ds, seeds, rng)
    assert any((g < 0).any() for g in groups[1:])     # short rows leave empty slots
    table = m._table.detach().double().cpu().requires_grad_(True)
    emb, loss, grad = _ref(table, groups, depths, children, L, FAN)
    return dict(m=m, ds=ds, tree=_dev_tree(groups), triples=(users, pos, neg), table=table,
                host=(groups, depths, children), emb=emb, loss=loss, grad=grad)


def _rel(got, ref):
    got = got.detach().double().cpu().reshape(-1)
    ref = ref.detach().double().cpu().reshape(-1)
    assert torch.isfinite(got).all()
    return float((got - ref).abs().max() / ref.abs().max())


def _fwd_bwd(m, tree, dseed):
    """(emb, loss, dense table gradient) of one forward / backward."""
    m._table.grad = None
    emb = m.forward(tree, dropout_seed=dseed)
    loss = m.loss_fused(emb)
    loss.backward()
    assert m._table.grad is None and m._tg.pending     # the sorted, non-dense form
    grad = m._tg.materialize(m._table.detach())
    assert torch.equal(grad, m.table_grad_dense())
    return emb.detach().clone(), float(loss.detach()), grad


def test_forward_loss_and_gradient(setup):
    m = setup["m"]
    m.train()
    assert [n for n, _ in m.named_parameters()] == ["_table"]
    emb, loss, grad = _fwd_bwd(m, setup["tree"], 3)
    r = _rel(emb, setup["emb"])
    print(f"[lightsage] forward: rel {r:.2e}")
    assert emb.shape == (3 * B, D) and r <= TOL
    assert abs(loss - setup["loss"]) <= TOL * abs(setup["loss"])
    # the norm term is there, and it is 2 |I| + |U|, not 2 |U| + |I|
    t = setup["table"].detach()
    term = DECAY * float(2 * t[NU:].norm(2) + t[:NU].norm(2)) / B
    other = DECAY * float(2 * t[:NU].norm(2) + t[NU:].norm(2)) / B
    assert term > 100 * TOL * abs(setup["loss"]) and abs(term - other) > 10 * TOL * abs(setup["loss"])
    assert float(setup["grad"].abs().max()) > 0
    r = _rel(grad, setup["grad"])
    print(f"[lightsage] grad table: rel {r:.2e}")
    assert r <= TOL
    # the unfused loss is the same function
    emb2 = m.forward(setup["tree"], dropout_seed=3)
    l2 = m.loss(emb2[:B], emb2[B:2 * B], emb2[2 * B:])
    assert abs(float(l2.detach()) - setup["loss"]) <= TOL * abs(setup["loss"])
    m._tg.pending = False


def test_stage_one_is_adam_on_the_restatement(setup):
    m = _model()                                      # same seed: the fixture's table
    assert torch.equal(m._table, setup["m"]._table)
    p0 = m._table.detach().clone()
    users, pos, neg = (torch.from_numpy(x) for x in setup["triples"])
    loss = m.stageOne(users, pos, neg, tree=setup["tree"])
    assert abs(float(loss) - setup["loss"]) <= TOL * abs(setup["loss"])
    r0 = setup["table"].detach().clone()
    r1 = r0.clone().requires_grad_(True)
    opt = torch.optim.Adam([r1], lr=LR)
    r1.grad = setup["grad"].clone()
    opt.step()
    d_got = (m._table.detach() - p0).double().cpu().reshape(-1)
    d_ref = (r1.detach() - r0).reshape(-1)
    g = setup["grad"].reshape(-1)
    settled = g.abs() > 1e-3 * g.abs().max()
    assert settled.any()
    # p1 - p0 in float32 carries the rounding of p: one ulp of |p| <= 1
    slack = 1e-3 * LR + 2.0 ** -23 * p0.abs().max().item()
    assert (d_got - d_ref)[settled].abs().max() <= slack
    assert d_got.abs().max() <= LR * (1 + 1e-3) + slack
    # the fused Adam left the slice norms for the next forward
    assert m._cached_norms() is not None
    n2 = m._cached_norms().cpu()
    want = torch.stack([m._table[:NU].norm(2), m._table[NU:].norm(2)]).cpu()
    assert _rel(n2, want) <= TOL
    # and the second step takes them: the same loss as a model without a cache
    m2 = _model()
    with torch.no_grad():
        m2._table.copy_(m._table)
    assert m2._cached_norms() is None
    l2, l2_ref = m.stageOne(users, pos, neg, tree=setup["tree"]), \
        m2.stageOne(users, pos, neg, tree=setup["tree"])
    assert abs(float(l2) - float(l2_ref)) <= TOL * abs(float(l2_ref))


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_fused_and_composed_forms_agree(setup, p, monkeypatch):
    """FUSED_HOP on / off: the same embeddings and table gradient, and with
    dropout both are the float64 restatement under the host-made mask."""
    from furusato_recommend_amd import lightsage
    m = _model(dropout_p=p)
    m.train()
    groups, depths, children = setup["host"]
    dseed = 5
    table = m._table.detach().double().cpu().requires_grad_(True)
    emb_ref, loss_ref, grad_ref = _ref(table, groups, depths, children, L, FAN, p, dseed)
    if p > 0:
        assert not torch.equal(emb_ref, setup["emb"])
    out = {}
    for fused in (True, False):
        monkeypatch.setattr(lightsage, "FUSED_HOP", fused)
        out[fused] = _fwd_bwd(m, setup["tree"], dseed)
        m._tg.pending = False
    for fused, (emb, loss, grad) in out.items():
        r_e, r_g = _rel(emb, emb_ref), _rel(grad, grad_ref)
        print(f"[lightsage] p={p} fused={fused}: emb rel {r_e:.2e} grad rel {r_g:.2e}")
        assert r_e <= TOL and r_g <= TOL and abs(loss - loss_ref) <= TOL * abs(loss_ref)
    assert _rel(out[True][0], out[False][0]) <= TOL
    assert _rel(out[True][2], out[False][2]) <= TOL


def test_get_users_rating_is_the_dense_full_graph_form(setup):
    m, ds = setup["m"], setup["ds"]
    rowptr, col = gc.host_csr(ds.trainUser, ds.trainItem, NU, MI)
    x = lc.dense_full(setup["table"].detach(), rowptr, col, L)
    users = np.array([0, 7, 39, 12])
    want = x[users] @ x[NU:].t()
    m.eval()
    got = m.getUsersRating(torch.from_numpy(users))
    assert got.shape == (4, MI) and _rel(got, want) <= TOL
    assert _rel(m.propagated(), x) <= TOL
    # not the reference's accumulator (2 x_L - x_{L-1}) / (L + 1)
    assert torch.equal(m.propagated(), m.propagated())
    m.train()


def test_tree_is_the_full_rows_when_the_fanouts_cover_every_degree():
    u, i, nu, mi = gc.small_graph_edges()

    class Small:
        trainUser, trainItem, n_users, m_items = u, i, nu, mi

    rowptr, col = gc.host_csr(u, i, nu, mi)
    k = int(np.diff(rowptr).max())
    assert np.diff(rowptr).min() == 0                 # the isolated item
    m = _model(ds=Small(), fanouts=[k, k])
    m.eval()
    seeds = torch.arange(nu + mi, dtype=torch.int32, device="cuda")
    tree = m.sample_tree(seeds, seed=5)
    kids = tree.groups[tree.children[(0, 1)]][0].cpu().numpy().reshape(nu + mi, k)
    assert np.array_equal((kids >= 0).sum(1), np.diff(rowptr))   # every neighbour, once
    with torch.no_grad():
        emb = m.forward(tree)
    full = m.propagated()
    assert _rel(emb, full) <= TOL
    ref = lc.dense_full(m._table.detach().double().cpu(), rowptr, col, L)
    assert _rel(full, ref) <= TOL


@pytest.mark.parametrize("layers,fan", [(1, [3]), (3, [3, 2, 2])])
def test_other_depths(layers, fan):
    ds = DS()
    m = _model(layer=layers, fanouts=fan, dropout_p=0.2)
    m.train()
    rng = np.random.default_rng(layers)
    users, pos, neg = _triples(ds, rng)
    seeds = np.concatenate([users, NU + pos, NU + neg])
    groups, depths, children = _host_tree(ds, seeds, rng, layers, fan)
    table = m._table.detach().double().cpu().requires_grad_(True)
    emb_ref, loss_ref, grad_ref = _ref(table, groups, depths, children, layers, fan, 0.2, 9)
    emb, loss, grad = _fwd_bwd(m, _dev_tree(groups, layers), 9)
    assert _rel(emb, emb_ref) <= TOL and abs(loss - loss_ref) <= TOL * abs(loss_ref)
    assert _rel(grad, grad_ref) <= TOL


def test_state_dict_round_trip(setup):
    m = setup["m"]
    sd = m.state_dict()
    assert set(sd) == {"_table"} and sd["_table"].shape == (NU + MI, D)
    m2 = _model(seed=123)
    assert not torch.equal(m2._table, m._table)
    m2.load_state_dict(sd)
    assert torch.equal(m2.propagated(), m.propagated())


def test_config_errors():
    with pytest.raises(ValueError):
        _model(recdim=18)                  # not a multiple of 4
    with pytest.raises(ValueError):
        _model(fanouts=[3, 0])
    with pytest.raises(ValueError):
        _model(fanouts=[3])
    with pytest.raises(ValueError):
        _model(dropout_p=1.0)
    assert _model(fanouts=[70, 1]).sizes == [70, 1]     # no fanout limit but >= 1


def test_default_config_at_d128_runs_a_step():
    cfg = _cfg(recdim=128)
    from furusato_recommend_amd import LightSAGE
    torch.manual_seed(0)
    m = LightSAGE(cfg, DS())
    u, p, n = m.sample(B, seed=1)
    loss = m.stageOne(u, p, n)
    assert torch.isfinite(loss) and torch.isfinite(m._table).all()
    assert torch.isfinite(m.getUsersRating(torch.arange(5))).all()
    assert LightSAGE({k: v for k, v in cfg.items() if k != "dropout_p"}, DS()).dropout_p == 0.2


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
    from furusato_recommend_amd.evaluate import evaluate, evaluate_ranked, score_topk
    m = setup["m"]
    m.eval()
    ue, ie = m.eval_embeddings()
    assert ue.shape == (NU, D) and ie.shape == (MI, D)
    test = {0: [1, 2], 7: [3], 39: [0, 14], 20: [4, 5, 6]}
    res = evaluate(m, test, topks=(3, 5))
    for k in ("precision", "recall", "ndcg", "hr"):
        assert np.isfinite(res[k]).all() and (res[k] >= 0).all()
    ranked = evaluate_ranked(m, test, topks=(3, 5))
    for k in ("precision", "recall", "ndcg", "hr"):
        assert np.isfinite(ranked[k]).all()
        assert np.allclose(ranked[k], res[k])
    assert np.isfinite(ranked["mrr"]) and np.isfinite(ranked["auc"])
    users = torch.tensor([0, 7, 39], device="cuda")
    val, idx = score_topk(ue[users.long()], ie, users, m.graph, 5)
    dense = m.getUsersRating(users)
    assert val.shape == (3, 5) and int(idx.min()) >= 0 and int(idx.max()) < MI
    assert _rel(val[:, 0], torch.gather(dense, 1, idx[:, :1].long())[:, 0]) <= TOL
    m.train()


def test_dropout_steps_repeat_bitwise():
    a, b = _model(seed=5, dropout_p=0.3), _model(seed=5, dropout_p=0.3)
    u, p, n = a.sample(B, seed=4)
    for step in range(3):
        la, lb = a.stageOne(u, p, n), b.stageOne(u, p, n)
        assert torch.equal(la, lb), step
    assert torch.equal(a._table, b._table)
    # and dropout does something: the same step without it gives another loss
    c = _model(seed=5, dropout_p=0.0)
    assert float(c.stageOne(u, p, n)) != float(_model(seed=5, dropout_p=0.3).stageOne(u, p, n))
