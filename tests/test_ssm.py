"""The sampled-softmax loss on the GPU through the engine and the model:
PropagationEngine.train_step_ssm (frontier pruning, long-row segments, the
first backward layer's filters, fused Adam), LightGCN with config["loss"] =
"ssm" (stageOne, OneEpoch, softmax_loss, sample), its combinations with edge
weights, edge dropout and rAdjGCN, the 'lgnssm' registry entry, the Trainer
and the refusals.

The float64 reference (tests/ssm_common.py, Ref): dense propagation matrices
of tests/test_edge_dropout.py's kind of graph (300 users x 40 items, a hub
item beyond narrow_max, an isolated item, multi-edges), the loss of DESIGN.md
§18 in torch autograd and torch.optim.Adam, two consecutive steps.

Tolerance: the project's 1e-4 relative error in the max norm against float64
(tests/test_gpu_parity.py, tests/test_edge_dropout.py), on the losses and on
the stepped tables."""
import numpy as np
import pytest
import torch

from tests.ssm_common import MI, NU, N, Ref, rel

pytestmark = pytest.mark.gpu
TOL = 1e-4
SPLITS = [None, 32]
LR, DECAY = 1e-2, 1e-3


@pytest.fixture(scope="module")
def ref():
    r = Ref()
    deg = r.deg
    assert deg[NU] >= 300 and deg[N - 1] == 0              # the hub, the isolated item
    cell = r.rows * N + r.col
    assert len(np.unique(cell)) < len(cell)                # multi-edges
    u, p, n = r.batches[0]
    assert n[0, 1] == n[0, 0] and n[1, 0] == p[1]
    return r


@pytest.fixture(scope="module", params=SPLITS, ids=lambda s: f"split{s}")
def graph(request, ref):
    from furusato_recommend_amd.graph import DEFAULT_SPLIT, Graph
    split = request.param
    g = Graph.from_interactions(ref.ds.trainUser, ref.ds.trainItem, NU, MI, "cuda:0",
                                split=DEFAULT_SPLIT if split is None else split)
    assert np.array_equal(g.col_host, ref.col)
    if split is not None:
        assert g.n_long >= 1 and g.n_seg >= 10             # the hub runs as segments + finalize
    else:
        assert g.n_seg == 0
    return g


def _dev(batch):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda().int().contiguous()
                 for a in batch)


_WANT = {}


def _want(ref, d, L, K, temp, seed=0):
    """Two float64 steps on the plain graph, computed once per configuration."""
    key = (d, L, K, temp, seed)
    if key not in _WANT:
        _WANT[key] = ref.steps(ref.emb(d, seed), L, [ref.dense()] * 2,
                               [ref.batch(t, K) for t in range(2)], LR, DECAY, temp)
    return _WANT[key]


def _run_engine(eng, ref, d, K, temp, seed=0, bpr=False):
    from furusato_recommend_amd.engine import AdamState
    E = ref.emb(d, seed).clone().cuda()
    adam = AdamState(E, lr=LR)
    tabs, losses = [], []
    for t in range(2):
        u, p, n = _dev(ref.batch(t, K))
        if bpr:
            loss = eng.train_step(E, adam, u, p, n[:, 0].contiguous(), DECAY)
        else:
            loss = eng.train_step_ssm(E, adam, u, p, n, DECAY, temp)
        losses.append(float(loss))
        tabs.append(E.clone())
    torch.cuda.synchronize()
    return tabs, losses


def _check(tag, tabs, losses, want_tabs, want_loss):
    for t in range(2):
        e_l = abs(losses[t] - want_loss[t]) / abs(want_loss[t])
        e_t = rel(tabs[t], want_tabs[t])
        print(f"{tag} step {t}: loss {e_l:.2e} table {e_t:.2e}")
        assert e_l < TOL and e_t < TOL


# -------------------------------------------------------------- engine steps
@pytest.mark.parametrize("temp", [1.0, 0.2])
@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("prune", [True, False])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("d", [16, 64])
def test_engine_steps_match_float64_autograd(ref, graph, d, L, prune, K, temp):
    from furusato_recommend_amd.engine import PropagationEngine
    want_tabs, want_loss = _want(ref, d, L, K, temp)
    runs = []
    for _ in range(2):                                     # two engines: bitwise repeatable
        eng = PropagationEngine(graph, d, L, 64, prune=prune, n_neg=K)
        runs.append(_run_engine(eng, ref, d, K, temp))
        assert eng._seeds is None and not eng._masks_ready
        assert int(eng.slot.max()) == -1                   # the slot map is reset
    (tabs, losses), (tabs2, losses2) = runs
    assert losses == losses2 and all(torch.equal(a, b) for a, b in zip(tabs, tabs2))
    _check(f"d={d} L={L} prune={prune} K={K} temp={temp}", tabs, losses, want_tabs, want_loss)
    # the loss is this one: the K = 1, temp = 1 steps are visibly elsewhere
    if K != 1:
        other, _ = _want(ref, d, L, 1, 1.0)
        assert rel(other[1], want_tabs[1]) > 10 * TOL


@pytest.mark.parametrize("variant", ["row_mask", "bytemap", "slot", "dense", "wave_only",
                                     "n_neg_larger"])
def test_engine_step_variants_match_float64(ref, graph, variant):
    """The pruned L = 3 step through the launch forms the defaults do not
    take: rows by byte map without row lists, the first backward layer's
    neighbour filters, narrow_max = 0 (every row by a whole wave), and an
    engine built for more negatives than the batch carries."""
    from furusato_recommend_amd.engine import PropagationEngine
    d, L, K, temp = 64, 3, 8, 0.2
    want_tabs, want_loss = _want(ref, d, L, K, temp, seed=1)
    eng = PropagationEngine(graph, d, L, 64, prune=True, n_neg=16 if variant == "n_neg_larger"
                            else K)
    if variant == "row_mask":
        eng.use_hop_list = False
    elif variant == "wave_only":
        eng.narrow_max = 0
    elif variant != "n_neg_larger":
        eng.sparse_filter = variant
    tabs, losses = _run_engine(eng, ref, d, K, temp, seed=1)
    _check(variant, tabs, losses, want_tabs, want_loss)


@pytest.mark.parametrize("d,L", [(16, 1), (64, 3)])
def test_k1_temp1_is_bpr(ref, graph, d, L):
    """K = 1, temp = 1: the SSM steps, the float64 SSM reference, the float64
    BPR reference and the engine's BPR steps on the same triples all agree
    within the tolerance (not bitwise: softplus against log-sum-exp)."""
    from furusato_recommend_amd.engine import PropagationEngine
    want_tabs, want_loss = _want(ref, d, L, 1, 1.0)
    E = ref.emb(d).double().clone().requires_grad_(True)
    opt = torch.optim.Adam([E], lr=LR)
    for t in range(2):                                     # the BPR loss in float64
        opt.zero_grad()
        loss = Ref.bpr_loss(E, L, torch.from_numpy(ref.dense()), ref.batch(t, 1), DECAY)
        loss.backward()
        opt.step()
        assert abs(float(loss) - want_loss[t]) / abs(want_loss[t]) < 1e-12
    assert rel(E, want_tabs[1]) < 1e-9
    ssm = _run_engine(PropagationEngine(graph, d, L, 64, n_neg=1), ref, d, 1, 1.0)
    bpr = _run_engine(PropagationEngine(graph, d, L, 64), ref, d, 1, 1.0, bpr=True)
    _check("ssm", *ssm, want_tabs, want_loss)
    _check("bpr", *bpr, want_tabs, want_loss)
    assert rel(ssm[0][1], bpr[0][1]) < TOL


# --------------------------------------------------------------------- model
def _cfg(split=None, **over):
    cfg = {"recdim": 64, "layer": 3, "lr": LR, "decay": DECAY, "device": "cuda:0",
           "bpr_batch_size": 64, "seed": 2020}
    if split is not None:
        cfg["csr_split"] = split
    cfg.update(over)
    return cfg


def _model(ref, split=None, cls=None, **over):
    from furusato_recommend_amd import LightGCN
    m = (cls or LightGCN)(_cfg(split, **over), ref.ds)
    with torch.no_grad():
        m.all_embedding.weight.copy_(ref.emb(64))
    return m


@pytest.mark.parametrize("split", SPLITS)
def test_model_stage_one_is_the_engine_step(ref, split):
    m = _model(ref, split, loss="ssm", neg_size=8, ssm_temp=0.2)
    plain = _model(ref, split)                             # no keys: drives an engine by hand
    from furusato_recommend_amd.engine import PropagationEngine
    eng = PropagationEngine(plain.graph, 64, 3, 64, n_neg=8)
    assert m.loss_name == "ssm" and m.engine.n_neg == 8 and plain.engine.n_neg == 1
    for t in range(2):
        u, p, n = _dev(ref.batch(t, 8))
        la = m.stageOne(u, p, n)
        lb = eng.train_step_ssm(plain.all_embedding.weight, plain.optim, u, p, n, DECAY, 0.2)
        assert torch.equal(la, lb)
        assert torch.equal(m.all_embedding.weight, plain.all_embedding.weight)
    want_tabs, _ = _want(ref, 64, 3, 8, 0.2)
    assert rel(m.all_embedding.weight, want_tabs[1]) < TOL


def test_model_one_epoch_and_sample(ref):
    m = _model(ref, loss="ssm", neg_size=8, ssm_temp=0.2)
    b = [ref.batch(t, 8) for t in range(3)]
    u, p, n = (np.concatenate([x[k] for x in b]) for k in range(3))
    assert len(u) == 150 and n.shape == (150, 8)
    got = m.OneEpoch(*_dev((u, p, n)))                     # batches of 64, 64, 22
    E = ref.emb(64).double().clone().requires_grad_(True)
    opt = torch.optim.Adam([E], lr=LR)
    total = 0.0
    for t in range(3):
        opt.zero_grad()
        loss = Ref.ssm_loss(E, 3, torch.from_numpy(ref.dense()), b[t], DECAY, 0.2)
        loss.backward()
        opt.step()
        total += float(loss)
    want = total / (150 // 64 + 1)
    assert abs(float(got) - want) / want < TOL
    assert rel(m.all_embedding.weight, E) < TOL
    # sample(): [n, K] negatives, the BPR sampler's first three columns
    su, sp, sn = m.sample(500, seed=3, offset=40)
    bu, bp, bn = _model(ref).sample(500, seed=3, offset=40)
    assert sn.shape == (500, 8) and sn.dtype == torch.int32 and int(m._sample_err.item()) == 0
    assert torch.equal(su, bu) and torch.equal(sp, bp) and torch.equal(sn[:, 0], bn)


@pytest.mark.parametrize("split", SPLITS)
def test_model_softmax_loss_backward_matches_float64(ref, split):
    m = _model(ref, split, loss="ssm", neg_size=8, ssm_temp=0.2)
    batch = ref.batch(0, 8)
    loss, reg = m.softmax_loss(*_dev(batch))
    (loss + DECAY * reg).backward()
    E = ref.emb(64).double().requires_grad_(True)
    want = Ref.ssm_loss(E, 3, torch.from_numpy(ref.dense()), batch, DECAY, 0.2)
    want.backward()
    got, want = float((loss + DECAY * reg).detach()), float(want.detach())
    e_l, e_g = abs(got - want) / abs(want), rel(m.all_embedding.weight.grad, E.grad)
    print(f"split={split}: loss {e_l:.2e} grad {e_g:.2e}")
    assert e_l < TOL and e_g < TOL


def test_get_users_rating_is_unchanged(ref):
    a, b = _model(ref, loss="ssm", neg_size=8), _model(ref)
    users = torch.arange(0, NU, 7).cuda()
    assert torch.equal(a.getUsersRating(users), b.getUsersRating(users))


def _model_steps(m, ref, K):
    losses = []
    for t in range(2):
        losses.append(float(m.stageOne(*_dev(ref.batch(t, K)))))
    return losses


def test_combined_with_edge_weight(ref):
    m = _model(ref, loss="ssm", neg_size=8, ssm_temp=0.2, edge_weight=ref.weight)
    losses = _model_steps(m, ref, 8)
    M = ref.dense(weight=ref.weight)
    assert rel(M, ref.dense()) > 0.1
    want_tabs, want_loss = ref.steps(ref.emb(64), 3, [M] * 2, [ref.batch(t, 8) for t in range(2)],
                                     LR, DECAY, 0.2)
    for t in range(2):
        assert abs(losses[t] - want_loss[t]) / abs(want_loss[t]) < TOL
    assert rel(m.all_embedding.weight, want_tabs[1]) < TOL


def test_combined_with_edge_dropout(ref):
    m = _model(ref, loss="ssm", neg_size=8, ssm_temp=0.2, dropout=1, keep_prob=0.6)
    losses = _model_steps(m, ref, 8)
    mats = [ref.dense(drop=(m.dropout_seed(t), 0.6)) for t in range(2)]
    want_tabs, want_loss = ref.steps(ref.emb(64), 3, mats, [ref.batch(t, 8) for t in range(2)],
                                     LR, DECAY, 0.2)
    for t in range(2):
        assert abs(losses[t] - want_loss[t]) / abs(want_loss[t]) < TOL
    assert rel(m.all_embedding.weight, want_tabs[1]) < TOL
    assert m._drop_step == 2 and m.engine._drop is None
    assert rel(_want(ref, 64, 3, 8, 0.2)[0][1], want_tabs[1]) > 10 * TOL   # dropped steps


def test_combined_with_radj(ref):
    from furusato_recommend_amd import rAdjGCN
    m = _model(ref, cls=rAdjGCN, r=0.3, loss="ssm", neg_size=8, ssm_temp=0.2)
    losses = _model_steps(m, ref, 8)
    M = ref.dense(r=0.3)
    assert rel(M, M.T) > 0.1
    want_tabs, want_loss = ref.steps(ref.emb(64), 3, [M] * 2, [ref.batch(t, 8) for t in range(2)],
                                     LR, DECAY, 0.2)
    for t in range(2):
        assert abs(losses[t] - want_loss[t]) / abs(want_loss[t]) < TOL
    assert rel(m.all_embedding.weight, want_tabs[1]) < TOL


def test_registry_entry_defaults_to_ssm(ref):
    from furusato_recommend_amd import MODELS, LightGCNSSM
    assert MODELS["lgnssm"] is LightGCNSSM
    m = MODELS["lgnssm"](_cfg(neg_size=4), ref.ds)
    assert m.loss_name == "ssm" and m.neg_size == 4 and m.ssm_temp == 1.0
    assert m.engine.n_neg == 4 and m.engine.loss_name == "ssm"
    assert MODELS["lgnssm"](_cfg(), ref.ds).neg_size == 1
    assert MODELS["lgnssm"](_cfg(loss="bpr"), ref.ds).loss_name == "bpr"
    assert MODELS["lgn"](_cfg(), ref.ds).loss_name == "bpr"


def test_config_without_the_keys_is_the_model_as_it_was(ref):
    a, b = _model(ref, loss="bpr", neg_size=1), _model(ref)
    for t in range(2):
        u, p, n = _dev(ref.batch(t, 1))
        n = n[:, 0].contiguous()
        assert torch.equal(a.stageOne(u, p, n), b.stageOne(u, p, n))
    assert torch.equal(a.all_embedding.weight, b.all_embedding.weight)
    assert b.loss_name == "bpr" and b.engine.n_neg == 1 and b.engine.g_u is None
    assert b.engine.seed_p.shape[0] == 3 * 64 and b.engine.coef.shape[0] == 64
    # and the BPR steps are the float64 BPR steps
    want_tabs, _ = _want(ref, 64, 3, 1, 1.0)
    assert rel(b.all_embedding.weight, want_tabs[1]) < TOL


def test_trainer_runs_an_epoch(ref):
    from furusato_recommend_amd.trainer import Trainer
    cfg = _cfg(loss="ssm", neg_size=4, ssm_temp=0.5)
    m = _model(ref, loss="ssm", neg_size=4, ssm_temp=0.5)
    before = m.all_embedding.weight.detach().clone()
    loss = float(Trainer(cfg, ref.ds, m).train())
    assert np.isfinite(loss) and loss > 0
    assert not torch.equal(before, m.all_embedding.weight)
    assert bool(torch.isfinite(m.all_embedding.weight).all())


# ------------------------------------------------------------------ refusals
def test_refusals(ref):
    from furusato_recommend_amd.dist import DataParallel
    from furusato_recommend_amd.engine import PropagationEngine
    from furusato_recommend_amd.train_dp import wrap
    from furusato_recommend_amd.trainer import Trainer
    with pytest.raises(ValueError, match="loss"):
        _model(ref, loss="softmax")
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="neg_size"):
            _model(ref, loss="ssm", neg_size=bad)
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ssm_temp"):
            _model(ref, loss="ssm", ssm_temp=bad)
    m = _model(ref, loss="ssm", neg_size=4)
    u, p, n = _dev(ref.batch(0, 8))
    for wrong in (n, n[:, 0].contiguous(), n[:32, :4].contiguous()):
        with pytest.raises(ValueError, match="neg"):
            m.stageOne(u, p, wrong)
        with pytest.raises(ValueError, match="neg"):
            m.OneEpoch(u, p, wrong)
        with pytest.raises(ValueError, match="neg"):
            m.softmax_loss(u, p, wrong)
    with pytest.raises(ValueError, match="ddp_capped"):
        Trainer(_cfg(loss="ssm", neg_size=4, sampler="ddp_capped"), ref.ds, m)
    with pytest.raises(NotImplementedError, match="softmax"):
        wrap(m)
    with pytest.raises(NotImplementedError, match="softmax"):
        DataParallel(m.engine, m.all_embedding.weight.data, m.optim)
    eng = PropagationEngine(m.graph, 64, 3, 64, n_neg=2)   # n_neg > 1 alone is refused too
    with pytest.raises(NotImplementedError, match="softmax"):
        DataParallel(eng, m.all_embedding.weight.data, m.optim)
    with pytest.raises(ValueError, match="n_neg"):
        PropagationEngine(m.graph, 64, 3, 64, n_neg=0)
    with pytest.raises(ValueError, match="n_neg"):
        eng.train_step_ssm(m.all_embedding.weight, m.optim, u, p, n, DECAY, 1.0)  # K = 8 > 2
    with pytest.raises(ValueError, match="temp"):
        eng.ssm(eng.acc, m.all_embedding.weight, u, p, n[:, :2].contiguous(), DECAY, 0.0)
    assert not eng._masks_ready and eng._seeds is None

