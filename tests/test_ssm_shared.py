"""The shared-negative sampled-softmax loss on the GPU through
the engine and the model: PropagationEngine.train_step_ssm_shared (frontier
pruning, fused Adam), LightGCN with config["neg_shared"] (stageOne, OneEpoch,
sample, softmax_loss), its combinations with edge weights, edge dropout and
rAdjGCN, the 'lgnssm' registry entry, the Trainer and the refusals.

The float64 reference: tests/ssm_common.Ref's graph (300 users x 40 items, hub
item 0, isolated item 39, multi-edges), batches and dense propagation
matrices, with this loss in torch autograd and torch.optim.Adam, two
consecutive steps.  The shared set is the 24 ids [0, 39, 5, 5, 10 .. 29]: the
hub (masked for every pair), the isolated item, a repeated id.  On that graph
and those batches 0.20 - 0.23 of the [B, 24] cells are masked, no pair is
fully masked or fully unmasked and 14 - 41 pairs per batch have their ``pos``
in the set (the ``ref`` fixture asserts the share and the first two facts).

Tolerance: the project's 1e-4 relative error in the max norm against float64
(tests/test_ssm.py), on the losses and on the stepped tables."""
import ctypes

import numpy as np
import pytest
import torch

from tests.ssm_common import MI, NU, N, Ref, rel

pytestmark = pytest.mark.gpu
TOL = 1e-4
SPLITS = [None, 32]
LR, DECAY = 1e-2, 1e-3
SHARED = np.array([0, 39, 5, 5] + list(range(10, 30)), np.int64)


def _mask(r, u, p, shared):
    member = np.zeros((NU, MI), bool)
    user_rows = r.rows < NU
    member[r.rows[user_rows], r.col[user_rows] - NU] = True
    return member[u][:, shared] | (np.asarray(shared)[None, :] == np.asarray(p)[:, None])


@pytest.fixture(scope="module")
def ref():
    r = Ref()
    assert r.deg[NU] >= 300 and r.deg[N - 1] == 0          # the hub, the isolated item
    assert len(SHARED) == 24
    for u, p, _ in r.batches:
        m = _mask(r, u, p, SHARED)
        assert 0.1 < m.mean() < 0.3                        # neither vacuous nor total
        assert not m.all(1).any() and not (~m).all(1).any()
        assert m[:, 0].all() and np.isin(p, SHARED).sum() >= 10
    return r


@pytest.fixture(scope="module", params=SPLITS, ids=lambda s: f"split{s}")
def graph(request, ref):
    from furusato_recommend_amd.graph import DEFAULT_SPLIT, Graph
    split = request.param
    g = Graph.from_interactions(ref.ds.trainUser, ref.ds.trainItem, NU, MI, "cuda:0",
                                split=DEFAULT_SPLIT if split is None else split)
    assert np.array_equal(g.col_host, ref.col)
    return g


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().int().contiguous()


def shared_loss(r, E, L, M, u, p, shared, decay, temp):
    """The loss of DESIGN.md §19 in torch (any dtype of E): masked
    candidates leave the softmax, a shared row's norm counts once per slot."""
    out = Ref.out(E, L, M)
    mask = torch.from_numpy(_mask(r, u, p, shared))
    ut, pt, st = (torch.from_numpy(np.asarray(a)).long() for a in (u, p, shared))
    pt, st = pt + NU, st + NU
    sp = (out[ut] * out[pt]).sum(1) / temp
    sn = (out[ut] @ out[st].T / temp).masked_fill(mask, float("-inf"))
    terms = torch.logsumexp(torch.cat([sp[:, None], sn], 1), 1) - sp
    reg = 0.5 * (E[ut].pow(2).sum() + E[pt].pow(2).sum() + E[st].pow(2).sum()) / len(u)
    return terms.mean() + decay * reg


def _steps(r, E0, L, mats, temp, shared=SHARED, n=2):
    E = E0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([E], lr=LR)
    tabs, losses = [], []
    for t in range(n):
        u, p, _ = r.batches[t]
        opt.zero_grad()
        loss = shared_loss(r, E, L, torch.from_numpy(mats[t]), u, p, shared, DECAY, temp)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        tabs.append(E.detach().clone())
    return tabs, losses


_WANT = {}


def _want(r, d, L, temp):
    key = (d, L, temp)
    if key not in _WANT:
        _WANT[key] = _steps(r, r.emb(d), L, [r.dense()] * 2, temp)
    return _WANT[key]


def _run_engine(eng, r, d, temp, shared=SHARED):
    from furusato_recommend_amd.engine import AdamState
    E = r.emb(d).clone().cuda()
    adam = AdamState(E, lr=LR)
    sh = _i32(shared)
    tabs, losses = [], []
    for t in range(2):
        u, p, _ = r.batches[t]
        loss = eng.train_step_ssm_shared(E, adam, _i32(u), _i32(p), sh, DECAY, temp)
        losses.append(float(loss))
        tabs.append(E.clone())
    torch.cuda.synchronize()
    return tabs, losses


def _check(tag, tabs, losses, want_tabs, want_loss):
    for t in range(len(losses)):
        e_l = abs(losses[t] - want_loss[t]) / abs(want_loss[t])
        e_t = rel(tabs[t], want_tabs[t])
        print(f"{tag} step {t}: loss {e_l:.2e} table {e_t:.2e}")
        assert e_l < TOL and e_t < TOL


# -------------------------------------------------------------- engine steps
@pytest.mark.parametrize("temp", [1.0, 0.2])
@pytest.mark.parametrize("prune", [True, False])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("d", [16, 64])
def test_engine_steps_match_float64_autograd(ref, graph, d, L, prune, temp):
    from furusato_recommend_amd.engine import PropagationEngine
    want_tabs, want_loss = _want(ref, d, L, temp)
    runs = []
    for _ in range(2):                                     # two engines: bitwise repeatable
        eng = PropagationEngine(graph, d, L, 64, prune=prune, n_shared=24)
        runs.append(_run_engine(eng, ref, d, temp))
        assert eng._seeds is None and not eng._masks_ready
        assert int(eng.slot.max()) == -1                   # the slot map is reset
    (tabs, losses), (tabs2, losses2) = runs
    assert losses == losses2 and all(torch.equal(a, b) for a, b in zip(tabs, tabs2))
    _check(f"d={d} L={L} prune={prune} temp={temp}", tabs, losses, want_tabs, want_loss)
    # the loss is this one: the K = 8 per-pair steps are visibly elsewhere
    key = ("per-pair", d, L, temp)
    if key not in _WANT:
        _WANT[key] = ref.steps(ref.emb(d), L, [ref.dense()] * 2,
                               [ref.batch(t, 8) for t in range(2)], LR, DECAY, temp)
    assert rel(_WANT[key][0][1], want_tabs[1]) > 10 * TOL


def test_all_masked_set_leaves_the_reg_term(ref, graph):
    """shared = [0]: the hub masks every pair, the loss is decay * reg and the
    table moves by the reg gradient alone."""
    from furusato_recommend_amd.engine import PropagationEngine
    d, L = 64, 3
    shared = np.array([0], np.int64)
    want_tabs, want_loss = _steps(ref, ref.emb(d), L, [ref.dense()] * 2, 0.2, shared=shared)
    E0 = ref.emb(d).double()
    u, p, _ = ref.batches[0]
    reg = 0.5 * (E0[u].pow(2).sum() + E0[p + NU].pow(2).sum() + E0[NU].pow(2).sum()) / len(u)
    assert abs(want_loss[0] - DECAY * float(reg)) <= 1e-15
    tabs, losses = _run_engine(PropagationEngine(graph, d, L, 64, n_shared=1), ref, d, 0.2,
                               shared=shared)
    _check("all masked", tabs, losses, want_tabs, want_loss)
    touched = np.unique(np.r_[u, p + NU, NU])
    rest = np.setdiff1d(np.arange(N), touched)
    assert torch.equal(tabs[0][rest].cpu(), ref.emb(d)[rest])   # no gradient elsewhere


def test_oversized_engine(ref, graph):
    from furusato_recommend_amd.engine import PropagationEngine
    want_tabs, want_loss = _want(ref, 64, 3, 0.2)
    eng = PropagationEngine(graph, 64, 3, 128, n_shared=200)
    assert eng.seed_p.shape[0] == 2 * 128 + 200 and eng.self_list.shape[0] == 2 * 128 + 200
    tabs, losses = _run_engine(eng, ref, 64, 0.2)
    _check("oversized", tabs, losses, want_tabs, want_loss)
    same = _run_engine(PropagationEngine(graph, 64, 3, 64, n_shared=24), ref, 64, 0.2)
    assert losses == same[1] and torch.equal(tabs[1], same[0][1])
    # n_shared = 0 leaves every buffer at its size
    plain = PropagationEngine(graph, 64, 3, 64)
    assert plain.seed_p.shape[0] == 3 * 64 and plain.keys.shape[0] == 3 * 64
    assert plain.self_list.shape[0] == 3 * 64 and plain._shared is None


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


_SH = dict(loss="ssm", neg_shared=24, ssm_temp=0.2)


@pytest.mark.parametrize("split", SPLITS)
def test_model_stage_one_is_the_engine_step(ref, split):
    from furusato_recommend_amd.engine import PropagationEngine
    m = _model(ref, split, **_SH)
    plain = _model(ref, split)
    eng = PropagationEngine(plain.graph, 64, 3, 64, n_shared=24)
    assert m.neg_shared == 24 and m.engine.n_shared == 24 and plain.engine.n_shared == 0
    sh = _i32(SHARED)
    for t in range(2):
        u, p, _ = ref.batches[t]
        la = m.stageOne(_i32(u), _i32(p), sh)
        lb = eng.train_step_ssm_shared(plain.all_embedding.weight, plain.optim, _i32(u), _i32(p),
                                       sh, DECAY, 0.2)
        assert torch.equal(la, lb)
        assert torch.equal(m.all_embedding.weight, plain.all_embedding.weight)
    assert rel(m.all_embedding.weight, _want(ref, 64, 3, 0.2)[0][1]) < TOL


def test_model_one_epoch_over_sample(ref):
    from furusato_recommend_amd import _lib
    a, b = _model(ref, **_SH), _model(ref, **_SH)
    u, p, sets = a.sample(150, seed=3, offset=40)
    bu, bp, _ = _model(ref).sample(150, seed=3, offset=40)
    assert torch.equal(u, bu) and torch.equal(p, bp) and int(a._sample_err.item()) == 0
    assert sets.shape == (3, 24) and sets.dtype == torch.int32
    host = np.full(3 * 24, -7, np.int32)
    assert _lib.lib.mirec_cpu_shared_sample(MI, 3, 24, ctypes.c_uint64(3), ctypes.c_uint64(40),
                                            host.ctypes.data, 1) == 0
    assert np.array_equal(sets.cpu().numpy().reshape(-1), host)
    got = a.OneEpoch(u, p, sets)                           # batches of 64, 64, 22
    total = 0.0
    for k, i in enumerate(range(0, 150, 64)):
        total += float(b.stageOne(u[i:i + 64], p[i:i + 64], sets[k]))
    assert torch.equal(a.all_embedding.weight, b.all_embedding.weight)
    assert abs(float(got) - total / 3) <= 1e-6 * abs(total / 3)
    # and against float64, with the sampled sets
    E = ref.emb(64).double().clone().requires_grad_(True)
    opt = torch.optim.Adam([E], lr=LR)
    un, pn, sn = u.cpu().numpy(), p.cpu().numpy(), sets.cpu().numpy()
    for k, i in enumerate(range(0, 150, 64)):
        opt.zero_grad()
        shared_loss(ref, E, 3, torch.from_numpy(ref.dense()), un[i:i + 64], pn[i:i + 64], sn[k],
                    DECAY, 0.2).backward()
        opt.step()
    assert rel(a.all_embedding.weight, E) < TOL


@pytest.mark.parametrize("split", SPLITS)
def test_model_softmax_loss_backward_matches_float64(ref, split):
    m = _model(ref, split, **_SH)
    u, p, _ = ref.batches[0]
    loss, reg = m.softmax_loss(_i32(u), _i32(p), _i32(SHARED))
    (loss + DECAY * reg).backward()
    E = ref.emb(64).double().requires_grad_(True)
    want = shared_loss(ref, E, 3, torch.from_numpy(ref.dense()), u, p, SHARED, DECAY, 0.2)
    want.backward()
    got, want = float((loss + DECAY * reg).detach()), float(want.detach())
    e_l, e_g = abs(got - want) / abs(want), rel(m.all_embedding.weight.grad, E.grad)
    print(f"split={split}: loss {e_l:.2e} grad {e_g:.2e}")
    assert e_l < TOL and e_g < TOL


def test_get_users_rating_is_unchanged(ref):
    a, b = _model(ref, **_SH), _model(ref)
    users = torch.arange(0, NU, 7).cuda()
    assert torch.equal(a.getUsersRating(users), b.getUsersRating(users))


def test_config_without_the_key_is_the_model_as_it_was(ref):
    for over in (dict(loss="ssm", neg_size=8, ssm_temp=0.2), dict()):
        a, b = _model(ref, neg_shared=None, **over), _model(ref, **over)
        assert a.neg_shared is None and b.neg_shared is None and a.engine.n_shared == 0
        for t in range(2):
            u, p, n = (_i32(x) for x in ref.batch(t, 8))
            if not over:
                n = n[:, 0].contiguous()
            assert torch.equal(a.stageOne(u, p, n), b.stageOne(u, p, n))
        assert torch.equal(a.all_embedding.weight, b.all_embedding.weight)
        assert a.engine._shared is None and a.engine.seed_p.shape == b.engine.seed_p.shape
    want_tabs, _ = ref.steps(ref.emb(64), 3, [ref.dense()] * 2,
                             [ref.batch(t, 1) for t in range(2)], LR, DECAY, 1.0)
    assert rel(a.all_embedding.weight, want_tabs[1]) < TOL   # the BPR steps, as before


def _model_steps(m, ref):
    sh = _i32(SHARED)
    return [float(m.stageOne(_i32(ref.batches[t][0]), _i32(ref.batches[t][1]), sh))
            for t in range(2)]


def _check_model(m, losses, want_tabs, want_loss):
    for t in range(2):
        assert abs(losses[t] - want_loss[t]) / abs(want_loss[t]) < TOL
    assert rel(m.all_embedding.weight, want_tabs[1]) < TOL


def test_combined_with_edge_weight(ref):
    m = _model(ref, edge_weight=ref.weight, **_SH)
    losses = _model_steps(m, ref)
    _check_model(m, losses, *_steps(ref, ref.emb(64), 3, [ref.dense(weight=ref.weight)] * 2, 0.2))


def test_combined_with_edge_dropout(ref):
    m = _model(ref, dropout=1, keep_prob=0.6, **_SH)
    losses = _model_steps(m, ref)
    mats = [ref.dense(drop=(m.dropout_seed(t), 0.6)) for t in range(2)]
    want_tabs, want_loss = _steps(ref, ref.emb(64), 3, mats, 0.2)
    _check_model(m, losses, want_tabs, want_loss)
    assert m._drop_step == 2 and m.engine._drop is None
    assert rel(_want(ref, 64, 3, 0.2)[0][1], want_tabs[1]) > 10 * TOL   # dropped steps


def test_combined_with_radj(ref):
    from furusato_recommend_amd import rAdjGCN
    m = _model(ref, cls=rAdjGCN, r=0.3, **_SH)
    losses = _model_steps(m, ref)
    _check_model(m, losses, *_steps(ref, ref.emb(64), 3, [ref.dense(r=0.3)] * 2, 0.2))


def test_registry_entry_and_trainer(ref):
    from furusato_recommend_amd import MODELS
    from furusato_recommend_amd.trainer import Trainer
    cfg = _cfg(neg_shared=24, ssm_temp=0.5)
    m = MODELS["lgnssm"](cfg, ref.ds)
    assert m.loss_name == "ssm" and m.neg_shared == 24 and m.engine.n_shared == 24
    losses = _model_steps(m, ref)
    assert all(np.isfinite(x) and x > 0 for x in losses)
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
    with pytest.raises(ValueError, match="neg_shared"):
        _model(ref, loss="bpr", neg_shared=24)
    with pytest.raises(ValueError, match="neg_shared"):
        _model(ref, neg_shared=24)                         # LightGCN's default loss is BPR
    with pytest.raises(ValueError, match="neg_shared"):
        _model(ref, loss="ssm", neg_size=4, neg_shared=24)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="neg_shared"):
            _model(ref, loss="ssm", neg_shared=bad)
    m = _model(ref, **_SH)
    u, p, n = (_i32(x) for x in ref.batch(0, 8))
    sh = _i32(SHARED)
    for wrong in (n, sh[:23].contiguous(), sh[None, :].contiguous()):
        with pytest.raises(ValueError, match="neg"):
            m.stageOne(u, p, wrong)
        with pytest.raises(ValueError, match="neg"):
            m.softmax_loss(u, p, wrong)
    for wrong in (sh, sh[None, :].repeat(2, 1).contiguous(), n):
        with pytest.raises(ValueError, match="neg"):
            m.OneEpoch(u, p, wrong)                        # 64 pairs: one set of 24 expected
    with pytest.raises(ValueError, match="ddp_capped"):
        Trainer(_cfg(sampler="ddp_capped", **_SH), ref.ds, m)
    with pytest.raises(NotImplementedError, match="softmax"):
        wrap(m)
    with pytest.raises(NotImplementedError, match="softmax"):
        DataParallel(m.engine, m.all_embedding.weight.data, m.optim)
    with pytest.raises(ValueError, match="n_shared"):
        PropagationEngine(m.graph, 64, 3, 64, n_shared=-1)
    eng = PropagationEngine(m.graph, 64, 3, 64, n_shared=8)
    with pytest.raises(ValueError, match="n_shared"):
        eng.train_step_ssm_shared(m.all_embedding.weight, m.optim, u, p, sh, DECAY, 1.0)
    with pytest.raises(ValueError, match="temp"):
        eng.ssm_shared(eng.acc, m.all_embedding.weight, u, p, sh[:8].contiguous(), DECAY, 0.0)
    with pytest.raises(ValueError, match="int32"):
        eng.ssm_shared(eng.acc, m.all_embedding.weight, u, p, sh[:8].long(), DECAY, 1.0)
    assert not eng._masks_ready and eng._seeds is None
    assert int(eng.slot.max()) == -1
