"""The layer sum of a pruned forward on the batch rows only
(``PropagationEngine.layer_sum_rows``).

The loss reads ``acc`` on S alone, so with "self" every layer below the last
adds to it on the rows of S only (out_mask = bm_self); "hop" is the earlier
behaviour (F1 rows through layer L-1).  Neither changes an operand or an
order of a sum: on S, and in everything a training step leaves behind, the
two are equal bit for bit, and the layer buffers ``xs`` do not see the switch."""
import pytest
import torch

pytestmark = pytest.mark.gpu
D, B = 64, 64
SIZES = dict(wave_items=(40, 256), wave_users=(100, 64), max_grid=16)


@pytest.fixture(scope="module")
def dataset():
    from furusato_recommend_amd import SyntheticBipartite
    return SyntheticBipartite(3000, 700, 40000, seed=1, test_frac=0)


def run(ds, n_layers, mode, repeat=False):
    from furusato_recommend_amd.engine import AdamState, PropagationEngine, sample_triples
    from furusato_recommend_amd.graph import Graph
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    eng = PropagationEngine(g, D, n_layers, B)
    eng.set_sweep_sizes(**SIZES)
    eng.layer_sum_rows = mode
    for x in eng.xs:
        x.zero_()
    torch.manual_seed(0)
    emb = (0.1 * torch.randn(g.n_nodes, D)).cuda()
    adam = AdamState(emb, lr=1e-2)
    u = torch.empty(B, dtype=torch.int32, device="cuda")
    p, n = torch.empty_like(u), torch.empty_like(u)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    res = {}
    for s in range(2):
        sample_triples(g, B, 0, s * B, u, p, n, err)
        if repeat:  # the same user, positive and negative several times over
            u[1:4], p[1:3], n[5] = u[0], p[0], n[0]
        if s == 0:
            acc = eng.forward_for_batch(emb, u, p, n)
            rows = torch.cat([u, p + g.n_users, n + g.n_users]).long().unique()
            res["rows"], res["acc_S"] = rows, acc[rows].clone()
            res["xs"] = [x.clone() for x in eng.xs]
        res[f"loss{s}"] = float(eng.train_step(emb, adam, u, p, n, 1e-4))
    torch.cuda.synchronize()
    res["state"] = (emb, adam.exp_avg, adam.exp_avg_sq)
    return res


@pytest.mark.parametrize("n_layers,repeat", [(1, False), (2, False), (3, False), (4, False),
                                             (3, True)])
def test_self_equals_hop(dataset, n_layers, repeat):
    a, b = run(dataset, n_layers, "self", repeat), run(dataset, n_layers, "hop", repeat)
    assert torch.equal(a["rows"], b["rows"]) and a["rows"].numel() > B
    assert float(a["acc_S"].abs().max()) > 0
    assert torch.equal(a["acc_S"], b["acc_S"])
    assert a["loss0"] == b["loss0"] and a["loss1"] == b["loss1"]
    for x, y in zip(a["state"], b["state"]):
        assert torch.equal(x, y)
    assert len(a["xs"]) == min(n_layers, 2)
    for x, y in zip(a["xs"], b["xs"]):
        assert torch.equal(x, y)


def test_switch_is_checked(dataset):
    from furusato_recommend_amd.engine import PropagationEngine
    from furusato_recommend_amd.graph import Graph
    ds = dataset
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    eng = PropagationEngine(g, D, 3, B)
    eng.layer_sum_rows = "all"
    with pytest.raises(ValueError):
        eng.forward(torch.zeros(g.n_nodes, D, device="cuda"))
