"""Full-rank evaluation on the host: rank_metrics against
brute force, evaluate_ranked on a CPU model against evaluate(), and the
Trainer option."""
import numpy as np
import torch

from tests.rank_common import (brute_counts, brute_mrr_auc, make_targets, sorted_lists,
                               train_mask)


def test_rank_metrics_match_brute_force():
    """rank_metrics on exact counts of heavily tied float64 scores (integer
    embeddings in [-2, 2], d = 8, 40 users x 57 items): precision / recall /
    ndcg / hr at k = 1, 5, 20, 57 are test_one_batch's sums on the fully
    sorted non-train lists, mrr and auc the direct computation.  User 0's
    only test item is a train positive; user 1 has no negatives (every
    non-train item is a test item)."""
    from furusato_recommend_amd.metric import rank_metrics, test_one_batch
    rng = np.random.default_rng(0)
    n, m, d = 40, 57, 8
    U = rng.integers(-2, 3, (n, d)).astype(np.float64)
    I = rng.integers(-2, 3, (m, d)).astype(np.float64)
    s = U @ I.T
    train_lists = [rng.choice(m, size=rng.integers(1, 12), replace=False) for _ in range(n)]
    test_lists = []
    for u in range(n):
        free = np.setdiff1d(np.arange(m), train_lists[u])
        pick = rng.choice(free, size=rng.integers(1, 6), replace=False).tolist()
        if u % 7 == 3:  # a train positive among the test items
            pick.append(int(train_lists[u][0]))
        test_lists.append(sorted(pick))
    test_lists[0] = [int(train_lists[0][0])]
    test_lists[1] = np.setdiff1d(np.arange(m), train_lists[1]).tolist()
    train = train_mask(train_lists, np.arange(n), m)
    tptr, targets = make_targets(test_lists)
    score, gt, eq, eql, masked = brute_counts(s, train, tptr, targets)
    assert masked[tptr[0]] and masked.sum() >= 2
    topks = (1, 5, 20, 57)
    n_gt = np.array([len(x) for x in test_lists])
    n_train = train.sum(1)
    r = rank_metrics(tptr, score, gt, eq, eql, masked, n_gt, n_train, m, topks,
                     return_ranks=True)
    lists = sorted_lists(s, train)
    ref = test_one_batch(lists, test_lists, topks)
    for key in ("precision", "recall", "ndcg", "hr"):
        assert np.array_equal(r[key], ref[key]), key
    # ranks: the position in the sorted list, 0 for a masked target
    slot = np.repeat(np.arange(n), np.diff(tptr))
    for p, t in enumerate(targets):
        where = np.nonzero(lists[slot[p]] == t)[0]
        assert r["ranks"][p] == (0 if masked[p] else where[0] + 1)
    mrr, auc, n_auc = brute_mrr_auc(s, train, test_lists)
    assert n_auc == r["auc_users"] == n - 2  # users 0 (no P) and 1 (no N) left out
    assert abs(r["mrr"] - mrr) < 1e-12
    assert abs(r["auc"] - auc) < 1e-12


def _cpu_mf():
    from furusato_recommend_amd import MF, SyntheticBipartite
    ds = SyntheticBipartite(400, 90, 5000, test_frac=0.3)
    torch.manual_seed(3)
    m = MF({"latent_dim_rec": 32, "lr": 1e-3, "decay": 1e-4, "device": "cpu",
            "bpr_batch_size": 256, "n_threads": 2}, ds)
    return ds, m


def test_evaluate_ranked_cpu_model_matches_evaluate():
    """A CPU MF model: the four shared metrics of evaluate_ranked equal
    evaluate()'s exactly at (10, 20); (50, 90) — where evaluate() would need
    torch.topk of the whole row — runs, and the AUC agrees with the direct
    float64 computation on the same f32 scores."""
    from furusato_recommend_amd.evaluate import evaluate, evaluate_ranked
    ds, m = _cpu_mf()
    a = evaluate(m, ds.testDict, (10, 20), batch=150)
    b = evaluate_ranked(m, ds.testDict, (10, 20), batch=150, return_ranks=True)
    for key in ("precision", "recall", "ndcg", "hr"):
        assert np.array_equal(a[key], b[key]), key
    assert 0.0 < b["mrr"] <= 1.0 and 0.0 < b["auc"] < 1.0
    users = sorted(ds.testDict)
    assert b["ranks"].shape == (sum(len(set(ds.testDict[u])) for u in users),)
    c = evaluate_ranked(m, ds.testDict, (50, 90), batch=150)
    assert np.all(c["recall"] >= b["recall"][-1]) and c["recall"][1] <= 1.0
    assert c["mrr"] == b["mrr"] and c["auc"] == b["auc"]
    # mrr / auc against the rows themselves
    Ue, Ie = m.eval_embeddings()
    s = (Ue[torch.tensor(users)] @ Ie.t()).double().numpy()
    train = train_mask(ds.allPos, users, ds.m_items)
    mrr, auc, n_auc = brute_mrr_auc(s, train, [ds.testDict[u] for u in users])
    assert abs(b["mrr"] - mrr / len(users)) < 1e-12
    assert abs(b["auc"] - auc / n_auc) < 1e-12


def test_trainer_eval_rank_option():
    """Trainer.test: config["eval_rank"] adds "mrr" and "auc" and leaves the
    four shared metrics as they are; without it the keys are as before."""
    from furusato_recommend_amd.trainer import Trainer
    ds, m = _cpu_mf()
    plain = Trainer({"topks": (10, 20), "test_u_batch_size": 200}, ds, m).test()
    assert sorted(plain) == ["hr", "ndcg", "precision", "recall"]
    ranked = Trainer({"topks": (10, 20), "test_u_batch_size": 200, "eval_rank": True}, ds,
                     m).test()
    assert sorted(ranked) == ["auc", "hr", "mrr", "ndcg", "precision", "recall"]
    for key in plain:
        assert np.array_equal(plain[key], ranked[key]), key
