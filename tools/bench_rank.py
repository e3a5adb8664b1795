"""Full-rank evaluation on the C2 shape (1 M users x 100 K items, 20 M
edges; a batch of 10 K users): mirec_score_rank against mirec_score_topk at
k = 20 on the same inputs and against the dense way it replaces (library
GEMM writes the [batch, M] ratings, train positives set to -1024, a
compare-and-sum against the thresholds).  The three alternate inside every
repetition; one JSON line per (width, targets, path): the median ms per
10 K users of --reps repetitions after a warm-up.

Targets: "split" — the test split's own items (SyntheticBipartite moves one
edge per test user, so one pair per user) — and "x5", five distinct items
per user, which shows what a row per pair costs when users have several.

    python tools/bench_rank.py [--dims 64,256] [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--dims", default="64,256")
    ap.add_argument("--batch", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from furusato_recommend_amd import SyntheticBipartite
    from furusato_recommend_amd.evaluate import _train_pairs, score_rank, score_topk
    from furusato_recommend_amd.graph import Graph
    ds = SyntheticBipartite(a.users, a.items, a.edges, seed=0, test_frac=0.1)
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, "cuda:0")
    test_users = np.array(sorted(ds.testDict), dtype=np.int64)[: a.batch]
    n = len(test_users)
    bu = torch.from_numpy(test_users).cuda()
    rng = np.random.default_rng(0)
    sets = {"split": [np.unique(ds.testDict[int(u)]) for u in test_users],
            "x5": [np.sort(rng.choice(a.items, size=5, replace=False)) for _ in test_users]}
    rows, its = _train_pairs(g, test_users, a.items)
    rows, its = torch.from_numpy(rows).cuda(), torch.from_numpy(its).cuda()
    lines = []
    for d in [int(x) for x in a.dims.split(",")]:
        gen = torch.Generator(device="cuda").manual_seed(d)
        U = 0.1 * torch.randn(n, d, device="cuda", generator=gen)
        I = 0.1 * torch.randn(a.items, d, device="cuda", generator=gen)
        for name, lists in sets.items():
            tptr = np.zeros(n + 1, dtype=np.int64)
            tptr[1:] = np.cumsum([len(x) for x in lists])
            targets = torch.from_numpy(np.concatenate(lists)).cuda()
            slot = torch.from_numpy(np.repeat(np.arange(n), np.diff(tptr))).cuda()

            def rank():
                return score_rank(U, I, bu, tptr, targets, g)

            def topk():
                return score_topk(U, I, bu, g, a.k)

            def dense():
                rating = U @ I.t()
                thr = rating[slot, targets]
                rating[rows, its] = -1024.0
                out = []
                for c in range(0, len(targets), n):  # a [n, M] compare per round of pairs
                    r, th = rating[slot[c:c + n]], thr[c:c + n, None]
                    out.append(((r > th).sum(1), (r == th).sum(1)))
                return out

            paths = (("score_rank", rank), ("score_topk", topk), ("dense", dense))
            ms = {p: [] for p, _ in paths}
            for rep in range(a.reps + 2):
                for p, fn in paths:
                    s, e = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                    s.record()
                    fn()
                    e.record()
                    torch.cuda.synchronize()
                    if rep >= 2:
                        ms[p].append(s.elapsed_time(e))
            for p, _ in paths:
                line = {"path": p, "dim": d, "targets": name, "pairs": int(tptr[-1]),
                        "batch_users": n, "items": a.items,
                        "ms_per_batch_median": round(statistics.median(ms[p]), 3),
                        "ms_min": round(min(ms[p]), 3), "ms_max": round(max(ms[p]), 3),
                        "reps": a.reps, "device": torch.cuda.get_device_name(0)}
                if p == "score_topk":
                    line["k"] = a.k
                lines.append(json.dumps(line))
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
