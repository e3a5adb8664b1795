"""Cost of an edge-dropped propagation launch, and of a dropped training
step, at the C2 shape.

Times ONE full PRESCALED launch with addend, `out` and `xs_out` (every row, no
masks: a forward layer of an unpruned pass) of LightGCN d = 64 on the bench.py
C2 graph (1 M users, 100 k items, 20 M interactions, uniform):

  drop_1.0 / drop_0.8 / drop_0.6   the dropout instantiation at that keep_prob
                                   (1.0 hashes and keeps everything)
  row                              the undropped row kernel (use_sweep = False)
  shipped                          the undropped launch as shipped (column sweep)

interleaved, then a training step (B = 2048, L = 3, frontier pruning) undropped
and at keep_prob 0.6 with a new mask per step, interleaved too.  Each figure is
the median (and p10-p90) of --reps device-event timings after --warmup rounds;
prints one JSON line (and writes --out).

    python tools/bench_edge_dropout.py --out profiles/edge_dropout_c2.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from furusato_recommend_amd import SyntheticBipartite  # noqa: E402
from furusato_recommend_amd._lib import IN_PRESCALED  # noqa: E402
from furusato_recommend_amd.engine import (AdamState, PropagationEngine,  # noqa: E402
                                           prop_launch_bytes, sample_triples)
from furusato_recommend_amd.graph import Graph  # noqa: E402

KEEP = (1.0, 0.8, 0.6)


def stat(ts):
    ts = sorted(ts)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(ts[0], 4),
            "max_ms": round(ts[-1], 4),
            "p10_ms": round(ts[len(ts) // 10], 4), "p90_ms": round(ts[-1 - len(ts) // 10], 4)}


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_edge_dropout: needs a HIP device")
    dev = "cuda:0"
    ds = SyntheticBipartite(args.users, args.items, args.edges, seed=0, kind="uniform")
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, dev)
    D, L, B = args.dim, args.layers, args.batch
    eng = PropagationEngine(g, D, L, B)
    x = torch.randn(g.n_nodes, D, device=dev) * 0.1
    add = torch.randn(g.n_nodes, D, device=dev) * 0.1
    out, xs = torch.empty_like(x), torch.empty_like(x)
    it = 0

    def launch(keep_prob, sweep):
        eng.use_sweep = sweep
        eng.set_dropout(keep_prob, 1000 + it)  # None: the full graph; a new mask per round
        eng._prop(in_mode=IN_PRESCALED, x_in=x, addend=add, out=out, xs_out=xs)
        eng.set_dropout(None)

    legs = {f"drop_{p}": (p, False) for p in KEEP}
    legs.update(row=(None, False), shipped=(None, True))
    times = {k: [] for k in legs}
    for it in range(args.warmup + args.reps):
        for name, (p, sweep) in legs.items():
            t = timed(lambda: launch(p, sweep))
            if it >= args.warmup:
                times[name].append(t)
    eng.use_sweep = True

    # a training step, undropped and dropped, on the same table and triples
    emb = (torch.randn(g.n_nodes, D, device=dev) * 0.1).contiguous()
    adam = AdamState(emb, lr=1e-3)
    u, p_, n = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    steps = {"step_undropped": None, "step_drop_0.6": 0.6}
    t_step = {k: [] for k in steps}
    for it in range(args.warmup + args.reps):
        sample_triples(g, B, 7, it * B, u, p_, n, err)
        for name, kp in steps.items():
            drop = None if kp is None else (kp, PropagationEngine.dropout_seed(2020, it))
            t = timed(lambda: eng.train_step(emb, adam, u, p_, n, 1e-4, dropout=drop))
            if it >= args.warmup:
                t_step[name].append(t)

    kw = dict(xs_out=True, addend=True, out=True)
    b0 = prop_launch_bytes(IN_PRESCALED, g.n_nodes, g.nnz, D, **kw)
    gathered = g.nnz * D * 4
    res = {"workload": f"C2-uniform-d{D}-full-prescaled-launch", "nnz": g.nnz,
           "n_nodes": g.n_nodes, "reps": args.reps,
           "sweep_in_use": eng.sweep_wave is not None or eng.sweep is not None,
           "launch_bytes": {"undropped": b0,
                            **{f"drop_{p}": int(b0 - (1.0 - p) * gathered) for p in KEEP}},
           "step": {"batch": B, "layers": L, "prune": True}}
    for k, ts in times.items():
        res[k] = stat(ts)
    for k, ts in t_step.items():
        res[k] = stat(ts)
    for p in KEEP:
        res[f"drop_{p}_over_row"] = round(res[f"drop_{p}"]["median_ms"]
                                          / res["row"]["median_ms"], 4)
    res["drop_0.6_over_shipped"] = round(res["drop_0.6"]["median_ms"]
                                         / res["shipped"]["median_ms"], 4)
    res["step_drop_over_undropped"] = round(res["step_drop_0.6"]["median_ms"]
                                            / res["step_undropped"]["median_ms"], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
