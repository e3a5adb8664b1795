"""Cost of the edge-weighted propagation launch at the C2 shape.

Times ONE full PRESCALED launch (every row, no masks: a forward layer of an
unpruned pass) of LightGCN d = 64 on the bench.py C2 graph (1 M users, 100 k
items, 20 M interactions, uniform) three ways:

  weighted     the weighted kernel on the graph built with per-interaction weights
  row          the unweighted row kernel (use_sweep = False)
  shipped      the unweighted launch as shipped (column sweep of the item rows)

and the per-entry dot kernel (mirec_edge_dot) on the same graph.  Each timing
is the median of --reps device-event timings after --warmup launches, the
three launches interleaved; prints one JSON line (and writes --out).

    python tools/bench_edge_weight.py --out profiles/edge_weight_c2.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from furusato_recommend_amd import SyntheticBipartite  # noqa: E402
from furusato_recommend_amd._lib import IN_PRESCALED  # noqa: E402
from furusato_recommend_amd.engine import PropagationEngine, edge_dot, prop_launch_bytes  # noqa: E402
from furusato_recommend_amd.graph import Graph  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_edge_weight: needs a HIP device")
    dev = "cuda:0"
    ds = SyntheticBipartite(args.users, args.items, args.edges, seed=0, kind="uniform")
    w = np.random.default_rng(1).uniform(0.25, 4.0, len(ds.trainUser)).astype(np.float32)
    g0 = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, dev)
    gw = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, dev,
                                 weight=w)
    D = args.dim
    e_w, e_0 = PropagationEngine(gw, D, 3, 2048), PropagationEngine(g0, D, 3, 2048)
    assert e_w.sweep is None
    x = torch.randn(g0.n_nodes, D, device=dev) * 0.1
    add = torch.randn(g0.n_nodes, D, device=dev) * 0.1
    out, xs = torch.empty_like(x), torch.empty_like(x)

    def launch(eng, sweep):
        eng.use_sweep = sweep
        eng._prop(in_mode=IN_PRESCALED, x_in=x, addend=add, out=out, xs_out=xs)

    legs = {"weighted": (e_w, False), "row": (e_0, False), "shipped": (e_0, True)}
    times = {k: [] for k in legs}
    for it in range(args.warmup + args.reps):
        for name, (eng, sweep) in legs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            launch(eng, sweep)
            e.record()
            e.synchronize()
            if it >= args.warmup:
                times[name].append(s.elapsed_time(e))
    dots = torch.empty(gw.nnz, dtype=torch.float32, device=dev)
    t_dot = []
    for it in range(args.warmup + args.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        edge_dot(gw, add, x, dots)
        e.record()
        e.synchronize()
        if it >= args.warmup:
            t_dot.append(s.elapsed_time(e))

    def stat(ts):
        ts = sorted(ts)
        return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(ts[0], 4),
                "max_ms": round(ts[-1], 4),
                "p10_ms": round(ts[len(ts) // 10], 4), "p90_ms": round(ts[-1 - len(ts) // 10], 4)}

    kw = dict(xs_out=True, addend=True, out=True)
    b0 = prop_launch_bytes(IN_PRESCALED, g0.n_nodes, g0.nnz, D, **kw)
    bw = prop_launch_bytes(IN_PRESCALED, g0.n_nodes, g0.nnz, D, weighted=True, **kw)
    res = {"workload": f"C2-uniform-d{D}-full-prescaled-launch", "nnz": g0.nnz,
           "n_nodes": g0.n_nodes, "reps": args.reps, "sweep_in_use": e_0.sweep is not None,
           "launch_bytes": {"unweighted": b0, "weighted": bw,
                            "weight_share": round((bw - b0) / b0, 5)},
           "edge_dot_bytes": g0.nnz * (2 * D * 4 + 4 + 4) + (g0.n_nodes + 1) * 8}
    for k, ts in times.items():
        res[k] = stat(ts)
    res["edge_dot"] = stat(t_dot)
    res["weighted_over_row"] = round(res["weighted"]["median_ms"] / res["row"]["median_ms"], 4)
    res["weighted_over_shipped"] = round(res["weighted"]["median_ms"]
                                         / res["shipped"]["median_ms"], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
