"""Cost of the r-adjusted normalisation (rAdjGCN) on the training step.

The bench.py C2 workload (1 M users, 100 k items, 20 M interactions, uniform;
d = 64, L = 3, B = 2048, pruning on, UniformSample + stageOne per step) run
in one process on one device, r = 0.5 legs (no scale vectors: the unscaled
kernels, LightGCN's launches) alternating with legs at --r (the kScaled
kernels: three scale pointers per launch, N·4 more bytes where the next
layer's scale differs from the row sum's): (0.5, r, 0.5, r, ...), each
--steps timed steps after --warmup; the spread between the r = 0.5 legs is
the yardstick for the r legs.  One JSON line per leg, a summary line and
the per-launch device times of both, appended to --out.

By default both kinds of leg run on ONE model: an rAdjGCN whose graph has
its scale vectors detached for the r = 0.5 legs, so the table, the moments,
the scratch buffers and the CSR are the same allocations and only the
kernels and the scale reads differ.  --two-models gives each r a model of
its own (LightGCN and rAdjGCN) instead; then the legs also differ by where
their buffers lie, which at this size moves a step by about as much as
two processes of the same code differ (profiles/radj_ab_two_models.jsonl).
--scaled-half adds a third kind of leg, "0.5s": the kScaled kernels with
dinv itself in all three roles (r = 0.5 computed by the scaled kernels, every
scale read hitting the one vector), which separates what the kernels cost
from what reading a second per-row vector costs.

    python tools/bench_radj.py --out profiles/radj_ab.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from furusato_recommend_amd import LightGCN, SyntheticBipartite, rAdjGCN  # noqa: E402
from furusato_recommend_amd.engine import sample_triples  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--r", type=float, default=0.3)
    ap.add_argument("--legs", type=int, default=3, help="legs per model")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launch-steps", type=int, default=40,
                    help="steps per model with per-launch device events after the legs (0 = off)")
    ap.add_argument("--two-models", action="store_true",
                    help="a model per r instead of one model with its scales detached")
    ap.add_argument("--scaled-half", action="store_true",
                    help="also time r = 0.5 on the scaled kernels (dinv in all three roles)")
    ap.add_argument("--seed", type=int, default=2020)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_radj: needs a HIP device")
    ds = SyntheticBipartite(args.users, args.items, args.edges, seed=0, kind="uniform")
    cfg = {"recdim": args.dim, "layer": args.layers, "lr": 1e-3, "decay": 1e-4,
           "device": "cuda:0", "bpr_batch_size": args.batch, "prune": True}
    torch.manual_seed(args.seed)
    if args.r == 0.5:
        sys.exit("bench_radj: --r 0.5 is the baseline leg itself")
    radj = rAdjGCN(dict(cfg, r=args.r), ds)
    models = {0.5: LightGCN(cfg, ds) if args.two_models else radj, args.r: radj}
    scales = (radj.graph.scale_src, radj.graph.scale_dst)
    assert scales[0] is not None
    if args.scaled_half:
        if args.two_models:
            sys.exit("bench_radj: --scaled-half runs on the one model")
        models = {0.5: radj, "0.5s": radj, args.r: radj}

    def select(r):
        """Attach (r) or detach (0.5) the one model's scale vectors."""
        if args.two_models:
            return
        g = radj.graph
        g.scale_src, g.scale_dst = {0.5: (None, None), "0.5s": (g.dinv, g.dinv)}.get(r, scales)
        radj.engine.invalidate_prescaled()  # x0s was scaled for the other leg
    B = args.batch
    u = torch.empty(B, dtype=torch.int32, device="cuda:0")
    p, n = torch.empty_like(u), torch.empty_like(u)
    err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    done = {r: 0 for r in models}

    def run(r, steps):
        m = models[r]
        select(r)
        emb = m.all_embedding.weight.data
        for _ in range(steps):
            sample_triples(m.graph, B, args.seed, done[r] * B, u, p, n, err)
            m.engine.train_step(emb, m.optim, u, p, n, cfg["decay"])
            done[r] += 1

    lines = []
    for leg in range(args.legs):
        for r in models:
            run(r, args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(r, args.steps)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            eng = models[r].engine
            lines.append({"leg": leg, "r": r, "ms_per_step": round(ms, 4), "steps": args.steps,
                          "sweep": eng.sweep_wave is not None, "sweep_form": eng.sweep_form,
                          "sweep_users": eng.sweep_users, "two_models": args.two_models})
            print(json.dumps(lines[-1]), flush=True)
    base = [x["ms_per_step"] for x in lines if x["r"] == 0.5]
    legs_r = [x["ms_per_step"] for x in lines if x["r"] == args.r]
    summary = {"workload": f"C2-uniform-d{args.dim}-L{args.layers}-B{B}", "r": args.r,
               "r05_ms": base, "r_ms": legs_r, "r05_spread_ms": round(max(base) - min(base), 4),
               "r_inside_r05_spread": bool(min(base) <= min(legs_r) and max(legs_r) <= max(base)),
               "mean_ratio": round(sum(legs_r) / len(legs_r) / (sum(base) / len(base)), 4)}
    if args.scaled_half:
        summary["r05_scaled_ms"] = [x["ms_per_step"] for x in lines if x["r"] == "0.5s"]
    print(json.dumps(summary), flush=True)
    tail = [summary]
    if args.launch_steps > 0:
        # where a difference sits: device-event time of every propagation
        # launch of a step (events idle the GPU a little, so these steps are
        # not the timed ones), median over --launch-steps steps per model,
        # the models alternating step by step
        ev = {r: [] for r in models}
        for _ in range(args.launch_steps):
            for r in models:
                models[r].engine.prop_events = step_ev = []
                run(r, 1)
                models[r].engine.prop_events = None
                torch.cuda.synchronize()
                ev[r].append([(s.elapsed_time(e), kind, nbytes) for s, e, kind, nbytes in step_ev])
        for r in models:
            n_launch = len(ev[r][0])
            rows = []
            for k in range(n_launch):
                ts = sorted(step[k][0] for step in ev[r])
                _, kind, nbytes = ev[r][0][k]
                rows.append({"launch": k, "in_mode": kind[0], "in_mask": kind[1],
                             "row_mask": kind[2], "out_mask": kind[3], "bytes": nbytes,
                             "median_ms": round(ts[len(ts) // 2], 4)})
            tail.append({"r": r, "launches": rows,
                         "sum_ms": round(sum(x["median_ms"] for x in rows), 4)})
            print(json.dumps(tail[-1]), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for x in lines + tail:
                f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
