"""Cost of the sampled-softmax loss on the training step.

The bench.py C2 workload (1 M users, 100 k items, 20 M interactions, uniform;
d = 64, L = 3, B = 2048, pruning on, one sampler call + one fused step per
step) run in one process on one device: BPR legs (mirec_bpr_sample_ex +
train_step) alternating with sampled-softmax legs (mirec_ssm_sample +
train_step_ssm) at every --neg K and shared-negative legs (mirec_bpr_sample_ex
+ mirec_shared_sample + train_step_ssm_shared) at every
--shared M: (bpr, K1, K2, ..., M1, M2, ..., bpr, ...), each --steps timed steps after --warmup; the spread between the BPR legs is the
yardstick for the others.  Every case has a model of its own on the one
shared dataset (the engines' buffers are sized by n_neg).  One JSON line per
leg, then per case a summary line, the device time of its loss + seed stage
(mirec_ssm_forward / mirec_bpr_loss / mirec_ssm_seed, resp. the mask, forward,
loss and seed calls of ssm_shared(), between two events, median over --stage-steps steps run after the legs) and the mean sizes of
the batch's node set S and of its one-hop frontier S ∪ N(S); appended to
--out.

    python tools/bench_ssm.py --out profiles/ssm_bench_lines.txt
    python tools/bench_ssm.py --neg 8 64 --shared 512 2048 4096 \
        --out profiles/ssm_shared_bench_lines.txt
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from furusato_recommend_amd import LightGCN, SyntheticBipartite  # noqa: E402
from furusato_recommend_amd.engine import (sample_pairs, sample_shared,  # noqa: E402
                                           sample_triples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--neg", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--shared", type=int, nargs="*", default=[],
                    help="sizes M of a negative set shared by the batch (neg_shared)")
    ap.add_argument("--temp", type=float, default=0.2)
    ap.add_argument("--legs", type=int, default=3, help="legs per case")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--stage-steps", type=int, default=20,
                    help="steps per case with events around the loss + seed stage (0 = off)")
    ap.add_argument("--seed", type=int, default=2020)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ssm: needs a HIP device")
    ds = SyntheticBipartite(args.users, args.items, args.edges, seed=0, kind="uniform")
    cfg = {"recdim": args.dim, "layer": args.layers, "lr": 1e-3, "decay": 1e-4,
           "device": "cuda:0", "bpr_batch_size": args.batch, "prune": True}
    torch.manual_seed(args.seed)
    B, dev = args.batch, "cuda:0"
    cases = {"bpr": LightGCN(cfg, ds)}
    for k in args.neg:
        cases[f"ssm{k}"] = LightGCN(dict(cfg, loss="ssm", neg_size=k, ssm_temp=args.temp), ds)
    for k in args.shared:
        cases[f"shared{k}"] = LightGCN(dict(cfg, loss="ssm", neg_shared=k, ssm_temp=args.temp), ds)
    u = torch.empty(B, dtype=torch.int32, device=dev)
    p = torch.empty_like(u)
    unused = torch.empty_like(u)  # the BPR sampler's negative under neg_shared
    negs = {c: torch.empty((m.neg_shared,) if m.neg_shared else (B, m.neg_size)
                           if m.loss_name == "ssm" else (B,), dtype=torch.int32, device=dev)
            for c, m in cases.items()}
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    done = {c: 0 for c in cases}

    def step(c, split=None):
        """One sampler call + one training step of case c; ``split`` = a pair
        of events recorded around the loss + seed stage."""
        m, n = cases[c], negs[c]
        eng, emb = m.engine, m.all_embedding.weight.data
        if m.neg_shared:
            sample_triples(m.graph, B, args.seed, done[c] * B, u, p, unused, err)
            sample_shared(m.num_items, 1, m.neg_shared, args.seed, done[c], n)
        elif m.loss_name == "ssm":
            sample_pairs(m.graph, B, m.neg_size, args.seed, done[c] * B, u, p, n, err)
        else:
            sample_triples(m.graph, B, args.seed, done[c] * B, u, p, n, err)
        done[c] += 1
        if split is None:
            if m.neg_shared:
                eng.train_step_ssm_shared(emb, m.optim, u, p, n, cfg["decay"], m.ssm_temp)
            elif m.loss_name == "ssm":
                eng.train_step_ssm(emb, m.optim, u, p, n, cfg["decay"], m.ssm_temp)
            else:
                eng.train_step(emb, m.optim, u, p, n, cfg["decay"])
            return
        if m.neg_shared:
            eng.frontier_ssm_shared(u, p, n)
        elif m.loss_name == "ssm":
            eng.frontier_ssm(u, p, n)
        else:
            eng.compute_frontier(u, p, n)
        out = eng.forward(emb, pruned=eng.prune)
        split[0].record()
        if m.neg_shared:
            eng.ssm_shared(out, emb, u, p, n, cfg["decay"], m.ssm_temp)
        elif m.loss_name == "ssm":
            eng.ssm(out, emb, u, p, n, cfg["decay"], m.ssm_temp)
        else:
            eng.bpr(out, emb, u, p, n, cfg["decay"])
        split[1].record()
        sizes = (eng.self_count.clone(), eng.list_counts.clone())
        eng.backward(emb, adam=m.optim)
        return sizes

    lines = []
    for leg in range(args.legs):
        for c in cases:
            for _ in range(args.warmup):
                step(c)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(c)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            lines.append({"leg": leg, "case": c, "ms_per_step": round(ms, 4), "steps": args.steps})
            print(json.dumps(lines[-1]), flush=True)
    assert int(err.item()) == 0
    base = [x["ms_per_step"] for x in lines if x["case"] == "bpr"]
    tail = []
    for c, m in cases.items():
        legs = [x["ms_per_step"] for x in lines if x["case"] == c]
        s = {"workload": f"C2-uniform-d{args.dim}-L{args.layers}-B{B}", "case": c,
             "neg_size": m.neg_size, "neg_shared": m.neg_shared, "temp": m.ssm_temp if m.loss_name == "ssm" else None,
             "ms": legs, "mean_ms": round(sum(legs) / len(legs), 4),
             "bpr_spread_ms": round(max(base) - min(base), 4),
             "ratio_to_bpr": round(sum(legs) / len(legs) / (sum(base) / len(base)), 4)}
        if args.stage_steps > 0:
            ts, s_self, s_hop = [], [], []
            for _ in range(args.stage_steps):
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                sc, lc = step(c, ev)
                torch.cuda.synchronize()
                ts.append(ev[0].elapsed_time(ev[1]))
                s_self.append(int(sc.item()))
                s_hop.append(int(lc[2].item()) + int(lc[3].item()))
            ts.sort()
            s.update(loss_seed_stage_median_ms=round(ts[len(ts) // 2], 4),
                     mean_S=round(sum(s_self) / len(s_self), 1),
                     mean_hop=round(sum(s_hop) / len(s_hop), 1), n_nodes=m.graph.n_nodes)
        tail.append(s)
        print(json.dumps(s), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for x in lines + tail:
                f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
