"""Config C3 with LightSAGE: the 'lightsage' model, 2-hop fanout [25, 10], d =
128, B = 2048 on the C2 synthetic graph (1M users x 100K items / 20M edges),
one GPU.  Prints one line per measurement and a JSON summary:

  * ms per training step with lightsage.FUSED_HOP on (csrc/lightsage.hip, the
    leaf-gather form) and off (the composition of GraphSAGE's kernels) on ONE
    model, alternating in rounds of --round steps inside one run (the spread
    over the rounds is printed), and GraphSAGE's step in the same run for
    scale;
  * the step's phases (sample, forward, loss, backward, Adam) between device
    events, both forms;
  * the three new kernels between two device events over --reps launches
    after 3, on a tree sampled from the graph: mirec_fanout_resmean_gather at
    layer 0's shape (all targets, the real table and ids), mirec_fanout_resmean
    and mirec_fanout_resmean_bwd at layer 1's (the seeds over their hop-1
    children), with their algorithmic bytes per second next to the 8 TB/s HBM
    peak.  Bytes (v = valid slots, n = targets, e = n k slots):
      gather    4 d (v + n_self + n) + 4 (e + n)
      resmean   4 d (v + 2 n)        + 4 e
      bwd       4 d (2 n + e)        + 4 e     (every child row is written)

    python tools/bench_lightsage.py [--steps K --warmup W]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0
PHASES = ("sample", "forward", "loss", "backward", "adam")


def timed(fn, reps, warmup=3):
    """Mean ms of fn() over reps launches between two device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run_steps(m, B, first, count):
    """ms per step of ``count`` steps (host clock around a synchronise)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(first, first + count):
        u, p, n = m.sample(B, seed=7, offset=i * B)
        m.stageOne(u, p, n)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / count


def phase_ms(m, B, first, count):
    """Mean ms per phase of TreeModel.stageOne's sequence, between device
    events (the same calls, written out)."""
    tot = [0.0] * len(PHASES)
    for i in range(first, first + count):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(PHASES) + 1)]
        u, p, n = m.sample(B, seed=7, offset=i * B)
        seed = 12345 + i
        m._table.grad = None
        ev[0].record()
        tree = m.sample_tree(m._seed_nodes(u, p, n), seed)
        ev[1].record()
        emb = m.forward(tree, dropout_seed=seed)
        ev[2].record()
        loss = m.loss_fused(emb)
        ev[3].record()
        loss.backward()
        ev[4].record()
        m.optimizer_step()
        ev[5].record()
        torch.cuda.synchronize()
        for j in range(len(PHASES)):
            tot[j] += ev[j].elapsed_time(ev[j + 1])
    return {ph: round(t / count, 4) for ph, t in zip(PHASES, tot)}


def kernel_rows(m, B, D, fan, reps):
    """The three kernels on a sampled tree's ids."""
    from furusato_recommend_amd import _lib
    from furusato_recommend_amd._lib import check, lib
    from furusato_recommend_amd.lightsage import _Plan
    st = _lib.stream_handle()
    dev = m.device
    u, p, n = m.sample(B, seed=7, offset=0)
    tree = m.sample_tree(m._seed_nodes(u, p, n), 99)
    plan = _Plan(tree, len(fan), fan)
    table = m._table.detach()
    rows = []

    def row(name, ms, nbytes, **kw):
        r = dict(kernel=name, ms=round(ms, 4), MB=round(nbytes / 1e6, 1),
                 GBps=round(nbytes / ms / 1e6, 1),
                 share_of_peak=round(nbytes / ms / 1e6 / HBM_PEAK_GBPS, 3), **kw)
        rows.append(r)
        print("kernel " + json.dumps(r), flush=True)

    seed = ctypes.c_uint64(77)
    for pdrop in (0.2, 0.0):
        n0, k0 = plan.rows[0], plan.k0
        out = torch.empty(n0, D, device=dev)
        v = int((plan.child_ids >= 0).sum())
        ns = int((plan.self_ids >= 0).sum())
        ms = timed(lambda: check(lib.mirec_fanout_resmean_gather(
            table.data_ptr(), plan.self_ids.data_ptr(), plan.child_ids.data_ptr(), n0, k0, D,
            pdrop, seed, out.data_ptr(), st), "fanout_resmean_gather"), reps)
        row("fanout_resmean_gather", ms, 4 * D * (v + ns + n0) + 4 * (n0 * k0 + n0), targets=n0,
            k=k0, valid_slots=v, p=pdrop)
        if len(fan) < 2:
            continue
        gi, n_t, so, co, valid, k = plan.pairs[1][0]
        x = torch.randn(n0, D, device=dev)
        o1 = torch.empty(n_t, D, device=dev)
        v1 = int((valid >= 0).sum())
        ms = timed(lambda: check(lib.mirec_fanout_resmean(
            x[so:].data_ptr(), x[co:].data_ptr(), valid.data_ptr(), n_t, k, D, pdrop, seed,
            o1.data_ptr(), st), "fanout_resmean"), reps)
        row("fanout_resmean", ms, 4 * D * (v1 + 2 * n_t) + 4 * n_t * k, targets=n_t, k=k,
            valid_slots=v1, p=pdrop)
        g = torch.randn(n_t, D, device=dev)
        gin = torch.empty(n0, D, device=dev)
        ms = timed(lambda: check(lib.mirec_fanout_resmean_bwd(
            g.data_ptr(), valid.data_ptr(), n_t, k, D, pdrop, seed, gin[so:].data_ptr(),
            gin[co:].data_ptr(), st), "fanout_resmean_bwd"), reps)
        row("fanout_resmean_bwd", ms, 4 * D * (2 * n_t + n_t * k) + 4 * n_t * k, targets=n_t, k=k,
            valid_slots=v1, p=pdrop)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--round", type=int, default=5, help="steps per alternation round")
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--fanouts", default="25,10")
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=20, help="launches per kernel timing")
    ap.add_argument("--sage", type=int, default=1, help="also time the GraphSAGE step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lightsage: no HIP device (there is no CPU path)")
    from furusato_recommend_amd import GraphSAGE, LightSAGE, SyntheticBipartite, lightsage
    dev = torch.device("cuda", 0)
    ds = SyntheticBipartite(args.users, args.items, args.edges, seed=0)
    fan = [int(x) for x in args.fanouts.split(",")]
    B, D = args.batch, args.dim
    cfg = {"recdim": D, "layer": len(fan), "fanouts": fan, "lr": 1e-3, "decay": 1e-7,
           "device": str(dev), "bpr_batch_size": B}
    torch.manual_seed(2020)
    m = LightSAGE(cfg, ds)
    m.train()
    default = lightsage.FUSED_HOP
    step = 0
    for fused in (True, False):
        lightsage.FUSED_HOP = fused
        run_steps(m, B, step, args.warmup)
        step += args.warmup
    rounds = {True: [], False: []}
    n_rounds = max(1, args.steps // args.round)
    for _ in range(n_rounds):
        for fused in (True, False):
            lightsage.FUSED_HOP = fused
            rounds[fused].append(run_steps(m, B, step, args.round))
            step += args.round
    ms = {f: sum(r) / len(r) for f, r in rounds.items()}
    for fused in (True, False):
        r = rounds[fused]
        print(f"lightsage step FUSED_HOP={fused}: {ms[fused]:.3f} ms (rounds of {args.round}: "
              f"{' '.join(f'{x:.3f}' for x in r)}; B={B}, fanouts {fan}, d={D})", flush=True)
    res = {"metric": "LightSAGE BPR positive-edges/sec (C3 shape)",
           "value": round(B / (ms[True] * 1e-3), 1), "unit": "positive-edges/s",
           "ms_per_step_fused": round(ms[True], 3), "ms_per_step_composed": round(ms[False], 3),
           "rounds_fused": [round(x, 3) for x in rounds[True]],
           "rounds_composed": [round(x, 3) for x in rounds[False]],
           "fused_over_composed": round(ms[True] / ms[False], 3),
           "steps": n_rounds * args.round, "default_fused_hop": bool(default)}
    res["phases"] = {}
    for fused in (True, False):
        lightsage.FUSED_HOP = fused
        ph = phase_ms(m, B, step, args.round)
        step += args.round
        res["phases"]["fused" if fused else "composed"] = ph
        print(f"phases FUSED_HOP={fused} " + json.dumps(ph), flush=True)
    lightsage.FUSED_HOP = default
    res["kernels"] = kernel_rows(m, B, D, fan, args.reps)
    del m
    torch.cuda.empty_cache()
    if args.sage:
        torch.manual_seed(2020)
        sage = GraphSAGE(cfg, ds)
        run_steps(sage, B, 0, args.warmup)
        sage_ms = run_steps(sage, B, args.warmup, n_rounds * args.round)
        res.update(graphsage_ms_per_step=round(sage_ms, 3),
                   lightsage_over_graphsage=round(ms[True] / sage_ms, 3))
        print(f"graphsage step: {sage_ms:.3f} ms; lightsage / graphsage = "
              f"{ms[True] / sage_ms:.3f}", flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
