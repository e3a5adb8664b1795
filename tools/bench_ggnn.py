"""Config C3 with the gated hop: the 'gnn' model with conv = 'ggnn' 2-hop
fanout [25, 10] d = 128 B = 2048 on the C2 synthetic graph (1M users x 100K
items / 20M edges), one GPU.  Prints one line per measurement and a JSON
summary:

  * ms per training step of conv = 'ggnn', conv = 'gat' (H = 4) and GraphSAGE
    in the same run (tools/bench_gnn.py's step loop);
  * mirec_gru_gate and mirec_gru_gate_bwd at the row counts of the tree's
    layers (all target groups of a layer go through one launch), device
    events around repeated launches, with their algorithmic bytes per second:
    forward 4 d n 8 (gi, gh, h read = 7 d, out written = d), backward 4 d n 16
    (grad_out, gi, gh, h, out read = 9 d; grad_gi, grad_gh, grad_h written =
    7 d), next to the 8 TB/s HBM peak;
  * GGNNHop.full over the whole graph (the CSR mean, the three GEMMs and the
    gate), and the gate's launch alone at that row count.

    python tools/bench_ggnn.py [--steps K --warmup W]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0


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


def step_ms(m, B, steps, warmup):
    def step(i):
        u, p, n = m.sample(B, seed=7, offset=i * B)
        m.stageOne(u, p, n)
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(warmup, warmup + steps):
        step(i)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def gate_row(lib, check, st, n, D, reps, dev):
    """Both gate kernels at n rows: ms and algorithmic GB/s."""
    gi = torch.randn(n, 3 * D, device=dev)
    gh = torch.randn(n, 3 * D, device=dev)
    h = torch.randn(n, D, device=dev)
    g = torch.randn(n, D, device=dev)
    out = torch.empty_like(h)
    d_gi, d_gh, d_h = torch.empty_like(gi), torch.empty_like(gh), torch.empty_like(h)

    def fwd():
        check(lib.mirec_gru_gate(gi.data_ptr(), gh.data_ptr(), h.data_ptr(), n, D, 1,
                                 out.data_ptr(), st), "gru_gate")

    def bwd():
        check(lib.mirec_gru_gate_bwd(g.data_ptr(), gi.data_ptr(), gh.data_ptr(), h.data_ptr(),
                                     out.data_ptr(), n, D, d_gi.data_ptr(), d_gh.data_ptr(),
                                     d_h.data_ptr(), st), "gru_gate_bwd")

    t_fwd, t_bwd = timed(fwd, reps), timed(bwd, reps)
    b_fwd, b_bwd = 4 * D * n * 8, 4 * D * n * 16
    return {"rows": n, "D": D,
            "gru_gate_ms": round(t_fwd, 4), "gru_gate_GBps": round(b_fwd / t_fwd / 1e6, 1),
            "gru_gate_share_of_peak": round(b_fwd / t_fwd / 1e6 / HBM_PEAK_GBPS, 3),
            "gru_gate_bwd_ms": round(t_bwd, 4),
            "gru_gate_bwd_GBps": round(b_bwd / t_bwd / 1e6, 1),
            "gru_gate_bwd_share_of_peak": round(b_bwd / t_bwd / 1e6 / HBM_PEAK_GBPS, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--heads", type=int, default=4, help="of the 'gat' step")
    ap.add_argument("--fanouts", default="25,10")
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=20, help="launches per kernel timing")
    ap.add_argument("--others", type=int, default=1, help="also time the gat and GraphSAGE steps")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ggnn: no HIP device (there is no CPU path)")
    from furusato_recommend_amd import GNN, GraphSAGE, SyntheticBipartite, _lib
    from furusato_recommend_amd._lib import check, lib
    from furusato_recommend_amd.graphsage import SampleTree
    dev = torch.device("cuda", 0)
    ds = SyntheticBipartite(args.users, args.items, args.edges, seed=0)
    fan = [int(x) for x in args.fanouts.split(",")]
    B, D = args.batch, args.dim
    cfg = {"recdim": D, "layer": len(fan), "fanouts": fan, "lr": 1e-3, "decay": 1e-7,
           "device": str(dev), "bpr_batch_size": B}
    torch.manual_seed(2020)
    m = GNN(dict(cfg, conv="ggnn"), ds)
    ggnn_ms = step_ms(m, B, args.steps, args.warmup)
    print(f"ggnn step: {ggnn_ms:.3f} ms (B={B}, fanouts {fan}, d={D})", flush=True)
    res = {"metric": "GNN (ggnn) BPR positive-edges/sec (C3 shape)",
           "value": round(B / (ggnn_ms * 1e-3), 1), "unit": "positive-edges/s",
           "ms_per_step": round(ggnn_ms, 3), "steps": args.steps, "kernels": []}

    # rows per layer: every target group of the layer, through one launch
    st = _lib.stream_handle()
    L = len(fan)
    depths, children = SampleTree.canonical_layout(L)
    size = [3 * B] + [0] * (len(depths) - 1)
    for (gi, hop), ci in sorted(children.items(), key=lambda kv: kv[1]):
        size[ci] = size[gi] * fan[hop - 1]
    layer_rows = [sum(size[gi] for gi, dep in enumerate(depths) if dep <= hop - 1)
                  for hop in range(L, 0, -1)]
    for n in sorted(set(layer_rows)):
        row = gate_row(lib, check, st, n, D, args.reps, dev)
        res["kernels"].append(row)
        print("kernel " + json.dumps(row), flush=True)

    # full-graph layer (getUsersRating's pass) and the gate alone at N rows
    N = m.n_user + m.m_item
    x = torch.randn(N, D, device=dev)
    conv = m.convs[0]
    t_full = timed(lambda: conv.full(m.graph, x), max(args.reps // 4, 3))
    row = gate_row(lib, check, st, N, D, max(args.reps // 4, 3), dev)
    res["full"] = {"rows": N, "nnz": int(m.graph.nnz), "layer_ms": round(t_full, 3),
                   "gate_ms": row["gru_gate_ms"], "gate_GBps": row["gru_gate_GBps"]}
    print("full " + json.dumps(res["full"]), flush=True)
    del x, m, conv
    torch.cuda.empty_cache()

    if args.others:
        torch.manual_seed(2020)
        gat = GNN(dict(cfg, conv="gat", heads=args.heads), ds)
        gat_ms = step_ms(gat, B, args.steps, args.warmup)
        del gat
        torch.cuda.empty_cache()
        torch.manual_seed(2020)
        sage = GraphSAGE(cfg, ds)
        sage_ms = step_ms(sage, B, args.steps, args.warmup)
        res.update(gat_ms_per_step=round(gat_ms, 3), graphsage_ms_per_step=round(sage_ms, 3),
                   ggnn_over_gat=round(ggnn_ms / gat_ms, 3),
                   ggnn_over_graphsage=round(ggnn_ms / sage_ms, 3))
        print(f"gat step: {gat_ms:.3f} ms; graphsage step: {sage_ms:.3f} ms; ggnn / gat = "
              f"{ggnn_ms / gat_ms:.3f}; ggnn / graphsage = {ggnn_ms / sage_ms:.3f}", flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
