"""Config C3 with the attention hop: the 'gnn' model (conv = 'gat', H = 4) 2-hop
fanout [25, 10] d = 128 B = 2048 on the C2 synthetic graph (1M users x 100K
items / 20M edges), one GPU.  Prints one line per measurement and a JSON
summary:

  * ms per training step of 'gnn' and, in the same run, of GraphSAGE
    (tools/bench_sage.py's model, stepped directly) — the yardstick step;
  * mirec_fanout_gat, mirec_fanout_gat_bwd and mirec_fanout_mean at every
    (n_t, k) of the tree, device events around repeated launches, with their
    algorithmic bytes per second: forward 4 D n_t (k + 2) (child rows, self
    row, output), backward 4 D n_t (3 k + 4) with the child rows counted
    TWICE (the kernel reads them in both passes, the second from cache: 2 k
    read + k written, grad_out + z_self read, grad_z_self written; alpha is
    left out), mean 4 D n_t (k + 1);
  * mirec_csr_gat over the whole graph (logits launch included);
  * the leaf projection (the layer-0 GEMM over every gathered row, forward
    and backward) and its share of the step.

    python tools/bench_gnn.py [--steps K --warmup W]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--fanouts", default="25,10")
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=20, help="launches per kernel timing")
    ap.add_argument("--sage", type=int, default=1, help="also time the GraphSAGE step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gnn: no HIP device (there is no CPU path)")
    from furusato_recommend_amd import GNN, GraphSAGE, SyntheticBipartite, _lib
    from furusato_recommend_amd._lib import check, lib
    dev = torch.device("cuda", 0)
    ds = SyntheticBipartite(args.users, args.items, args.edges, seed=0)
    fan = [int(x) for x in args.fanouts.split(",")]
    B, D, H = args.batch, args.dim, args.heads
    cfg = {"recdim": D, "layer": len(fan), "fanouts": fan, "lr": 1e-3, "decay": 1e-7,
           "device": str(dev), "bpr_batch_size": B, "heads": H}
    torch.manual_seed(2020)
    m = GNN(cfg, ds)
    gnn_ms = step_ms(m, B, args.steps, args.warmup)
    print(f"gnn step: {gnn_ms:.3f} ms (B={B}, fanouts {fan}, d={D}, H={H})", flush=True)
    res = {"metric": "GNN (gat) BPR positive-edges/sec (C3 shape)",
           "value": round(B / (gnn_ms * 1e-3), 1), "unit": "positive-edges/s",
           "ms_per_step": round(gnn_ms, 3), "steps": args.steps, "kernels": []}

    st = _lib.stream_handle()
    C = D // H
    conv = m.convs[0]
    a_s, a_d = conv.att_src.detach().reshape(-1), conv.att_dst.detach().reshape(-1)
    bias = conv.bias.detach()
    L = len(fan)
    n_seed = 3 * B
    # group sizes of the canonical tree, then the (n_t, k) of every (target
    # group, child group) launch of a step
    from furusato_recommend_amd.graphsage import SampleTree
    depths, children = SampleTree.canonical_layout(L)
    size = [n_seed] + [0] * (len(depths) - 1)
    for (gi, hop), ci in sorted(children.items(), key=lambda kv: kv[1]):
        size[ci] = size[gi] * fan[hop - 1]
    shapes = [(size[gi], fan[hop - 1]) for hop in range(L, 0, -1)
              for gi, dep in enumerate(depths) if dep <= hop - 1]
    for n_t, k in sorted(set(shapes)):
        zc = torch.randn(n_t * k, D, device=dev)
        zs = torch.randn(n_t, D, device=dev)
        g = torch.randn(n_t, D, device=dev)
        valid = torch.randint(0, 1000, (n_t * k,), dtype=torch.int32, device=dev)
        valid[torch.rand(n_t * k, device=dev) < 0.1] = -1
        out = torch.empty_like(zs)
        alpha = torch.empty(n_t, k + 1, H, device=dev)
        gzc, gzs = torch.empty_like(zc), torch.empty_like(zs)
        gs, gd = torch.empty(D, device=dev), torch.empty(D, device=dev)
        work = torch.empty(max(int(lib.mirec_fanout_gat_bwd_work_floats(n_t, k, H, C)), 1),
                           device=dev)

        def fwd():
            check(lib.mirec_fanout_gat(zc.data_ptr(), zs.data_ptr(), valid.data_ptr(),
                                       a_s.data_ptr(), a_d.data_ptr(), bias.data_ptr(), n_t, k, H,
                                       C, 0.2, out.data_ptr(), alpha.data_ptr(), st), "gat")

        def bwd():
            check(lib.mirec_fanout_gat_bwd(g.data_ptr(), zc.data_ptr(), zs.data_ptr(),
                                           valid.data_ptr(), a_s.data_ptr(), a_d.data_ptr(),
                                           alpha.data_ptr(), n_t, k, H, C, 0.2, gzc.data_ptr(),
                                           gzs.data_ptr(), gs.data_ptr(), gd.data_ptr(),
                                           work.data_ptr(), st), "gat_bwd")

        def mean():
            check(lib.mirec_fanout_mean(zc.data_ptr(), valid.data_ptr(), n_t, k, D, 0.0,
                                        ctypes.c_uint64(0), out.data_ptr(), st), "mean")

        t_mean = timed(mean, args.reps)
        t_fwd = timed(fwd, args.reps)
        t_bwd = timed(bwd, args.reps)
        b_fwd, b_bwd, b_mean = 4 * D * n_t * (k + 2), 4 * D * n_t * (3 * k + 4), 4 * D * n_t * (k + 1)
        row = {"n_t": n_t, "k": k, "D": D,
               "fanout_gat_ms": round(t_fwd, 4), "fanout_gat_GBps": round(b_fwd / t_fwd / 1e6, 1),
               "fanout_gat_bwd_ms": round(t_bwd, 4),
               "fanout_gat_bwd_GBps": round(b_bwd / t_bwd / 1e6, 1),
               "fanout_mean_ms": round(t_mean, 4),
               "fanout_mean_GBps": round(b_mean / t_mean / 1e6, 1),
               "gat_over_mean": round(t_fwd / t_mean, 3)}
        res["kernels"].append(row)
        print("kernel " + json.dumps(row), flush=True)
        del zc, zs, g, valid, out, alpha, gzc, gzs, work

    # full-graph attention layer (getUsersRating's hot launch)
    N = m.n_user + m.m_item
    z = torch.randn(N, D, device=dev)
    outf = torch.empty_like(z)
    logits = torch.empty(N, 2 * H, device=dev)

    def full():
        check(lib.mirec_csr_gat(m.graph.csr_ptr(), z.data_ptr(), a_s.data_ptr(), a_d.data_ptr(),
                                bias.data_ptr(), H, C, 0.2, outf.data_ptr(), logits.data_ptr(),
                                st), "csr_gat")

    t_csr = timed(full, max(args.reps // 4, 3))
    nnz = int(m.graph.nnz)
    b_csr = 4 * D * (nnz + 2 * N) + 4 * nnz + 8 * N
    res["csr_gat"] = {"rows": N, "nnz": nnz, "ms": round(t_csr, 3),
                      "GBps": round(b_csr / t_csr / 1e6, 1),
                      "bytes": "4 D (nnz + 2 N) gathered rows, self rows and output, + col and rowptr"}
    print("csr_gat " + json.dumps(res["csr_gat"]), flush=True)
    del z, outf, logits

    # the leaf projection: layer 0's GEMM over every gathered row
    rows_n = sum(size)
    x = torch.randn(rows_n, D, device=dev, requires_grad=True)
    w = conv.lin.weight

    def proj():
        w.grad = None
        x.grad = None
        y = conv.project(x)
        y.backward(y.detach())

    t_proj = timed(proj, 5, warmup=2)
    res["leaf_projection"] = {"rows": rows_n, "fwd_bwd_ms": round(t_proj, 3),
                              "share_of_step": round(t_proj / gnn_ms, 3)}
    print("leaf_projection " + json.dumps(res["leaf_projection"]), flush=True)
    del x

    if args.sage:
        del m
        torch.cuda.empty_cache()
        torch.manual_seed(2020)
        sage = GraphSAGE({k_: v for k_, v in cfg.items() if k_ != "heads"}, ds)
        sage_ms = step_ms(sage, B, args.steps, args.warmup)
        res["graphsage_ms_per_step"] = round(sage_ms, 3)
        res["gnn_over_graphsage"] = round(gnn_ms / sage_ms, 3)
        print(f"graphsage step: {sage_ms:.3f} ms; gnn / graphsage = {gnn_ms / sage_ms:.3f}",
              flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
