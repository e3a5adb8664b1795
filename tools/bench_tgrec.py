"""Config C3 with the dot-product attention hop: the 'tgrec' model
(TransformerConv hops, H = 8) 2-hop fanout [25, 10] d = 128 B = 2048 on the C2
synthetic graph (1M users x 100K items / 20M edges), one GPU.  Prints one line
per measurement and a JSON summary, everything from one run so the yardsticks
share the box:

  * ms per training step of 'tgrec' and, in the same run, of 'gnn' (conv =
    'gat', H = 4: tools/bench_gnn.py's model) — the yardstick step;
  * mirec_fanout_tattn, mirec_fanout_tattn_bwd, mirec_fanout_gat and
    mirec_fanout_gat_bwd at every (n_t, k) of the tree, device events around
    repeated launches, with their algorithmic bytes per second.  The tattn
    kernels run in the model's fused layout (stride 2 D).  Bytes:
      tattn forward   4 D n_t (2 k + 3): k key rows and k value rows, the
                      query row, the skip row, the output row;
      tattn backward  4 D n_t (5 k + 4): the value rows counted TWICE (the
                      kernel reads them in both passes, the second from
                      cache) and the key rows once: 3 k read; grad_key and
                      grad_value: 2 k written; grad_out and the query row
                      read, grad_query and grad_skip written: 4;
      gat forward     4 D n_t (k + 2), gat backward 4 D n_t (3 k + 4)
                      (tools/bench_gnn.py);
    alpha is left out of all four;
  * mirec_csr_tattn over the whole graph beside mirec_csr_gat;
  * the two leaf projections (layer 0's k|v GEMM over every leaf row and its
    q|skip GEMM over every other row, forward and backward) and their share of
    the step.

    python tools/bench_tgrec.py [--steps K --warmup W]
"""
import argparse
import json
import math
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
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--gat-heads", type=int, default=4)
    ap.add_argument("--fanouts", default="25,10")
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=20, help="launches per kernel timing")
    ap.add_argument("--gnn", type=int, default=1, help="also time the 'gnn' step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tgrec: no HIP device (there is no CPU path)")
    from furusato_recommend_amd import GNN, SyntheticBipartite, TGRec, _lib
    from furusato_recommend_amd._lib import check, lib
    from furusato_recommend_amd.graphsage import SampleTree
    dev = torch.device("cuda", 0)
    ds = SyntheticBipartite(args.users, args.items, args.edges, seed=0)
    fan = [int(x) for x in args.fanouts.split(",")]
    B, D, H, HG = args.batch, args.dim, args.heads, args.gat_heads
    cfg = {"recdim": D, "layer": len(fan), "fanouts": fan, "lr": 1e-3, "decay": 1e-7,
           "device": str(dev), "bpr_batch_size": B, "heads": H}
    torch.manual_seed(2020)
    m = TGRec(cfg, ds)
    tg_ms = step_ms(m, B, args.steps, args.warmup)
    print(f"tgrec step: {tg_ms:.3f} ms (B={B}, fanouts {fan}, d={D}, H={H})", flush=True)
    res = {"metric": "TGRec BPR positive-edges/sec (C3 shape)",
           "value": round(B / (tg_ms * 1e-3), 1), "unit": "positive-edges/s",
           "ms_per_step": round(tg_ms, 3), "steps": args.steps, "kernels": []}

    st = _lib.stream_handle()
    C, CG = D // H, D // HG
    scale = 1.0 / math.sqrt(C)
    L = len(fan)
    # group sizes of the canonical tree, then the (n_t, k) of every (target
    # group, child group) launch of a step
    depths, children = SampleTree.canonical_layout(L)
    size = [3 * B] + [0] * (len(depths) - 1)
    for (gi, hop), ci in sorted(children.items(), key=lambda kv: kv[1]):
        size[ci] = size[gi] * fan[hop - 1]
    shapes = [(size[gi], fan[hop - 1]) for hop in range(L, 0, -1)
              for gi, dep in enumerate(depths) if dep <= hop - 1]
    a_s, a_d, bias = (torch.randn(D, device=dev) * 0.1 for _ in range(3))
    for n_t, k in sorted(set(shapes)):
        kv = torch.randn(n_t * k, 2 * D, device=dev)
        qs = torch.randn(n_t, 2 * D, device=dev)
        g = torch.randn(n_t, D, device=dev)
        valid = torch.randint(0, 1000, (n_t * k,), dtype=torch.int32, device=dev)
        valid[torch.rand(n_t * k, device=dev) < 0.1] = -1
        out = torch.empty(n_t, D, device=dev)
        alpha = torch.empty(n_t, k, H, device=dev)
        gkv, gqs = torch.empty_like(kv), torch.empty_like(qs)
        o4, o8 = 4 * D, 2 * D

        def fwd():
            check(lib.mirec_fanout_tattn(qs.data_ptr(), qs.data_ptr() + o4, o8, kv.data_ptr(),
                                         kv.data_ptr() + o4, o8, valid.data_ptr(), n_t, k, H, C,
                                         scale, out.data_ptr(), alpha.data_ptr(), st), "tattn")

        def bwd():
            check(lib.mirec_fanout_tattn_bwd(g.data_ptr(), qs.data_ptr(), o8, kv.data_ptr(),
                                             kv.data_ptr() + o4, o8, valid.data_ptr(),
                                             alpha.data_ptr(), n_t, k, H, C, scale,
                                             gqs.data_ptr(), gqs.data_ptr() + o4, o8,
                                             gkv.data_ptr(), gkv.data_ptr() + o4, o8, st),
                  "tattn_bwd")

        t_fwd = timed(fwd, args.reps)
        t_bwd = timed(bwd, args.reps)
        del kv, gkv, gqs
        # the yardstick: the GAT hop on rows of the same width
        zc = torch.randn(n_t * k, D, device=dev)
        zs = torch.randn(n_t, D, device=dev)
        galpha = torch.empty(n_t, k + 1, HG, device=dev)
        gzc, gzs = torch.empty_like(zc), torch.empty_like(zs)
        gsrc, gdst = torch.empty(D, device=dev), torch.empty(D, device=dev)
        work = torch.empty(max(int(lib.mirec_fanout_gat_bwd_work_floats(n_t, k, HG, CG)), 1),
                           device=dev)

        def gat():
            check(lib.mirec_fanout_gat(zc.data_ptr(), zs.data_ptr(), valid.data_ptr(),
                                       a_s.data_ptr(), a_d.data_ptr(), bias.data_ptr(), n_t, k,
                                       HG, CG, 0.2, out.data_ptr(), galpha.data_ptr(), st), "gat")

        def gat_bwd():
            check(lib.mirec_fanout_gat_bwd(g.data_ptr(), zc.data_ptr(), zs.data_ptr(),
                                           valid.data_ptr(), a_s.data_ptr(), a_d.data_ptr(),
                                           galpha.data_ptr(), n_t, k, HG, CG, 0.2, gzc.data_ptr(),
                                           gzs.data_ptr(), gsrc.data_ptr(), gdst.data_ptr(),
                                           work.data_ptr(), st), "gat_bwd")

        t_gat = timed(gat, args.reps)
        t_gat_bwd = timed(gat_bwd, args.reps)
        b_fwd, b_bwd = 4 * D * n_t * (2 * k + 3), 4 * D * n_t * (5 * k + 4)
        b_gat, b_gat_bwd = 4 * D * n_t * (k + 2), 4 * D * n_t * (3 * k + 4)
        row = {"n_t": n_t, "k": k, "D": D,
               "fanout_tattn_ms": round(t_fwd, 4),
               "fanout_tattn_GBps": round(b_fwd / t_fwd / 1e6, 1),
               "fanout_tattn_bwd_ms": round(t_bwd, 4),
               "fanout_tattn_bwd_GBps": round(b_bwd / t_bwd / 1e6, 1),
               "fanout_gat_ms": round(t_gat, 4), "fanout_gat_GBps": round(b_gat / t_gat / 1e6, 1),
               "fanout_gat_bwd_ms": round(t_gat_bwd, 4),
               "fanout_gat_bwd_GBps": round(b_gat_bwd / t_gat_bwd / 1e6, 1),
               "tattn_over_gat": round(t_fwd / t_gat, 3),
               "tattn_bwd_over_gat_bwd": round(t_bwd / t_gat_bwd, 3)}
        res["kernels"].append(row)
        print("kernel " + json.dumps(row), flush=True)
        del zc, zs, g, valid, out, alpha, galpha, gzc, gzs, work, qs

    # full-graph attention layer (getUsersRating's hot launch) beside GAT's
    N = m.n_user + m.m_item
    nnz = int(m.graph.nnz)
    kv = torch.randn(N, 2 * D, device=dev)
    qs = torch.randn(N, 2 * D, device=dev)
    outf = torch.empty(N, D, device=dev)

    def full():
        check(lib.mirec_csr_tattn(m.graph.csr_ptr(), qs.data_ptr(), qs.data_ptr() + 4 * D, 2 * D,
                                  kv.data_ptr(), kv.data_ptr() + 4 * D, 2 * D, H, C, scale,
                                  outf.data_ptr(), st), "csr_tattn")

    t_csr = timed(full, max(args.reps // 4, 3))
    b_csr = 4 * D * (2 * nnz + 3 * N) + 4 * nnz + 8 * N
    res["csr_tattn"] = {"rows": N, "nnz": nnz, "ms": round(t_csr, 3),
                        "GBps": round(b_csr / t_csr / 1e6, 1),
                        "bytes": "4 D (2 nnz + 3 N) gathered key and value rows, query, skip "
                                 "and output rows, + col and rowptr"}
    print("csr_tattn " + json.dumps(res["csr_tattn"]), flush=True)
    del kv, qs
    z = torch.randn(N, D, device=dev)
    logits = torch.empty(N, 2 * HG, device=dev)

    def full_gat():
        check(lib.mirec_csr_gat(m.graph.csr_ptr(), z.data_ptr(), a_s.data_ptr(), a_d.data_ptr(),
                                bias.data_ptr(), HG, CG, 0.2, outf.data_ptr(), logits.data_ptr(),
                                st), "csr_gat")

    t_cg = timed(full_gat, max(args.reps // 4, 3))
    b_cg = 4 * D * (nnz + 2 * N) + 4 * nnz + 8 * N
    res["csr_gat"] = {"ms": round(t_cg, 3), "GBps": round(b_cg / t_cg / 1e6, 1)}
    print("csr_gat " + json.dumps(res["csr_gat"]), flush=True)
    del z, outf, logits

    # the two leaf projections: layer 0's stacked GEMMs, forward and backward
    conv = m.convs[0]
    n_leaf = sum(s for s, dep in zip(size, depths) if dep == L)
    n_rest = sum(size) - n_leaf

    def proj(x, f):
        def run():
            for p in conv.parameters():
                p.grad = None
            x.grad = None
            y = f(x)
            y.backward(y.detach())
        return run

    x = torch.randn(n_leaf, D, device=dev, requires_grad=True)
    t_kv = timed(proj(x, conv.project_kv), 5, warmup=2)
    del x
    x = torch.randn(n_rest, D, device=dev, requires_grad=True)
    t_qs = timed(proj(x, conv.project_qs), 5, warmup=2)
    del x
    res["leaf_projections"] = {"kv_rows": n_leaf, "kv_fwd_bwd_ms": round(t_kv, 3),
                               "qs_rows": n_rest, "qs_fwd_bwd_ms": round(t_qs, 3),
                               "share_of_step": round((t_kv + t_qs) / tg_ms, 3)}
    print("leaf_projections " + json.dumps(res["leaf_projections"]), flush=True)

    if args.gnn:
        del m
        torch.cuda.empty_cache()
        torch.manual_seed(2020)
        gnn = GNN(dict(cfg, heads=HG), ds)
        gnn_ms = step_ms(gnn, B, args.steps, args.warmup)
        res["gnn_ms_per_step"] = round(gnn_ms, 3)
        res["tgrec_over_gnn"] = round(tg_ms / gnn_ms, 3)
        print(f"gnn step: {gnn_ms:.3f} ms (H={HG}); tgrec / gnn = {tg_ms / gnn_ms:.3f}", flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
