"""One full PRESCALED launch (forward layer 1's arguments, unpruned) of
LightGCN d = 64 on the bench.py C2 graph in the forms of the column sweep:

  row          the row kernel for every row (use_sweep = False)
  group        item rows by the group form of the sweep
  wave         item rows by the wave form (§14), user rows by the row kernel
  wave+users   both blocks by the wave form
  wave+users8  the same with 8-byte slot streams (sweep_packed off, §26; not
               in the default --forms)

and, with --sizes, the wave form at other (tile_rows, band_rows); with --pace,
both blocks swept and one of them paced per XCD.  With
--inmask the launch is instead the second backward layer's of a pruned step
(in_mask = the frontier F1 of one sampled batch, every row written to xs_out;
§27) with the engine's sweep_inmask switch off / items / users / both: "off"
is the row kernel for both blocks, "items" and "users" sweep that block with
the masked form and leave the other to the row kernel.  The forms
alternate inside one process; each figure is the median of --reps device-event
timings after --warmup launches.  Prints one JSON line per form.

  python tools/bench_sweep_forms.py [--reps 10] [--sizes items:196x2048,...]
  python tools/bench_sweep_forms.py --inmask [--batch 2048]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--sizes", default="",
                    help="comma list of block:TILExBAND, block = items or users")
    ap.add_argument("--pace", default="",
                    help="comma list of block:LEAD/EVERY/NAP (per-XCD pacing of that block)")
    ap.add_argument("--forms", default="row,group,wave,wave+users")
    ap.add_argument("--inmask", action="store_true",
                    help="time the in-masked backward launch per sweep_inmask value instead")
    ap.add_argument("--batch", type=int, default=2048, help="--inmask: the frontier's batch")
    args = ap.parse_args()
    from furusato_recommend_amd import SyntheticBipartite
    from furusato_recommend_amd._lib import IN_PRESCALED
    from furusato_recommend_amd.engine import PropagationEngine
    from furusato_recommend_amd.graph import Graph
    dev = torch.device("cuda:0")
    ds = SyntheticBipartite(args.users, args.items, args.edges, seed=0)
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, dev)
    D = 64
    if args.inmask:
        return inmask(args, g, D)
    forms = {"row": {"use_sweep": False}, "group": {"sweep_form": "group"},
             "wave": {"sweep_form": "wave", "sweep_users": False},
             "wave+users": {"sweep_form": "wave", "sweep_users": True},
             "wave+users8": {"sweep_form": "wave", "sweep_users": True, "sweep_packed": False}}
    engines = {}
    for name, sw in forms.items():
        if name not in args.forms.split(","):
            continue
        engines[name] = (PropagationEngine(g, D, 3, 2048), sw, None)
    for spec in filter(None, args.sizes.split(",")):
        block, size = spec.split(":")
        tile, band = (int(v) for v in size.split("x"))
        eng = PropagationEngine(g, D, 3, 2048)
        sw = {"sweep_form": "wave", "sweep_users": block == "users"}
        engines[spec] = (eng, sw, {"wave_" + block: (tile, band)})
    # paced rows: both blocks swept, one block paced
    for spec in filter(None, args.pace.split(",")):
        block, v = spec.split(":")
        pace = {"items": None, "users": None}
        pace[block] = tuple(int(t) for t in v.split("/"))
        eng = PropagationEngine(g, D, 3, 2048)
        engines["pace " + spec] = (eng, {"sweep_form": "wave", "sweep_users": True,
                                         "sweep_pace": pace}, None)
    for name, (eng, sw, sizes) in engines.items():
        for k, v in sw.items():
            setattr(eng, k, v)
        if sizes:
            eng.set_sweep_sizes(**sizes)
    x = torch.randn(g.n_nodes, D, device=dev) * 0.1
    add = torch.randn(g.n_nodes, D, device=dev) * 0.1
    out, xs = torch.empty_like(x), torch.empty_like(x)
    times = {k: [] for k in engines}
    for it in range(args.warmup + args.reps):
        for name, (eng, _, _) in engines.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            eng._prop(in_mode=IN_PRESCALED, x_in=x, addend=add, out=out, xs_out=xs)
            e.record()
            e.synchronize()
            if it >= args.warmup:
                times[name].append(s.elapsed_time(e))
    for name, (eng, sw, _) in engines.items():
        ts = sorted(times[name])
        res = {"form": name, "ms_median": round(statistics.median(ts), 4),
               "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4)}
        if sw.get("sweep_form") == "wave":
            for blk, lay in (("items", eng.sweep_wave),
                             ("users", eng.sweep_wave_users if eng.sweep_users else None)):
                if lay is not None:
                    d = lay.desc
                    res[blk] = {"tile_rows": d.tile_rows, "band_rows": d.band_rows,
                                "tiles": d.n_tiles, "grid": d.grid,
                                "passes": -(-d.n_tiles // d.grid), "slots": d.n_slots,
                                "pad_share": round(1 - lay.n_entries / d.n_slots, 4)}
        print(json.dumps(res), flush=True)


def inmask(args, g, D):
    from furusato_recommend_amd._lib import IN_PRESCALED
    from furusato_recommend_amd.engine import PropagationEngine, sample_triples
    dev, B = g.device, args.batch
    eng = PropagationEngine(g, D, 3, B)
    u = torch.empty(B, dtype=torch.int32, device=dev)
    p, n = torch.empty_like(u), torch.empty_like(u)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    sample_triples(g, B, 0, 0, u, p, n, err)
    eng.compute_frontier(u, p, n)
    f1 = eng.bm_hop.view(torch.uint8)[:g.n_nodes].bool()
    share = {"users": round(float(f1[:g.n_users].float().mean()), 4),
             "items": round(float(f1[g.n_users:].float().mean()), 4)}
    x = torch.randn(g.n_nodes, D, device=dev) * 0.1
    xs = torch.empty_like(x)
    variants = ("off", "items", "users", "both")
    times = {k: [] for k in variants}
    for it in range(args.warmup + args.reps):
        for name in variants:
            eng.sweep_inmask = name
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            eng._prop(in_mode=IN_PRESCALED, x_in=x, in_mask=eng.bm_hop, xs_out=xs,
                      direction="bwd", inmask_sweep=True)
            e.record()
            e.synchronize()
            if it >= args.warmup:
                times[name].append(s.elapsed_time(e))
    for name in variants:
        ts = sorted(times[name])
        print(json.dumps({"sweep_inmask": name, "ms_median": round(statistics.median(ts), 4),
                          "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4),
                          "f1_share": share}), flush=True)


if __name__ == "__main__":
    main()
