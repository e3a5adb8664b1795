"""How far apart in band the workgroups of one XCD run during a swept full
launch: one full PRESCALED launch (forward layer 1's
arguments, unpruned) of LightGCN d = 64 on the bench.py C2 graph, each block
through the stamping instantiation of the wave-form kernel
(mirec_sweep_wave_stamp: wave 0 of every workgroup notes the 100 MHz wall
clock at each band advance; no store inside the batch loop).

Per block and XCD (the XCC id the workgroup read), at --samples equally spaced
moments at which every workgroup of the XCD is running: progress = band
advances of a workgroup since the launch's start (carried on across its
tiles), spread = max - min of it over the XCD's workgroups.  Reports the p50 and
p90 of the spread over moments and XCDs (and per XCD), the same for the band
index inside the current tile, and whether blockIdx.x % 8 labels an XCD.

  python tools/sweep_drift.py [--out profiles/sweep_pace_drift.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TICK_US = 0.01  # wall_clock64: 100 MHz


def spreads(stamps: np.ndarray, meta: np.ndarray, samples: int) -> dict:
    """stamps [tiles, bands + 1] (tile start, advances 1 .. bands - 1, tile
    end), meta [tiles, 2] (workgroup, XCC id)."""
    n_tiles, nb1 = stamps.shape
    bands = nb1 - 1
    wg, xcc = meta[:, 0], meta[:, 1]
    t0 = stamps[:, 0].min()
    per_xcd, all_prog, all_band = {}, [], []
    for x in np.unique(xcc):
        groups = []
        for w in np.unique(wg[xcc == x]):
            tiles = np.flatnonzero(wg == w)
            tiles = tiles[np.argsort(stamps[tiles, 0])]
            adv = np.sort(stamps[tiles, 1:bands].ravel())      # band advances, all tiles
            starts = stamps[tiles, 0]
            groups.append((adv, starts, stamps[tiles[0], 0], stamps[tiles[-1], bands]))
        lo = max(g[2] for g in groups)
        hi = min(g[3] for g in groups)
        if hi <= lo or len(groups) < 2:
            continue
        ts = np.linspace(lo, hi, samples + 2)[1:-1]
        prog = np.stack([np.searchsorted(g[0], ts, side="right") for g in groups])
        # band inside the current tile: advances since that tile's start
        tile_no = np.stack([np.searchsorted(g[1], ts, side="right") - 1 for g in groups])
        band = prog - tile_no * (bands - 1)
        sp, sb = prog.max(0) - prog.min(0), band.max(0) - band.min(0)
        per_xcd[int(x)] = {"workgroups": len(groups),
                           "progress_p50": float(np.percentile(sp, 50)),
                           "progress_p90": float(np.percentile(sp, 90)),
                           "band_p50": float(np.percentile(sb, 50)),
                           "band_p90": float(np.percentile(sb, 90))}
        all_prog.append(sp)
        all_band.append(sb)
    sp, sb = np.concatenate(all_prog), np.concatenate(all_band)
    # does blockIdx.x % 8 label an XCD?  (one XCC id per residue, all different)
    ids = [sorted(set(xcc[wg % 8 == r].tolist())) for r in range(8) if (wg % 8 == r).any()]
    labels = all(len(i) == 1 for i in ids) and len({i[0] for i in ids}) == len(ids)
    first =np.array([stamps[wg == w, 0].min() for w in np.unique(wg)]) - t0
    return {"tiles": int(n_tiles), "bands": int(bands), "workgroups": int(len(np.unique(wg))),
            "launch_us": float((stamps[:, bands].max() - t0) * TICK_US),
            "start_skew_us_max": float(first.max() * TICK_US),
            "progress_spread_p50": float(np.percentile(sp, 50)),
            "progress_spread_p90": float(np.percentile(sp, 90)),
            "band_spread_p50": float(np.percentile(sb, 50)),
            "band_spread_p90": float(np.percentile(sb, 90)),
            "blockidx_mod8_labels_xcd": bool(labels), "xcc_ids_per_residue": ids,
            "per_xcd": per_xcd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--samples", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_pace_drift.json"))
    args = ap.parse_args()
    from furusato_recommend_amd import SyntheticBipartite
    from furusato_recommend_amd._lib import IN_PRESCALED
    from furusato_recommend_amd.engine import PropagationEngine
    from furusato_recommend_amd.graph import Graph
    dev = torch.device("cuda:0")
    ds = SyntheticBipartite(args.users, args.items, args.edges, seed=0)
    g = Graph.from_interactions(ds.trainUser, ds.trainItem, ds.n_users, ds.m_items, dev)
    D = 64
    eng = PropagationEngine(g, D, 3, 2048)
    eng.sweep_form, eng.sweep_users = "wave", True
    x = torch.randn(g.n_nodes, D, device=dev) * 0.1
    add = torch.randn(g.n_nodes, D, device=dev) * 0.1
    out, xs = torch.empty_like(x), torch.empty_like(x)
    launch = dict(in_mode=IN_PRESCALED, x_in=x, addend=add, out=out, xs_out=xs)
    res = {"graph": {"users": args.users, "items": args.items, "edges": args.edges},
           "l2_bands": {}, "blocks": {}}
    for block in ("items", "users"):
        lay = eng.sweep_wave if block == "items" else eng.sweep_wave_users
        res["l2_bands"][block] = round(4 * 2 ** 20 / (lay.desc.band_rows * 256), 2)
        for _ in range(args.warmup):
            eng._prop(**launch)
        stamps, meta = eng.sweep_stamp(block, **launch)
        torch.cuda.synchronize()
        r = spreads(stamps.cpu().numpy(), meta.cpu().numpy(), args.samples)
        res["blocks"][block] = r
        print(json.dumps({block: {k: v for k, v in r.items() if k != "per_xcd"}}), flush=True)
    res["gate"] = {b: res["blocks"][b]["progress_spread_p90"] for b in res["blocks"]}
    res["part1_has_a_case"] = any(v > 2 for v in res["gate"].values())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
