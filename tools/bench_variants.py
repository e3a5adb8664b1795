"""A/B timing of engine tuning switches on the C2 training step (1 GPU).

Prints, per variant, ms/step and the average time of every propagation
launch of the step in launch order (forward layers 1..L, backward layers
L-1..0), measured with HIP events on the launch stream.

  python tools/bench_variants.py [--steps 20] [--variants a,b,...]

An alternative build of libmirec.so is selected with MIREC_LIB=<path>.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = {
    "base": {},
    "no_hop_list": {"use_hop_list": False},
    "no_reuse": {"reuse_prescaled": False},
    "mask_only": {"use_hop_list": False, "reuse_prescaled": False},
    "no_sweep": {"use_sweep": False},
    # the column sweep's forms: a stream per lane group, a
    # stream per wave for the item rows, and the wave form for both blocks
    "sweep_group": {"sweep_form": "group", "sweep_users": False},
    "sweep_wave": {"sweep_form": "wave", "sweep_users": False},
    "sweep_wave_users": {"sweep_form": "wave", "sweep_users": True},
    # per-XCD pacing of the swept launches and the layer sum of a pruned
    # forward on S only; --pace sets sweep_pace_on's parameters
    "sweep_pace_off": {"sweep_pace": None},
    "sweep_pace_on": {"sweep_pace": {"items": (8, 16, 16), "users": (4, 4, 16)}},
    "layer_sum_hop": {"layer_sum_rows": "hop"},
    "layer_sum_self": {"layer_sum_rows": "self"},
    # the first backward layer through the LDS-prefiltered list kernel
    # 
    "seeded_first_off": {"seeded_first": False},
    "seeded_first_on": {"seeded_first": True},
    # the full launches' three stages of DESIGN.md §26, each on top of the one
    # before: 8-byte slots / 256-row user tiles / plain Adam is the form before
    "full_before": {"sweep_packed": False, "sweep_user_tile": 256, "adam_stream": False},
    "full_packed": {"sweep_packed": True, "sweep_user_tile": 256, "adam_stream": False},
    "full_tile280": {"sweep_packed": True, "sweep_user_tile": 280, "adam_stream": False},
    "full_tile320": {"sweep_packed": True, "sweep_user_tile": 320, "adam_stream": False},
    "full_stream": {"sweep_packed": True, "sweep_user_tile": 280, "adam_stream": True},
    # the in-masked backward launch (launch 5 of 6) through the masked wave
    # sweep, per block of rows
    "inmask_off": {"sweep_inmask": "off"},
    "inmask_items": {"sweep_inmask": "items"},
    "inmask_users": {"sweep_inmask": "users"},
    "inmask_both": {"sweep_inmask": "both"},
}


def parse_pace(spec: str) -> dict:
    """items:LEAD/EVERY/NAP,users:LEAD/EVERY/NAP (a block left out: unpaced)"""
    pace = {"items": None, "users": None}
    for part in filter(None, spec.split(",")):
        block, v = part.split(":")
        pace[block] = tuple(int(t) for t in v.split("/"))
    return pace


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--pace", default="", help="sweep_pace_on: items:LEAD/EVERY/NAP,users:...")
    args = ap.parse_args()
    if args.pace:
        VARIANTS["sweep_pace_on"] = {"sweep_pace": parse_pace(args.pace)}
    from furusato_recommend_amd import LightGCN, SyntheticBipartite
    from furusato_recommend_amd.engine import sample_triples
    dev = torch.device("cuda:0")
    ds = SyntheticBipartite(args.users, args.items, args.edges, seed=0)
    torch.manual_seed(0)
    cfg = {"recdim": args.dim, "layer": 3, "lr": 1e-3, "decay": 1e-4, "device": "cuda:0",
           "bpr_batch_size": args.batch}
    model = LightGCN(cfg, ds)
    eng = model.engine
    emb = model.all_embedding.weight.data
    B = args.batch
    u = torch.empty(B, dtype=torch.int32, device=dev)
    p, n = torch.empty_like(u), torch.empty_like(u)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    step_no = [0]

    def step():
        sample_triples(model.graph, B, 0, step_no[0] * B, u, p, n, err)
        step_no[0] += 1
        eng.train_step(emb, model.optim, u, p, n, 1e-4)

    for name in args.variants.split(","):
        defaults = {k: getattr(eng, k) for k in VARIANTS[name]}
        for k, v in VARIANTS[name].items():
            setattr(eng, k, v)
        eng.invalidate_prescaled()
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        eng.prop_events = []
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        ev, eng.prop_events = eng.prop_events, None
        per = len(ev) // args.steps
        launches = []
        for j in range(per):
            ms = [ev[s * per + j][0].elapsed_time(ev[s * per + j][1]) for s in range(args.steps)]
            launches.append(round(sum(ms) / len(ms), 4))
        print(json.dumps({"variant": name, "ms_per_step": round(dt * 1e3, 4),
                          "launch_ms": launches, "prop_sum_ms": round(sum(launches), 4)}))
        for k, v in defaults.items():
            setattr(eng, k, v)


if __name__ == "__main__":
    main()
