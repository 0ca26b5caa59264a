#!/usr/bin/env python3
"""Per-leg foothold counts and choice (lrm_footholds_dev) on the config-3 shape of bench_positionability.py: terrain(316),
100 000 lattice bodies, 6 M2 legs, optionally Morton-ordered.  The nominal point of each leg is its foot at mid-range joint
angles (lrm_fk_cpu).  Times lrm_footholds_dev and lrm_reach_any_dev on the same inputs with HIP events after warm-up and
prints one JSON line; --check N compares N random bodies with the host loop lrm_footholds_cpu."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def neutral_tips(lrm_amd, legs):
    """the foot of each leg at the middle of its joint limits {coxa, femur, tibia}, relative to the body"""
    mid = np.stack([[(l[8] + l[9]) / 2, (l[12] + l[13]) / 2, (l[10] + l[11]) / 2] for l in legs]).astype(np.float32)
    return np.concatenate([lrm_amd.apply_fk_cpu(mid[i:i + 1], legs[i])[0] for i in range(len(legs))])


def timed(torch, fn, warm, reps):
    for _ in range(max(warm, 1)):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=100_000)
    ap.add_argument("--terrain-side", type=int, default=316)  # 316^2 = 99 856 points
    ap.add_argument("--legs", type=int, default=6)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warm", type=int, default=50, help="untimed launches first: the GPU needs ~50 ms of load to reach its steady clocks")
    ap.add_argument("--check", type=int, default=0, help="verify this many random bodies against lrm_footholds_cpu")
    ap.add_argument("--mode", choices=["strict", "fast"], default="fast")
    ap.add_argument("--morton", action="store_true", help="feed both clouds in Morton order (lrm_morton_order)")
    args = ap.parse_args()
    import torch
    import lrm_amd
    from lrm_amd import workloads
    lrm_amd.set_mode(lrm_amd.MODE_FAST if args.mode == "fast" else lrm_amd.MODE_STRICT)
    ground = workloads.terrain(args.terrain_side)
    bodies = workloads.body_lattice(ground, args.bodies)
    if args.morton:
        ground = ground[lrm_amd.morton_order(ground)]
        bodies = bodies[lrm_amd.morton_order(bodies)]
    legs = workloads.hexapod(lrm_amd.get_M2_leg, args.legs)
    nominal = neutral_tips(lrm_amd, legs)
    tb = torch.from_numpy(np.ascontiguousarray(bodies.T)).cuda()
    tt = torch.from_numpy(np.ascontiguousarray(ground.T)).cuda()
    nl, nb = len(legs), len(bodies)
    count = torch.empty((nl, nb), dtype=torch.int32, device="cuda")
    best = torch.empty((nl, nb), dtype=torch.int32, device="cuda")
    best_d2 = torch.empty((nl, nb), dtype=torch.float32, device="cuda")
    out = torch.empty((nl, nb), dtype=torch.uint8, device="cuda")
    alll = torch.empty(nb, dtype=torch.uint8, device="cuda")
    foot = lambda: lrm_amd.device.footholds(tb[0], tb[1], tb[2], tt[0], tt[1], tt[2], legs, None, nominal, count, best, best_d2)
    anyr = lambda: lrm_amd.device.reach_any(tb[0], tb[1], tb[2], tt[0], tt[1], tt[2], legs, None, out=out, all_legs=alll)
    ms_any = timed(torch, anyr, args.warm, args.reps)
    ms_foot = timed(torch, foot, args.warm, args.reps)
    got = count.cpu().numpy(), best.cpu().numpy(), best_d2.cpu().numpy()
    res = {"workload": f"config 3: {nb} body poses x {len(ground)} terrain points x {nl} legs", "mode": args.mode,
           "morton_order": bool(args.morton), "footholds_ms": ms_foot, "reach_any_ms": ms_any,
           "footholds_over_reach_any": ms_foot / ms_any, "reachable_pairs": int(got[0].astype(np.int64).sum()),
           "body_leg_per_s": nl * nb / (ms_foot * 1e-3),
           "count_gt0_equals_reach_any": bool(np.array_equal((got[0] > 0).astype(np.uint8), out.cpu().numpy()))}
    if args.check:
        idx = np.sort(np.random.default_rng(0).choice(nb, args.check, replace=False))
        t0 = time.time()
        want = lrm_amd.footholds_cpu(bodies[idx], ground, legs, None, nominal)
        same = all(np.array_equal(np.ascontiguousarray(g[:, idx]).view(np.uint32), np.ascontiguousarray(w).view(np.uint32))
                   for g, w in zip(got, want[:3]))
        res["cpu_check"] = {"bodies": int(args.check), "seconds": time.time() - t0, "identical": bool(same)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
