#!/usr/bin/env python3
"""Static stability per stance (lrm_stance_stability_dev) on config 3: the reference terrain
(tests/golden/terrain_ground.npz: 65 536 targets, 89 600 near-ground lattice bodies), 6 M2 legs, one unit quaternion of the
reference's sweep per pose, the clouds in Morton order (--raster: as stored).  One stance per pose: foot = footholds()'s
choice about a ring of nominal points, as in the chain update -> footholds -> stance_stability.  HIP events, the median of
--reps single calls after warm-up.  In the same run: footholds(), then the new call with 1, 7 ("each"), 64 (every subset of
six legs) and 256 lift sets, each next to the host loop's own time for the same shape.  Prints one JSON line; --check
compares every answer of every run with the host loop lrm_stance_stability_cpu."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_footholds_posed import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=0, help="0 = every body of the reference lattice (89 600)")
    ap.add_argument("--legs", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=30, help="untimed launches first: the GPU needs ~50 ms of load to reach its steady clocks")
    ap.add_argument("--com", type=float, nargs=3, default=(40.0, -25.0, -20.0), help="centre of mass in the BODY frame (mm)")
    ap.add_argument("--min-margin", type=float, default=10.0)
    ap.add_argument("--raster", action="store_true")
    ap.add_argument("--no-host", action="store_true", help="skip the host loop's timings")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import torch
    import lrm_amd
    from lrm_amd import workloads
    t = dict(np.load(os.path.join(ROOT, "tests", "golden", "terrain_ground.npz")))
    ground = np.ascontiguousarray(t["ground"], np.float32)
    bodies = np.ascontiguousarray(t["bodies"], np.float32)
    if args.poses:
        bodies = bodies[:args.poses]
    legs = workloads.hexapod(lrm_amd.get_M2_leg, args.legs)
    sweep = np.asarray(workloads.reference_sweep_quats(), np.float32)
    nb, nl, nt = len(bodies), len(legs), len(ground)
    quats = np.ascontiguousarray(sweep[np.random.default_rng(1).integers(0, len(sweep), nb)])
    if not args.raster:
        ground = ground[lrm_amd.morton_order(ground)]
        perm = lrm_amd.morton_order(bodies)
        bodies, quats = np.ascontiguousarray(bodies[perm]), np.ascontiguousarray(quats[perm])
    az = 2 * np.pi * np.arange(nl) / nl
    nominal = np.column_stack([260.0 * np.cos(az), 260.0 * np.sin(az), np.full(nl, -160.0)]).astype(np.float32)
    ps = lrm_amd.PoseSet(legs, nb, footholds=True, nominal=nominal)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device="cuda")
    count, best, d2, alll = i32(nl, nb), i32(nl, nb), f32(nl, nb), u8(nb)
    tt = torch.from_numpy(np.ascontiguousarray(ground.T)).cuda()
    qt, bt = torch.from_numpy(quats).cuda(), torch.from_numpy(bodies).cuda()
    ps.update(qt, bt)
    res = {"workload": f"config 3: {nb} stances (one per pose) x {nl} legs, feet chosen among {nt} reference terrain points",
           "order": "raster" if args.raster else "morton", "com": list(args.com), "min_margin": args.min_margin}
    res["footholds_posed_ms"] = median_ms(torch, lambda: ps.footholds(tt[0], tt[1], tt[2], count, best, d2, alll), args.warm, args.reps)
    res["positionable_poses"] = int(alll.sum().item())
    foot_h = best.cpu().numpy()
    subsets = np.arange(1 << nl, dtype=np.uint8)
    lifts = {"1": None, str(nl + 1): "each", str(len(subsets)): subsets, "256": np.resize(subsets, 256)}
    for name, lift in lifts.items():
        nm = len(lrm_amd.stance_lift(lift, nl))
        margin, edge, stable, feet = f32(nm, nb), u8(nm, nb), u8(nm, nb), u8(nb)
        call = lambda: ps.stance_stability(tt[0], tt[1], tt[2], best, qt, bt, None, args.com, None, lift, args.min_margin, None, margin, edge,
                                           stable, feet)
        r = {"stance_stability_ms": median_ms(torch, call, args.warm, args.reps), "stable_answers": int(stable.sum(dtype=torch.int64).item()),
             "answers": nm * nb}
        if not args.no_host or args.check:
            want = lrm_amd.stance_stability_cpu(ground, foot_h, quats, bodies, None, args.com, None, lift, args.min_margin)
            r["host_loop_ms"] = want[4]
            if args.check:
                got = (margin, edge, stable, feet)
                r["identical_to_host"] = bool(all(np.array_equal(np.ascontiguousarray(g.cpu().numpy()).view(np.uint8),
                                                                 np.ascontiguousarray(w).view(np.uint8)) for g, w in zip(got, want[:4])))
        res[f"nmasks_{name}"] = r
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
