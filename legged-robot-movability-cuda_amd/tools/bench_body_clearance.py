#!/usr/bin/env python3
"""Body clearance per pose (lrm_body_clearance_posed_dev) on config 3: the reference terrain
(tests/golden/terrain_ground.npz: 65 536 targets, 89 600 near-ground lattice bodies), 6 M2 legs, one unit quaternion of the
reference's sweep per pose, the clouds in raster and in Morton order.  The cylinder is the reference's: the leg's body
radius, 250 mm above and 110 mm below the body origin, the column looked at down to --floor mm.  HIP events, the median of
--reps single calls after warm-up.  Per order, in the same run: the new call with live_in NULL and with
live_in = all_legs, lrm_footholds_posed_dev on the same tables (the same traversal with an expensive pair test), and
lrm_any_in_cylinder_dev on the same bodies and cloud (the unposed predicate: one axis-aligned cylinder, one byte).
Prints one JSON line per order; --check N compares N random poses with the host loop lrm_body_clearance_posed_cpu."""
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
    ap.add_argument("--minus-z", type=float, default=-110.0)
    ap.add_argument("--floor", type=float, default=-410.0)
    ap.add_argument("--check", type=int, default=0)
    args = ap.parse_args()
    import torch
    import lrm_amd
    from lrm_amd import workloads
    t = dict(np.load(os.path.join(ROOT, "tests", "golden", "terrain_ground.npz")))
    ground0 = np.ascontiguousarray(t["ground"], np.float32)
    bodies0 = np.ascontiguousarray(t["bodies"], np.float32)
    if args.poses:
        bodies0 = bodies0[:args.poses]
    legs = workloads.hexapod(lrm_amd.get_M2_leg, args.legs)
    sweep = np.asarray(workloads.reference_sweep_quats(), np.float32)
    nb, nl, nt = len(bodies0), len(legs), len(ground0)
    quats0 = np.ascontiguousarray(sweep[np.random.default_rng(1).integers(0, len(sweep), nb)])
    cyl = (float(legs[0][1]), 250.0, args.minus_z, args.floor)
    ps = lrm_amd.PoseSet(legs, nb, footholds=True)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device="cuda")
    count, best, d2, alll = i32(nl, nb), i32(nl, nb), f32(nl, nb), u8(nb)
    hits, top, height, free, coll = i32(nb), i32(nb), f32(nb), u8(nb), u8(nb)
    for order in ("raster", "morton"):
        ground, bodies, quats = ground0, bodies0, quats0
        if order == "morton":
            ground = ground0[lrm_amd.morton_order(ground0)]
            perm = lrm_amd.morton_order(bodies0)
            bodies, quats = np.ascontiguousarray(bodies0[perm]), np.ascontiguousarray(quats0[perm])
        tt = torch.from_numpy(np.ascontiguousarray(ground.T)).cuda()
        bb = torch.from_numpy(np.ascontiguousarray(bodies.T)).cuda()
        ps.update(torch.from_numpy(quats).cuda(), torch.from_numpy(np.ascontiguousarray(bodies)).cuda())
        res = {"workload": f"config 3: {nb} poses x {nt} reference terrain points", "order": order,
               "cylinder": {"radius": cyl[0], "plus_z": cyl[1], "minus_z": cyl[2], "floor_z": cyl[3]}}
        res["footholds_posed_ms"] = median_ms(torch, lambda: ps.footholds(tt[0], tt[1], tt[2], count, best, d2, alll), args.warm, args.reps)
        res["positionable_poses"] = int(alll.sum().item())
        res["any_in_cylinder_ms"] = median_ms(torch, lambda: lrm_amd.device.any_in_cylinder(bb[0], bb[1], bb[2], tt[0], tt[1], tt[2], cyl[0], cyl[1],
                                                                                            cyl[2], coll), args.warm, args.reps)
        res["clearance_live_all_legs_ms"] = median_ms(torch, lambda: ps.body_clearance(tt[0], tt[1], tt[2], *cyl, alll, hits, top, height, free),
                                                      args.warm, args.reps)
        res["free_and_positionable_poses"] = int(free.sum().item())
        res["clearance_ms"] = median_ms(torch, lambda: ps.body_clearance(tt[0], tt[1], tt[2], *cyl, None, hits, top, height, free),
                                        args.warm, args.reps)
        res["colliding_poses"] = int((hits > 0).sum().item())
        res["empty_columns"] = int((top < 0).sum().item())
        res["hit_pairs"] = int(hits.sum(dtype=torch.int64).item())
        if args.check:
            pick = np.sort(np.random.default_rng(0).choice(nb, args.check, replace=False))
            want = lrm_amd.body_clearance_posed_cpu(ground, quats[pick], bodies[pick], legs, *cyl)
            got = hits.cpu().numpy()[pick], top.cpu().numpy()[pick], height.cpu().numpy()[pick], free.cpu().numpy()[pick]
            same = all(np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
                       for g, w in zip(got, want[:4]))
            res["cpu_check"] = {"poses": int(args.check), "identical": bool(same)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
