#!/usr/bin/env python3
"""Leg link clearance per (pose, leg) (lrm_leg_clearance_posed_dev) on config 3: the reference terrain
(tests/golden/terrain_ground.npz: 65 536 targets, 89 600 near-ground lattice bodies), 6 M2 legs, one unit quaternion of the
reference's sweep per pose, the clouds in raster and in Morton order.  The angles are ik()'s on footholds()'s choice, as in
the chain update -> footholds -> ik -> leg_clearance.  HIP events, the median of --reps single calls after warm-up.  Per
order, in the same run: the new call with live_in NULL and with live_in = all_legs, leg_joints(), and next to them
body_clearance() (the same traversal with one cylinder per pose instead of three capsules per leg), footholds() and ik().
Prints one JSON line per order; --check N compares N random poses with the host loop lrm_leg_clearance_posed_cpu."""
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
    ap.add_argument("--radius", type=float, nargs=3, default=(28.0, 22.0, 16.0), help="coxa, femur, tibia link radius (mm)")
    ap.add_argument("--margin", type=float, default=10.0)
    ap.add_argument("--tip-clear", type=float, default=30.0)
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
    cyl = (float(legs[0][1]), 250.0, -110.0, -410.0)
    leg = (tuple(args.radius), args.margin, args.tip_clear)
    ps = lrm_amd.PoseSet(legs, nb, ik=True, footholds=True)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device="cuda")
    count, best, d2, alll = i32(nl, nb), i32(nl, nb), f32(nl, nb), u8(nb)
    ang, st, joints = f32(3, nl * nb), u8(nl * nb), f32(nl, nb, 4, 3)
    bhits, btop, bheight, bfree = i32(nb), i32(nb), f32(nb), u8(nb)
    hits, links, worst, pen, free = i32(nl, nb), u8(nl, nb), i32(nl, nb), f32(nl, nb), u8(nb)
    pi, li = lrm_amd.device.footholds_layout(nb, nl, "cuda")
    for order in ("raster", "morton"):
        ground, bodies, quats = ground0, bodies0, quats0
        if order == "morton":
            ground = ground0[lrm_amd.morton_order(ground0)]
            perm = lrm_amd.morton_order(bodies0)
            bodies, quats = np.ascontiguousarray(bodies0[perm]), np.ascontiguousarray(quats0[perm])
        tt = torch.from_numpy(np.ascontiguousarray(ground.T)).cuda()
        ps.update(torch.from_numpy(quats).cuda(), torch.from_numpy(np.ascontiguousarray(bodies)).cuda())
        res = {"workload": f"config 3: {nb} poses x {nl} legs x {nt} reference terrain points", "order": order,
               "links": {"radius": list(leg[0]), "margin": leg[1], "tip_clear": leg[2]}}
        res["footholds_posed_ms"] = median_ms(torch, lambda: ps.footholds(tt[0], tt[1], tt[2], count, best, d2, alll), args.warm, args.reps)
        res["positionable_poses"] = int(alll.sum().item())
        res["ik_ms"] = median_ms(torch, lambda: ps.ik(tt[0], tt[1], tt[2], pi, li, target_idx=best.view(-1), out=ang, status=st, check=False),
                                 args.warm, args.reps)
        res["body_clearance_ms"] = median_ms(torch, lambda: ps.body_clearance(tt[0], tt[1], tt[2], *cyl, None, bhits, btop, bheight, bfree),
                                             args.warm, args.reps)
        res["leg_joints_ms"] = median_ms(torch, lambda: ps.leg_joints(ang, leg[2], joints), args.warm, args.reps)
        res["leg_clearance_live_all_legs_ms"] = median_ms(torch, lambda: ps.leg_clearance(tt[0], tt[1], tt[2], ang, *leg, alll, hits, links, worst, pen,
                                                                                           free), args.warm, args.reps)
        res["free_and_positionable_poses"] = int(free.sum().item())
        res["leg_clearance_ms"] = median_ms(torch, lambda: ps.leg_clearance(tt[0], tt[1], tt[2], ang, *leg, None, hits, links, worst, pen, free),
                                            args.warm, args.reps)
        res["hit_legs"] = int((hits > 0).sum().item())
        res["near_legs"] = int((worst >= 0).sum().item())
        res["skipped_legs"] = int((st == 0).sum().item())
        res["hit_pairs"] = int(hits.sum(dtype=torch.int64).item())
        if args.check:
            pick = np.sort(np.random.default_rng(0).choice(nb, args.check, replace=False))
            a = ang.cpu().numpy().T.reshape(nl, nb, 3)[:, pick].reshape(-1, 3)
            want = lrm_amd.leg_clearance_posed_cpu(ground, quats[pick], bodies[pick], legs, a, *leg)
            got = [x.cpu().numpy()[..., pick] for x in (hits, links, worst, pen, free)]
            same = all(np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
                       for g, w in zip(got, want[:5]))
            res["cpu_check"] = {"poses": int(args.check), "identical": bool(same)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
