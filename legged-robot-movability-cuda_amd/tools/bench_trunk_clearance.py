#!/usr/bin/env python3
"""Trunk-leg clearance per set (lrm_trunk_clearance_posed_dev) on config 3: the reference terrain
(tests/golden/terrain_ground.npz: 65 536 targets, 89 600 near-ground lattice bodies), 6 M2 legs, one unit quaternion of the
reference's sweep per pose, the clouds in Morton order (--raster: as stored).  One set per pose: the angles are ik()'s on
footholds()'s choice about a ring of nominal points, as in the chain update -> footholds -> ik -> trunk_clearance ->
self_clearance.  The trunk is a cylinder a little beyond the legs' mounts (--trunk).  HIP events, the median of --reps single
calls after warm-up.  In the same run: ik() and self_clearance(), then the new call on the chain's angles and on random
angles (every leg valid), next to the host loop's own time.
Prints one JSON line; --check compares every answer with the host loop lrm_trunk_clearance_posed_cpu."""
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
    ap.add_argument("--trunk", type=float, nargs=3, default=None, help="trunk_radius plus_z minus_z (mm); default: 5 mm past the farthest mount, 40, -80")
    ap.add_argument("--links", type=int, default=0b110, help="bit k set: link k is tested (0 coxa, 1 femur, 2 tibia)")
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
    ps = lrm_amd.PoseSet(legs, nb, ik=True, footholds=True, nominal=nominal)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device="cuda")
    count, best, d2, alll = i32(nl, nb), i32(nl, nb), f32(nl, nb), u8(nb)
    tt = torch.from_numpy(np.ascontiguousarray(ground.T)).cuda()
    qt, bt = torch.from_numpy(quats).cuda(), torch.from_numpy(bodies).cuda()
    ps.update(qt, bt)
    ps.footholds(tt[0], tt[1], tt[2], count, best, d2, alll)
    pi, li = lrm_amd.device.footholds_layout(nb, nl, "cuda")
    ang, st = f32(3, nl * nb), u8(nl * nb)
    res = {"workload": f"config 3: {nb} sets (one per pose) x {nl} legs, angles from ik() on footholds()'s choice among {nt} reference terrain points",
           "order": "raster" if args.raster else "morton", "radius": list(args.radius), "margin": args.margin, "tip_clear": args.tip_clear}
    res["ik_posed_ms"] = median_ms(torch, lambda: ps.ik(tt[0], tt[1], tt[2], pi, li, target_idx=best.view(-1), out=ang, status=st, check=False),
                                   args.warm, args.reps)
    trunk = tuple(args.trunk) if args.trunk else (float(np.abs(np.asarray(legs, np.float32).reshape(-1, 14)[:, 1]).max()) + 5.0, 40.0, -80.0)  # column 1: the body offset of the mount
    res["trunk"], res["links"] = list(trunk), args.links
    hits, with_, slinks, sworst, spen, sfree = i32(nl, nb), u8(nl, nb), u8(nl, nb), u8(nl, nb), f32(nl, nb), u8(nb)
    res["self_clearance_ms"] = median_ms(torch, lambda: ps.self_clearance(ang, args.radius, args.margin, args.tip_clear, None, None, hits, with_,
                                                                         slinks, sworst, spen, sfree), args.warm, args.reps)
    rng = np.random.default_rng(2)
    rnd = np.stack([rng.uniform(-1.2, 1.2, nl * nb), rng.uniform(-1.4, 1.0, nl * nb), rng.uniform(-2.4, 0.2, nl * nb)]).astype(np.float32)
    hit, worst, pen, free = u8(nl, nb), u8(nl, nb), f32(nl, nb), u8(nb)
    for name, a in (("chain_angles", ang), ("random_angles", torch.from_numpy(rnd).cuda())):
        call = lambda: ps.trunk_clearance(a, args.radius, trunk[0], trunk[1], trunk[2], args.margin, args.tip_clear, args.links, None, None, hit,
                                          worst, pen, free)
        r = {"trunk_clearance_ms": median_ms(torch, call, args.warm, args.reps), "free_sets": int(free.sum().item()),
             "hit_legs": int((hit != 0).sum().item()), "femur_hits": int(((hit >> 1) & 1).sum().item()),
             "tibia_hits": int(((hit >> 2) & 1).sum().item()), "near_legs": int((worst != 255).sum().item())}
        if not args.no_host or args.check:
            want = lrm_amd.trunk_clearance_posed_cpu(quats, legs, np.ascontiguousarray(a.cpu().numpy().T), args.radius, trunk[0], trunk[1],
                                                     trunk[2], args.margin, args.tip_clear, args.links)
            r["host_loop_ms"] = want[4]
            if args.check:
                got = (hit, worst, pen, free)
                r["identical_to_host"] = bool(all(np.array_equal(np.ascontiguousarray(g.cpu().numpy()).view(np.uint8),
                                                                 np.ascontiguousarray(w).view(np.uint8)) for g, w in zip(got, want[:4])))
        res[name] = r
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
