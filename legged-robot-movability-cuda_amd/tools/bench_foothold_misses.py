#!/usr/bin/env python3
"""Nearest-miss footholds per (pose, leg) (lrm_foothold_misses_posed_dev) on config 3: the reference terrain
(tests/golden/terrain_ground.npz: 65 536 targets, 89 600 near-ground lattice bodies), 6 M2 legs, one unit quaternion of the
reference's sweep per pose, the clouds in raster and in Morton order.  Every --lift-every-th body is raised by --lift mm,
so that a share of the legs is footless; the share is measured and printed.  HIP events, the median of --reps single
launches after warm-up.  Per order: lrm_footholds_posed_dev (whose count_out is the new call's count_in), the new call at
margins 0, 100 and 400 with near_out's total (the distance evaluations done) and the number of entries answered, and the
same answers through existing calls only: PoseSet.reach_dist over EVERY target for each footless (pose, leg) of the first
--route-entries footless entries plus the torch reduction (m2, mask and argmin per entry), scaled per footless entry.
Prints one JSON line per order; --check N compares N random poses with the host loop lrm_foothold_misses_posed_cpu."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_footholds_posed import median_ms  # noqa: E402

MARGINS = (0.0, 100.0, 400.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=0, help="0 = every body of the reference lattice (89 600)")
    ap.add_argument("--legs", type=int, default=6)
    ap.add_argument("--lift", type=float, default=200.0, help="mm by which every --lift-every-th body is raised")
    ap.add_argument("--lift-every", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=30, help="untimed launches first: the GPU needs ~50 ms of load to reach its steady clocks")
    ap.add_argument("--route-entries", type=int, default=192, help="footless (pose, leg) entries answered through reach_dist + torch")
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
    bodies0 = bodies0.copy()
    bodies0[::args.lift_every, 2] += np.float32(args.lift)
    legs = workloads.hexapod(lrm_amd.get_M2_leg, args.legs)
    sweep = np.asarray(workloads.reference_sweep_quats(), np.float32)
    nb, nl, nt = len(bodies0), len(legs), len(ground0)
    quats0 = np.ascontiguousarray(sweep[np.random.default_rng(1).integers(0, len(sweep), nb)])
    ps = lrm_amd.PoseSet(legs, nb, footholds=True)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    count, best, d2, alll = i32(nl, nb), i32(nl, nb), f32(nl, nb), torch.empty(nb, dtype=torch.uint8, device="cuda")
    miss, near, m2, shift = i32(nl, nb), i32(nl, nb), f32(nl, nb), f32(3, nl, nb)
    for order in ("raster", "morton"):
        ground, bodies, quats = ground0, bodies0, quats0
        if order == "morton":
            ground = ground0[lrm_amd.morton_order(ground0)]
            perm = lrm_amd.morton_order(bodies0)
            bodies, quats = np.ascontiguousarray(bodies0[perm]), np.ascontiguousarray(quats0[perm])
        tt = torch.from_numpy(np.ascontiguousarray(ground.T)).cuda()
        ps.update(torch.from_numpy(quats).cuda(), torch.from_numpy(np.ascontiguousarray(bodies)).cuda())
        res = {"workload": f"config 3: {nb} poses x {nt} reference terrain points x {nl} legs, every {args.lift_every}th body +{args.lift:g} mm",
               "order": order}
        res["footholds_posed_ms"] = median_ms(torch, lambda: ps.footholds(tt[0], tt[1], tt[2], count, best, d2, alll), args.warm, args.reps)
        footless = int((count == 0).sum().item())
        res["footless_entries"] = footless
        res["footless_share"] = footless / (nl * nb)
        for margin in MARGINS:
            ms = median_ms(torch, lambda: ps.foothold_misses(tt[0], tt[1], tt[2], margin, count, miss, m2, shift, near), args.warm, args.reps)
            res[f"misses_m{margin:g}_ms"] = ms
            res[f"misses_m{margin:g}_us_per_footless_entry"] = 1e3 * ms / max(footless, 1)
            res[f"misses_m{margin:g}_distance_evaluations"] = int(near.sum(dtype=torch.int64).item())
            res[f"misses_m{margin:g}_answered"] = int((miss >= 0).sum().item())
        if args.check:
            pick = np.sort(np.random.default_rng(0).choice(nb, args.check, replace=False))
            want = lrm_amd.foothold_misses_posed_cpu(ground, quats[pick], bodies[pick], legs, MARGINS[-1], count.cpu().numpy()[:, pick])
            got = miss.cpu().numpy()[:, pick], m2.cpu().numpy()[:, pick], shift.cpu().numpy()[:, :, pick], near.cpu().numpy()[:, pick]
            same = all(np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
                       for g, w in zip(got, want[:4]))
            res["cpu_check"] = {"poses": int(args.check), "margin": MARGINS[-1], "identical": bool(same)}
        # the query route: reach_dist over every target for each footless (pose, leg), then the reduction in torch
        ent = torch.nonzero((count == 0).view(-1))[:args.route_entries, 0]  # o = l*nb + p
        ne = int(ent.numel())
        if ne:
            pose_idx = (ent % nb).to(torch.int32).repeat_interleave(nt)
            leg_idx = (ent // nb).to(torch.uint8).repeat_interleave(nt)
            qx, qy, qz = tt[0].repeat(ne), tt[1].repeat(ne), tt[2].repeat(ne)
            mask = torch.empty(ne * nt, dtype=torch.uint8, device="cuda")
            field = f32(3, ne * nt)
            valid = torch.empty(ne * nt, dtype=torch.uint8, device="cuda")

            def route():
                ps.reach_dist(qx, qy, qz, pose_idx, leg_idx, mask, field, valid, check=False)
                v = (field[0] * field[0] + field[1] * field[1]) + field[2] * field[2]
                v = torch.where((mask == 0) & (v < float("inf")), v, torch.full_like(v, float("inf")))
                mn, arg = v.view(ne, nt).min(dim=1)
                return mn, arg, field.view(3, ne, nt).gather(2, arg.view(1, ne, 1).expand(3, ne, 1))

            ms = median_ms(torch, route, 3, max(3, args.reps // 4))
            res["route_entries"] = ne
            res["route_ms"] = ms
            res["route_us_per_footless_entry"] = 1e3 * ms / ne
            res["route_over_misses_m400_per_entry"] = res["route_us_per_footless_entry"] / res["misses_m400_us_per_footless_entry"]
            del pose_idx, leg_idx, qx, qy, qz, mask, field, valid
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
