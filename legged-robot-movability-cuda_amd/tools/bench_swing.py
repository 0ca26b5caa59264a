#!/usr/bin/env python3
"""Swing-foot transit (lrm_swing_transit_posed_dev) on config 3: bench_edge_transit.py's scene -- the reference terrain
(tests/golden/terrain_ground.npz: 65 536 targets, 89 600 near-ground lattice bodies), 6 M2 legs, one unit quaternion of the
reference's sweep per pose, the clouds in Morton order (--raster: as stored), one edge per body to its +x neighbour (50 mm) plus
the same edges into a copy of the neighbour yawed by --yaw degrees.  Edge e lifts leg e mod nlegs, which goes from footholds()'s
best under pose a to its best under pose b (swing_layout); the other legs are not swinging.
HIP events, the median of --reps single calls after warm-up, for every --samples S: once with foot_radius = 0 (the reach kernel
alone) and once with --radius (reach and terrain kernels behind the cloud's boxes).  Next to it, in the same run:
  1. edge_transit() on the same edges with foot = foothold_edges()'s best (six planted legs per edge against one swinging);
  2. the host loop of the same call (lrm_swing_transit_posed_cpu, which consults no box), on --host-edges edges scaled to all.
Prints one JSON line; identical_to_host compares every output of those edges with the host loop."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_edge_transit import plus_x_edges, yawed  # noqa: E402
from bench_footholds_posed import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=0, help="0 = every body of the reference lattice (89 600)")
    ap.add_argument("--legs", type=int, default=6)
    ap.add_argument("--samples", type=int, nargs="+", default=[5, 9, 33])
    ap.add_argument("--yaw", type=float, default=10.0)
    ap.add_argument("--lift", type=float, default=40.0)
    ap.add_argument("--radius", type=float, default=12.0, help="foot_radius of the run with the terrain part")
    ap.add_argument("--margin", type=float, default=15.0)
    ap.add_argument("--skip", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=30, help="untimed launches first: the GPU needs ~50 ms of load to reach its steady clocks")
    ap.add_argument("--host-edges", type=int, default=200, help="edges the host loop is timed on (scaled to all); 0 = skip")
    ap.add_argument("--raster", action="store_true")
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
    a, b = plus_x_edges(bodies)
    quats = np.ascontiguousarray(np.concatenate([quats, yawed(quats, args.yaw)]))
    bodies = np.ascontiguousarray(np.concatenate([bodies, bodies]))
    ea, eb = np.concatenate([a, a]), np.concatenate([b, nb + b]).astype(np.int32)
    ne = len(ea)
    az = 2 * np.pi * np.arange(nl) / nl
    nominal = np.column_stack([260.0 * np.cos(az), 260.0 * np.sin(az), np.full(nl, -160.0)]).astype(np.float32)
    ps = lrm_amd.PoseSet(legs, 2 * nb, footholds=True, nominal=nominal)
    tt = torch.from_numpy(np.ascontiguousarray(ground.T)).cuda()
    qt, bt = torch.from_numpy(quats).cuda(), torch.from_numpy(bodies).cuda()
    at, btt = torch.from_numpy(ea).cuda(), torch.from_numpy(eb).cuda()
    ps.update(qt, bt)
    _, best, _, _ = ps.footholds(tt[0], tt[1], tt[2])
    _, common, _, _ = ps.foothold_edges(tt[0], tt[1], tt[2], at, btt, check=False)
    lift_mask = torch.from_numpy((1 << (np.arange(ne) % nl)).astype(np.uint8)).cuda()
    ff, ft = lrm_amd.swing_layout(best, at, btt, lift_mask)
    res = {"workload": f"config 3: {ne} edges ({ne // 2} to the +x neighbour, {ne // 2} into its copy yawed by {args.yaw} degrees) x {nl} legs, "
                       f"one lifted leg per edge between footholds()'s best among {nt} reference terrain points",
           "order": "raster" if args.raster else "morton", "lift": args.lift, "foot_radius": args.radius, "margin": args.margin,
           "skip": args.skip, "swinging_entries": int(((ff >= 0) & (ft >= 0)).sum().item())}
    kw = dict(lift=args.lift, margin=args.margin, skip=args.skip)
    out = planted = None
    for S in args.samples:
        reach_only = lambda: ps.swing_transit(tt[0], tt[1], tt[2], qt, bt, at, btt, ff, ft, S, foot_radius=0.0, check=False,
                                              **kw, **dict(zip(KEYS, out or ())))
        both = lambda: ps.swing_transit(tt[0], tt[1], tt[2], qt, bt, at, btt, ff, ft, S, foot_radius=args.radius, check=False,
                                        **kw, **dict(zip(KEYS, out or ())))
        transit = lambda: ps.edge_transit(tt[0], tt[1], tt[2], qt, bt, at, btt, common, S, None, *(planted or ()), check=False)
        out, planted = both(), transit()
        r = {"swing_reach_only_ms": median_ms(torch, reach_only, args.warm, args.reps),
             "swing_reach_and_terrain_ms": median_ms(torch, both, args.warm, args.reps),
             "edge_transit_ms": median_ms(torch, transit, args.warm, args.reps)}
        out = both()
        torch.cuda.synchronize()
        mask, reached, first_miss, worst, worst_d2, hits, hit_seg, near, pen, swinging, clear = out
        swg = reached >= 0
        r.update(losing_entries=int((swg & (reached < S)).sum().item()), hitting_entries=int((hits > 0).sum().item()),
                 near_entries=int((near >= 0).sum().item()), clear_edges=int(((clear != 0) & (swinging != 0)).sum().item()))
        if args.host_edges:
            k = min(ne, args.host_edges)
            sel = np.linspace(0, ne - 1, k).astype(np.int64)
            f, g = ff.cpu().numpy(), ft.cpu().numpy()
            want = lrm_amd.swing_transit_posed_cpu(ground, quats, bodies, legs, ea[sel], eb[sel], np.ascontiguousarray(f[:, sel]),
                                                   np.ascontiguousarray(g[:, sel]), S, args.lift, None, args.radius, args.margin, args.skip)
            r["host_loop_ms"] = want[11] * ne / k
            r["host_loop_edges"] = k
            got = [np.ascontiguousarray(x.cpu().numpy()[..., sel]) for x in out]
            r["identical_to_host"] = bool(all(np.array_equal(x.view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
                                              for x, w in zip(got, want[:11])))
        res[f"S{S}"] = r
    print(json.dumps(res), flush=True)


KEYS = ("mask", "reached", "first_miss", "worst", "worst_d2", "hits", "hit_seg", "near", "pen", "swinging", "clear")

if __name__ == "__main__":
    main()
