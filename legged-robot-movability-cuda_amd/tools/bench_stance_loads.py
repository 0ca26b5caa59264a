#!/usr/bin/env python3
"""Static foot loads and joint torques (lrm_stance_loads_posed_dev) on config 3: the reference terrain
(tests/golden/terrain_ground.npz: 65 536 targets, 89 600 near-ground lattice bodies), 6 M2 legs, one unit quaternion of the
reference's sweep per pose, the clouds in Morton order (--raster: as stored).  One set per pose: the angles are ik()'s on
footholds()'s choice about a ring of nominal points, as in the chain update -> footholds -> ik -> stance_loads.  HIP events,
the median of --reps single calls after warm-up.  In the same process: ik() and stance_stability(), then the new call with
1, 7 ("each"), 64 (every subset of six legs) and 256 lift sets, stance_stability() timed next to it for each count, and the
host loop's own time for the same shape.  Prints one JSON line; --check compares every answer of every run with the host loop
lrm_stance_loads_posed_cpu."""
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
    ap.add_argument("--tau-max", type=float, nargs=3, default=(float("inf"), 60.0, 30.0), help="coxa, femur, tibia (weight x mm)")
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
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device="cuda")
    tt = torch.from_numpy(np.ascontiguousarray(ground.T)).cuda()
    qt, bt = torch.from_numpy(quats).cuda(), torch.from_numpy(bodies).cuda()
    ps.update(qt, bt)
    best = ps.footholds(tt[0], tt[1], tt[2])[1]
    pi, li = lrm_amd.device.footholds_layout(nb, nl, "cuda")
    ang, st = f32(3, nl * nb), u8(nl * nb)
    ik = lambda: ps.ik(tt[0], tt[1], tt[2], pi, li, target_idx=best.view(-1), out=ang, status=st, check=False)
    res = {"workload": f"config 3: {nb} sets (one per pose) x {nl} legs, angles from ik() on the feet chosen among {nt} reference terrain points",
           "order": "raster" if args.raster else "morton", "com": list(args.com), "tau_max": list(args.tau_max)}
    res["ik_posed_ms"] = median_ms(torch, ik, args.warm, args.reps)
    res["legs_with_angles"] = int((st != 0).sum().item())
    ang_h = np.ascontiguousarray(ang.cpu().numpy().T)
    subsets = np.arange(1 << nl, dtype=np.uint8)
    lifts = {"1": None, str(nl + 1): "each", str(len(subsets)): subsets, "256": np.resize(subsets, 256)}
    for name, lift in lifts.items():
        nm = len(lrm_amd.stance_lift(lift, nl))
        out = (u8(nm, nb), u8(nm, nb), f32(nm, nb), u8(nm, nb), f32(nm, nl, nb), f32(nm, nl, 3, nb))
        margin, edge, stable, feet = f32(nm, nb), u8(nm, nb), u8(nm, nb), u8(nb)
        call = lambda: ps.stance_loads(ang, qt, args.tau_max, None, args.com, None, lift, None, *out)
        lean = lambda: ps.stance_loads(ang, qt, args.tau_max, None, args.com, None, lift, None, out[0], out[1], out[2], want_peak_at=False,
                                       want_load=False, want_tau=False)
        stab = lambda: ps.stance_stability(tt[0], tt[1], tt[2], best, qt, bt, None, args.com, None, lift, 0.0, None, margin, edge, stable, feet)
        r = {"stance_loads_ms": median_ms(torch, call, args.warm, args.reps),
             "stance_loads_without_load_and_tau_ms": median_ms(torch, lean, args.warm, args.reps),
             "stance_stability_ms": median_ms(torch, stab, args.warm, args.reps), "answers": nm * nb}
        call()
        torch.cuda.synchronize()
        r["statuses_0_to_4"] = [int(v) for v in torch.bincount(out[0].view(-1).to(torch.int64), minlength=5).cpu()]
        r["holdable_answers"] = int(out[1].sum(dtype=torch.int64).item())
        if not args.no_host or args.check:
            want = lrm_amd.stance_loads_posed_cpu(quats, legs, ang_h, args.tau_max, None, args.com, None, lift)
            r["host_loop_ms"] = want[6]
            if args.check:
                r["identical_to_host"] = bool(all(np.array_equal(np.ascontiguousarray(g.cpu().numpy()).view(np.uint8),
                                                                 np.ascontiguousarray(w).view(np.uint8)) for g, w in zip(out, want[:6])))
        res[f"nmasks_{name}"] = r
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
