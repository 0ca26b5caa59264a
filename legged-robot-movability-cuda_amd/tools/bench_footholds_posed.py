#!/usr/bin/env python3
"""Foothold counts and choice per (pose, leg) (PoseSet(footholds=True): lrm_pose_compile_dev +
lrm_pose_footholds_compile_dev + lrm_footholds_posed_dev) on the config-3 shape of bench_footholds.py: terrain(316),
100 000 lattice bodies, 6 M2 legs, optionally Morton-ordered.  HIP events, the median of --reps single launches after
warm-up.  Times
  (a) footholds() with one random orientation of the reference's 45-orientation sweep per pose,
  (b) footholds() with the identity quaternion everywhere,
  (c) lrm_footholds_dev under LRM_MODE_STRICT on the same clouds: the strict pair kernel with the legs as kernel
      arguments, the like-for-like baseline of (b) up to reachable_rotate_leg's gravity gate,
and update() (both compile launches) on its own.  Every quaternion here is unit: a pose with a non-unit one gets the
sphere that excludes nothing, is tested against the whole cloud and would be the launch's tail (include/lrm.h).  Prints one JSON line; --check N compares N random poses of (a) with the
host loop lrm_footholds_posed_cpu."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from bench_footholds import neutral_tips  # noqa: E402


def median_ms(torch, fn, warm, reps):
    for _ in range(max(warm, 1)):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=100_000)
    ap.add_argument("--terrain-side", type=int, default=316)  # 316^2 = 99 856 points
    ap.add_argument("--legs", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=30, help="untimed launches first: the GPU needs ~50 ms of load to reach its steady clocks")
    ap.add_argument("--check", type=int, default=0, help="verify this many random poses of (a) against lrm_footholds_posed_cpu")
    ap.add_argument("--morton", action="store_true", help="feed both clouds in Morton order (lrm_morton_order)")
    args = ap.parse_args()
    import torch
    import lrm_amd
    from lrm_amd import workloads
    ground = workloads.terrain(args.terrain_side)
    bodies = workloads.body_lattice(ground, args.poses)
    if args.morton:
        ground = ground[lrm_amd.morton_order(ground)]
        bodies = bodies[lrm_amd.morton_order(bodies)]
    legs = workloads.hexapod(lrm_amd.get_M2_leg, args.legs)
    nominal = neutral_tips(lrm_amd, legs)  # body frame
    sweep = np.asarray(workloads.reference_sweep_quats(), np.float32)
    nb, nl = len(bodies), len(legs)
    q_sweep = np.ascontiguousarray(sweep[np.random.default_rng(1).integers(0, len(sweep), nb)])
    q_ident = np.tile(np.array([1, 0, 0, 0], np.float32), (nb, 1))
    tb = torch.from_numpy(np.ascontiguousarray(bodies.T)).cuda()
    tt = torch.from_numpy(np.ascontiguousarray(ground.T)).cuda()
    body_d = torch.from_numpy(np.ascontiguousarray(bodies)).cuda()
    qs_d, qi_d = torch.from_numpy(q_sweep).cuda(), torch.from_numpy(q_ident).cuda()
    count = torch.empty((nl, nb), dtype=torch.int32, device="cuda")
    best = torch.empty((nl, nb), dtype=torch.int32, device="cuda")
    best_d2 = torch.empty((nl, nb), dtype=torch.float32, device="cuda")
    alll = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ps = lrm_amd.PoseSet(legs, nb, footholds=True, nominal=nominal)
    posed = lambda: ps.footholds(tt[0], tt[1], tt[2], count, best, best_d2, alll)

    ps.update(qs_d, body_d)
    ms_sweep = median_ms(torch, posed, args.warm, args.reps)
    got = count.cpu().numpy(), best.cpu().numpy(), best_d2.cpu().numpy(), alll.cpu().numpy()
    ms_update = median_ms(torch, lambda: ps.update(qs_d, body_d), 5, args.reps)
    ps.update(qi_d, body_d)
    ms_ident = median_ms(torch, posed, args.warm, args.reps)
    pairs_ident = int(count.sum().item())

    lrm_amd.set_mode(lrm_amd.MODE_STRICT)
    base = lambda: lrm_amd.device.footholds(tb[0], tb[1], tb[2], tt[0], tt[1], tt[2], legs, None, nominal, count, best, best_d2)
    ms_base = median_ms(torch, base, args.warm, args.reps)
    pairs_base = int(count.sum().item())
    lrm_amd.set_mode(lrm_amd.MODE_FAST)

    res = {"workload": f"config 3: {nb} poses x {len(ground)} terrain points x {nl} legs", "morton_order": bool(args.morton),
           "posed_sweep_ms": ms_sweep, "posed_identity_ms": ms_ident, "footholds_dev_strict_ms": ms_base,
           "identity_over_strict_baseline": ms_ident / ms_base, "sweep_over_identity": ms_sweep / ms_ident,
           "update_both_compiles_ms": ms_update, "reachable_pairs_sweep": int(got[0].astype(np.int64).sum()),
           "reachable_pairs_identity": pairs_ident, "reachable_pairs_baseline": pairs_base,
           "positionable_poses_sweep": int(got[3].sum()), "pose_leg_per_s_sweep": nl * nb / (ms_sweep * 1e-3)}
    if args.check:
        idx = np.sort(np.random.default_rng(0).choice(nb, args.check, replace=False))
        t0 = time.time()
        want = lrm_amd.footholds_posed_cpu(ground, q_sweep[idx], bodies[idx], legs, nominal)
        same = all(np.array_equal(np.ascontiguousarray(g[..., idx]).view(np.uint32 if g.dtype != np.uint8 else np.uint8),
                                  np.ascontiguousarray(w).view(np.uint32 if w.dtype != np.uint8 else np.uint8))
                   for g, w in zip(got, want[:4]))
        res["cpu_check"] = {"poses": int(args.check), "seconds": time.time() - t0, "identical": bool(same)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
