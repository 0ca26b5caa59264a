#!/usr/bin/env python3
"""Reachable-foothold lists per (pose, leg) (lrm_footholds_posed_dev -> lrm_foothold_offsets_dev ->
lrm_foothold_lists_posed_dev) on config 3: the reference terrain (tests/golden/terrain_ground.npz: 65 536 targets,
89 600 near-ground bodies), 6 M2 legs, unit quaternions.  HIP events, the median of --reps single launches after
warm-up, for the cloud in raster and in Morton order and for one sweep orientation per pose and the identity
everywhere.  Per combination: the time of the count launch, of the scan, of the fill launch with and without d2_out,
the total list length and the ratio fill / count from the same run.  Prints one JSON line per combination; --check N
compares N random poses with the host loop lrm_foothold_lists_posed_cpu; --only-count times nothing but
lrm_footholds_posed_dev (for a library variant given by LRM_LIB_PATH that lacks the list calls)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_footholds import neutral_tips  # noqa: E402
from bench_footholds_posed import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=0, help="0 = every body of the reference lattice (89 600)")
    ap.add_argument("--legs", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=30, help="untimed launches first: the GPU needs ~50 ms of load to reach its steady clocks")
    ap.add_argument("--check", type=int, default=0)
    ap.add_argument("--only-count", action="store_true")
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
    nominal = neutral_tips(lrm_amd, legs)  # body frame
    sweep = np.asarray(workloads.reference_sweep_quats(), np.float32)
    nb, nl = len(bodies0), len(legs)
    quats = {"sweep": np.ascontiguousarray(sweep[np.random.default_rng(1).integers(0, len(sweep), nb)]),
             "identity": np.tile(np.array([1, 0, 0, 0], np.float32), (nb, 1))}
    ps = lrm_amd.PoseSet(legs, nb, footholds=True, nominal=nominal)
    count = torch.empty((nl, nb), dtype=torch.int32, device="cuda")
    best = torch.empty((nl, nb), dtype=torch.int32, device="cuda")
    best_d2 = torch.empty((nl, nb), dtype=torch.float32, device="cuda")
    alll = torch.empty(nb, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(nl * nb + 1, dtype=torch.int64, device="cuda")
    written = torch.empty((nl, nb), dtype=torch.int32, device="cuda")
    for order in ("raster", "morton"):
        ground, bodies = ground0, bodies0
        if order == "morton":
            ground = ground0[lrm_amd.morton_order(ground0)]
            bodies = bodies0[lrm_amd.morton_order(bodies0)]
        tt = torch.from_numpy(np.ascontiguousarray(ground.T)).cuda()
        body_d = torch.from_numpy(np.ascontiguousarray(bodies)).cuda()
        for qname, q in quats.items():
            ps.update(torch.from_numpy(q).cuda(), body_d)
            res = {"workload": f"config 3: {nb} poses x {len(ground)} reference terrain points x {nl} legs", "order": order,
                   "quaternions": qname}
            res["footholds_posed_ms"] = median_ms(torch, lambda: ps.footholds(tt[0], tt[1], tt[2], count, best, best_d2, alll),
                                                  args.warm, args.reps)
            if not args.only_count:
                res["offsets_ms"] = median_ms(torch, lambda: lrm_amd.device.foothold_offsets(count, offsets), 5, args.reps)
                total = int(offsets[-1].item())
                idx = torch.empty(total, dtype=torch.int32, device="cuda")
                d2 = torch.empty(total, dtype=torch.float32, device="cuda")
                fill = lambda want: ps.foothold_lists(tt[0], tt[1], tt[2], offsets=offsets, capacity=total, idx=idx, d2=d2,
                                                      written=written, want_d2=want)
                res["lists_with_d2_ms"] = median_ms(torch, lambda: fill(True), args.warm, args.reps)
                res["lists_without_d2_ms"] = median_ms(torch, lambda: fill(False), args.warm, args.reps)
                res["total_list_length"] = total
                res["written_equals_count"] = bool(torch.equal(written, count))
                res["lists_with_d2_over_footholds_posed"] = res["lists_with_d2_ms"] / res["footholds_posed_ms"]
                res["lists_without_d2_over_footholds_posed"] = res["lists_without_d2_ms"] / res["footholds_posed_ms"]
                if args.check:
                    fill(True)
                    torch.cuda.synchronize()
                    pick = np.sort(np.random.default_rng(0).choice(nb, args.check, replace=False))
                    off = offsets.cpu().numpy()
                    hc = count.cpu().numpy()[:, pick].reshape(-1).astype(np.int64)
                    hoff = np.concatenate([[0], np.cumsum(hc)])
                    hidx, hd2, hw, _ = lrm_amd.foothold_lists_posed_cpu(ground, q[pick], bodies[pick], legs, hoff, int(hoff[-1]), nominal)
                    gi, gd = idx.cpu().numpy(), d2.cpu().numpy()
                    same = np.array_equal(hw.reshape(-1), hc)
                    for l in range(nl):
                        for k, p in enumerate(pick):
                            a, b = off[l * nb + p], hoff[l * len(pick) + k]
                            n = hc[l * len(pick) + k]
                            same = same and np.array_equal(gi[a:a + n], hidx[b:b + n]) and \
                                np.array_equal(gd[a:a + n].view(np.uint32), hd2[b:b + n].view(np.uint32))
                    res["cpu_check"] = {"poses": int(args.check), "identical": bool(same)}
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
