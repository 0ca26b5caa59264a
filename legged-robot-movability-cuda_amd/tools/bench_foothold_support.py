#!/usr/bin/env python3
"""Per-target foothold support (lrm_foothold_support_posed_dev) on config 3: the reference terrain
(tests/golden/terrain_ground.npz: 65 536 targets, 89 600 near-ground lattice bodies), 6 M2 legs, one unit quaternion of the
reference's sweep per pose, the clouds in raster and in Morton order.  HIP events, the median of --reps single calls after
warm-up.  Per order: lrm_footholds_posed_dev (whose all_legs_out is one of the two pose_live forms), the new call with
pose_live NULL and with pose_live = all_legs, and the route it replaces, timed in the same run: footholds +
foothold_offsets + foothold_lists into a buffer of the exact size, then the transposition in torch -- the pose of every
list entry by repeat_interleave, bincount over leg * nt + target for the counts and scatter_reduce(amin) of
(d2 bits << 32 | pose) for the choice.  The two routes' answers are compared.  Prints one JSON line per order; --check N
compares N random targets with the host loop lrm_foothold_support_posed_cpu."""
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
    ap.add_argument("--check", type=int, default=0)
    ap.add_argument("--no-route", action="store_true", help="time the new call only (A/B runs of kernel variants through LRM_LIB_PATH)")
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
    ps = lrm_amd.PoseSet(legs, nb, footholds=True)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    count, best, d2, alll = i32(nl, nb), i32(nl, nb), f32(nl, nb), torch.empty(nb, dtype=torch.uint8, device="cuda")
    scount, spose, sd2, smask = i32(nl, nt), i32(nl, nt), f32(nl, nt), torch.empty(nt, dtype=torch.uint8, device="cuda")
    grid = lrm_amd.dbg_foothold_support_grid(nt, nb)
    for order in ("raster", "morton"):
        ground, bodies, quats = ground0, bodies0, quats0
        if order == "morton":
            ground = ground0[lrm_amd.morton_order(ground0)]
            perm = lrm_amd.morton_order(bodies0)
            bodies, quats = np.ascontiguousarray(bodies0[perm]), np.ascontiguousarray(quats0[perm])
        tt = torch.from_numpy(np.ascontiguousarray(ground.T)).cuda()
        ps.update(torch.from_numpy(quats).cuda(), torch.from_numpy(np.ascontiguousarray(bodies)).cuda())
        res = {"workload": f"config 3: {nb} poses x {nt} reference terrain points x {nl} legs", "order": order, "grid": grid}
        res["footholds_posed_ms"] = median_ms(torch, lambda: ps.footholds(tt[0], tt[1], tt[2], count, best, d2, alll), args.warm, args.reps)
        res["positionable_poses"] = int(alll.sum().item())
        res["support_live_all_legs_ms"] = median_ms(torch, lambda: ps.foothold_support(tt[0], tt[1], tt[2], alll, scount, spose, sd2, smask),
                                                    args.warm, args.reps)
        res["support_live_all_legs_triples"] = int(scount.sum(dtype=torch.int64).item())
        res["support_ms"] = median_ms(torch, lambda: ps.foothold_support(tt[0], tt[1], tt[2], None, scount, spose, sd2, smask),
                                      args.warm, args.reps)
        res["support_triples"] = int(scount.sum(dtype=torch.int64).item())
        res["targets_no_leg_reaches"] = int((smask == 0).sum().item())
        if args.check:
            pick = np.sort(np.random.default_rng(0).choice(nt, args.check, replace=False))
            want = lrm_amd.foothold_support_posed_cpu(ground[pick], quats, bodies, legs)
            got = scount.cpu().numpy()[:, pick], spose.cpu().numpy()[:, pick], sd2.cpu().numpy()[:, pick], smask.cpu().numpy()[pick]
            same = all(np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
                       for g, w in zip(got, want[:4]))
            res["cpu_check"] = {"targets": int(args.check), "identical": bool(same)}
        if args.no_route:
            print(json.dumps(res), flush=True)
            continue
        # the route the call replaces: CSR lists, then their transposition in torch
        offsets = lrm_amd.foothold_offsets(count.view(-1))
        total = int(offsets[-1].item())
        idx, ld2, written = i32(total), f32(total), i32(nl, nb)
        entry = torch.arange(nl * nb, dtype=torch.int64, device="cuda")
        big = torch.iinfo(torch.int64).max

        def lists():
            ps.footholds(tt[0], tt[1], tt[2], count, best, d2, alll)
            lrm_amd.foothold_offsets(count.view(-1), offsets)
            ps.foothold_lists(tt[0], tt[1], tt[2], offsets=offsets, capacity=total, idx=idx, d2=ld2, written=written)

        def transpose():
            o = torch.repeat_interleave(entry, count.view(-1).to(torch.int64), output_size=total)  # o = l*nb + p per list entry
            bins = (o // nb) * nt + idx.to(torch.int64)
            key = (ld2.view(torch.int32).to(torch.int64) << 32) | (o % nb)
            c = torch.bincount(bins, minlength=nl * nt)
            k = torch.full((nl * nt,), big, dtype=torch.int64, device="cuda").scatter_reduce_(0, bins, key, "amin")
            return c, k

        res["csr_entries"] = total
        res["csr_lists_ms"] = median_ms(torch, lists, 3, args.reps)
        res["csr_transpose_ms"] = median_ms(torch, transpose, 3, args.reps)
        res["csr_route_ms"] = res["csr_lists_ms"] + res["csr_transpose_ms"]
        res["csr_route_over_support"] = res["csr_route_ms"] / res["support_ms"]
        c, k = transpose()
        have = c > 0
        res["routes_agree"] = bool(torch.equal(c.to(torch.int32), scount.view(-1)) and
                                   torch.equal((k[have] & 0xFFFFFFFF).to(torch.int32), spose.view(-1)[have]) and
                                   torch.equal((k[have] >> 32).to(torch.int32), sd2.view(-1)[have].view(torch.int32)))
        del idx, ld2, written, entry, c, k, have, offsets
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
