#!/usr/bin/env python3
"""Common-foothold counts and choice per pose transition (lrm_foothold_edges_posed_dev) on config 3: the reference terrain
(tests/golden/terrain_ground.npz: 65 536 targets, 89 600 near-ground lattice bodies, 50 mm apart), 6 M2 legs, one unit
quaternion of the reference's sweep per pose, the clouds in raster and in Morton order.  Edge sets: every pose to its +x
lattice neighbour (one edge per pose), and to its 8 neighbours in the lattice plane (eight per pose); a pose without that
neighbour is paired with itself, so the sets hold exactly nposes and 8 x nposes edges.  HIP events, the median of --reps
single launches after warm-up.  Per (order, edge set): the edge call; in the same run lrm_footholds_posed_dev (the
yardstick: time per pose against time per edge) and the count -> offsets -> lists chain whose intersection the edge call
replaces; the total common count and the share of edges feasible with all feet planted.  Prints one JSON line per
combination; --check N compares N random edges of each with the host loop lrm_foothold_edges_posed_cpu; --only-count
times nothing but lrm_footholds_posed_dev (for a library variant given by LRM_LIB_PATH that lacks the newer calls)."""
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

STEP = 50.0  # the lattice's voxel (tests/golden/make_terrain.py)
PLANE8 = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]


def lattice_neighbours(bodies, steps):
    """[len(steps), nb] int32: the index of the body at (ix + dx, iy + dy, iz), or the body's own index without one.  Host numpy
    on a lattice with a known step; device.pose_edges() / PoseSet.edges() now builds edges on the device from any poses
    (tools/bench_pose_edges.py)."""
    ijk = np.rint((bodies.astype(np.float64) - bodies.min(0)) / STEP).astype(np.int64)
    dim = ijk.max(0) + 3
    key = lambda a: ((a[:, 2] + 1) * dim[1] + (a[:, 1] + 1)) * dim[0] + (a[:, 0] + 1)
    mine = key(ijk)
    order = np.argsort(mine, kind="stable")
    sorted_keys = mine[order]
    assert (np.diff(sorted_keys) > 0).all(), "two bodies on one lattice node"
    out = np.empty((len(steps), len(bodies)), np.int32)
    for k, (dx, dy) in enumerate(steps):
        want = key(ijk + np.array([dx, dy, 0]))
        pos = np.clip(np.searchsorted(sorted_keys, want), 0, len(bodies) - 1)
        found = sorted_keys[pos] == want
        out[k] = np.where(found, order[pos], np.arange(len(bodies)))
    return out


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
    quats0 = np.ascontiguousarray(sweep[np.random.default_rng(1).integers(0, len(sweep), nb)])
    ps = lrm_amd.PoseSet(legs, nb, footholds=True, nominal=nominal)
    count1 = torch.empty((nl, nb), dtype=torch.int32, device="cuda")
    best1 = torch.empty((nl, nb), dtype=torch.int32, device="cuda")
    d21 = torch.empty((nl, nb), dtype=torch.float32, device="cuda")
    all1 = torch.empty(nb, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(nl * nb + 1, dtype=torch.int64, device="cuda")
    written = torch.empty((nl, nb), dtype=torch.int32, device="cuda")
    for order in ("raster", "morton"):
        ground, bodies, quats = ground0, bodies0, quats0
        if order == "morton":
            ground = ground0[lrm_amd.morton_order(ground0)]
            perm = lrm_amd.morton_order(bodies0)
            bodies, quats = np.ascontiguousarray(bodies0[perm]), np.ascontiguousarray(quats0[perm])
        tt = torch.from_numpy(np.ascontiguousarray(ground.T)).cuda()
        ps.update(torch.from_numpy(quats).cuda(), torch.from_numpy(np.ascontiguousarray(bodies)).cuda())
        base = {"workload": f"config 3: {nb} poses x {len(ground)} reference terrain points x {nl} legs", "order": order}
        base["footholds_posed_ms"] = median_ms(torch, lambda: ps.footholds(tt[0], tt[1], tt[2], count1, best1, d21, all1),
                                               args.warm, args.reps)
        base["footholds_posed_us_per_pose"] = 1e3 * base["footholds_posed_ms"] / nb
        if args.only_count:
            print(json.dumps(base), flush=True)
            continue
        # the chain the edge call replaces: every pose's lists written out, to be intersected afterwards
        base["offsets_ms"] = median_ms(torch, lambda: lrm_amd.device.foothold_offsets(count1, offsets), 5, args.reps)
        total = int(offsets[-1].item())
        idx = torch.empty(total, dtype=torch.int32, device="cuda")
        base["lists_without_d2_ms"] = median_ms(torch, lambda: ps.foothold_lists(tt[0], tt[1], tt[2], offsets=offsets, capacity=total, idx=idx,
                                                                                 written=written, want_d2=False), args.warm, args.reps)
        base["total_list_length"] = total
        base["count_offsets_lists_ms"] = base["footholds_posed_ms"] + base["offsets_ms"] + base["lists_without_d2_ms"]
        del idx
        nbr = lattice_neighbours(bodies, PLANE8)
        own = np.arange(nb, dtype=np.int32)
        for name, ea, eb in (("plus_x", own, nbr[0]), ("plane_8", np.tile(own, 8), nbr.reshape(-1))):
            ne = len(ea)
            ta, tb = torch.from_numpy(np.ascontiguousarray(ea)).cuda(), torch.from_numpy(np.ascontiguousarray(eb)).cuda()
            count = torch.empty((nl, ne), dtype=torch.int32, device="cuda")
            best = torch.empty((nl, ne), dtype=torch.int32, device="cuda")
            d2 = torch.empty((nl, ne), dtype=torch.float32, device="cuda")
            alll = torch.empty(ne, dtype=torch.uint8, device="cuda")
            res = dict(base, edge_set=name, edges=ne, self_edges=int((ea == eb).sum()))
            res["foothold_edges_ms"] = median_ms(torch, lambda: ps.foothold_edges(tt[0], tt[1], tt[2], ta, tb, count, best, d2, alll, check=False),
                                                 args.warm if ne <= nb else 5, args.reps)
            res["foothold_edges_us_per_edge"] = 1e3 * res["foothold_edges_ms"] / ne
            res["per_edge_over_per_pose"] = res["foothold_edges_us_per_edge"] / base["footholds_posed_us_per_pose"]
            res["total_common"] = int(count.sum(dtype=torch.int64).item())
            res["feasible_edge_share"] = float(alll.float().mean().item())
            if args.check:
                pick = np.sort(np.random.default_rng(0).choice(ne, args.check, replace=False))
                used, inv = np.unique(np.concatenate([ea[pick], eb[pick]]), return_inverse=True)
                ha, hb = inv[:len(pick)].astype(np.int32), inv[len(pick):].astype(np.int32)
                want = lrm_amd.foothold_edges_posed_cpu(ground, quats[used], bodies[used], legs, ha, hb, nominal)
                got = count.cpu().numpy()[:, pick], best.cpu().numpy()[:, pick], d2.cpu().numpy()[:, pick], alll.cpu().numpy()[pick]
                same = all(np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
                           for g, w in zip(got, want[:4]))
                res["cpu_check"] = {"edges": int(args.check), "identical": bool(same)}
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
