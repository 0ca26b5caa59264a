#!/usr/bin/env python3
"""Pose-graph routes (lrm_pose_routes_dev) on config 3: the reference terrain (tests/golden/terrain_ground.npz: 65 536 targets,
89 600 near-ground lattice bodies, 50 mm apart), 6 M2 legs, one unit quaternion of the reference's sweep per pose, the clouds
in Morton order.  Two edge sets: `plus_x`, bench_edge_transit.py's (every body to its +x neighbour, and into a copy of that
neighbour yawed by --yaw degrees: 2 x 89 600 poses), and `plane_8`, bench_foothold_edges.py's (every body to its 8 neighbours in
the lattice plane).  The live bytes are the chain's own: pose_live = footholds()'s all_legs, edge_live = foothold_edges()'s
all_legs (`chain_bytes`: no edge cost, cost = hops).  Those bytes cut config 3 into small pieces, so a second workload, `all_live`,
runs the same edges with every byte live and a cost of 1..8 per edge: the lattice itself, with long routes.  Direction 0, ONE
source: of the live poses with the most usable edges the one that reaches the most (eight are tried on the host).
Per edge set, HIP events, the median of --reps calls after --warm warm ones:
  launches      the relax launches that did work in an eager call (its done);
  fixed_ms      one call with sync=False and rounds = launches plus a half: the time to the proven fixed point;
  doubled_ms    the same call with rounds doubled: what the idle launches cost;
  host_loop_ms  lrm_pose_routes_cpu on the same graph; every device answer is compared with it bit for bit.
The sweeps per launch K and the chunk C are compile-time (make variant FLAGS=-DLRM_ROUTES_SWEEPS=n, LRM_LIB_PATH selects the
library); the plan in force is printed.  One JSON line per edge set and workload."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_edge_transit import plus_x_edges, yawed  # noqa: E402
from bench_foothold_edges import PLANE8, lattice_neighbours  # noqa: E402
from bench_footholds_posed import median_ms  # noqa: E402

KEYS = ("cost", "hops", "pred_edge", "pred_pose")


def best_source(lrm_amd, npz, ea, eb, el, pl, wcost):
    """ONE source: among the live poses with the most usable edges, eight spread over the index range are tried on the host
    and the one that reaches the most poses is kept"""
    usable = (ea != eb) & (el != 0 if el is not None else True) & ((pl[ea] != 0) & (pl[eb] != 0) if pl is not None else True)
    degree = np.bincount(np.concatenate([ea[usable], eb[usable]]), minlength=npz)
    top = np.nonzero(degree == degree.max())[0]
    tries = top[np.unique(np.linspace(0, len(top) - 1, 8).astype(np.int64))]
    reach = [lrm_amd.pose_routes_cpu(npz, ea, eb, np.array([s], np.int32), el, pl, wcost, want_cost=False, want_pred_edge=False,
                                     want_pred_pose=False)[4] for s in tries]
    return np.array([tries[int(np.argmax(reach))]], np.int32), int(usable.sum())


def measure(args, torch, lrm_amd, ps, name, live, npz, ea, eb, at, bt, host_in, dev_in, nt):
    el, pl, wcost = host_in
    ne = len(ea)
    source, usable = best_source(lrm_amd, npz, ea, eb, el, pl, wcost)
    st = torch.from_numpy(source).cuda()
    kw = dict(edge_live=dev_in[0], pose_live=dev_in[1], edge_cost=dev_in[2])
    cost, hops, pe, pp, reached, host_ms = lrm_amd.pose_routes_cpu(npz, ea, eb, source, el, pl, wcost)
    want = dict(zip(KEYS, (cost, hops, pe, pp)))
    res = {"workload": f"config 3, {name}, {live}: {npz} poses, {ne} edges, {nt} reference terrain points, one source",
           "plan": lrm_amd.dbg_pose_routes_plan(ne), "live_poses": npz if pl is None else int((pl != 0).sum()), "usable_edges": usable,
           "reached": int(reached), "deepest_hops": int(hops.max()), "host_loop_ms": host_ms}
    same, proven = [], []

    def compare(out):
        torch.cuda.synchronize()
        proven.append(out[5].item() >= 1)  # False: rounds was too small for this call's launch count; the answer is then unspecified
        same.append(bool(all(np.array_equal(out[i].cpu().numpy(), want[k]) for i, k in enumerate(KEYS)) and out[4].item() == reached))

    out = ps.routes(at, bt, st, rounds=4096, **kw)  # one call of the library, so that done counts every launch that did work
    compare(out)
    launches = int(out[5].item())
    res["launches"] = launches
    enough = launches + max(4, launches // 2)  # the count varies from call to call: loads within a launch may be stale
    for key, rounds in (("fixed_ms", enough), ("doubled_ms", 2 * enough)):
        rounds = min(rounds, 4096)
        ws = lrm_amd.device.pose_routes_workspace(npz, rounds, "cuda")
        call = lambda: ps.routes(at, bt, st, rounds=rounds, sync=False, workspace=ws, cost=out[0], hops=out[1], pred_edge=out[2],
                                 pred_pose=out[3], reached=out[4], done=out[5], **kw)
        res[key] = median_ms(torch, call, args.warm, args.reps)
        res[key.replace("_ms", "_rounds")] = rounds
        compare(out)
    res["idle_launch_us"] = 1e3 * (res["doubled_ms"] - res["fixed_ms"]) / max(1, res["doubled_rounds"] - res["fixed_rounds"])
    res["fixed_point_proven"] = all(proven)
    res["identical_to_host"] = all(same)
    res["host_over_device"] = host_ms / res["fixed_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=0, help="0 = every body of the reference lattice (89 600)")
    ap.add_argument("--legs", type=int, default=6)
    ap.add_argument("--yaw", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=30, help="untimed calls first: the GPU needs ~50 ms of load to reach its steady clocks")
    ap.add_argument("--sets", nargs="+", default=["plus_x", "plane_8"])
    ap.add_argument("--live", nargs="+", default=["chain_bytes", "all_live"])
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
    nb, nl = len(bodies), len(legs)
    quats = np.ascontiguousarray(sweep[np.random.default_rng(1).integers(0, len(sweep), nb)])
    ground = ground[lrm_amd.morton_order(ground)]
    perm = lrm_amd.morton_order(bodies)
    bodies, quats = np.ascontiguousarray(bodies[perm]), np.ascontiguousarray(quats[perm])
    az = 2 * np.pi * np.arange(nl) / nl
    nominal = np.column_stack([260.0 * np.cos(az), 260.0 * np.sin(az), np.full(nl, -160.0)]).astype(np.float32)
    tt = torch.from_numpy(np.ascontiguousarray(ground.T)).cuda()
    for name in args.sets:
        if name == "plus_x":
            a, b = plus_x_edges(bodies)
            q = np.ascontiguousarray(np.concatenate([quats, yawed(quats, args.yaw)]))
            bd = np.ascontiguousarray(np.concatenate([bodies, bodies]))
            ea, eb = np.concatenate([a, a]).astype(np.int32), np.concatenate([b, nb + b]).astype(np.int32)
        else:
            nbr = lattice_neighbours(bodies, PLANE8)
            q, bd = quats, bodies
            ea, eb = np.tile(np.arange(nb, dtype=np.int32), 8), np.ascontiguousarray(nbr.reshape(-1))
        npz, ne = len(q), len(ea)
        ps = lrm_amd.PoseSet(legs, npz, footholds=True, nominal=nominal)
        at, bt = torch.from_numpy(ea).cuda(), torch.from_numpy(eb).cuda()
        ps.update(torch.from_numpy(q).cuda(), torch.from_numpy(bd).cuda())
        pose_live = ps.footholds(tt[0], tt[1], tt[2])[3]
        edge_live = ps.foothold_edges(tt[0], tt[1], tt[2], at, bt, check=False)[3]
        pl, el = pose_live.cpu().numpy(), edge_live.cpu().numpy()
        # all_live: the same edges with every byte live and a cost of 1..8 per edge -- the lattice itself, whose routes are long
        # (the chain's bytes cut config 3 into small pieces: the call then costs its chain of launches and little else)
        wcost = (1 + ((np.arange(ne, dtype=np.uint64) * 2654435761 % 2 ** 32) >> 29)).astype(np.int32)
        for live, host_in, dev_in in (("chain_bytes", (el, pl, None), (edge_live, pose_live, None)),
                                      ("all_live", (None, None, wcost), (None, None, torch.from_numpy(wcost).cuda()))):
            if live not in args.live:
                continue
            res = measure(args, torch, lrm_amd, ps, name, live, npz, ea, eb, at, bt, host_in, dev_in, len(ground))
            print(json.dumps(res), flush=True)
        del ps


if __name__ == "__main__":
    main()
