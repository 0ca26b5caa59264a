#!/usr/bin/env python3
"""Planted-foot reach along pose transitions (lrm_edge_transit_posed_dev) on config 3: the reference terrain
(tests/golden/terrain_ground.npz: 65 536 targets, 89 600 near-ground lattice bodies), 6 M2 legs, one unit quaternion of the
reference's sweep per pose, the clouds in Morton order (--raster: as stored).  One edge per body to its +x neighbour on the
lattice (50 mm), plus the same edges into a copy of the neighbour yawed by --yaw degrees; foot = foothold_edges()'s best.
HIP events, the median of --reps single calls after warm-up, for every --samples S.  Next to it:
  1. the host loop of the same call (lrm_edge_transit_posed_cpu), on --host-edges edges scaled to all;
  2. the only device route without the call: the sampled poses interpolated by torch, PoseSet.update() on them and
     reach_dist(mask only) on one query per (edge, leg, sample), in chunks of --chunk edges; its pose table is
     nedges * S * nlegs records of 512 bytes, of which a chunk's worth exists at a time.
Prints one JSON line; --check compares every answer with the host loop (all edges: minutes at S = 33)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_footholds_posed import median_ms  # noqa: E402


def plus_x_edges(bodies, step=50.0):
    """(a, b): every body with a body one lattice step further in x at the same y and z.  Host numpy on a lattice with a known
    step; device.pose_edges() / PoseSet.edges() now builds edges on the device from any poses (tools/bench_pose_edges.py)."""
    key = np.round((bodies.astype(np.float64) - bodies.min(0)) / step).astype(np.int64)
    code = lambda k: (k[:, 0] * 100003 + k[:, 1]) * 100003 + k[:, 2]
    order = np.argsort(code(key))
    sorted_codes = code(key)[order]
    want = code(key + [1, 0, 0])
    pos = np.searchsorted(sorted_codes, want)
    pos[pos >= len(order)] = 0
    has = sorted_codes[pos] == want
    return np.nonzero(has)[0].astype(np.int32), order[pos[has]].astype(np.int32)


def yawed(quats, deg):
    """(cos, 0, 0, sin)(deg / 2) * q: the pose turned about the world's z"""
    c, s = np.cos(np.radians(deg) / 2), np.sin(np.radians(deg) / 2)
    w, x, y, z = (quats[:, k].astype(np.float64) for k in range(4))
    return np.ascontiguousarray(np.column_stack([c * w - s * z, c * x - s * y, c * y + s * x, c * z + s * w]), np.float32)


def route2(torch, lrm_amd, legs, tt, qt, bt, ea, eb, foot, S, chunk, mask_bits):
    """the sampled poses by torch (the blend of include/lrm.h in float32 tensor operations; no claim on the last bit), then
    update() + reach_dist(mask only) per chunk of edges; mask_bits[l, e] receives the packed bits"""
    nl, ne = foot.shape
    ps = lrm_amd.PoseSet(legs, chunk * S)
    u = (torch.arange(S, device="cuda", dtype=torch.float32) / (S - 1))[None, :, None]
    shifts = torch.arange(S, device="cuda", dtype=torch.int64)[None, None, :]
    for e0 in range(0, ne, chunk):
        a, b = ea[e0:e0 + chunk].long(), eb[e0:e0 + chunk].long()
        n = a.numel()
        qa, qb = qt[a], qt[b]
        sg = torch.where((qa * qb).sum(1, keepdim=True) < 0, -1.0, 1.0)
        m = (1 - u) * qa[:, None, :] + u * (sg * qb)[:, None, :]
        q = m / m.norm(dim=2, keepdim=True)
        q[:, 0], q[:, S - 1] = qa, qb
        body = bt[a][:, None, :] + u * (bt[b] - bt[a])[:, None, :]
        ps.update(q.reshape(-1, 4).contiguous(), body.reshape(-1, 3).contiguous())
        f = foot[:, e0:e0 + n]
        tgt = f.clamp(min=0).long()[:, :, None].expand(nl, n, S).reshape(-1)
        pose = (torch.arange(n * S, device="cuda", dtype=torch.int32).reshape(1, n, S)).expand(nl, n, S).reshape(-1).contiguous()
        leg = torch.arange(nl, device="cuda", dtype=torch.uint8)[:, None, None].expand(nl, n, S).reshape(-1).contiguous()
        mask, _, _ = ps.reach_dist(tt[0][tgt], tt[1][tgt], tt[2][tgt], pose, leg, want_dist=False, check=False)
        bits = (mask.reshape(nl, n, S).long() << shifts).sum(2)
        mask_bits[:, e0:e0 + n] = torch.where(f >= 0, bits, torch.zeros_like(bits))
    return mask_bits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=0, help="0 = every body of the reference lattice (89 600)")
    ap.add_argument("--legs", type=int, default=6)
    ap.add_argument("--samples", type=int, nargs="+", default=[5, 9, 33])
    ap.add_argument("--yaw", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=30, help="untimed launches first: the GPU needs ~50 ms of load to reach its steady clocks")
    ap.add_argument("--chunk", type=int, default=8192, help="edges per chunk of route 2")
    ap.add_argument("--host-edges", type=int, default=2000, help="edges the host loop is timed on (scaled to all); 0 = skip")
    ap.add_argument("--raster", action="store_true")
    ap.add_argument("--no-route2", action="store_true")
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
    a, b = plus_x_edges(bodies)
    # poses nb .. 2 nb - 1: the same bodies yawed; edges (a, b) keep the orientation family, (a, nb + b) turn on the way
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
    ps.footholds(tt[0], tt[1], tt[2])
    _, best, _, all_legs = ps.foothold_edges(tt[0], tt[1], tt[2], at, btt, check=False)
    feasible = all_legs != 0
    res = {"workload": f"config 3: {ne} edges ({ne // 2} to the +x neighbour, {ne // 2} into its copy yawed by {args.yaw} degrees) x {nl} legs, "
                       f"foot = foothold_edges()'s best among {nt} reference terrain points",
           "order": "raster" if args.raster else "morton", "feasible_edges": int(feasible.sum().item()),
           "planted_entries": int((best >= 0).sum().item())}
    out = None
    for S in args.samples:
        call = lambda: ps.edge_transit(tt[0], tt[1], tt[2], qt, bt, at, btt, best, S, None, *(out or ()), check=False)
        out = call()
        r = {"edge_transit_ms": median_ms(torch, call, args.warm, args.reps)}
        mask, reached, first_miss, worst, worst_d2, planted, clear, advance = out
        lose = (reached >= 0) & (reached < S)
        r.update(losing_entries=int(lose.sum().item()), feasible_not_clear=int((feasible & (clear == 0)).sum().item()),
                 feasible_not_clear_translation=int((feasible & (clear == 0))[:ne // 2].sum().item()),
                 worst_mm_max=float(worst_d2.max().sqrt().item()), table_bytes_saved=ne * S * nl * 512)
        if not args.no_route2:
            bits = torch.zeros((nl, ne), dtype=torch.int64, device="cuda")
            run2 = lambda: route2(torch, lrm_amd, legs, tt, qt, bt, at, btt, best, S, args.chunk, bits)
            r["route2_update_reach_dist_ms"] = median_ms(torch, run2, 2, 5)
            r["route2_chunk_table_bytes"] = min(args.chunk, ne) * S * nl * 512
            r["route2_mask_mismatches"] = int((bits != mask).sum().item())  # torch's blend is not bit-exact: a handful may differ
        if args.host_edges or args.check:
            k = ne if args.check else min(ne, args.host_edges)
            sel = np.linspace(0, ne - 1, k).astype(np.int64)
            foot = best.cpu().numpy()
            want = lrm_amd.edge_transit_posed_cpu(ground, quats, bodies, legs, ea[sel], eb[sel], np.ascontiguousarray(foot[:, sel]), S)
            r["host_loop_ms"] = want[8] * ne / k
            r["host_loop_edges"] = k
            got = [np.ascontiguousarray(g.cpu().numpy()[..., sel]) for g in out]
            r["identical_to_host"] = bool(all(np.array_equal(g.view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
                                              for g, w in zip(got, want[:8])))
        res[f"S{S}"] = r
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
