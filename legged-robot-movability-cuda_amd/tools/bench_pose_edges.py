#!/usr/bin/env python3
"""Pose-graph edges (lrm_pose_edge_counts_dev / lrm_pose_edges_dev) on config 3: the 89 600 near-ground lattice bodies of the
reference terrain (tests/golden/terrain_ground.npz, 50 mm apart) with max_step = one lattice diagonal (50 sqrt 2 mm, rounded
up), as two pose tables: `bodies`, one pose per body (no turn limit), and `sweep`, the reference's 45 orientations per body
(4 032 000 poses, pose = body * 45 + orientation) with a turn limit of 0.4 rad, which links the orientations one pi/8 step of
roll, pitch or yaw apart.  Each in `morton` order (lrm_morton_order of the bodies) and in `raster` order (the file's).
Per table and order, HIP events, the median of --reps calls after --warm warm ones, form "upper":
  counts_ms     pose_edge_counts (the box kernel and the walk);
  fill_ms       pose_edges with the offsets given (the box kernel and the walk again, and the stores);
  offsets_ms    foothold_offsets between the two;
  walk_ms       pose_edge_counts with max_step = 0 on a table of the same size whose chunk c sits alone at x = 1000 c mm: the box
                kernels, the walk over the boxes and the wave's own chunk, nothing else; walk_share = walk_ms / counts_ms;
  touch_ms      pose_edge_counts with max_step = 0 on the table itself: the walk plus every chunk whose box touches the wave's
                own (a lattice in Morton order has chunks whose boxes span a jump of the curve and touch many);
  footholds_ms  PoseSet.footholds() on the same poses and the reference ground in the same process (tables up to
                --footholds-limit poses);
  torch_ms      what a user can do today: a torch brute force in row blocks on the same GPU (squared distances and dots by
                broadcasting, nonzero per block); above --torch-limit poses only --torch-blocks blocks are timed and the figure
                is scaled to the whole table (torch_extrapolated);
  host_loop_ms  lrm_pose_edges_cpu (bodies table, morton order only: it is O(n^2)); the device lists are compared with it bit
                for bit, and every order must give the same number of edges.
One JSON line per table and order."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_footholds_posed import median_ms  # noqa: E402


def torch_brute(torch, q, b, step2, dot2, rows, first, last):
    """edges (a < b) of the rows [first, last) in blocks of `rows`: float32 broadcasting for the distances, a matrix product for the dots"""
    out = []
    n = len(q)
    col = torch.arange(n, device=q.device)
    norm = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
    for r0 in range(first, last, rows):
        r1 = min(r0 + rows, last)
        d = b[None, :, 0] - b[r0:r1, None, 0]
        d2 = d * d
        d = b[None, :, 1] - b[r0:r1, None, 1]
        d2 += d * d
        d = b[None, :, 2] - b[r0:r1, None, 2]
        d2 += d * d
        near = d2 <= step2
        if dot2 > 0:
            c = q[r0:r1] @ q.T
            near &= c * c >= dot2 * (norm[r0:r1, None] * norm[None, :])
        near &= col[None, :] > torch.arange(r0, r1, device=q.device)[:, None]
        out.append(near.nonzero())
    return out


def measure(args, torch, lrm_amd, name, order, quats, bodies, step, turn, ground_t, legs, nominal, host):
    dev = lrm_amd.device
    n = len(quats)
    q, b = torch.from_numpy(quats).cuda(), torch.from_numpy(bodies).cuda()
    ws = dev.pose_edges_workspace(n, "cuda")
    count = torch.empty(n, dtype=torch.int32, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    big = n > args.torch_limit
    warm, reps = (2, 5) if big else (args.warm, args.reps)
    res = {"workload": f"config 3, {name}, {order}: {n} poses, max_step {step:.4f} mm, max_turn {turn}", "plan": lrm_amd.dbg_pose_edges_plan(n)}
    res["counts_ms"] = median_ms(torch, lambda: dev.pose_edge_counts(q, b, step, turn, workspace=ws, count=count), warm, reps)
    res["offsets_ms"] = median_ms(torch, lambda: dev.foothold_offsets(count, out=offsets), warm, reps)
    total = int(offsets[n].item())
    res["edges"] = total
    ea = torch.full((total,), -1, dtype=torch.int32, device="cuda")
    eb = torch.empty(total, dtype=torch.int32, device="cuda")
    d2 = None if big else torch.empty(total, dtype=torch.float32, device="cuda")
    cos2 = None if big else torch.empty(total, dtype=torch.float32, device="cuda")
    written = torch.empty(n, dtype=torch.int32, device="cuda")
    fill = lambda: dev.pose_edges(q, b, step, turn, offsets=offsets, workspace=ws, edge_a=ea, edge_b=eb, d2=d2, cos2=cos2, written=written,
                                  want_d2=not big, want_cos2=not big)
    res["fill_ms"] = median_ms(torch, fill, warm, reps)
    res["lists"] = "edge_a, edge_b" + ("" if big else ", d2, cos2")
    scratch = torch.empty(n, dtype=torch.int32, device="cuda")
    alone = torch.zeros_like(b)
    alone[:, 0] = (torch.arange(n, device="cuda") // 64) * 1000.0
    res["walk_ms"] = median_ms(torch, lambda: dev.pose_edge_counts(q, alone, 0.0, turn, workspace=ws, count=scratch), warm, reps)
    res["touch_ms"] = median_ms(torch, lambda: dev.pose_edge_counts(q, b, 0.0, turn, workspace=ws, count=scratch), warm, reps)
    res["walk_share"] = res["walk_ms"] / res["counts_ms"]
    assert bool((written == count).all()) and int(ea.min().item()) >= 0
    if host is not None:
        hc, ho, ha, hb, hd, hs, _, ms = host
        same = all(np.array_equal(x.cpu().numpy().view(np.int32), y.view(np.int32)) for x, y in ((count, hc), (ea, ha), (eb, hb), (d2, hd), (cos2, hs)))
        res["host_loop_ms"], res["identical_to_host"] = ms, bool(same)
    if n <= args.footholds_limit:
        ps = lrm_amd.PoseSet(legs, n, footholds=True, nominal=nominal).update(q, b)
        res["footholds_ms"] = median_ms(torch, lambda: ps.footholds(ground_t[0], ground_t[1], ground_t[2]), warm, reps)
        del ps
    step2 = float(np.float32(step) * np.float32(step))
    dot2 = float(np.float32(lrm_amd.pose_edges_min_dot(turn)) ** 2)
    rows = args.torch_rows if not big else max(1, args.torch_rows * args.torch_limit // n)
    last = n if not big else min(n, rows * args.torch_blocks)
    brute = lambda: torch_brute(torch, q, b, step2, dot2, rows, 0, last)
    t = median_ms(torch, brute, 1, 3)
    res["torch_ms"], res["torch_extrapolated"], res["torch_rows"] = t * n / last, bool(big), rows
    if not big:
        res["torch_edges"] = int(sum(len(x) for x in brute()))
    res["torch_over_device"] = res["torch_ms"] / (res["counts_ms"] + res["offsets_ms"] + res["fill_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=0, help="0 = every body of the reference lattice (89 600)")
    ap.add_argument("--legs", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=30, help="untimed calls first: the GPU needs ~50 ms of load to reach its steady clocks")
    ap.add_argument("--tables", nargs="+", default=["bodies", "sweep"])
    ap.add_argument("--orders", nargs="+", default=["morton", "raster"])
    ap.add_argument("--max-turn", type=float, default=0.4)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--footholds-limit", type=int, default=1_000_000)
    ap.add_argument("--torch-limit", type=int, default=200_000, help="tables above this take the brute force on a few row blocks only")
    ap.add_argument("--torch-rows", type=int, default=1024)
    ap.add_argument("--torch-blocks", type=int, default=4)
    args = ap.parse_args()
    import torch
    import lrm_amd
    from lrm_amd import workloads
    assert torch.cuda.is_available(), "bench_pose_edges.py needs a GPU"
    t = dict(np.load(os.path.join(ROOT, "tests", "golden", "terrain_ground.npz")))
    ground = np.ascontiguousarray(t["ground"], np.float32)
    bodies = np.ascontiguousarray(t["bodies"], np.float32)
    if args.bodies:
        bodies = bodies[:args.bodies]
    ground = ground[lrm_amd.morton_order(ground)]
    ground_t = torch.from_numpy(np.ascontiguousarray(ground.T)).cuda()
    legs = workloads.hexapod(lrm_amd.get_M2_leg, args.legs)
    nl = len(legs)
    az = 2 * np.pi * np.arange(nl) / nl
    nominal = np.column_stack([260.0 * np.cos(az), 260.0 * np.sin(az), np.full(nl, -160.0)]).astype(np.float32)
    sweep = np.asarray(workloads.reference_sweep_quats(), np.float32)
    step = float(np.nextafter(np.float32(50.0 * 2 ** 0.5), np.float32(np.inf)))
    for name in args.tables:
        edges = set()
        for order in args.orders:
            bd = bodies[lrm_amd.morton_order(bodies)] if order == "morton" else bodies
            if name == "bodies":
                q, b, turn = np.ascontiguousarray(np.tile(sweep[:1], (len(bd), 1))), np.ascontiguousarray(bd), None
            else:
                q, b, turn = np.ascontiguousarray(np.tile(sweep, (len(bd), 1))), np.ascontiguousarray(np.repeat(bd, len(sweep), axis=0)), args.max_turn
            host = None
            if name == "bodies" and order == "morton" and not args.no_host:
                host = lrm_amd.pose_edges_cpu(q, b, step, lrm_amd.pose_edges_min_dot(turn))
            res = measure(args, torch, lrm_amd, name, order, q, b, step, turn, ground_t, legs, nominal, host)
            edges.add(res["edges"])
            print(json.dumps(res), flush=True)
        assert len(edges) == 1, f"{name}: the orders disagree on the number of edges: {edges}"


if __name__ == "__main__":
    main()
