#!/usr/bin/env python3
"""Joint angles per (target, pose, leg) (PoseSet(ik=True): lrm_pose_ik_compile_dev + lrm_ik_posed_dev), timed with HIP events
after warm-up (median of --reps):
  (a) one pose:     1e7 config-2 points, PoseSet.ik against lrm_ik_dev on the same cloud; next to it the same pair for
                    reach / distance (PoseSet.reach_dist against lrm_reach_dist_dev, LRM_MODE_STRICT), re-measured here
  (b) pair-major:   4096 poses x 6 moonbot legs x 64 targets
  (c) footholds:    100 000 bodies x 6 M2 legs in lrm_footholds_dev's [l*nb + b] order with target_idx = best: update() +
                    one PoseSet.ik launch, against the per-leg loop a caller writes today (gather the chosen targets with
                    torch, subtract the bodies, lrm_ik_dev), both end to end on one stream
One JSON line.

    python legged-robot-movability-cuda_amd/tools/bench_ik_posed.py [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def unit_quats(n, rng):
    q = rng.standard_normal((n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def timed(torch, fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--bodies", type=int, default=100_000)
    args = ap.parse_args()
    import torch
    import lrm_amd as lrm
    from lrm_amd import workloads
    rng = np.random.default_rng(42)
    out = {"tool": "bench_ik_posed", "device": torch.cuda.get_device_name(0)}
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    # (a) one pose against the single-pose calls
    n = args.n
    pts = workloads.random_cloud(n, seed=42)
    t = cu(pts.T)
    x, y, z = t[0], t[1], t[2]
    leg = lrm.get_M2_leg(0.0)
    q = np.array([1, 0, 0, 0], np.float32)
    ps = lrm.PoseSet([leg], 1, ik=True).update(cu(q[None]))
    ang, st = torch.empty((3, n), dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    ang2, st2 = torch.empty_like(ang), torch.empty_like(st)
    tip, mask, valid = torch.empty_like(ang), torch.empty_like(st), torch.empty_like(st)
    ms_single = timed(torch, lambda: lrm.device.ik(x, y, z, leg, q, out=ang2, status=st2), args.reps)
    ms_posed = timed(torch, lambda: ps.ik(x, y, z, out=ang, status=st, check=False), args.reps)
    ms_fk_single = timed(torch, lambda: lrm.device.fk(ang[0], ang[1], ang[2], leg, q, out=tip), args.reps)
    ms_fk_posed = timed(torch, lambda: ps.fk(ang[0], ang[1], ang[2], out=tip, check=False), args.reps)
    ms_rd_posed = timed(torch, lambda: ps.reach_dist(x, y, z, mask=mask, out=tip, valid=valid, check=False), args.reps)
    lrm.set_mode(lrm.MODE_STRICT)
    try:
        ms_rd_single = timed(torch, lambda: lrm.device.reach_dist(x, y, z, leg, q, mask=mask, out=tip), args.reps)
    finally:
        lrm.set_mode(lrm.MODE_FAST)
    torch.cuda.synchronize()
    same = bool(torch.equal(st, st2) and torch.equal(ang.view(torch.int32), ang2.view(torch.int32)))
    out["a_one_pose"] = dict(queries=n, ms_ik_posed=ms_posed, ms_ik_dev=ms_single, ik_ratio=ms_posed / ms_single,
                             ms_fk_posed=ms_fk_posed, ms_fk_dev=ms_fk_single, ms_reach_dist_posed=ms_rd_posed,
                             ms_reach_dist_dev_strict=ms_rd_single, reach_dist_ratio=ms_rd_posed / ms_rd_single,
                             ns_per_query=ms_posed * 1e6 / n, identical_to_single_pose=same)
    del x, y, z, t, ang, st, ang2, st2, tip, mask, valid, ps

    # (b) pair-major
    B, K = 4096, 64
    legs = workloads.hexapod(lrm.get_moonbot_leg).astype(np.float32)
    L = len(legs)
    quats = unit_quats(B, rng)
    body = (rng.random((B, 3), dtype=np.float32) * 8000 - 4000).astype(np.float32)
    pose = np.repeat(np.arange(B, dtype=np.int32), L * K)
    legi = np.tile(np.repeat(np.arange(L, dtype=np.uint8), K), B)
    off = rng.random((len(pose), 3), dtype=np.float32) * np.array([900, 900, 600], np.float32) - np.array([450, 450, 400], np.float32)
    t = cu((off + body[pose]).T.astype(np.float32))
    qt, bt, pi, li = cu(quats), cu(body), cu(pose), cu(legi)
    ps = lrm.PoseSet(legs, B, ik=True).update(qt, bt)
    nq = len(pose)
    ang, st = torch.empty((3, nq), dtype=torch.float32, device="cuda"), torch.empty(nq, dtype=torch.uint8, device="cuda")
    ms_update = timed(torch, lambda: ps.update(qt, bt), args.reps)
    ms_b = timed(torch, lambda: ps.ik(t[0], t[1], t[2], pi, li, out=ang, status=st, check=False), args.reps)
    out["b_pair_major"] = dict(poses=B, legs=L, targets_per_pair=K, queries=nq, ms=ms_b, ns_per_query=ms_b * 1e6 / nq,
                               ms_update_both_tables=ms_update,
                               per_query_over_a=(ms_b / nq) / (out["a_one_pose"]["ms_ik_posed"] / n))
    del t, qt, bt, pi, li, ang, st, ps

    # (c) the foothold pipeline's last step
    nb, L = args.bodies, 6
    ground = workloads.terrain(316)
    bodies = workloads.body_lattice(ground, nb)
    nb = len(bodies)
    legs = workloads.hexapod(lrm.get_M2_leg, L).astype(np.float32)
    tb, tt = cu(bodies.T), cu(ground.T)
    _, best, _ = lrm.device.footholds(tb[0], tb[1], tb[2], tt[0], tt[1], tt[2], legs)
    qt = cu(np.tile(np.array([1, 0, 0, 0], np.float32), (nb, 1)))
    bt = cu(bodies)
    ps = lrm.PoseSet(legs, nb, ik=True)
    pi, li = lrm.device.footholds_layout(nb, L, "cuda")
    nq = nb * L
    ang, st = torch.empty((3, nq), dtype=torch.float32, device="cuda"), torch.empty(nq, dtype=torch.uint8, device="cuda")
    ang2, st2 = torch.empty_like(ang), torch.empty_like(st)
    flat = best.view(-1)

    def one_launch():
        ps.update(qt, bt)
        ps.ik(tt[0], tt[1], tt[2], pi, li, target_idx=flat, out=ang, status=st, check=False)

    nan = torch.full((3, 1), float("nan"), device="cuda")

    def per_leg_loop():  # what a caller does today: per leg gather, subtract, lrm_ik_dev; -1 entries become nan points
        for l in range(L):
            b = best[l].long()
            p = torch.where((b >= 0)[None], tt[:, b.clamp(min=0)] - tb, nan).contiguous()
            lrm.device.ik(p[0], p[1], p[2], legs[l], out=ang2[:, l * nb:(l + 1) * nb], status=st2[l * nb:(l + 1) * nb])

    ms_one = timed(torch, one_launch, args.reps)
    ms_ik_only = timed(torch, lambda: ps.ik(tt[0], tt[1], tt[2], pi, li, target_idx=flat, out=ang, status=st, check=False), args.reps)
    ms_loop = timed(torch, per_leg_loop, args.reps)
    torch.cuda.synchronize()
    same = bool(torch.equal(st, st2) and torch.equal(torch.nan_to_num(ang).view(torch.int32), torch.nan_to_num(ang2).view(torch.int32)))
    out["c_footholds"] = dict(bodies=nb, legs=L, queries=nq, chosen=int((flat >= 0).sum()), ms_update_plus_ik=ms_one,
                              ms_ik_only=ms_ik_only, ns_per_query_ik_only=ms_ik_only * 1e6 / nq, ms_per_leg_loop=ms_loop,
                              speedup_vs_loop=ms_loop / ms_one, identical_to_loop=same,
                              status_counts=np.bincount(st.cpu().numpy(), minlength=5).tolist())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
