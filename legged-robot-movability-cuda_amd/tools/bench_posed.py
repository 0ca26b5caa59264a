#!/usr/bin/env python3
"""Batched multi-pose queries (PoseSet: lrm_pose_compile_dev + lrm_reach_dist_posed_dev), fused reach + distance, timed with
HIP events after warm-up (median of --reps launches):
  (a) pair-major:   4096 poses x 6 moonbot legs x 64 targets, [pose, leg, target]; also the per-(pose, leg) loop over
                    device.reach_dist (LRM_MODE_STRICT) on the same queries
  (b) interleaved:  B = 1.6e6 poses x 6 legs, one target per (pose, leg), leg fastest
  (c) one pose:     1e7 queries, against lrm_reach_dist_dev in LRM_MODE_STRICT on the same cloud
One JSON line.

    python legged-robot-movability-cuda_amd/tools/bench_posed.py [--reps 20] [--loop-reps 2]
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--loop-reps", type=int, default=2)
    args = ap.parse_args()
    import torch
    import lrm_amd as lrm
    from lrm_amd import workloads
    rng = np.random.default_rng(42)
    legs = workloads.hexapod(lrm.get_moonbot_leg).astype(np.float32)
    L = len(legs)
    out = {"tool": "bench_posed", "device": torch.cuda.get_device_name(0)}

    def cloud(n, body_of_query):
        off = rng.random((n, 3), dtype=np.float32) * np.array([900, 900, 600], np.float32) - np.array([450, 450, 400], np.float32)
        return torch.from_numpy(np.ascontiguousarray((off + body_of_query).T.astype(np.float32))).cuda()

    # (a) pair-major
    B, K = 4096, 64
    quats = unit_quats(B, rng)
    body = (rng.random((B, 3), dtype=np.float32) * 8000 - 4000).astype(np.float32)
    pose = np.repeat(np.arange(B, dtype=np.int32), L * K)
    leg = np.tile(np.repeat(np.arange(L, dtype=np.uint8), K), B)
    t = cloud(len(pose), body[pose])
    x, y, z = t[0], t[1], t[2]
    pi, li = torch.from_numpy(pose).cuda(), torch.from_numpy(leg).cuda()
    qt, bt = torch.from_numpy(quats).cuda(), torch.from_numpy(body).cuda()
    ps = lrm.PoseSet(legs, B)
    ps.update(qt, bt)
    n_a = len(pose)
    mask = torch.empty(n_a, dtype=torch.uint8, device="cuda")
    valid = torch.empty(n_a, dtype=torch.uint8, device="cuda")
    field = torch.empty((3, n_a), dtype=torch.float32, device="cuda")
    ms_update = timed(torch, lambda: ps.update(qt, bt), args.reps)
    ms_a = timed(torch, lambda: ps.reach_dist(x, y, z, pi, li, mask=mask, out=field, valid=valid, check=False), args.reps)
    # the per-(pose, leg) loop: one single-pose call per pair on its 64 targets (p = target - body on the device first)
    p = torch.stack([x, y, z]) - bt.T[:, torch.from_numpy(pose).cuda().long()]
    p = p.contiguous()
    lrm.set_mode(lrm.MODE_STRICT)
    try:
        def loop():
            for b in range(B):
                for k in range(L):
                    s = (b * L + k) * K
                    lrm.device.reach_dist(p[0, s:s + K], p[1, s:s + K], p[2, s:s + K], legs[k], quats[b],
                                          mask=mask[s:s + K], out=field[:, s:s + K])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop()
        torch.cuda.synchronize()
        ms_loop_first = (time.perf_counter() - t0) * 1e3
        ms_loop = timed(torch, loop, args.loop_reps, warmup=0)
    finally:
        lrm.set_mode(lrm.MODE_FAST)
    out["a_pair_major"] = dict(poses=B, legs=L, targets_per_pair=K, queries=n_a, ms=ms_a, ns_per_query=ms_a * 1e6 / n_a,
                               ms_update=ms_update, ms_per_pair_loop=ms_loop, ms_per_pair_loop_first=ms_loop_first,
                               speedup_vs_loop=ms_loop / ms_a)
    del x, y, z, pi, li, t, p, mask, valid, field, ps

    # (b) interleaved, one target per (pose, leg)
    B = 1_600_000
    quats = unit_quats(B, rng)
    body = (rng.random((B, 3), dtype=np.float32) * 8000 - 4000).astype(np.float32)
    pose = np.repeat(np.arange(B, dtype=np.int32), L)
    leg = np.tile(np.arange(L, dtype=np.uint8), B)
    t = cloud(len(pose), body[pose])
    x, y, z = t[0], t[1], t[2]
    pi, li = torch.from_numpy(pose).cuda(), torch.from_numpy(leg).cuda()
    qt, bt = torch.from_numpy(quats).cuda(), torch.from_numpy(body).cuda()
    ps = lrm.PoseSet(legs, B)
    ps.update(qt, bt)
    n_b = len(pose)
    mask = torch.empty(n_b, dtype=torch.uint8, device="cuda")
    valid = torch.empty(n_b, dtype=torch.uint8, device="cuda")
    field = torch.empty((3, n_b), dtype=torch.float32, device="cuda")
    ms_update = timed(torch, lambda: ps.update(qt, bt), args.reps)
    ms_b = timed(torch, lambda: ps.reach_dist(x, y, z, pi, li, mask=mask, out=field, valid=valid, check=False), args.reps)
    out["b_interleaved"] = dict(poses=B, legs=L, queries=n_b, ms=ms_b, ns_per_query=ms_b * 1e6 / n_b, ms_update=ms_update,
                                workspace_mb=ps.workspace.numel() / 2**20)
    del x, y, z, pi, li, t, mask, valid, field, ps

    # (c) one pose, 1e7 queries, against the single-pose strict call
    n_c = 10_000_000
    pts = workloads.random_cloud(n_c, seed=42)
    t = torch.from_numpy(np.ascontiguousarray(pts.T)).cuda()
    x, y, z = t[0], t[1], t[2]
    q = np.array([0.97, 0.05, -0.2, 0.1], np.float32)
    ps = lrm.PoseSet(legs[:1], 1).update(torch.from_numpy(q[None]).cuda())
    mask = torch.empty(n_c, dtype=torch.uint8, device="cuda")
    valid = torch.empty(n_c, dtype=torch.uint8, device="cuda")
    field = torch.empty((3, n_c), dtype=torch.float32, device="cuda")
    mask2 = torch.empty(n_c, dtype=torch.uint8, device="cuda")
    field2 = torch.empty((3, n_c), dtype=torch.float32, device="cuda")
    ms_c = timed(torch, lambda: ps.reach_dist(x, y, z, mask=mask, out=field, valid=valid, check=False), args.reps)
    ms_c_noval = timed(torch, lambda: ps.reach_dist(x, y, z, mask=mask, out=field, valid=None, check=False), args.reps)
    lrm.set_mode(lrm.MODE_STRICT)
    try:
        ms_strict = timed(torch, lambda: lrm.device.reach_dist(x, y, z, legs[0], q, mask=mask2, out=field2), args.reps)
    finally:
        lrm.set_mode(lrm.MODE_FAST)
    torch.cuda.synchronize()
    same = bool(torch.equal(mask, mask2) and torch.equal(field.view(torch.int32), field2.view(torch.int32)))
    out["c_one_pose"] = dict(queries=n_c, ms=ms_c, ms_without_valid=ms_c_noval, ms_single_pose_strict=ms_strict,
                             ratio=ms_c / ms_strict, identical_to_single_pose=same)
    ns_c = ms_c * 1e6 / n_c
    out["targets"] = dict(c_over_strict=ms_c / ms_strict, a_over_c_per_query=out["a_pair_major"]["ns_per_query"] / ns_c,
                          b_over_c_per_query=out["b_interleaved"]["ns_per_query"] / ns_c,
                          a_speedup_vs_loop=out["a_pair_major"]["speedup_vs_loop"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
