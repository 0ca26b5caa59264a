#!/usr/bin/env python3
"""Joint angles (lrm_ik_dev) on 1e7 config-2 points (random_cloud, seed 42) with the M2 leg, one GPU, timed with HIP events
after warm-up (median of --reps launches), against the strict fused call (lrm_reach_dist_dev in LRM_MODE_STRICT) on the same
cloud; plus lrm_fk_dev, and the ns/point of the RBDL-equivalent LM IK on the CPU (lrm_rbdl_equiv_cpu, the reference's own
IK comparison, bench.cpp compute index 4) on a sample.  One JSON line.  Goal: ik_over_strict <= 2.

    python legged-robot-movability-cuda_amd/tools/bench_ik.py [--reps 20] [--n 10000000] [--rbdl-n 100000]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


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
    ap.add_argument("--rbdl-n", type=int, default=100_000)
    args = ap.parse_args()
    import torch
    import lrm_amd as lrm
    from lrm_amd import workloads
    n = args.n
    pts = workloads.random_cloud(n, seed=42)
    leg = lrm.get_M2_leg(0.0)
    t = torch.from_numpy(np.ascontiguousarray(pts.T)).cuda()
    x, y, z = t[0], t[1], t[2]
    ang = torch.empty((3, n), dtype=torch.float32, device="cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    tip = torch.empty((3, n), dtype=torch.float32, device="cuda")
    mask = torch.empty(n, dtype=torch.uint8, device="cuda")
    field = torch.empty((3, n), dtype=torch.float32, device="cuda")
    ms_ik = timed(torch, lambda: lrm.device.ik(x, y, z, leg, out=ang, status=st), args.reps)
    ms_fk = timed(torch, lambda: lrm.device.fk(ang[0], ang[1], ang[2], leg, out=tip), args.reps)
    prev = lrm.get_mode()
    lrm.set_mode(lrm.MODE_STRICT)
    try:
        ms_strict = timed(torch, lambda: lrm.device.reach_dist(x, y, z, leg, mask=mask, out=field), args.reps)
    finally:
        lrm.set_mode(prev)
    torch.cuda.synchronize()
    s = st.cpu().numpy()
    same_mask = bool(np.array_equal(np.isin(s, (1, 3)), mask.cpu().numpy().astype(bool)))
    nr = min(args.rbdl_n, n)
    _, ms_rbdl = lrm.apply_rbdl_equiv(pts[:nr], leg)
    out = {"tool": "bench_ik", "device": torch.cuda.get_device_name(0), "points": n, "leg": "M2 az 0, identity",
           "ms_ik_dev": ms_ik, "ms_reach_dist_dev_strict": ms_strict, "ik_over_strict": ms_ik / ms_strict,
           "ms_fk_dev": ms_fk, "ns_per_point_ik_dev": ms_ik * 1e6 / n,
           "ns_per_point_rbdl_equiv_cpu": ms_rbdl * 1e6 / nr, "rbdl_sample": nr,
           "status_counts": np.bincount(s, minlength=5).tolist(), "status_mask_equals_strict_reach": same_mask}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
