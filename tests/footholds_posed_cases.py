"""Shared cases of the posed foothold tests (tests/test_footholds_posed_cpu.py, tests/test_gpu_footholds_posed.py):
pose tables whose bodies each have their own quaternion, and a brute force that skips nothing, built on the oracle's
reachability_global per (pose, leg) on target - body[pose] with count / argmin / d2 in numpy float32 (no contraction,
first occurrence of the minimum among the reachable targets).  nominal_w comes from the host table, whose layout
include/lrm.h documents: float32[nposes, nlegs, 8] = {cull_center[3], cull_r2, nominal_w[3], pad}."""
import numpy as np

import pair_cases as pc
import posed_cases

MAX_TRIPLES = 2e8  # per oracle brute force: the CPU side stays in seconds


def pose_quats(lrm, n, seed=5):
    """n quaternions: identity first, then fixture quats (unit and not), sweep quats and random unit quats
    (posed_cases.pose_table); every seventh from index 3 on is scaled to |q| in 0.5-2, index 4 (and every 23rd after it)
    holds a nan.  So the first five already are: identity, two fixture quats, a non-unit one, a nan one."""
    rng = np.random.default_rng(seed + 100)
    qs = posed_cases.pose_table(lrm, max(n, 8), seed)[0][:n].copy()
    for i in range(3, n, 7):
        s = rng.uniform(0.5, 0.9) if rng.random() < 0.5 else rng.uniform(1.15, 2.0)
        qs[i] = (qs[i].astype(np.float64) / np.linalg.norm(qs[i].astype(np.float64)) * s).astype(np.float32)
    for i in range(4, n, 23):
        qs[i, (i // 23) % 4] = np.nan
    return np.ascontiguousarray(qs, np.float32)


def sweep_pose_quats(lrm, n, seed=7):
    """one of the reference's 45 sweep orientations per pose, drawn at random"""
    from lrm_amd import workloads
    sweep = np.asarray(workloads.reference_sweep_quats(), np.float32)
    return np.ascontiguousarray(sweep[np.random.default_rng(seed).integers(0, len(sweep), n)])


def nominal_w_of(lrm, quats, legs, nominal):
    """[nposes, nlegs, 3] from the host table"""
    return lrm.dbg_pose_footholds_compile_host(quats, legs, nominal)[:, :, 4:7].copy()


def brute(oracle, targets, quats, body, legs, nominal_w, poses=None):
    """-> dict(count, best int32[L, P'], best_d2 float32[L, P'], all_legs uint8[P']) over the poses listed (all by
    default) from the oracle alone; nominal_w [P, L, 3] as the table holds it"""
    targets = np.ascontiguousarray(targets, np.float32).reshape(-1, 3)
    legs = np.ascontiguousarray(legs, np.float32).reshape(-1, 14)
    poses = np.arange(len(quats)) if poses is None else np.asarray(poses)
    nl, npz, nt = len(legs), len(poses), len(targets)
    assert nl * npz * nt <= MAX_TRIPLES, "brute force too large"
    count = np.zeros((nl, npz), np.int32)
    best = np.full((nl, npz), -1, np.int32)
    best_d2 = np.full((nl, npz), np.inf, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k, p in enumerate(poses):
            rel = (targets - body[p]).astype(np.float32)  # one f32 subtraction per component
            for l in range(nl):
                r = oracle.reach(rel, legs[l], quats[p]).astype(bool) if nt else np.zeros(0, bool)
                count[l, k] = r.sum()
                if not count[l, k]:
                    continue
                c = (body[p] + nominal_w[p, l]).astype(np.float32)  # one f32 add per component
                d = (targets - c).astype(np.float32)
                d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                masked = np.where(r, d2, np.float32(np.inf))
                mn = masked.min()
                best[l, k] = int(np.argmax(r & (masked == mn)))  # first reachable target at the minimum
                best_d2[l, k] = mn
    return {"count": count, "best": best, "best_d2": best_d2, "all_legs": (count > 0).all(0).astype(np.uint8)}


def scene(lrm, nposes, nt, seed, kind="rough"):
    """(quats, body, targets): bodies hovering over a cloud of pair_cases, each with its own quaternion"""
    if kind == "rough":
        body, targets = pc.rough(nposes, nt, seed, sort_x=True)
    elif kind == "dense_cluster":
        body, targets = pc.dense_cluster(nposes, nt, seed)
        body[4::5, 2] += np.float32(2000.0)
    elif kind == "sparse_tiles":
        body, targets = pc.sparse_tiles(nposes, max(1, nt // 1024), seed)
        body[4::5, 2] += np.float32(900.0)
    else:
        raise ValueError(kind)
    return pose_quats(lrm, nposes, seed), np.ascontiguousarray(body, np.float32), np.ascontiguousarray(targets, np.float32)


def assert_same(got, want):
    """got: (count, best, best_d2, all_legs) arrays (best_d2 / all_legs may be None); want: brute()'s or the host loop's"""
    count, best, best_d2, all_legs = got
    assert np.array_equal(count, want["count"])
    assert np.array_equal(best, want["best"])
    if best_d2 is not None:
        assert np.array_equal(pc.bits(best_d2), pc.bits(want["best_d2"]))
    if all_legs is not None:
        assert np.array_equal(all_legs, want["all_legs"])


def host(lrm, targets, quats, body, legs, nominal):
    count, best, best_d2, all_legs, _ = lrm.footholds_posed_cpu(targets, quats, body, legs, nominal)
    return {"count": count, "best": best, "best_d2": best_d2, "all_legs": all_legs}
