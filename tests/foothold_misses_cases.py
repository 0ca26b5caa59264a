"""Shared cases of the nearest-miss foothold tests (tests/test_foothold_misses_cpu.py, tests/test_gpu_foothold_misses.py):
pose tables in which many bodies are raised or pushed sideways off the terrain by a fraction of the leg length, so that
their legs reach nothing but come close, and a brute force that skips nothing, built from the oracle alone: the oracle's
reachability_global mask and distance_global vector per (pose, leg) on target - body[pose], with the candidate rule and m2
of include/lrm.h restated in numpy float32 (no contraction, first occurrence of the minimum).  The spheres come from the
host table, whose layout include/lrm.h documents: float32[nposes, nlegs, 8] = {cull_center[3], cull_r2, ...}."""
import numpy as np

import footholds_posed_cases as fc
import pair_cases as pc

MAX_TRIPLES = fc.MAX_TRIPLES
MARGINS = (0.0, 25.0, 400.0, np.inf)


def displaced(body, seed, reach=500.0):
    """poses 1, 4, 7, .. raised by 0.25-0.7 of `reach`, poses 2, 5, 8, .. pushed sideways by 0.5-1.6 of it (any
    horizontal direction); poses 0, 3, 6, .. stay (of which the scene lifts some out of every leg's reach already)"""
    rng = np.random.default_rng(seed + 700)
    body = body.astype(np.float64).copy()
    n = len(body)
    up = np.arange(n) % 3 == 1
    side = np.arange(n) % 3 == 2
    body[up, 2] += rng.uniform(0.25, 0.7, up.sum()) * reach
    ang, rad = rng.uniform(0, 2 * np.pi, side.sum()), rng.uniform(0.5, 1.6, side.sum()) * reach
    body[side, 0] += rad * np.cos(ang)
    body[side, 1] += rad * np.sin(ang)
    return np.ascontiguousarray(body, np.float32)


def scene(lrm, nposes, nt, seed, kind="rough"):
    """(quats, body, targets): footholds_posed_cases.scene with two thirds of the bodies displaced"""
    quats, body, targets = fc.scene(lrm, nposes, nt, seed, kind)
    return quats, displaced(body, seed, 500.0 if kind == "rough" else 250.0), targets


def spheres_of(lrm, quats, legs):
    """[nposes, nlegs, 4] = cull_center[3], cull_r2 from the host table"""
    return lrm.dbg_pose_footholds_compile_host(quats, legs, None)[:, :, 0:4].copy()


def rm2_of(cull_r2, margin):
    with np.errstate(over="ignore", invalid="ignore"):
        rm = np.float32(np.sqrt(np.float32(cull_r2)) + np.float32(margin))
        return np.float32(rm * rm)


def brute(oracle, targets, quats, body, legs, spheres, margin, count_in=None):
    """-> dict(miss int32[L, P], m2 float32[L, P], shift float32[3, L, P], near int32[L, P]) from the oracle alone"""
    targets = np.ascontiguousarray(targets, np.float32).reshape(-1, 3)
    legs = np.ascontiguousarray(legs, np.float32).reshape(-1, 14)
    nl, npz, nt = len(legs), len(quats), len(targets)
    assert nl * npz * nt <= MAX_TRIPLES, "brute force too large"
    miss = np.full((nl, npz), -1, np.int32)
    m2 = np.full((nl, npz), np.inf, np.float32)
    shift = np.full((3, nl, npz), np.nan, np.float32)
    near = np.zeros((nl, npz), np.int32)
    cin = None if count_in is None else np.asarray(count_in).reshape(nl, npz)
    with np.errstate(over="ignore", invalid="ignore"):
        for p in range(npz):
            q = (targets - body[p]).astype(np.float32)  # one f32 subtraction per component
            for l in range(nl):
                if cin is not None and cin[l, p] > 0:
                    continue
                e = (q - spheres[p, l, :3]).astype(np.float32)  # one f32 subtraction per component
                e2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
                cand = np.nonzero(e2 <= rm2_of(spheres[p, l, 3], margin))[0]  # false for a nan e2
                if not len(cand):
                    continue
                idx = cand[oracle.reach(q[cand], legs[l], quats[p]) == 0]
                near[l, p] = len(idx)
                if not len(idx):
                    continue
                d, _ = oracle.dist(q[idx], legs[l], quats[p])
                v = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                ok = v < np.float32(np.inf)  # false for nan
                if not ok.any():
                    continue
                mn = v[ok].min()
                k = int(np.argmax(ok & (v == mn)))  # the first eligible miss at the minimum
                miss[l, p], m2[l, p], shift[:, l, p] = idx[k], mn, d[k]
    return {"miss": miss, "m2": m2, "shift": shift, "near": near}


def host(lrm, targets, quats, body, legs, margin, count_in=None):
    miss, m2, shift, near, _ = lrm.foothold_misses_posed_cpu(targets, quats, body, legs, margin, count_in)
    return {"miss": miss, "m2": m2, "shift": shift, "near": near}


def assert_same(got, want):
    """got: (miss, m2, shift, near) arrays (m2 / shift / near may be None); want: brute()'s or the host loop's"""
    miss, m2, shift, near = got
    assert np.array_equal(miss, want["miss"])
    if m2 is not None:
        assert np.array_equal(pc.bits(m2), pc.bits(want["m2"]))
    if shift is not None:
        assert np.array_equal(pc.bits(shift), pc.bits(want["shift"]))
    if near is not None:
        assert np.array_equal(near, want["near"])
    empty = want["miss"] < 0
    assert np.isposinf(want["m2"][empty]).all() and (pc.bits(want["shift"][:, empty]) == 0x7FC00000).all()
    assert np.isfinite(want["m2"][~empty]).all() and np.isfinite(want["shift"][:, ~empty]).all()


def count_forms(count):
    """the count_in forms of the issue from footholds_posed's counts [L, P]: NULL, all zero, the counts, and the counts with
    negative entries (which are not skipped) in place of some zeros and some positives"""
    neg = count.copy()
    neg.reshape(-1)[::3] = -1 - neg.reshape(-1)[::3]
    return {"null": None, "zero": np.zeros_like(count), "counts": count, "negative": neg}


def assert_not_vacuous(count, want, share=0.25):
    """by the oracle alone (count: footholds_posed_cases.brute's; want: brute() without count_in): at least `share` of the
    (pose, leg) entries are footless with a miss, some are footless with no candidate at all, some have a foothold"""
    footless = count == 0
    with_miss = footless & (want["near"] > 0)
    assert with_miss.mean() >= share, float(with_miss.mean())
    assert (footless & (want["near"] == 0)).any() and (~footless).any()
    assert (want["miss"][with_miss] >= 0).mean() > 0.8  # the rest: nan quaternions, whose misses are not eligible
