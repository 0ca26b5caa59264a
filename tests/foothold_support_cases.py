"""Shared cases of the per-target foothold support tests (tests/test_foothold_support_cpu.py,
tests/test_gpu_foothold_support.py): the scenes of footholds_posed_cases with some poses duplicated (exact d2 ties between
two poses), and a brute force that skips nothing, built from the oracle alone: the oracle's reachability_global mask per
(pose, leg) on target - body[pose] in float32, d2 and its order in numpy float32 (no contraction), the first pose at the
minimum.  nominal_w comes from the host table, whose layout include/lrm.h documents."""
import numpy as np

import footholds_posed_cases as fc
import pair_cases as pc

MAX_TRIPLES = fc.MAX_TRIPLES


def scene(lrm, nposes, nt, seed, kind="rough", dup=0):
    """(quats, body, targets): footholds_posed_cases.scene; the last `dup` poses are copies of poses 0, 2, 4, ..: every
    copy ties with its original on every d2, and the original (the smaller index) must win"""
    quats, body, targets = fc.scene(lrm, nposes, nt, seed, kind)
    if dup:
        src = dup_pairs(nposes, dup)[0]
        quats[nposes - dup:] = quats[src]
        body[nposes - dup:] = body[src]
    return quats, body, targets


def brute(oracle, targets, quats, body, legs, nominal_w, pose_live=None):
    """-> dict(count, best_pose int32[L, T], best_d2 float32[L, T], legs_mask uint8[T]) from the oracle alone; nominal_w
    [P, L, 3] as the table holds it; pose_live None or [P], 0 = the pose does not count"""
    targets = np.ascontiguousarray(targets, np.float32).reshape(-1, 3)
    legs = np.ascontiguousarray(legs, np.float32).reshape(-1, 14)
    nl, npz, nt = len(legs), len(quats), len(targets)
    assert nl * npz * nt <= MAX_TRIPLES, "brute force too large"
    count = np.zeros((nl, nt), np.int32)
    best = np.full((nl, nt), -1, np.int32)
    best_d2 = np.full((nl, nt), np.inf, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for p in range(npz):  # ascending: a later pose wins only when strictly nearer
            if pose_live is not None and not pose_live[p]:
                continue
            rel = (targets - body[p]).astype(np.float32)  # one f32 subtraction per component
            for l in range(nl):
                r = oracle.reach(rel, legs[l], quats[p]).astype(bool) if nt else np.zeros(0, bool)
                if not r.any():
                    continue
                c = (body[p] + nominal_w[p, l]).astype(np.float32)  # one f32 add per component
                d = (targets - c).astype(np.float32)
                d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                take = r & ((count[l] == 0) | (d2 < best_d2[l]))
                best[l][take] = p
                best_d2[l][take] = d2[take]
                count[l] += r
    mask = np.zeros(nt, np.uint8)
    for l in range(nl):
        mask |= ((count[l] > 0).astype(np.uint8) << l).astype(np.uint8)
    return {"count": count, "best_pose": best, "best_d2": best_d2, "legs_mask": mask}


def host(lrm, targets, quats, body, legs, nominal=None, pose_live=None):
    count, best, best_d2, mask, _ = lrm.foothold_support_posed_cpu(targets, quats, body, legs, nominal, pose_live)
    return {"count": count, "best_pose": best, "best_d2": best_d2, "legs_mask": mask}


def assert_same(got, want):
    """got: (count, best_pose, best_d2, legs_mask) arrays (best_d2 / legs_mask may be None); want: brute()'s or the host loop's"""
    count, best, best_d2, mask = got
    assert np.array_equal(count, want["count"])
    assert np.array_equal(best, want["best_pose"])
    if best_d2 is not None:
        assert np.array_equal(pc.bits(best_d2), pc.bits(want["best_d2"]))
    if mask is not None:
        assert np.array_equal(mask, want["legs_mask"])
    empty = want["count"] == 0
    assert (want["best_pose"][empty] == -1).all() and np.isposinf(want["best_d2"][empty]).all()
    assert (want["best_pose"][~empty] >= 0).all()


def live_forms(lrm, targets, quats, body, legs, nominal=None):
    """the four pose_live forms of the issue: NULL, all 1, all 0, and all_legs of lrm_footholds_posed_cpu"""
    n = len(quats)
    all_legs = lrm.footholds_posed_cpu(targets, quats, body, legs, nominal)[3]
    return {"null": None, "ones": np.ones(n, np.uint8), "zeros": np.zeros(n, np.uint8), "all_legs": all_legs}


def dup_pairs(nposes, dup):
    """(originals, copies) of scene(..., dup=dup)"""
    return (2 * np.arange(dup)) % (nposes - dup), np.arange(nposes - dup, nposes)


def assert_not_vacuous(want, nposes, dup, share=0.25):
    """by the oracle alone (want: brute() with every pose live): at least `share` of the (target, leg) entries have a
    choice between two or more poses, some have none and some exactly one, and some winners are poses with a copy --
    an exact d2 tie between two reaching poses -- of which the brute force kept the smaller index: no copy ever wins"""
    c = want["count"]
    assert (c >= 2).mean() >= share, float((c >= 2).mean())
    assert (c == 0).any() and (c == 1).any()
    src, copies = dup_pairs(nposes, dup)
    assert np.isin(want["best_pose"], src).sum() > 10 and not np.isin(want["best_pose"], copies).any()
