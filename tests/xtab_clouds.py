"""Clouds for the bit-exact table-guided value chain (csrc/lrm_point_xtab.h), built in the coxa frame of the M2 leg (azimuth 0,
body upright) and mapped back to the body frame, so that the lanes the chain treats specially are there ON PURPOSE:

  twin      an INVALID point in front of the coxa with |yaw| < 0.5 rad: beyond the outer reach of its meridian plane, by
            0.5 .. 15 mm (a short vector: LRM_MODE_TOL_REL replays it) or by 20 .. 300 mm.  The flipped yaw candidate is
            mega-saturated onto the direct one (the flipped yaw lies beyond min_coxa - pi/2 or max_coxa + pi/2, i.e.
            |yaw| < pi/6 for this leg): two value chains that differ by rounding, picked by strict norms.  (For one yaw
            in six the flipped-twice yaw is the yaw itself, bit for bit: no twin.)
  alt       a VALID point whose yaw-limit plane is nearer than the boundary of its meridian plane (half as far): the
            yaw-limit alternative is taken (one_leg.cu:258-274).
  near      the same with the two distances equal up to a few 1e-6: the strict norms decide.
  clamped   a valid point up to 0.3 rad beyond a yaw limit: the candidate is clamped to the limit (th = -0).
  cube      points of the config-2 cube.

interleaved(n) deals the classes out lane by lane (period 8: three twins, two alt, one each of the others), so that every wave
of 64 consecutive points holds all of them.  The in-plane distance D of a meridian point comes from the strict host code
(lrm_dist_cpu at yaw 0, where no yaw limit is near); the outer reach of a meridian from a bisection on lrm_reach_cpu."""
import numpy as np

BODY, PITCH, COXA = 181.0, -0.7853982, 65.5
MAX_YAW, MIN_YAW = 1.0471976, -1.0471976
CLASSES = ("twin", "alt", "near", "clamped", "cube")
PATTERN = ("twin", "alt", "near", "twin", "clamped", "alt", "cube", "twin")


def to_body(r, yaw, zc):
    """coxa-frame cylinder coordinates (radius about the coxa axis, yaw, height) -> body-frame points (n, 3) float32"""
    xc, yc = r * np.cos(yaw), r * np.sin(yaw)
    phi = -PITCH  # place_over_coxa rotates (x - body, z) by -pitch (lrm_compile_head.h); this is its inverse
    x = xc * np.cos(phi) + zc * np.sin(phi) + BODY
    z = -xc * np.sin(phi) + zc * np.cos(phi)
    return np.stack([x, yc, z], axis=1).astype(np.float32)


def meridian_samples(lrm, leg, count, seed):
    """(r, zc, D, r_out): reachable meridian points with in-plane boundary distance D in [0.4, 12] mm, and the outer reach of
    their height zc (the first unreachable radius beyond them, to 1e-3 mm)"""
    rng = np.random.default_rng(seed)
    r = rng.uniform(COXA + 20.0, COXA + 260.0, 40 * count)
    zc = rng.uniform(-180.0, 120.0, 40 * count)
    p = to_body(r, np.zeros_like(r), zc)
    m, _ = lrm.apply_reach_cpu(p, leg)
    d, v, _ = lrm.apply_dist_cpu(p, leg)
    D = np.linalg.norm(d.astype(np.float64), axis=1)
    keep = np.flatnonzero((m != 0) & (v != 0) & (D > 0.4) & (D < 12.0))[:count]
    assert len(keep) == count, "not enough reachable meridian points"
    r, zc, D = r[keep], zc[keep], D[keep]
    lo, hi = r.copy(), np.full_like(r, COXA + 600.0)
    for _ in range(24):
        mid = 0.5 * (lo + hi)
        ok = lrm.apply_reach_cpu(to_body(mid, np.zeros_like(mid), zc), leg)[0] != 0
        lo, hi = np.where(ok, mid, lo), np.where(ok, hi, mid)
    return r, zc, D, hi


def class_points(lrm, leg, name, count, seed):
    rng = np.random.default_rng(seed + 1000)
    if name == "cube":
        lo, hi = np.array([-200, -500, -500], np.float32), np.array([700, 500, 300], np.float32)
        return (rng.random((count, 3), dtype=np.float32) * (hi - lo) + lo).astype(np.float32)
    r, zc, D, r_out = meridian_samples(lrm, leg, count, seed)
    side = rng.integers(0, 2, count) * 2 - 1  # which yaw limit
    limit = np.where(side > 0, MAX_YAW, MIN_YAW)
    if name == "twin":
        beyond = np.where(rng.random(count) < 0.5, rng.uniform(0.5, 15.0, count), rng.uniform(20.0, 300.0, count))
        return to_body(r_out + beyond, rng.uniform(-0.5, 0.5, count), zc)
    if name == "alt":
        return to_body(r, limit - side * np.arcsin(0.5 * D / r), zc)
    if name == "near":
        return to_body(r, limit - side * np.arcsin(D * (1.0 + rng.integers(-4, 5, count) * 1.0e-6) / r), zc)
    if name == "clamped":
        return to_body(r, limit + side * rng.uniform(0.001, 0.3, count), zc)
    raise ValueError(name)


def interleaved(lrm, leg, n, seed=42):
    """n points, class of point i = PATTERN[i % 8] -> (points, class index per point into CLASSES)"""
    which = np.array([CLASSES.index(PATTERN[i % len(PATTERN)]) for i in range(n)])
    pts = np.empty((n, 3), np.float32)
    for k, name in enumerate(CLASSES):
        idx = np.flatnonzero(which == k)
        pts[idx] = class_points(lrm, leg, name, len(idx), seed + k)
    return pts, which
