"""Threshold-shell clouds for LRM_MODE_TOL_REL: points whose distance vector is a chosen multiple of the kernel's replay
threshold.  numpy only; shared by tests/test_tol_shell_cpu.py, tests/test_gpu_tol_shell.py and tools/stress_tol.py.

LRM_MODE_TOL_REL replays every vector that comes out shorter than thr = max(LRM_TOL_REL_MM, LRM_TOL_REL_BANDS * band(p)) with the
reference's own operations; every longer one is as good as the FP32 arithmetic of lrm_tab_point, whose ABSOLUTE error is about
1e-4 mm whatever the vector's length.  The relative error is therefore worst just above thr, and a uniform cloud has only a few
per cent of its points there.  A shell puts most of a cloud there: from a seed point p with strict vector d0, b = p - d0 is the
nearest boundary point and u = d0 / |d0| the outward direction; the shell point is b + u * s with s = f * thr(b + u * s), f drawn
from [f_lo, f_hi], solved by three fixed-point rounds (thr moves by 3 % of the step).

thr() mirrors csrc/lrm_tol_kernels.hip (lrm_tol_rel_threshold) and csrc/lrm_compile.cpp (band_base, band_slope); its two headline
constants are read from csrc/lrm_launch.h, so a change of either moves the shells with it.  It is used to BUILD clouds and to
report figures next to it, never as the bound of an assertion about the kernel: those come from the oracle's vector alone."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "legged-robot-movability-cuda_amd", "csrc")

IDENTITY = (1.0, 0.0, 0.0, 0.0)
TILT_Y = (0.9848, 0.0, 0.1736, 0.0)   # the two tilted orientations of the golden fixtures
TILT_Z = (0.9397, 0.0, 0.0, 0.342)
FAMILIES = ("uni_shell", "grid_shell", "mix_shell", "axis_shell")
F_RANGE = {"uni_shell": (0.9, 1.6), "grid_shell": (0.9, 1.6), "mix_shell": (0.4, 1.6), "axis_shell": (0.9, 1.6)}
# conditions every case must meet, from the oracle alone: the share of points with thr <= |d_ref| < 2 thr, and for
# mix_shell also the share with 0 < |d_ref| < thr
MIN_IN_BAND = 0.30
MIN_SHORT_MIX = 0.30
BAND_SLOPE_UNITS = 1.7320508 + 1.5  # lrm_compile.cpp: S = fast_scale + (sqrt(3) + 1.5) (|p|_1 + body)


def constants():
    """(LRM_TOL_REL_MM, LRM_TOL_REL_BANDS, LRM_BAND) as the kernel sources define them"""
    launch = open(os.path.join(CSRC, "lrm_launch.h")).read()
    fast = open(os.path.join(CSRC, "lrm_point_fast.h")).read()
    mm = float(re.search(r"#define LRM_TOL_REL_MM\s+([0-9.eE+-]+)f", launch).group(1))
    bands = float(re.search(r"#define LRM_TOL_REL_BANDS\s+([0-9.eE+-]+)f", launch).group(1))
    band = float(re.search(r"#define LRM_BAND\s+([0-9.eE+-]+)f", fast).group(1))
    return mm, bands, band


def band_terms(lrm, leg, quat=None):
    """(band_base, band_slope) of lrm_compile_leg for (leg, quat): band(p) = band_base + band_slope * |p|_1 (mm)"""
    head = lrm.dbg_compile_leg_head(leg, quat)
    circles = head[:256].view(np.float32).reshape(16, 4).astype(np.float64)  # LrmCompiledLeg::lists: {x, y, r, attract}
    fast_scale = float(np.float32((np.abs(circles[:, 0]) + np.abs(circles[:, 1]) + circles[:, 2]).max()))
    k = float(np.float32(constants()[2]))
    body = abs(float(np.asarray(leg, np.float32).reshape(-1)[1]))
    return np.float32(k * (fast_scale + BAND_SLOPE_UNITS * body)), np.float32(k * BAND_SLOPE_UNITS)


def thr(points, terms):
    """the kernel's replay threshold (mm) at each point; terms = band_terms(lrm, leg, quat)"""
    mm, bands, _ = constants()
    p = np.abs(np.asarray(points, np.float32).reshape(-1, 3))
    l1 = (p[:, 0] + p[:, 1]) + p[:, 2]  # float32, in the kernel's order
    band = (l1.astype(np.float64) * float(terms[1]) + float(terms[0])).astype(np.float32)  # one rounding, as the FMA
    return np.maximum(np.float32(mm), np.float32(bands) * band)


def shell(seed_points, d0, terms, f_lo, f_hi, rng):
    """the shell of seed_points (float32 [n, 3]) whose strict vectors are d0; seeds with a zero or non-finite vector are dropped"""
    p = np.asarray(seed_points, np.float64).reshape(-1, 3)
    d0 = np.asarray(d0, np.float64).reshape(-1, 3)
    n0 = np.linalg.norm(d0, axis=1)
    keep = np.isfinite(d0).all(axis=1) & np.isfinite(n0) & (n0 > 0)
    p, d0, n0 = p[keep], d0[keep], n0[keep]
    b = p - d0
    u = d0 / n0[:, None]
    f = rng.uniform(f_lo, f_hi, len(p))
    s = f * thr(p, terms)
    for _ in range(3):
        s = f * thr(b + u * s[:, None], terms)
    return (b + u * s[:, None]).astype(np.float32)


def reach_of(leg):
    leg = np.asarray(leg, np.float64).reshape(-1)
    return float(leg[1] + leg[3] + leg[4] + leg[5])  # body + coxa + tibia + femur lengths


def rotate(q, v):
    """v (float64 [n, 3]) rotated by the unit quaternion q = (w, x, y, z)"""
    qw, qv = float(q[0]), np.asarray(q[1:], np.float64)
    t = 2 * np.cross(qv, v)
    return v + qw * t + np.cross(qv, t)


def coxa_axis_cloud(n, leg, quat, rng):
    """tools/stress_tol.py's coxa_axis cloud: within 60 mm of the coxa axis of (leg, quat), chosen in the coxa frame and mapped
    back to the body frame"""
    leg = np.asarray(leg, np.float64).reshape(-1)
    reach = reach_of(leg)
    rr = rng.uniform(0, 60, n)
    th = rng.uniform(-np.pi, np.pi, n)
    c = np.column_stack([rr * np.cos(th), rr * np.sin(th), rng.uniform(-1.1 * reach, 1.1 * reach, n)])
    cp, sp = np.cos(leg[2]), np.sin(leg[2])
    v = np.column_stack([c[:, 0] * cp - c[:, 2] * sp, c[:, 1], c[:, 0] * sp + c[:, 2] * cp])
    v[:, 0] += leg[1]
    cb, sb = np.cos(leg[0]), np.sin(leg[0])
    v = np.column_stack([v[:, 0] * cb - v[:, 1] * sb, v[:, 0] * sb + v[:, 1] * cb, v[:, 2]])
    return rotate(IDENTITY if quat is None else quat, v).astype(np.float32)


def seeds(family, n, leg, quat, rng):
    if family in ("uni_shell", "mix_shell"):
        return ((rng.random((n, 3), dtype=np.float32) * 2 - 1) * np.float32(1.15 * reach_of(leg))).astype(np.float32)
    if family == "grid_shell":
        return np.column_stack([rng.uniform(-100, 601, n), np.zeros(n), rng.uniform(-350, 51, n)]).astype(np.float32)
    if family == "axis_shell":
        return coxa_axis_cloud(n, leg, quat, rng)
    raise ValueError(family)


def make(family, n, lrm, leg, quat, strict_dist, seed):
    """n points of `family` for (leg, quat).  strict_dist(points) -> the strict vectors float32 [len, 3] (the oracle's, or
    lrm_dist_cpu's).  Seeds whose vector is zero (reachable points) give no shell point, so seeds are drawn in rounds of n
    until n shell points exist; the result is cut to n."""
    rng = np.random.default_rng([seed, FAMILIES.index(family)])
    terms = band_terms(lrm, leg, quat)
    f_lo, f_hi = F_RANGE[family]
    parts, have = [], 0
    for _ in range(8):
        sp = seeds(family, n, leg, quat, rng)
        parts.append(shell(sp, strict_dist(sp), terms, f_lo, f_hi, rng))
        have += len(parts[-1])
        if have >= n:
            break
    assert have >= n, f"{family}: only {have} of {n} shell points after 8 rounds of seeds"
    return np.ascontiguousarray(np.concatenate(parts)[:n])


def shares(points, d_ref, terms):
    """(share with thr <= |d_ref| < 2 thr, share with 0 < |d_ref| < thr) of a cloud"""
    t = thr(points, terms).astype(np.float64)
    nref = np.linalg.norm(np.asarray(d_ref, np.float64), axis=1)
    return float(((nref >= t) & (nref < 2 * t)).mean()), float(((nref > 0) & (nref < t)).mean())


def crossover(nref, err, thr_at, tol=1.0e-5):
    """Where the tolerance arithmetic stops meeting tol: over the vectors with err > tol |d_ref|, the longest (the crossover
    length L: every vector longer than L meets tol) and the largest |d_ref| / thr (the same as a fraction of the threshold at the
    vector's own point) -> dict(mm, thr_mm at that vector, frac, index); zeros and index -1 when no vector misses."""
    nref = np.asarray(nref, np.float64)
    bad = np.flatnonzero(np.asarray(err, np.float64) > tol * nref)
    if len(bad) == 0:
        return dict(mm=0.0, thr_mm=0.0, frac=0.0, index=-1)
    t = np.asarray(thr_at, np.float64)
    i = int(bad[np.argmax(nref[bad])])
    return dict(mm=float(nref[i]), thr_mm=float(t[i]), frac=float((nref[bad] / t[bad]).max()), index=i)


# ---- legs and orientations ------------------------------------------------------------------------------------------------
def scaled_m2(lrm, k):
    """M2 with its four lengths (body, coxa, tibia, femur: fields 1, 3, 4, 5) times k: the band term rules the threshold"""
    leg = lrm.get_M2_leg(0.0).copy()
    leg[[1, 3, 4, 5]] *= np.float32(k)
    return leg


def random_leg(lrm, rng):
    """one leg of tools/stress_tol.py's generator (the same eleven draws)"""
    return lrm.leg_factory(float(rng.uniform(-3.1, 3.1)), float(rng.uniform(60, 260)), float(rng.uniform(-60, 20)),
                           float(rng.uniform(30, 110)), float(rng.uniform(90, 180)), float(rng.uniform(90, 200)),
                           float(rng.uniform(25, 85)), float(rng.uniform(50, 100)), float(rng.uniform(80, 140)),
                           float(rng.uniform(-15, 10)), float(rng.uniform(-15, 10)))


def random_quat(rng, tilt=1.0):
    q = rng.normal(size=4) * np.array([1.0, 0.25 * tilt, 0.25 * tilt, 0.35 * tilt])
    q[0] = abs(q[0]) + 0.8
    return tuple(float(v) for v in (q / np.linalg.norm(q)).astype(np.float32))


RANDOM_LEG_SEED = 1
RANDOM_LEG_PICKS = (0, 13, 4, 5, 7, 12)


LEG_NAMES = ("m2_a", "m2_b", "moon_a", "moon_b", "m2_x2", "m2_x3", "rnd_0", "rnd_1", "rnd_2", "rnd_3", "rnd_4", "rnd_5")
ORIENTATIONS = {"id": IDENTITY, "tilt_y": TILT_Y, "tilt_z": TILT_Z}


def legs(lrm):
    """name -> (leg, its random quaternion or None).  The six random legs are numbers RANDOM_LEG_PICKS of the generator's sequence
    (seed RANDOM_LEG_SEED; each draw is a leg, then its quaternion).  They are picked by hand so that every case meets its
    conditions: all are eligible for the tolerance mode in the four orientations, two have a coxa pitch beyond +-45 degrees
    (-48.5 and -49.8), one faces away from the bench grid (azimuth -3.06).  Passed over: legs the mode refuses (numbers 6, 11, 15),
    and legs some shell of which collapses onto the workspace corner next to the coxa axis, where 29-80 % of it is in doubt and
    belongs to the fix-up (numbers 2, 3, 8)."""
    out = {"m2_a": (lrm.get_M2_leg(0.0), None), "m2_b": (lrm.get_M2_leg(-2.0), None),
           "moon_a": (lrm.get_moonbot_leg(0.7), None), "moon_b": (lrm.get_moonbot_leg(np.pi / 3), None),
           "m2_x2": (scaled_m2(lrm, 2.0), None), "m2_x3": (scaled_m2(lrm, 3.0), None)}
    rng = np.random.default_rng(RANDOM_LEG_SEED)
    drawn = [(random_leg(lrm, rng), random_quat(rng)) for _ in range(max(RANDOM_LEG_PICKS) + 1)]
    for i, k in enumerate(RANDOM_LEG_PICKS):
        out[f"rnd_{i}"] = drawn[k]
    assert tuple(out) == LEG_NAMES
    return out


def case_keys():
    """[(family, leg name, orientation name)], known without the library.  Every family meets every leg once; the orientation
    rotates with (leg, family) through identity, the two tilted fixture orientations and, for a random leg, its own quaternion
    ("rnd"), so that every family sees every kind of orientation and every leg at least three of them.  The tilted M2 uni_shell
    (the case that fills a workgroup's doubt segment) is ("uni_shell", "m2_a", "tilt_y")."""
    out = []
    for li, name in enumerate(LEG_NAMES):
        orients = ["id", "tilt_y", "tilt_z"] + (["rnd"] if name.startswith("rnd_") else [])
        for fi, family in enumerate(FAMILIES):
            out.append((family, name, orients[(li + fi + 1) % len(orients)]))
    return out


def case_id(key):
    return "-".join(key)


def resolve(lrm, key, _cache={}):
    """(leg, quat) of a case key"""
    if "legs" not in _cache:
        _cache["legs"] = legs(lrm)
    leg, rq = _cache["legs"][key[1]]
    return leg, (rq if key[2] == "rnd" else ORIENTATIONS[key[2]])
