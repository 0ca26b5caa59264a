"""Shared pieces of the joint-angle tests (tests/test_ik_cpu.py, tests/test_gpu_ik.py): an independent float64 forward
kinematics, the joint limits of oracle.rotate_leg_data, the leg / orientation families and the contract check of
include/lrm.h (lrm_ik_*) against the oracle's reach mask and distance vectors."""
import numpy as np

from conftest import golden_cases, load_case, random_cloud  # noqa: F401
from posed_cases import fixture_quats  # noqa: F401

# LegDimensions field order (include/lrm.h)
BODY_ANGLE, BODY, COXA_PITCH, COXA_LEN, TIBIA_LEN, FEMUR_LEN, ABS_POS, ABS_NEG = range(8)
MAX_COXA, MIN_COXA, MAX_TIBIA, MIN_TIBIA, MAX_FEMUR, MIN_FEMUR = range(8, 14)
AZIMUTHS = (0.0, 1.1, -2.4)
TOL = 2.5e-3  # mm: the kernel's 2e-3 status threshold plus float32 against float64


def qt_matrix(q):
    """qtRotate(q, .) (unified_math_cuda.cu.h:13-27, q[0] the scalar part) as a float64 3x3 matrix"""
    a, b, c, d = (float(v) for v in q)
    t2, t3, t4, t5, t6, t7, t8, t9, t10 = a * b, a * c, a * d, -b * b, b * c, b * d, -c * c, c * d, -d * d
    m = np.array([[t8 + t10, t6 - t4, t3 + t7], [t4 + t6, t5 + t10, t9 - t2], [t7 - t3, t2 + t9, t5 + t8]])
    return 2.0 * m + np.eye(3)


def back_matrix(q):
    """the inverse of qtInvRotate(q, .) = qtRotate(qtInvert(q), .) (unified_math_cuda.cu.h:29-38), float64: qtRotate(q, .)
    for a unit quaternion; the reference does not normalise, and for other quaternions only this inverse undoes the
    frame change the queries make"""
    a, b, c, d = (float(v) for v in q)
    n2 = a * a + b * b + c * c + d * d
    return np.linalg.inv(qt_matrix((a / n2, -b / n2, -c / n2, -d / n2)))


def fk64(angles, leg, quat=(1, 0, 0, 0)):
    """tip of (coxa, femur, tibia) in the caller's frame, float64: the reference's forward_kinematics in the coxa frame,
    then the coxa pitch, the body offset, the leg azimuth and the body orientation (back_matrix)"""
    a = np.asarray(angles, np.float64).reshape(-1, 3)
    c, f, t = a[:, 0], a[:, 1], a[:, 2]
    leg = np.asarray(leg, np.float64)
    h = leg[COXA_LEN] + leg[FEMUR_LEN] * np.cos(f) + leg[TIBIA_LEN] * np.cos(f + t)
    x, y, z = np.cos(c) * h, np.sin(c) * h, leg[FEMUR_LEN] * np.sin(f) + leg[TIBIA_LEN] * np.sin(f + t)
    cp, sp = np.cos(leg[COXA_PITCH]), np.sin(leg[COXA_PITCH])
    x, z = x * cp - z * sp + leg[BODY], x * sp + z * cp
    cb, sb = np.cos(leg[BODY_ANGLE]), np.sin(leg[BODY_ANGLE])
    x, y = x * cb - y * sb, x * sb + y * cb
    return np.stack([x, y, z], 1) @ back_matrix(quat).T


def limits(oracle, leg, quat):
    """joint limits after rotate_leg_data (float32): coxa, femur, tibia, femur + tibia as (lo, hi) pairs"""
    r = oracle.rotate_leg_data(quat, leg)
    return {"coxa": (r[MIN_COXA], r[MAX_COXA]), "femur": (r[MIN_FEMUR], r[MAX_FEMUR]),
            "tibia": (r[MIN_TIBIA], r[MAX_TIBIA]), "abs": (r[ABS_NEG], r[ABS_POS])}


def is_unit(q):
    """The reference does not normalise quaternions and four of the five fixture orientations are not unit (|q| - 1 up
    to -2.5e-2).  For those qtRotate(q, .) is not the inverse of qtInvRotate(q, .): the oracle's distance vector, rotated
    back by qtRotate, is not the displacement to its nearest point, and status 4 reports exactly that.  Contract item 5
    (no status 3 / 4 on the standard legs) is a statement about unit quaternions."""
    return abs(float(np.linalg.norm(np.asarray(q, np.float64))) - 1.0) < 1e-6


def unit(q):
    q = np.asarray(q, np.float64)
    return (q / np.linalg.norm(q)).astype(np.float32)


def standard_cases(lrm):
    """(name, leg, quat): M2 and moonbot at three azimuths under every fixture orientation, normalised (see is_unit)"""
    out = []
    for fam, make in (("m2", lrm.get_M2_leg), ("moonbot", lrm.get_moonbot_leg)):
        for az in AZIMUTHS:
            for k, q in enumerate(fixture_quats()):
                out.append((f"{fam}_az{az}_q{k}", make(az), unit(q)))
    return out


def random_legs(lrm, n=12):
    """the generator of tests/test_gpu_parity.py::test_random_legs_including_filter_ineligible_ones (rng 7), with the
    quaternion normalised: the joint-angle calls invert qtRotate, a rotation only for unit quaternions"""
    rng = np.random.default_rng(7)
    out = []
    for trial in range(n):
        coxa_deg = rng.uniform(30, 80) if trial % 3 else rng.uniform(95, 150)
        leg = lrm.leg_factory(rng.uniform(-3, 3), rng.uniform(80, 250), rng.uniform(-60, 30), rng.uniform(30, 90),
                              rng.uniform(90, 160), rng.uniform(90, 170), coxa_deg, rng.uniform(60, 100),
                              rng.uniform(90, 140), rng.uniform(-20, 10), rng.uniform(-20, 10))
        q = rng.normal(size=4).astype(np.float32)
        q[0] += 3.0
        out.append((f"random{trial}", leg, unit(q)))
    return out


def check_contract(oracle, pts, leg, quat, ang, st, clean=True):
    """Contract items 1-4 (and 5 when `clean`: no status 3 or 4) of lrm_ik_*; returns the measured margins"""
    pts = np.asarray(pts, np.float32)
    mask = oracle.reach(pts, leg, quat).astype(bool)
    d, _ = oracle.dist(pts, leg, quat)
    finite = np.isfinite(pts).all(1)
    # 1. status in {1, 3} <=> the reach mask; non-finite input: status 0 and nan angles
    assert np.array_equal(np.isin(st, (1, 3)), mask & finite)
    assert (st[~finite] == 0).all() and np.isnan(ang[~finite]).all()
    assert (st[finite] != 0).all() and np.isin(st, (0, 1, 2, 3, 4)).all()
    a = ang[finite]
    # 2. every angle within its limit (inclusive, float32), femur + tibia within the absolute limits up to 1e-6 rad
    L = limits(oracle, leg, quat)
    for j, k in enumerate(("coxa", "femur", "tibia")):
        assert (a[:, j] >= L[k][0]).all() and (a[:, j] <= L[k][1]).all(), k
    s = a[:, 1].astype(np.float64) + a[:, 2].astype(np.float64)
    assert (s >= float(L["abs"][0]) - 1e-6).all() and (s <= float(L["abs"][1]) + 1e-6).all()
    # 3. / 4. the tip against p
    p = pts[finite].astype(np.float64)
    miss = np.linalg.norm(fk64(a, leg, quat) - p, axis=1)
    dn = np.linalg.norm(d[finite].astype(np.float64), axis=1)
    sf = st[finite]
    r1, r2 = sf == 1, sf == 2
    # the status is decided in float32: the status-2 line is |d| + 2e-3 + 2^-22 |d| (include/lrm.h), and float32 against
    # float64 adds up to an ulp or two of |p| (6e-5 mm at 500 mm; far points, |p| = 1e6 mm, in the fixtures)
    slack = TOL + np.linalg.norm(p, axis=1) * 2.0 ** -22
    assert (miss[r1] <= slack[r1]).all(), f"status 1: max miss {miss[r1].max():.3e} mm"
    assert (miss[r2] <= dn[r2] * (1 + 2.0 ** -22) + slack[r2]).all(), \
        f"status 2: max excess {(miss[r2] - dn[r2]).max():.3e} mm"
    if clean:  # 5.
        assert not np.isin(sf, (3, 4)).any(), f"statuses 3/4 on a clean leg: {np.bincount(sf, minlength=5)}"
    return {"reached_max_mm": float(miss[r1].max()) if r1.any() else 0.0,
            "nearest_excess_max_mm": float((miss[r2] - dn[r2]).max()) if r2.any() else 0.0,
            "counts": np.bincount(sf, minlength=5)}
