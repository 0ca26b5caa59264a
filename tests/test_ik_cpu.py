"""Joint angles on the host (lrm_ik_cpu, lrm_fk_cpu): the contract of include/lrm.h against the oracle's reach mask and
distance vectors and an independent float64 forward kinematics, the FK / IK round trip, the seed rule, arguments."""
import ctypes as C

import numpy as np
import pytest

from ik_cases import (COXA_LEN, FEMUR_LEN, TIBIA_LEN, check_contract, fk64, golden_cases, is_unit, limits, load_case,
                      random_cloud, random_legs, standard_cases)


def test_golden_fixtures(lrm, oracle):
    """every fixture with its own quaternion: items 1-4; item 5 where the quaternion is unit (ik_cases.is_unit)"""
    for name in golden_cases():
        c = load_case(name)
        ang, st, ms = lrm.apply_ik_cpu(c["points"], c["leg"], c["quat"])
        assert ms >= 0
        check_contract(oracle, c["points"], c["leg"], c["quat"], ang, st, clean=is_unit(c["quat"]))


def test_standard_legs_every_azimuth_and_orientation(lrm, oracle):
    pts = random_cloud(1_000_000, seed=7)
    seen = np.zeros(5, np.int64)
    for name, leg, q in standard_cases(lrm):
        ang, st, _ = lrm.apply_ik_cpu(pts, leg, q)
        seen += check_contract(oracle, pts, leg, q, ang, st)["counts"]
    assert seen[1] > 100_000 and seen[2] > 1_000_000  # both goals are exercised


def test_random_legs_report_the_model_gap(lrm, oracle):
    """random geometries: items 1-4 hold on every leg; statuses 3 / 4 (the circle model against the joint limits) occur
    on some of them -- DESIGN.md records which"""
    pts = random_cloud(100_000, seed=7)
    gaps = {}
    for name, leg, q in random_legs(lrm):
        ang, st, _ = lrm.apply_ik_cpu(pts, leg, q)
        counts = check_contract(oracle, pts, leg, q, ang, st, clean=False)["counts"]
        if counts[3] or counts[4]:
            gaps[name] = (int(counts[3]), int(counts[4]))
    assert gaps, "no random leg produced status 3 or 4"
    assert len(gaps) < 12


def test_non_finite_input(lrm, oracle):
    leg = lrm.get_M2_leg(0.3)
    pts = np.array([[300, 0, -100], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [900, 900, 900]], np.float32)
    ang, st, _ = lrm.apply_ik_cpu(pts, leg)
    assert list(st) == [1, 0, 0, 0, 2] or (st[0] in (1, 2) and list(st[1:4]) == [0, 0, 0])
    assert np.isnan(ang[1:4]).all() and np.isfinite(ang[[0, 4]]).all()
    check_contract(oracle, pts, leg, (1, 0, 0, 0), ang, st)


def _grid(oracle, leg, q, n=20, margin=1e-3):
    L = limits(oracle, leg, q)
    axes = [np.linspace(lo, hi, n + 2)[1:-1] for lo, hi in (L["coxa"], L["femur"], L["tibia"])]
    g = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    s = g[:, 1] + g[:, 2]
    keep = (s > L["abs"][0] + margin) & (s < L["abs"][1] - margin)
    # off the coxa axis: there the yaw does not follow from the position
    lg = np.asarray(leg, np.float64)
    h = lg[COXA_LEN] + lg[FEMUR_LEN] * np.cos(g[:, 1]) + lg[TIBIA_LEN] * np.cos(s)
    return np.ascontiguousarray(g[keep & (np.abs(h) > 1.0)], np.float32)


@pytest.mark.parametrize("which", ["m2", "moonbot"])
def test_fk_ik_round_trip(lrm, oracle, which):
    leg = (lrm.get_M2_leg if which == "m2" else lrm.get_moonbot_leg)(0.7)
    q = np.array([0.9, 0.1, 0.2, -0.3], np.float32)
    q /= np.float32(np.linalg.norm(q))
    g = _grid(oracle, leg, q)
    assert len(g) > 2000
    xyz, ms = lrm.apply_fk_cpu(g, leg, q)
    assert ms >= 0
    assert np.linalg.norm(xyz - fk64(g, leg, q), axis=1).max() <= 1e-3
    ang, st, _ = lrm.apply_ik_cpu(xyz, leg, q, seed=g)
    assert (st == 1).all(), np.bincount(st, minlength=5)
    bent = np.abs(g[:, 2]) > 0.01
    assert np.abs(ang[bent] - g[bent]).max() <= 1e-3
    check_contract(oracle, xyz, leg, q, ang, st)


def _two_knees(leg, lim):
    """a point in front of the leg with both knees inside the limits -> (point, knee + angles, knee - angles)"""
    lg = np.asarray(leg, np.float64)
    F, T = lg[FEMUR_LEN], lg[TIBIA_LEN]
    for f, t in ((0.2, -0.9), (-0.3, -0.8), (0.4, -1.2), (0.0, -0.6)):
        p = fk64([[0.1, f, t]], leg)[0]
        # the other knee of the same (yaw, in-plane) goal
        t2 = -t
        alpha = f + np.arctan2(T * np.sin(t), F + T * np.cos(t))
        f2 = alpha - np.arctan2(T * np.sin(t2), F + T * np.cos(t2))
        a, b = np.array([0.1, f, t]), np.array([0.1, f2, t2])
        inside = all(lim[k][0] + 0.05 < v < lim[k][1] - 0.05 for s in (a, b)
                     for k, v in (("femur", s[1]), ("tibia", s[2]), ("abs", s[1] + s[2])))
        if inside:
            return p.astype(np.float32), a, b
    raise AssertionError("no two-knee point found")


def test_seed_selects_the_knee(lrm, oracle):
    leg = lrm.get_moonbot_leg(0.0)
    lim = limits(oracle, leg, (1, 0, 0, 0))
    p, a, b = _two_knees(leg, lim)
    for want in (a, b):
        ang, st, _ = lrm.apply_ik_cpu(p[None], leg, seed=(want + 0.05)[None])
        assert st[0] == 1 and np.abs(ang[0] - want).max() < 1e-3
    # no seed: the mid-range of each joint's limits, the nearer knee wins
    mid = np.array([np.mean(lim[k]) for k in ("coxa", "femur", "tibia")], np.float64)
    want = a if ((a - mid) ** 2).sum() < ((b - mid) ** 2).sum() else b
    ang, st, _ = lrm.apply_ik_cpu(p[None], leg)
    assert st[0] == 1 and np.abs(ang[0] - want).max() < 1e-3


def test_non_finite_and_far_seeds_only_break_ties(lrm, oracle):
    """a seed can only choose among the near-best candidates: nan / inf components mean "no seed" (the same angles as
    without one), a finite seed far enough for every distance to overflow keeps the best-residual candidate; the status
    never changes (a previous frame's nan output fed back as the seed must not report a model gap)"""
    leg = lrm.get_moonbot_leg(0.0)
    pts = np.array([[250, 40, -150], [300, 0, -100]], np.float32)
    a0, s0, _ = lrm.apply_ik_cpu(pts, leg)
    assert list(s0) == [1, 2]
    for v in (np.nan, np.inf, -np.inf, 1e20, -3e38):
        a, s, _ = lrm.apply_ik_cpu(pts, leg, seed=np.full((2, 3), v, np.float32))
        assert list(s) == [1, 2], v
        if not np.isfinite(v):
            assert np.array_equal(a, a0)
    cloud = random_cloud(100_000, seed=3)
    a0, s0, _ = lrm.apply_ik_cpu(cloud, leg)
    rng = np.random.default_rng(4)
    seed = (rng.random((len(cloud), 3), dtype=np.float32) * 2 - 1).astype(np.float32)
    bad = rng.integers(0, 5, len(cloud))
    seed[bad == 1, rng.integers(0, 3)] = np.nan
    seed[bad == 2] = np.inf
    seed[bad == 3, 1] = -np.inf
    seed[bad == 4] = 1e20
    a, s, _ = lrm.apply_ik_cpu(cloud, leg, seed=seed)
    assert np.array_equal(s, s0)
    nonfin = ~np.isfinite(seed).all(1)
    assert nonfin.sum() > 50_000 and np.array_equal(a[nonfin], a0[nonfin])
    check_contract(oracle, cloud, leg, (1, 0, 0, 0), a, s)


def test_arguments_and_errors(lrm):
    L = lrm.lib()
    leg = lrm.get_M2_leg(0.0)
    lp = leg.ctypes.data_as(C.c_void_p)
    ang, st, _ = lrm.apply_ik_cpu(np.zeros((0, 3), np.float32), leg)
    assert ang.shape == (0, 3) and st.shape == (0,)
    xyz, _ = lrm.apply_fk_cpu(np.zeros((0, 3), np.float32), leg)
    assert xyz.shape == (0, 3)
    pts = np.zeros((4, 3), np.float32)
    out = np.zeros((4, 3), np.float32)
    stb = np.zeros(4, np.uint8)
    pp, op, sp = (a.ctypes.data_as(C.c_void_p) for a in (pts, out, stb))
    assert L.lrm_ik_cpu(pp, 4, lp, None, None, None, sp, None) == -1
    assert L.lrm_ik_cpu(pp, 4, lp, None, None, op, None, None) == -1
    assert L.lrm_ik_cpu(pp, 4, None, None, None, op, sp, None) == -1
    assert L.lrm_fk_cpu(pp, 4, lp, None, None, None) == -1
    assert L.lrm_ik_cpu(None, 0, lp, None, None, None, None, None) == 0
    # a partial seed set is refused before anything else
    one = C.c_void_p(16)
    assert L.lrm_ik_dev(one, one, one, 4, lp, None, one, None, None, one, one, one, one, None) == -1
    assert L.lrm_ik_dev(one, one, one, 4, lp, None, None, None, one, one, one, one, one, None) == -1
    assert L.lrm_ik_dev(one, one, one, 4, None, None, None, None, None, one, one, one, one, None) == -1
    assert L.lrm_fk_dev(one, one, one, 4, lp, None, None, one, one, None) == -1
    if lrm.device_count() == 0:  # no GPU: the device calls report LRM_ENODEV, they never compute on the CPU
        assert L.lrm_ik_dev(one, one, one, 4, lp, None, None, None, None, one, one, one, one, None) == -2
        assert L.lrm_fk_dev(one, one, one, 4, lp, None, one, one, one, None) == -2
    else:
        assert L.lrm_ik_dev(None, None, None, 0, lp, None, None, None, None, None, None, None, None, None) == 0
        assert L.lrm_fk_dev(None, None, None, 0, lp, None, None, None, None, None) == 0
    with pytest.raises(ValueError):
        lrm.apply_ik_cpu(pts, leg, seed=np.zeros((3, 3), np.float32))


def test_symbols_are_declared_and_exported(lrm):
    names = {"lrm_ik_dev", "lrm_fk_dev", "lrm_ik_cpu", "lrm_fk_cpu"}
    assert names <= set(lrm.declared_symbols())
    assert names <= set(lrm.exported_symbols())
