"""Leg link clearance on the host (no GPU): lrm_leg_joints_posed_cpu against lrm_fk_posed_cpu bit for bit, and the host
loop lrm_leg_clearance_posed_cpu -- the reference of tests/test_gpu_leg_clearance.py -- against
leg_clearance_cases.brute_np, the numpy float32 restatement of include/lrm.h's arithmetic, bit for bit on every output."""
import ctypes as C

import numpy as np
import pytest

import footholds_posed_cases as fc
import ik_cases
import leg_clearance_cases as lc
import pair_cases as pc
import posed_cases

KEYS = ("hits", "links", "worst", "pen", "free")


def legs6(lrm):
    return pc.leg_families(lrm)["m2_6_tilted"][0]


def plus0(a):
    """bits with -0 turned into +0"""
    with np.errstate(invalid="ignore"):
        return pc.bits(np.asarray(a, np.float32) + np.float32(0))


def quat_sets(lrm, n):
    rng = np.random.default_rng(11)
    fix = np.asarray(ik_cases.fixture_quats(), np.float32)
    nonunit = posed_cases.random_unit_quats(n, rng) * rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
    return {"identity": np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1)), "fixture": fix[np.arange(n) % len(fix)],
            "random_unit": posed_cases.random_unit_quats(n, rng), "nonunit": np.ascontiguousarray(nonunit, np.float32)}


def leg_sets(lrm):
    """all leg families of ik_cases: M2 and moonbot at its azimuths, and its random legs (eight at a time)"""
    std = {}
    for name, leg, _ in ik_cases.standard_cases(lrm):
        std.setdefault(name.rsplit("_q", 1)[0], leg)
    rnd = [leg for _, leg, _ in ik_cases.random_legs(lrm)]
    return {"standard": np.stack(list(std.values())).astype(np.float32), "random_a": np.stack(rnd[:8]).astype(np.float32),
            "random_b": np.stack(rnd[4:12]).astype(np.float32)}


@pytest.mark.parametrize("qname", ["identity", "fixture", "random_unit", "nonunit"])
@pytest.mark.parametrize("lname", ["standard", "random_a", "random_b"])
def test_joints_are_the_fk_chain(lrm, qname, lname):
    """J3 + body = lrm_fk_posed_cpu's tip (tip_clear 0), J2 = that call with tibia_length 0, J1 with femur and tibia 0, J0 with
    all three 0, bit for bit (-0 compared as +0); with tip_clear > 0, J3 = the tip of the leg with tibia_length T'"""
    legs = leg_sets(lrm)[lname]
    n = 40
    quats = quat_sets(lrm, n)[qname]
    body = np.random.default_rng(2).uniform(-3000, 3000, (n, 3)).astype(np.float32)
    ang = lc.random_angles(n, len(legs), seed=4)
    for tip_clear in (0.0, 30.0, 1e4):  # 1e4 >= T: T' = 0, the tibia link shrinks to the knee
        got = lrm.leg_joints_posed_cpu(ang, quats, body, legs, tip_clear)[0]
        want = lc.joints_from_fk(lrm, ang, quats, body, legs, tip_clear)
        assert np.isfinite(want).all()
        assert np.array_equal(plus0(got), plus0(want))
        if tip_clear == 0.0:
            pi, li = lc.layout(n, len(legs))
            tip = lrm.apply_fk_posed_cpu(ang, pi, li, quats, body, legs)[0].reshape(len(legs), n, 3)
            assert np.array_equal(plus0(got[:, :, 3]), plus0(tip))
        if tip_clear == 1e4:
            assert np.array_equal(plus0(got[:, :, 3]), plus0(got[:, :, 2]))
    rel = lrm.leg_joints_posed_cpu(ang, quats, None, legs, 30.0)[0]  # body NULL: the relative joints the test itself uses
    assert np.array_equal(plus0(rel), plus0(lc.joints_from_fk(lrm, ang, quats, None, legs, 30.0)))


def test_joints_of_bad_angles_and_bad_arguments(lrm):
    legs = legs6(lrm)
    quats = quat_sets(lrm, 5)["random_unit"]
    ang = lc.random_angles(5, 6, seed=1)
    ang[0] = np.nan
    ang[7, 0] = 200.0   # outside the sincos range
    ang[9, 2] = np.inf
    J = lrm.leg_joints_posed_cpu(ang, quats, None, legs, 0.0)[0].reshape(30, 4, 3)
    bad = ~np.isfinite(J).all((1, 2))
    assert np.array_equal(np.flatnonzero(bad), [0, 7, 9]) and np.isfinite(J[:, 0]).all()  # J0 does not depend on the angles
    quats[3, 1] = np.nan  # a nan quaternion: every joint of the pose is nan, whatever route the nan took
    Jb = lrm.leg_joints_posed_cpu(ang, quats, np.full((5, 3), -70.0, np.float32), legs, 0.0)[0]
    assert np.isnan(Jb[:, 3]).all() and (pc.bits(Jb)[np.isnan(Jb)] == 0x7fc00000).all()  # stored as the canonical quiet nan
    for tc in (np.nan, -1.0, np.inf):
        with pytest.raises(lrm.LrmError):
            lrm.leg_joints_posed_cpu(ang, quats, None, legs, tc)
    with pytest.raises(ValueError):
        lrm.leg_joints_posed_cpu(ang[:-1], quats, None, legs, 0.0)
    assert lrm.leg_joints_posed_cpu(np.zeros((0, 3), np.float32), np.zeros((0, 4), np.float32), None, legs, 0.0)[0].size == 0


def compare(lrm, targets, quats, body, legs, ang, radius=lc.RADIUS, margin=lc.MARGIN, tip_clear=lc.TIP_CLEAR, live_in=None, detail=False):
    J = lc.joints_from_fk(lrm, ang, quats, None, legs, tip_clear)
    want = lc.brute_np(targets, body, J, radius, margin, live_in, detail=detail)
    got = lc.host(lrm, targets, quats, body, legs, ang, radius, margin, tip_clear, live_in)
    lc.assert_same(tuple(got[k] for k in KEYS), want)
    lc.assert_consequences(got, margin, live_in)
    return want


def test_main_scene_is_not_vacuous_and_matches(lrm):
    """by brute_np alone: of the live valid (pose, leg) pairs at least 10 % have hits, 10 % are near without a hit, 10 % have
    no near target; every winner has an exact tie (each target is present twice); no stance counts its own foothold"""
    legs = legs6(lrm)
    quats, body, targets = lc.main_scene(lrm)
    ang, st, best = lc.stance_angles(lrm, targets, quats, body, legs)
    assert lc.TIP_CLEAR > lc.RADIUS[2]
    want = compare(lrm, targets, quats, body, legs, ang, detail=True)
    v = want["valid"]
    assert v.sum() > 400 and np.array_equal(v.reshape(-1), st != 0)
    hit, near = (want["hits"] > 0)[v], want["near_any"][v]
    assert hit.mean() >= 0.10, float(hit.mean())
    assert (near & ~hit).mean() >= 0.10, float((near & ~hit).mean())
    assert (~near).mean() >= 0.10, float((~near).mean())
    assert 0 < want["free"].sum() < len(quats)
    own, hm = best.reshape(-1), want["hit"].reshape(-1, len(targets))
    has = np.flatnonzero(own >= 0)
    assert len(has) > 400 and not hm[has, own[has]].any()
    half = len(targets) // 2  # the twin of the winner sits in the other half: the smaller index must have won
    w = want["worst"][want["worst"] >= 0]
    assert len(w) > 200 and (w < half).all()


@pytest.mark.parametrize("kind,nt", [("rough", 2500), ("dense_cluster", 3000), ("sparse_tiles", 3 * 1024)])
@pytest.mark.parametrize("margin", [0.0, 12.0])
def test_host_loop_on_the_scenes(lrm, kind, nt, margin):
    """pose_quats holds non-unit and nan quaternions: skipped legs inside live poses; stance angles and free angles"""
    legs = legs6(lrm)
    quats, body, targets = lc.scene(lrm, 60, nt, seed=3, kind=kind)
    if kind == "dense_cluster":
        body[:, 2] -= np.float32(60.0)
    ang = lc.stance_angles(lrm, targets, quats, body, legs)[0]
    want = compare(lrm, targets, quats, body, legs, ang, margin=margin, detail=True)
    assert (~want["valid"]).any() and want["valid"].any()
    want = compare(lrm, targets, quats, body, legs, lc.random_angles(60, 6, seed=8), margin=margin)
    assert (want["hits"] > 0).any() and (want["worst"] < 0).any()


def test_bad_targets_bodies_and_angles(lrm):
    legs = legs6(lrm)
    quats, body, targets = lc.scene(lrm, 50, 2000, seed=5)
    ang = lc.random_angles(50, 6, seed=2)
    bad_t = targets.copy()
    bad_t[::7] = np.nan
    bad_t[3::11, 1] = np.inf
    bad_t[5::13] = -np.inf
    want = compare(lrm, bad_t, quats, body, legs, ang)
    assert (want["hits"] > 0).any()
    bad_b = body.copy()
    bad_b[1] = np.nan
    bad_b[2, 0] = np.inf
    bad_b[35] = -np.inf
    want = compare(lrm, targets, quats, bad_b, legs, ang)
    assert (want["hits"][:, [1, 2, 35]] == 0).all() and (want["free"][[1, 2, 35]] == 1).all()
    bad_a = ang.copy()
    bad_a[::5] = np.nan
    bad_a[3::17, 0] = 200.0   # out of the sincos range
    bad_a[4::19, 1] = -200.0
    bad_a[6::23, 2] = np.inf
    want = compare(lrm, targets, quats, body, legs, bad_a, detail=True)
    assert not want["valid"].reshape(-1)[::5].any() and not want["valid"].reshape(-1)[3::17].any()
    assert (want["hits"][~want["valid"]] == 0).all() and (want["worst"][~want["valid"]] == -1).all()


@pytest.mark.parametrize("radius", [(0.0, 22.0, 16.0), (28.0, 0.0, 16.0), (28.0, 22.0, 0.0), (0.0, 0.0, 16.0), (0.0, 0.0, 0.0)])
def test_a_radius_of_zero_switches_the_link_off(lrm, radius):
    legs = legs6(lrm)
    quats, body, targets = lc.scene(lrm, 50, 2000, seed=6)
    want = compare(lrm, targets, quats, body, legs, lc.random_angles(50, 6, seed=3), radius=radius, margin=15.0)
    off = sum(1 << k for k in range(3) if radius[k] == 0)
    assert (want["links"] & off == 0).all()
    if off == 7:
        assert (want["worst"] == -1).all() and (want["free"] == 1).all()
    else:
        assert (want["hits"] > 0).any()


def test_tip_clear_beyond_the_tibia(lrm):
    legs = legs6(lrm)
    T = float(legs[0][lc.TIBIA_LEN])
    quats, body, targets = lc.scene(lrm, 50, 2000, seed=7)
    ang = lc.random_angles(50, 6, seed=4)
    for tc in (T, T + 1.0, 1e6):
        compare(lrm, targets, quats, body, legs, ang, tip_clear=tc)
    compare(lrm, targets, quats, body, legs, ang, tip_clear=0.0)


def test_live_in_forms(lrm):
    legs = legs6(lrm)
    quats, body, targets = lc.scene(lrm, 80, 2400, seed=9)
    ang = lc.stance_angles(lrm, targets, quats, body, legs)[0]
    forms = lc.live_forms(lrm, targets, quats, body, legs)
    assert 0 < forms["all_legs"].sum() < 80
    for name, live in forms.items():
        want = compare(lrm, targets, quats, body, legs, ang, live_in=live)
        if name == "zeros":
            assert (want["free"] == 0).all()
    mixed = np.ones(80, np.uint8)
    mixed[10:30] = 0
    mixed[40] = 3
    compare(lrm, targets, quats, body, legs, ang, live_in=mixed)
    with pytest.raises(ValueError):
        lc.host(lrm, targets, quats, body, legs, ang, live_in=mixed[:-1])


def test_empty_inputs_null_outputs_and_sentinels(lrm):
    legs = legs6(lrm)
    quats, body, targets = lc.scene(lrm, 20, 600, seed=4)
    ang = lc.random_angles(20, 6, seed=5)
    live = np.ones(20, np.uint8)
    live[3] = 0
    got = lc.host(lrm, np.zeros((0, 3), np.float32), quats, body, legs, ang, live_in=live)  # nt == 0: the empty answer
    assert (got["hits"] == 0).all() and (got["links"] == 0).all() and (got["worst"] == -1).all() and np.isneginf(got["pen"]).all()
    assert np.array_equal(got["free"], live)
    got = lc.host(lrm, targets, np.zeros((0, 4), np.float32), np.zeros((0, 3), np.float32), legs, np.zeros((0, 3), np.float32))
    assert got["hits"].shape == (6, 0) and got["free"].shape == (0,)  # nposes == 0: a no-op
    full = lc.host(lrm, targets, quats, body, legs, ang)
    part = lc.host(lrm, targets, quats, body, legs, ang, want_pen=False, want_free=False)
    assert part["pen"] is None and part["free"] is None
    lc.assert_same(tuple(part[k] for k in KEYS), full)
    # sentinel-filled outputs through the raw C ABI: every entry is written
    L, p = lrm.load(), lambda a: a.ctypes.data_as(C.c_void_p)
    q, b, lg = np.ascontiguousarray(quats), np.ascontiguousarray(body), np.ascontiguousarray(legs, np.float32)
    r = np.array(lc.RADIUS, np.float32)
    hits, worst = np.full((6, 20), -7, np.int32), np.full((6, 20), -7, np.int32)
    links, pen, free = np.full((6, 20), 0xA5, np.uint8), np.full((6, 20), -7, np.float32), np.full(20, 0xA5, np.uint8)
    args = lambda live_p: (p(targets), len(targets), p(q), p(b), 20, p(lg), 6, p(ang), p(r), lc.MARGIN, lc.TIP_CLEAR, live_p)
    assert L.lrm_leg_clearance_posed_cpu(*args(p(live)), p(hits), p(links), p(worst), p(pen), p(free), None) == 0
    lc.assert_same((hits, links, worst, pen, free), lc.host(lrm, targets, quats, body, legs, ang, live_in=live))
    # every LRM_EINVAL: NULL outputs and inputs, sizes, scalars
    assert L.lrm_leg_clearance_posed_cpu(*args(None), None, p(links), p(worst), p(pen), p(free), None) != 0
    assert L.lrm_leg_clearance_posed_cpu(*args(None), p(hits), None, p(worst), p(pen), p(free), None) != 0
    assert L.lrm_leg_clearance_posed_cpu(*args(None), p(hits), p(links), None, p(pen), p(free), None) != 0
    a = list(args(None))
    for k in (0, 2, 5, 7, 8):  # targets, quats, legs, angles, radius
        bad = list(a)
        bad[k] = None
        assert L.lrm_leg_clearance_posed_cpu(*bad, p(hits), p(links), p(worst), p(pen), p(free), None) != 0
    for k, v in ((1, 2 ** 31), (6, 0), (6, 9), (4, 2 ** 31)):  # nt, nlegs, nposes
        bad = list(a)
        bad[k] = v
        assert L.lrm_leg_clearance_posed_cpu(*bad, p(hits), p(links), p(worst), p(pen), p(free), None) != 0
    for kw in ({"margin": np.nan}, {"margin": -1.0}, {"margin": np.inf}, {"tip_clear": np.nan}, {"tip_clear": -0.5},
               {"tip_clear": np.inf}, {"radius": (np.nan, 1.0, 1.0)}, {"radius": (1.0, -1.0, 1.0)}, {"radius": (1.0, 1.0, np.inf)}):
        with pytest.raises(lrm.LrmError):
            lc.host(lrm, targets, quats, body, legs, ang, **kw)
        with pytest.raises(lrm.LrmError):  # the scalars are checked before the nposes == 0 no-op
            lc.host(lrm, targets, np.zeros((0, 4), np.float32), None, legs, np.zeros((0, 3), np.float32), **kw)


def test_the_symbols_are_declared_and_exported(lrm):
    names = {"lrm_leg_clearance_posed_dev", "lrm_leg_clearance_posed_cpu", "lrm_leg_joints_posed_dev", "lrm_leg_joints_posed_cpu"}
    assert names <= set(lrm._capi.declared_symbols()) and names <= set(lrm._capi.exported_symbols())
