"""Stance stability on the host: lrm_stance_stability_cpu against stance_cases.brute_np (a numpy float32 restatement of
include/lrm.h) bit for bit, into sentinel-filled outputs through the raw C call where the binding would allocate, and
against a float64 hull (stance_cases.margin64) within the arithmetic's error."""
import ctypes as C

import numpy as np
import pytest

import pair_cases as pc
import stance_cases as sc
import stance_model64 as sm

F = np.float32
EINVAL = -1  # LRM_EINVAL


@pytest.fixture(scope="module")
def main(lrm):
    return sc.main_scene(lrm)


def raw(lrm, targets, foot, quats, body, pose_idx, com, plane, lift, min_margin, live_in, nposes=None, nlegs=None, nstances=None,
        edge=True, feet=True, margin=True, stable=True):
    """the C call itself into sentinel-filled outputs -> (rc, margin, edge, stable, feet)"""
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    targets = np.ascontiguousarray(targets, F).reshape(-1, 3)
    foot = np.ascontiguousarray(foot, np.int32)
    nl, ns = foot.shape
    quats = None if quats is None else np.ascontiguousarray(quats, F).reshape(-1, 4)
    body = None if body is None else np.ascontiguousarray(body, F).reshape(-1, 3)
    pose_idx = None if pose_idx is None else np.ascontiguousarray(pose_idx, np.int32)
    live_in = None if live_in is None else np.ascontiguousarray(live_in, np.uint8)
    com = None if com is None else np.ascontiguousarray(com, F)
    plane = None if plane is None else np.ascontiguousarray(plane, F).reshape(6)
    lift = None if lift is None else np.ascontiguousarray(lift, np.uint8)
    nm = 1 if lift is None else len(lift)
    m, e = np.full((nm, max(ns, 1)), -7.0, F), np.full((nm, max(ns, 1)), 0xA5, np.uint8)
    st, ft = np.full((nm, max(ns, 1)), 0xA5, np.uint8), np.full(max(ns, 1), 0xA5, np.uint8)
    ms = C.c_double(-1)
    rc = lrm.load().lrm_stance_stability_cpu(p(targets), len(targets), p(quats), p(body), (0 if quats is None else len(quats)) if nposes is None else nposes,
                                             p(pose_idx), p(foot), ns if nstances is None else nstances, nl if nlegs is None else nlegs, p(com), p(plane), p(lift), nm,
                                             float(min_margin), p(live_in), p(m) if margin else None, p(e) if edge else None,
                                             p(st) if stable else None, p(ft) if feet else None, C.addressof(ms))
    return rc, m, e, st, ft


def check(lrm, targets, foot, quats, body=None, pose_idx=None, com=None, plane=None, lift=None, min_margin=0.0, live_in=None):
    lift = lrm.stance_lift(lift, len(foot))
    want = sc.brute_np(targets, foot, quats, body, pose_idx, com, plane, lift, min_margin, live_in)
    rc, m, e, st, ft = raw(lrm, targets, foot, quats, body, pose_idx, com, plane, lift, min_margin, live_in)
    assert rc == 0
    sc.assert_same((m, e, st, ft), want)
    sc.assert_consequences(want, min_margin)
    return want


def test_main_holds_every_kind_of_answer_by_the_reference_alone(main):
    targets, foot, quats, body, legs = main
    want = sc.brute_np(targets, foot, quats, body, com=sc.COM, lift=sc.lift_each(6))
    stable, unstable, none = sc.kinds(want)
    assert min(stable, unstable, none) >= 0.10, (stable, unstable, none)


@pytest.mark.parametrize("lift", ["none", "each", "tripods", "all64"])
def test_main_against_the_restatement(lrm, main, lift):
    targets, foot, quats, body, legs = main
    lf = {"none": None, "each": "each", "tripods": sc.TRIPODS, "all64": sc.lift_all(6)}[lift]
    want = check(lrm, targets, foot, quats, body, com=sc.COM, lift=lf)
    assert want["margin"].shape[0] == {"none": 1, "each": 7, "tripods": 2, "all64": 64}[lift]
    if lift == "all64":  # lifting everything leaves nothing to stand on; lifting more never adds a planted foot
        assert np.isneginf(want["margin"][63]).all()


@pytest.mark.parametrize("nlegs", [1, 2, 3, 4, 6, 8])
def test_leg_counts(lrm, nlegs):
    targets, foot, quats, body = sc.synthetic(150, nlegs, seed=nlegs)
    want = check(lrm, targets, foot, quats, body, com=[20.0, -10.0, 5.0], lift=sc.lift_all(nlegs))
    if nlegs < 3:
        assert np.isneginf(want["margin"]).all()
    else:
        assert (want["stable"] == 1).any() and np.isneginf(want["margin"]).any()
    if nlegs == 8:
        assert want["margin"].shape[0] == 256


def test_bad_feet_and_targets(lrm):
    targets, foot, quats, body = sc.synthetic(200, 6, seed=11, missing=0.0)
    nt = len(targets)
    foot[0, ::7], foot[1, 1::7], foot[2, 2::7], foot[3, 3::7] = -1, nt, np.iinfo(np.int32).min, np.iinfo(np.int32).max
    targets[foot[4, 4::9]] = np.nan
    targets[foot[5, 5::11], 1] = np.inf
    targets[foot[0, 6::13]] = -np.inf
    want = check(lrm, targets, foot, quats, body, com=[10.0, 0.0, 0.0], lift="each")
    assert (want["feet"] != 63).sum() > 60 and (want["feet"] == 63).any()


def test_bad_quaternions_bodies_and_pose_idx(lrm):
    targets, foot, quats, body = sc.synthetic(120, 6, seed=12, missing=0.02)
    quats[3, 1], quats[9, 0], quats[20] = np.nan, np.inf, quats[20] * F(1.7)
    quats[21] = 0
    # a zero com: the quaternion is never consulted, the stance stays live
    want = check(lrm, targets, foot, quats, body, lift="each")
    assert want["feet"][3] != 0 and want["feet"][9] != 0
    want0 = check(lrm, targets, foot, quats, body, com=[0.0, 0.0, 0.0], lift="each")
    assert np.array_equal(pc.bits(want0["margin"]), pc.bits(want["margin"]))
    # a non-zero com: nan and inf quaternions kill the stance, a non-unit one only scales the centre of mass
    want = check(lrm, targets, foot, quats, body, com=[30.0, 10.0, -5.0], lift="each")
    assert want["feet"][3] == 0 and want["feet"][9] == 0 and want["feet"][20] != 0 and np.isneginf(want["margin"][:, [3, 9]]).all()
    bad_b = body.copy()
    bad_b[5], bad_b[6, 0], bad_b[7, 2] = np.nan, np.inf, -np.inf
    want = check(lrm, targets, foot, quats, bad_b, com=[30.0, 10.0, -5.0], lift="each")
    assert (want["feet"][[5, 6, 7]] == 0).all()
    check(lrm, targets, foot, quats, None, com=[30.0, 10.0, -5.0])  # body NULL
    rng = np.random.default_rng(4)
    for pose_idx in (rng.permutation(120), rng.integers(0, 120, 120), np.full(120, 17)):
        check(lrm, targets, foot, quats, body, pose_idx.astype(np.int32), com=[30.0, 10.0, -5.0], lift="each")
    pi = np.arange(120, dtype=np.int32)
    pi[[0, 50]], pi[[1, 51]], pi[2] = -1, 120, np.iinfo(np.int32).min
    want = check(lrm, targets, foot, quats, body, pi, com=[30.0, 10.0, -5.0], lift="each")
    assert (want["feet"][[0, 1, 2, 50, 51]] == 0).all()
    # more stances than poses through pose_idx
    t2, f2, _, _ = sc.synthetic(500, 6, seed=13)
    check(lrm, t2, f2, quats, body, rng.integers(0, 120, 500).astype(np.int32), com=[30.0, 10.0, -5.0], lift="each")


def test_live_in_forms(lrm):
    targets, foot, quats, body = sc.synthetic(130, 6, seed=14)
    live = np.ones(130, np.uint8)
    live[::3], live[7] = 0, 200
    for lv in (None, np.ones(130, np.uint8), np.zeros(130, np.uint8), live):
        want = check(lrm, targets, foot, quats, body, com=[15.0, 5.0, 0.0], lift="each", live_in=lv)
        if lv is not None:
            assert (want["feet"][lv == 0] == 0).all() and np.isneginf(want["margin"][:, lv == 0]).all()


def test_plane_forms(lrm):
    targets, foot, quats, body = sc.synthetic(140, 6, seed=15)
    com = [25.0, -15.0, 10.0]
    a = check(lrm, targets, foot, quats, body, com=com, lift="each")
    b = check(lrm, targets, foot, quats, body, com=com, lift="each", plane=[[1, 0, 0], [0, 1, 0]])
    assert np.array_equal(pc.bits(a["margin"]), pc.bits(b["margin"])) and np.array_equal(a["edge"], b["edge"])
    t = np.deg2rad(20.0)  # gravity tilted about x by 20 degrees: u = x, v = (0, cos, sin)
    tilt = check(lrm, targets, foot, quats, body, com=com, lift="each", plane=[[1, 0, 0], [0, np.cos(t), np.sin(t)]])
    assert not np.array_equal(pc.bits(a["margin"]), pc.bits(tilt["margin"]))
    swap = check(lrm, targets, foot, quats, body, com=com, lift="each", plane=[[0, 1, 0], [1, 0, 0]])  # a mirrored basis turns the hull round
    assert (swap["stable"] == 1).any()


@pytest.mark.parametrize("min_margin", [0.0, 25.0])
def test_min_margin(lrm, main, min_margin):
    targets, foot, quats, body, legs = main
    want = check(lrm, targets, foot, quats, body, com=sc.COM, lift="each", min_margin=min_margin)
    between = (want["margin"] > 0) & (want["margin"] <= F(25.0))
    assert between.any() and (want["stable"][between] == (min_margin == 0.0)).all()


@pytest.mark.parametrize("name", sorted(sc.hand_made()))
def test_hand_made_stances(lrm, name):
    targets, foot, com, expect = sc.hand_made()[name]
    want = check(lrm, targets, foot, sc.IDENTITY, None, com=com)
    assert float(want["margin"][0, 0]) == expect["margin"] and int(want["edge"][0, 0]) == expect["edge"]
    assert int(want["stable"][0, 0]) == expect["stable"]
    check(lrm, targets, foot, sc.IDENTITY, None, com=com, lift=sc.lift_all(len(foot)))


def test_empty_cloud_no_stances_and_null_outputs(lrm):
    targets, foot, quats, body = sc.synthetic(40, 6, seed=16)
    want = check(lrm, np.zeros((0, 3), F), foot, quats, body, com=[1.0, 2.0, 3.0], lift="each")
    assert (want["feet"] == 0).all() and np.isneginf(want["margin"]).all()
    rc, m, e, st, ft = raw(lrm, targets, foot[:, :0], quats, body, None, None, None, [0], 0.0, None)  # nstances == 0: nothing is touched
    assert rc == 0 and (m == -7.0).all() and (ft == 0xA5).all()
    ref = sc.brute_np(targets, foot, quats, body, com=[1.0, 2.0, 3.0], lift=sc.lift_each(6))
    for kw in ({"edge": False}, {"feet": False}, {"edge": False, "feet": False}):
        rc, m, e, st, ft = raw(lrm, targets, foot, quats, body, None, [1.0, 2.0, 3.0], None, sc.lift_each(6), 0.0, None, **kw)
        assert rc == 0
        sc.assert_same((m, e if kw.get("edge", True) else None, st, ft if kw.get("feet", True) else None), ref)
        assert kw.get("edge", True) or (e == 0xA5).all()
        assert kw.get("feet", True) or (ft == 0xA5).all()
    margin, edge, stable, feet, ms = lrm.stance_stability_cpu(targets, foot, quats, body, com=[1.0, 2.0, 3.0], lift="each", want_edge=False,
                                                              want_feet=False)
    assert edge is None and feet is None and ms >= 0 and np.array_equal(pc.bits(margin), pc.bits(ref["margin"]))


def test_every_einval(lrm):
    targets, foot, quats, body = sc.synthetic(10, 6, seed=17)
    ok = dict(targets=targets, foot=foot, quats=quats, body=body, pose_idx=None, com=[1.0, 0.0, 0.0], plane=None, lift=[0, 1], min_margin=0.0,
              live_in=None)
    assert raw(lrm, **ok)[0] == 0
    big = 2 ** 31
    bad = [dict(nlegs=0), dict(nlegs=9), dict(lift=np.zeros(0, np.uint8)), dict(nposes=big), dict(nstances=big),
           dict(lift=[0, 64]), dict(lift=[128]), dict(lift=None), dict(min_margin=float("nan")), dict(min_margin=-1.0),
           dict(min_margin=float("inf")), dict(com=[np.nan, 0, 0]), dict(com=[0, np.inf, 0]), dict(plane=[1, 0, 0, 0, np.nan, 0]),
           dict(plane=[1, 0, 0, 0, 1, -np.inf]), dict(nposes=9), dict(foot=None), dict(quats=None, nposes=10), dict(margin=False),
           dict(stable=False)]
    for kw in bad:
        args = dict(ok)
        if kw.get("foot", 0) is None:  # a NULL foot array: through the C call with the sizes kept
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            m, st = np.zeros((2, 10), F), np.zeros((2, 10), np.uint8)
            lf = np.array([0, 1], np.uint8)
            rc = lrm.load().lrm_stance_stability_cpu(p(targets), len(targets), p(quats), p(body), 10, None, None, 10, 6, None, None, p(lf), 2, 0.0,
                                                     None, p(m), None, p(st), None, None)
        else:
            args.update(kw)
            rc = raw(lrm, **args)[0]
        assert rc == EINVAL, kw
    # nt past INT32_MAX and nmasks * nstances past 2^32 - 1 are refused before anything is read
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lf = np.zeros(256, np.uint8)
    L = lrm.load()
    assert L.lrm_stance_stability_cpu(p(targets), big, p(quats), p(body), 10, None, p(foot), 10, 6, None, None, p(lf), 1, 0.0, None, None, None, None, None, None) == EINVAL
    assert L.lrm_stance_stability_cpu(p(targets), 10, p(quats), p(body), 2 ** 25, None, p(foot), 2 ** 24, 6, None, None, p(lf), 256, 0.0, None, None, None, None, None, None) == EINVAL
    assert L.lrm_stance_stability_cpu(p(targets), 10, p(quats), p(body), 10, None, p(foot), 10, 6, None, None, p(lf), 257, 0.0, None, None, None, None, None, None) == EINVAL
    with pytest.raises(ValueError):
        lrm.stance_lift("all", 6)
    with pytest.raises(ValueError):
        lrm.stance_lift([256], 6)
    with pytest.raises(ValueError):
        lrm.stance_lift(np.zeros(257, np.uint8), 6)
    with pytest.raises(lrm.LrmError):
        lrm.stance_stability_cpu(targets, foot, quats, body, lift=[64])
    assert np.array_equal(lrm.stance_lift("each", 3), [0, 1, 2, 4]) and np.array_equal(lrm.stance_lift(None, 3), [0])


def test_agreement_with_the_float64_hull(lrm, main):
    """|margin - margin64| <= stance_model64.BAND["main"] (3e-4 mm: four times the worst that tests/test_stance_float64_cpu.py
    measures on this scene against the independent model, itself a wider comparison than this one, whose hull takes the restated
    float32 plane points) wherever both are finite and the relative coordinates stay below 2000 mm; stable agrees wherever
    margin64 is further than that from min_margin; -inf answers agree exactly.  Nothing is left out: the cap of 1 % is not used."""
    targets, foot, quats, body, legs = main
    lift = sc.lift_each(6)
    for min_margin in (0.0, 25.0):
        got = sc.host(lrm, targets, foot, quats, body, com=sc.COM, lift=lift, min_margin=min_margin)
        m64 = sc.margin64(targets, foot, quats, body, com=sc.COM, lift=lift)
        assert (sc.max_rel_coordinate(targets, foot, quats, body, com=sc.COM) < 2000.0).all()
        assert np.array_equal(np.isneginf(got["margin"]), np.isneginf(m64))
        fin = np.isfinite(m64)
        assert np.isfinite(got["margin"][fin]).all() and fin.mean() > 0.5
        diff = np.abs(got["margin"][fin].astype(np.float64) - m64[fin])
        print(f"worst |margin - margin64| = {diff.max():.3e} mm over {int(fin.sum())} answers (band {sm.BAND['main']:g})")
        assert diff.max() <= sm.BAND["main"]
        clear = np.abs(m64 - min_margin) > sm.BAND["main"]
        assert np.array_equal(got["stable"][clear], (m64 > min_margin)[clear].astype(np.uint8))
