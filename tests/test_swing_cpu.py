"""Swing-foot transit on the host (no GPU): lrm_swing_transit_posed_cpu, the serial unculled loop that the GPU tests compare
with bit for bit, tied to things that are not its own code:

* the reach outputs to lrm_reach_dist_posed_cpu, one query per (edge, leg, sample), on a pose table made of
  lrm_dbg_edge_transit_samples_host's sample poses with the feet restated in numpy float32 from include/lrm.h (mask and d2 bit
  for bit);
* the degenerate step (lift = 0, from == to, foot_radius = 0) to lrm_edge_transit_posed_cpu, bit for bit;
* the terrain outputs to tests/swing_model64.py, an independent float64 model of the path and of the point-to-polyline
  distance: hits and hit segments agree wherever the float64 distance is further than BAND from foot_radius;
* hand-made steps whose answers are known; non-vacuity of the main scene; every refusal and every no-op."""
import numpy as np
import pytest

import swing_cases as sw
import swing_model64 as m64
import transit_cases as tr

F = np.float32

# |d32 - d64| of the host loop on the corpus of test_the_band_is_measured (12 seeds x S in 2, 3, 5, 9, 33, 64 x 64 entries: steps
# of 0 to 600 mm, footholds up to 4e6 mm from the origin, lifts of -40 to 250 mm, probes 0 to 120 mm from the path): the worst
# is 1.3008e-5 mm (a probe 0.0096 mm from a 64-sample path 285 m from the origin; typical figures are 3e-6 to 9e-6).  d32 is
# read off the host loop itself: with foot_radius = 1e-30 and margin = 1e30 every target is near and pen = -d exactly.
# BAND is four times the measured worst: rounding grows with the coordinates and the corpus is finite.
MEASURED = 1.3008e-5
BAND = 4 * MEASURED  # 5.2e-5 mm; tests/test_gpu_swing.py holds the device to the host loop bit for bit, and so to the same band


@pytest.fixture(scope="module")
def main(lrm):
    return sw.main_scene(lrm)


@pytest.fixture(scope="module")
def every(lrm):
    return sw.all_legs_scene(lrm)


# ---- the reach part against existing calls --------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [2, 3, 5, 9, 33, 64])
def test_reach_outputs_are_reach_dist_on_the_restated_feet(lrm, every, S):
    quats, body, targets, ea, eb, legs, ffrom, fto = every
    for lift, up in ((0.0, None), (20.0, None), (-35.0, None), (80.0, [0.3, -0.1, 0.9])):
        want = sw.brute_reach(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, S, lift, up)
        got = sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, S, lift=lift, up=up)
        sw.assert_same(got, want, sw.REACH_KEYS + ("swinging",))
        if S > 2 and lift == 20.0:  # entries that keep the foot and entries that lose it
            swg = want["reached"] >= 0
            assert (swg & (want["reached"] == S)).any() and (swg & (want["reached"] < S)).any()


def test_reach_outputs_with_live_in_bad_indices_and_no_body(lrm, every):
    quats, body, targets, ea, eb, legs, ffrom, fto = every
    live = (np.arange(len(ea)) % 3 != 1).astype(np.uint8)
    f, t = sw.hostile_feet(ffrom, fto, len(targets))
    a, b = tr.hostile_edges(ea, eb, len(quats), [0, 7, 20, 47])
    for bd in (body, None):
        want = sw.brute_reach(lrm, targets, quats, bd, legs, a, b, f, t, 9, 20.0, None, live)
        got = sw.host(lrm, targets, quats, bd, legs, a, b, f, t, 9, live, lift=20.0, **{k: v for k, v in sw.MAIN.items() if k != "lift"})
        sw.assert_same(got, want, sw.REACH_KEYS + ("swinging",))
        sw.assert_consistent(got, 9)
        dead = ~tr.live_of(len(quats), a, b, live)
        assert dead.any() and (got["clear"][dead] == 0).all() and (got["swinging"][dead] == 0).all()


@pytest.mark.parametrize("S", [2, 3, 9, 64])
def test_the_degenerate_step_is_edge_transit(lrm, main, S):
    """lift = 0, from == to, foot_radius = 0: every reach output is lrm_edge_transit_posed_cpu's with foot = from, bit for bit"""
    quats, body, targets, ea, eb, legs, _, _ = main
    foot, _ = tr.foot_of(lrm, targets, quats, body, legs, sw.pc.nominal_for(6), ea, eb)
    foot = tr.hostile_feet(foot, len(targets))
    want = tr.host(lrm, targets, quats, body, legs, ea, eb, foot, S)
    for up in (None, [0.5, 0.5, -2.0]):
        got = sw.host(lrm, targets, quats, body, legs, ea, eb, foot, foot, S, up=up)
        for k in sw.REACH_KEYS:
            assert np.array_equal(np.asarray(got[k]).view(np.uint8), np.asarray(want[k]).view(np.uint8)), k
        assert np.array_equal(got["swinging"], want["planted"]) and np.array_equal(got["clear"], want["clear"])
        assert (got["hits"] == 0).all() and (got["hit_seg"] == -1).all() and (got["near"] == -1).all() and (got["pen"] == -np.inf).all()
    assert ((want["reached"] >= 0) & (want["reached"] < S)).any() or S == 2


# ---- hand-made steps ------------------------------------------------------------------------------------------------------

def flat(lrm, targets, ffrom, fto, S, **kw):
    """one pose, one leg, one edge per entry of ffrom"""
    n = len(ffrom)
    quats = np.array([[1, 0, 0, 0]], F)
    z = np.zeros(n, np.int32)
    return sw.host(lrm, np.asarray(targets, F), quats, None, lrm.get_M2_leg(F(0.5)), z, z, np.asarray(ffrom, np.int32)[None, :],
                   np.asarray(fto, np.int32)[None, :], S, **kw)


def test_known_answers_on_a_straight_step(lrm):
    """a 100 mm step along x at S = 5: segments [0, 25], [25, 50], [50, 75], [75, 100]"""
    T = [[0, 0, 0], [100, 0, 0],  # 0 from, 1 to
         [50, 5, 0],              # 2: 5 mm off the joint of segments 1 and 2: the first is 1
         [50, -5, 0],             # 3: as deep as 2: the tie goes to 2
         [10, 0, 3],              # 4: 3 mm off segment 0: the deepest, and the first segment hit when skip = 0
         [90, 12, 0],             # 5: 12 mm off segment 3: near (margin), not hit
         [130, 0, 0],             # 6: 30 mm past the landing: neither
         [0, 0, 0], [100, 0, 0]]  # 7, 8: copies of the footholds: tested (only the indices from and to are not) and 0 mm off
    o = flat(lrm, T[:7], [0], [1], 5, foot_radius=10.0, margin=5.0)
    assert (o["hits"][0, 0], o["hit_seg"][0, 0], o["near"][0, 0], o["pen"][0, 0], o["clear"][0]) == (3, 0, 4, F(7.0), 0)
    o = flat(lrm, T[:7], [0], [1], 5, foot_radius=10.0, margin=5.0, skip=1)  # segment 0 and 3 are out: 4 is 15.3 mm off segment 1
    assert (o["hits"][0, 0], o["hit_seg"][0, 0], o["near"][0, 0], o["pen"][0, 0]) == (2, 1, 2, F(5.0))
    o = flat(lrm, T[:7], [0], [1], 5, foot_radius=4.0, margin=0.0)  # only 4 is inside 4 mm
    assert (o["hits"][0, 0], o["hit_seg"][0, 0], o["near"][0, 0], o["pen"][0, 0]) == (1, 0, 4, F(1.0))
    o = flat(lrm, T[:7], [0], [1], 5, foot_radius=2.0, margin=1.5)  # 4 is near and not hit: pen < 0
    assert (o["hits"][0, 0], o["hit_seg"][0, 0], o["near"][0, 0], o["pen"][0, 0]) == (0, -1, 4, F(-1.0))
    o = flat(lrm, T[:7], [0], [1], 5, foot_radius=2.0, margin=0.0)
    assert (o["hits"][0, 0], o["hit_seg"][0, 0], o["near"][0, 0], o["pen"][0, 0]) == (0, -1, -1, F(-np.inf))
    o = flat(lrm, T, [0], [1], 5, foot_radius=10.0, margin=5.0)  # the copies are hit at pen = radius; the smaller index wins
    assert (o["hits"][0, 0], o["hit_seg"][0, 0], o["near"][0, 0], o["pen"][0, 0]) == (5, 0, 7, F(10.0))
    # lifted 40 mm the middle of the path clears 2 and 3 (P_2 = (50, 0, 40)); 4 stays 3 mm off the take-off point ... which skip = 1 leaves out
    o = flat(lrm, T[:7], [0], [1], 5, lift=40.0, foot_radius=10.0, margin=0.0, skip=1)
    assert (o["hits"][0, 0], o["near"][0, 0]) == (0, -1)
    # lift and put down: from == to, the path goes up and comes back; a target 20 mm above the foothold is hit by a 30 mm lift
    T2 = [[0, 0, 0], [0, 0, 20], [15, 0, 0]]
    o = flat(lrm, T2, [0], [0], 5, lift=30.0, foot_radius=2.0, margin=0.0)
    assert (o["hits"][0, 0], o["near"][0, 0], o["pen"][0, 0]) == (1, 1, F(2.0))
    o = flat(lrm, T2, [0], [0], 5, lift=30.0, up=[1, 0, 0], foot_radius=2.0, margin=0.0)  # up is used as given
    assert (o["hits"][0, 0], o["near"][0, 0], o["pen"][0, 0]) == (1, 2, F(2.0))


# ---- the float64 model ----------------------------------------------------------------------------------------------------

def measure(lrm, seeds, sizes, n=64):
    worst = 0.0
    for seed in seeds:
        for S in sizes:
            T, lift, up = m64.corpus(n, seed)
            idx = 3 * np.arange(n, dtype=np.int32)
            o = flat(lrm, T, idx, idx + 1, S, lift=lift, up=up, foot_radius=1e-30, margin=1e30)
            assert (o["near"] >= 0).all()
            for e in range(n):
                d32 = -float(o["pen"][0, e])  # fl(1e-30 - d) = -d
                path = m64.path64(T[3 * e], T[3 * e + 1], S, lift, up)[0]
                d64 = m64.segment_dist64(path, T[[o["near"][0, e], 3 * e + 2]]).min(1)  # the deepest target, and the entry's own probe
                assert d64[0] <= d64[1] + BAND  # as deep as the probe, in the model too
                worst = max(worst, abs(d32 - d64[0]))
    return worst


def test_the_band_is_measured(lrm):
    worst = measure(lrm, range(12), (2, 3, 5, 9, 33, 64))
    print("largest |d32 - d64|:", worst, "band:", BAND)
    assert worst <= MEASURED * 1.0001  # the figure written above is this corpus's
    assert worst > 1e-7  # float32 distances, not the model's own
    assert measure(lrm, range(100, 102), (4, 17, 63)) <= BAND  # and a corpus it was not measured on stays inside the band


def model_check(lrm, scene, S, lift, up, foot_radius, margin, skip):
    """the host loop against the float64 model on one scene -> (pairs within 2 x foot_radius, those inside the band)"""
    quats, body, targets, ea, eb, legs, ffrom, fto = scene
    o = sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, S, lift=lift, up=up, foot_radius=foot_radius, margin=margin, skip=skip)
    sw.assert_consistent(o, S)
    ks = np.array(list(m64.tested(S, skip)))
    close = inside = exact = 0
    for l, e in np.argwhere(o["reached"] >= 0):
        d = m64.entry64(targets, ffrom[l, e], fto[l, e], S, lift, up, skip)
        close += int((d < 2 * foot_radius).sum())
        doubt = np.abs(d - foot_radius) <= BAND
        inside += int(doubt.sum())
        sure = d < foot_radius - BAND
        lo, hi = int(sure.any(1).sum()), int((sure | doubt).any(1).sum())
        assert lo <= o["hits"][l, e] <= hi, (l, e)
        if not doubt.any():  # nothing within the band: hits and the hit segment are the model's
            exact += 1
            assert o["hits"][l, e] == lo
            assert o["hit_seg"][l, e] == (ks[np.argmax(sure.any(0))] if lo else -1), (l, e)
        # the deepest near target: within the band as deep as the model's deepest, and its pen the model's
        dmin = d.min(1)
        if o["near"][l, e] >= 0:
            i = o["near"][l, e]
            assert abs((foot_radius - dmin[i]) - float(o["pen"][l, e])) <= BAND + 1e-6 * foot_radius
            assert dmin[i] <= dmin.min() + 2 * BAND
        else:
            assert dmin.min() >= F(foot_radius + margin) - BAND
    assert exact > 0
    return close, inside


@pytest.mark.parametrize("S", [3, 5, 9, 33, 64])
def test_hits_and_hit_segments_against_the_float64_model(lrm, main, every, S):
    close = inside = 0
    for scene in (main, every) if S <= 9 else (main,):  # every leg of every edge, or the one lifted leg per edge
        for kw in (sw.MAIN, dict(lift=45.0, up=[0.2, 0.1, 0.95], foot_radius=20.0, margin=0.0, skip=0)):
            skip = kw["skip"] if 2 * kw["skip"] < S - 1 else 0  # S = 3 has two segments: both are tested
            c, i = model_check(lrm, scene, S, kw["lift"], kw.get("up"), kw["foot_radius"], kw["margin"], skip)
            close, inside = close + c, inside + i
    print(S, "pairs within 2 x foot_radius:", close, "inside the band:", inside)
    assert close > 1000 and inside <= 0.01 * close  # the corpus lets the model decide


def test_the_model_far_from_the_origin(lrm, main):
    """the main scene 4e6 mm away: the path is formed about A, so the band holds there too"""
    quats, body, targets, ea, eb, legs, ffrom, fto = main
    shift = np.array([4e6, -3e6, 1e6], F)
    scene = (quats, (body + shift).astype(F), (targets + shift).astype(F), ea, eb, legs, ffrom, fto)
    c, i = model_check(lrm, scene, 9, **{**sw.MAIN, "up": None})
    assert c > 100 and i <= 0.01 * c


# ---- non-vacuity ----------------------------------------------------------------------------------------------------------

def test_the_main_scene_has_every_class(lrm, main):
    quats, body, targets, ea, eb, legs, ffrom, fto = main
    o = sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, 9, **sw.MAIN)
    sw.assert_consistent(o, 9)
    swg = o["reached"] >= 0
    has = swg.any(0)
    by_reach, by_terrain = (swg & (o["reached"] < 9)).any(0), (swg & (o["hits"] > 0)).any(0)
    classes = {"clear": has & (o["clear"] == 1), "reach only": by_reach & ~by_terrain, "terrain only": ~by_reach & by_terrain,
               "both": by_reach & by_terrain}
    print({k: int(v.sum()) for k, v in classes.items()})
    for k, v in classes.items():
        assert v.sum() >= 1, k
    assert np.array_equal(o["clear"] == 1, ~by_reach & ~by_terrain)  # every edge of the scene is live
    assert (swg & (o["hits"] == 0)).any() and (swg & (o["hits"] > 0)).any()
    assert (o["pen"][swg & (o["near"] >= 0)] < 0).any()  # near without a hit occurs
    assert (swg.sum(0) <= 1).all() and (has.sum() >= 30)  # one lifted leg per edge


# ---- refusals and no-ops --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,skip", [(2, 1), (3, 1), (9, 4), (9, 63), (33, 16), (64, 32), (64, 63), (5, 2)])
def test_a_skip_that_leaves_no_segment_tests_nothing(lrm, main, S, skip):
    quats, body, targets, ea, eb, legs, ffrom, fto = main
    kw = {**sw.MAIN, "foot_radius": 500.0}
    o = sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, S, **{**kw, "skip": skip})
    assert (o["hits"] == 0).all() and (o["hit_seg"] == -1).all() and (o["near"] == -1).all() and (o["pen"] == -np.inf).all()
    sw.assert_same(o, sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, S, lift=kw["lift"]), sw.REACH_KEYS + sw.EDGE_KEYS)
    if 2 * (skip - 1) < S - 1:  # one less leaves a segment, and 500 mm hit something
        o = sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, S, **{**kw, "skip": skip - 1})
        assert (o["hits"] > 0).any() and (o["hit_seg"][o["hits"] > 0] >= skip - 1).all() and (o["hit_seg"] < S - 1 - (skip - 1)).all()


def test_foot_radius_zero_tests_nothing(lrm, main):
    quats, body, targets, ea, eb, legs, ffrom, fto = main
    o = sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, 9, lift=20.0, foot_radius=0.0, margin=1e6)
    assert (o["hits"] == 0).all() and (o["near"] == -1).all() and (o["pen"] == -np.inf).all()
    swg = o["reached"] >= 0
    assert np.array_equal(o["clear"] == 1, ~(swg & (o["reached"] < 9)).any(0))


def test_nonfinite_targets_quaternions_and_bodies(lrm, main):
    (quats, body, targets, ea, eb, legs, ffrom, fto), bad = sw.nonfinite_scene(main)
    l, e = zip(*bad)
    for S in (3, 9, 64):
        o = sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, S, **sw.MAIN)
        sw.assert_consistent(o, S)
        sw.assert_same(o, sw.brute_reach(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, S, sw.MAIN["lift"]), ("mask", "reached", "first_miss", "swinging"))
        for k in range(3):  # a non-finite tested path point: the empty terrain answer, and the reach part decides
            assert o["reached"][l[k], e[k]] >= 0 and o["hits"][l[k], e[k]] == 0 and o["near"][l[k], e[k]] == -1
            assert o["clear"][e[k]] == (o["reached"][l[k], e[k]] == S)
    # with skip the non-finite END is not a tested point: S = 9, skip = 1 tests P_1 .. P_7, and P_7 = 7/8 D is infinite all the same
    o = sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, 9, **sw.MAIN)
    assert o["hits"][l[1], e[1]] == 0


def test_indices_of_every_kind(lrm, every):
    quats, body, targets, ea, eb, legs, ffrom, fto = every
    nt = len(targets)
    for bad in (-1, nt, sw.I32.min, sw.I32.max, nt + 1, -2):
        for which in (0, 1):
            f, t = ffrom.copy(), fto.copy()
            (f, t)[which][::2, ::3] = bad
            o = sw.host(lrm, targets, quats, body, legs, ea, eb, f, t, 5, **sw.MAIN)
            sw.assert_consistent(o, 5)
            out = ((f < 0) | (f >= nt) | (t < 0) | (t >= nt))
            assert np.array_equal(o["reached"] == -1, out) and (o["mask"][out] == 0).all() and (o["worst_d2"][out] == 0).all()
    a, b = tr.hostile_edges(ea, eb, len(quats), range(0, 48, 5))
    o = sw.host(lrm, targets, quats, body, legs, a, b, ffrom, fto, 5, **sw.MAIN)
    dead = ~tr.live_of(len(quats), a, b)
    assert dead.sum() == 10 and (o["reached"][:, dead] == -1).all() and (o["clear"][dead] == 0).all() and (o["swinging"][dead] == 0).all()
    # nt == 0 lets nothing swing; an edge without a swinging leg is clear
    o = sw.host(lrm, np.zeros((0, 3), F), quats, body, legs, ea, eb, ffrom, fto, 5, **sw.MAIN)
    assert (o["reached"] == -1).all() and (o["swinging"] == 0).all() and (o["clear"] == 1).all()


def test_every_optional_pointer_null(lrm, main):
    quats, body, targets, ea, eb, legs, ffrom, fto = main
    full = sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, 9, **sw.MAIN)
    for kw in ({"want_mask": False}, {"want_worst": False}, {"want_pen": False}, {"want_edge": False},
               {"want_mask": False, "want_worst": False, "want_pen": False, "want_edge": False}):
        got = sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, 9, **sw.MAIN, **kw)
        assert sum(v is None for v in got.values()) == sum({"want_mask": 1, "want_worst": 2, "want_pen": 1, "want_edge": 2}[k] for k in kw)
        sw.assert_same(got, full)
    sw.assert_same(sw.host(lrm, targets, quats, None, legs, ea, eb, ffrom, fto, 9, **sw.MAIN),
                   sw.host(lrm, targets, quats, np.zeros_like(body), legs, ea, eb, ffrom, fto, 9, **sw.MAIN))
    sw.assert_same(sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, 9, up=[0, 0, 1], **sw.MAIN), full)


def test_refusals_in_their_order(lrm, main):
    quats, body, targets, ea, eb, legs, ffrom, fto = main
    L = lrm.load()
    buf = np.zeros(4096, np.int32)
    d = buf.ctypes.data
    up3 = np.array([0, 0, 1], F)
    nan, inf = float("nan"), float("inf")

    def raw(nt=4, nposes=1, nlegs=2, nedges=1, S=9, lift=10.0, up=up3.ctypes.data, fr=5.0, margin=1.0, skip=0, tg=d, qs=d, lgs=legs.ctypes.data,
            a=d, b=d, ff=d, ft=d, rc=d, fm=d, hi=d, hs=d, nr=d):
        rc_ = L.lrm_swing_transit_posed_cpu(tg, nt, qs, None, nposes, lgs, nlegs, a, b, nedges, ff, ft, S, lift, up, fr, margin, skip, None,
                                            None, rc, fm, None, None, hi, hs, nr, None, None, None, None)
        return rc_, L.lrm_last_error().decode()

    assert raw()[0] == 0
    bad_up = [np.array(v, F) for v in ([nan, 0, 1], [0, inf, 1], [0, 0, -inf])]
    for kw in ({"nlegs": 0}, {"nlegs": 9}, {"S": 1}, {"S": 65}, {"nt": 2 ** 31}, {"nposes": 2 ** 31}, {"nedges": 2 ** 31, "nlegs": 2},
               {"lift": nan}, {"lift": inf}, {"lift": -inf}, {"fr": nan}, {"fr": inf}, {"margin": nan}, {"margin": inf}, {"fr": -1.0},
               {"margin": -1e-30}, {"skip": 64}, {"skip": 2 ** 32 - 1}, *({"up": u.ctypes.data} for u in bad_up),
               {"qs": None}, {"lgs": None}, {"a": None}, {"b": None}, {"ff": None}, {"ft": None}, {"rc": None}, {"fm": None}, {"hi": None},
               {"hs": None}, {"nr": None}, {"tg": None}):
        assert raw(**kw)[0] == -1, kw
    # the order: edge_transit's range checks, then the scalars, all before the nedges == 0 no-op and the NULL checks
    assert "nlegs" in raw(nlegs=0, lift=nan, nedges=0)[1]
    assert "nsamples" in raw(S=1, fr=-1.0, skip=99)[1]
    assert "finite" in raw(lift=nan, fr=-1.0, skip=99, up=bad_up[0].ctypes.data, qs=None)[1]
    assert ">= 0" in raw(fr=-1.0, skip=99, up=bad_up[0].ctypes.data, qs=None)[1]
    assert "skip" in raw(skip=99, up=bad_up[0].ctypes.data, qs=None)[1]
    assert "up" in raw(up=bad_up[0].ctypes.data, qs=None, nedges=0)[1]
    assert raw(nedges=0, fr=-1.0)[0] == -1 and raw(nedges=0, skip=64)[0] == -1
    assert raw(nedges=0, qs=None, a=None, rc=None, hi=None, tg=None)[0] == 0  # then the no-op
    assert raw(nt=0, tg=None)[0] == 0 and raw(up=None)[0] == 0 and raw(skip=63, S=64)[0] == 0 and raw(fr=0.0, margin=0.0, lift=-1e30)[0] == 0
    with pytest.raises(ValueError):
        sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom[:5], fto, 9)
    with pytest.raises(ValueError):
        sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, 9, up=[0, 1])
    with pytest.raises(ValueError):
        sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, 9, skip=64)
    with pytest.raises(lrm.LrmError):
        sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, 9, foot_radius=-1.0)


def test_swing_layout_on_host_tensors(lrm):
    """device.swing_layout is tensor operations only: on CPU tensors it is swing_cases.lift_one, and a bad end swings nothing"""
    import torch
    rng = np.random.default_rng(0)
    best = rng.integers(-1, 50, (6, 20)).astype(np.int32)
    ea, eb = rng.integers(0, 20, 33).astype(np.int32), rng.integers(0, 20, 33).astype(np.int32)
    ea[3], eb[5], ea[7] = -1, 20, sw.I32.max
    ok = (ea >= 0) & (ea < 20) & (eb >= 0) & (eb < 20)
    layout = lambda m: [x.numpy() for x in lrm.swing_layout(torch.from_numpy(best), torch.from_numpy(ea), torch.from_numpy(eb), torch.from_numpy(m))]
    f, t = layout((1 << (np.arange(33) % 6)).astype(np.uint8))
    wf, wt = sw.lift_one(best, ea, eb)
    wf[:, ~ok], wt[:, ~ok] = -1, -1
    assert np.array_equal(f, wf) and np.array_equal(t, wt) and f.dtype == np.int32
    masks = rng.integers(0, 256, 33).astype(np.uint8)
    f, t = layout(masks)
    on = ((masks[None, :] >> np.arange(6)[:, None]) & 1).astype(bool) & ok[None, :]
    assert np.array_equal(f, np.where(on, best[:, np.clip(ea, 0, 19)], -1)) and np.array_equal(t, np.where(on, best[:, np.clip(eb, 0, 19)], -1))
    with pytest.raises(ValueError):
        lrm.swing_layout(torch.from_numpy(best), torch.from_numpy(ea), torch.from_numpy(eb), torch.from_numpy(masks[:-1]))
