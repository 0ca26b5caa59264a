"""Leg-leg self clearance on the host (no GPU): lrm_dbg_link_pair_dist_host against self_clearance_cases.pair_dist_np, the
numpy float32 restatement of include/lrm.h's link-pair distance, bit for bit, and against the same formulas in float64; the
host loop lrm_self_clearance_posed_cpu -- the reference of tests/test_gpu_self_clearance.py -- against
self_clearance_cases.brute_np bit for bit on every output; what the call is for (crossing legs and shared footholds on the
chain's own scene); the consequences, forms and refusals of the contract."""
import numpy as np
import pytest

import leg_clearance_cases as lc
import pair_cases as pc
import posed_cases
import self_clearance_cases as sc

F = np.float32
BAND = 1e-2  # mm: the band of test_gpu_stance.py's float64 hull


def legs6(lrm):
    return sc.legs_n(lrm, 6)


@pytest.fixture(scope="module")
def pairs():
    hm = sc.hand_made_pairs()
    hm["random"] = sc.random_pairs()
    return hm


@pytest.fixture(scope="module")
def main(lrm):
    """(quats, body, targets, legs, stance angles, IK status, best): leg_clearance_cases.main_scene under the chain's own choice"""
    legs = legs6(lrm)
    quats, body, targets = lc.main_scene(lrm)
    ang, st, best = lc.stance_angles(lrm, targets, quats, body, legs)
    return quats, body, targets, legs, ang, st, best


def check(lrm, quats, legs, angles, radius=sc.RADIUS, margin=sc.MARGIN, tip_clear=sc.TIP_CLEAR, pose_idx=None, live_in=None):
    """the host loop against the brute force, bit for bit, and the consequences -> the host's answer"""
    want = sc.host(lrm, quats, legs, angles, radius, margin, tip_clear, pose_idx, live_in)
    ns = want["hits"].shape[1]
    _, live = sc.set_poses(len(quats), ns, pose_idx, live_in)
    brute = sc.brute_np(sc.joints_of_sets(lrm, angles, quats, legs, tip_clear, pose_idx), radius, margin, live)
    sc.assert_same(tuple(want[k] for k in sc.KEYS), brute)
    sc.assert_consequences(want, margin, live)
    return want


# ---- the pair distance ----

def test_pair_distance_is_the_contracts_bit_for_bit(lrm, pairs):
    taken, den_neg, fold = np.zeros(6, int), 0, np.zeros(4, int)
    for kind, g in pairs.items():
        d, det = sc.pair_dist_np(g, F, detail=True)
        assert np.array_equal(pc.bits(lrm.dbg_link_pair_dist_host(g)), pc.bits(d)), kind
        assert (d >= 0).all() and np.abs(g).max() <= 600.0
        taken += np.bincount(det["branch"], minlength=6)
        den_neg += int((det["general"] & ~det["den_pos"]).sum())
        fold += det["fold"].sum(0)
    # every branch of the distance is taken: the six cases of s and t, den <= 0 in the general case, each of the four folds
    assert (taken > 0).all(), dict(zip(sc.BRANCHES, taken))
    assert den_neg > 0 and (fold > 0).all(), (den_neg, fold)


def test_pair_distance_special_values(lrm):
    """exact answers: identical links 0, a 3-4-5 offset between parallel links, points; nan and inf coordinates give no number
    below any reach"""
    g = np.array([[0, 0, 0, 100, 0, 0, 0, 0, 0, 100, 0, 0], [0, 0, 0, 100, 0, 0, 20, 3, 4, 80, 3, 4], [1, 2, 3, 1, 2, 3, 1, 2, 15, 1, 2, 15],
                  [0, 0, 0, 10, 0, 0, 13, 4, 0, 50, 4, 0], [0, 0, 0, 0, 0, 100, -50, 0, 50, 50, 0, 50], [0, 0, 0, 0, 0, 100, -50, 6, 50, 50, 6, 50]], F)
    assert lrm.dbg_link_pair_dist_host(g).tolist() == [0.0, 5.0, 12.0, 5.0, 0.0, 6.0]
    bad = np.tile(g[1], (4, 1))
    bad[0, 0], bad[1, 7], bad[2, 5], bad[3, 9] = np.nan, np.nan, np.inf, -np.inf
    d = lrm.dbg_link_pair_dist_host(bad)
    with np.errstate(invalid="ignore"):
        assert not (d < F(3.0e38)).any()
    assert np.array_equal(np.isnan(d), np.isnan(sc.pair_dist_np(bad)))
    assert len(lrm.dbg_link_pair_dist_host(np.zeros((0, 12), F))) == 0


def test_pair_distance_against_float64(lrm, pairs):
    """the float32 distance stays within BAND of the same formulas in float64 (measured worst per kind: DESIGN.md 3.20)"""
    for kind, g in pairs.items():
        err = np.abs(lrm.dbg_link_pair_dist_host(g).astype(np.float64) - sc.pair_dist_np(g, np.float64))
        print(f"{kind}: worst |d32 - d64| = {err.max():.3g} mm over {len(g)} pairs")
        assert err.max() <= BAND, (kind, err.max())


# ---- the host loop against the brute force ----

@pytest.mark.parametrize("tip_clear", [0.0, 30.0])
@pytest.mark.parametrize("margin", [0.0, 10.0])
@pytest.mark.parametrize("angles", ["stance", "random"])
def test_host_loop_is_the_brute_force(lrm, main, angles, margin, tip_clear):
    quats, _, _, legs, ang, _, _ = main
    if angles == "random":
        ang = lc.random_angles(len(quats), 6, seed=6)
    want = check(lrm, quats, legs, ang, sc.RADIUS, margin, tip_clear)
    assert 0 < (want["hits"] > 0).sum() and 0 < want["free"].sum() < len(quats)
    if margin:
        assert ((want["worst"] != 255) & (want["hits"] == 0)).any()  # near without a hit


def test_the_chain_calls_colliding_stances_feasible(lrm, main):
    """non-vacuity on the chain's own scene: free and not-free live poses, at least three of the nine link kinds hit; a thick
    coxa link brings coxa bits"""
    quats, _, _, legs, ang, _, _ = main
    want = check(lrm, quats, legs, ang)
    blocked = int((want["free"] == 0).sum())
    print(f"{blocked} of {len(quats)} poses have a leg-leg hit")
    assert 0 < blocked < len(quats)
    brute = sc.brute_np(sc.joints_of_sets(lrm, ang, quats, legs, sc.TIP_CLEAR), sc.RADIUS, sc.MARGIN, detail=True)
    kinds = {(ka, kb) for _, _, ka, kb, d, ok, rr, _ in brute["pairs"] if (ok & (d < rr)).any()}
    assert len(kinds) >= 3, kinds
    assert (want["links"] & 1 == 0).all()  # no coxa link in a hit under the test radii
    thick = check(lrm, quats, legs, ang, sc.RADIUS_COXA)
    assert (thick["links"] & 1).any() and (thick["links"] & 6).any()


def test_shared_footholds_are_hits(lrm, main):
    """tip_clear 0: two valid legs of a pose that chose the same target touch there, and each has the other's bit"""
    quats, _, _, legs, ang, _, best = main
    want = check(lrm, quats, legs, ang, sc.RADIUS, 0.0, 0.0)
    valid = np.isfinite(ang.reshape(6, -1, 3)).all(2)
    shared = 0
    for i in range(6):
        for j in range(i + 1, 6):
            both = (best[i] == best[j]) & (best[i] >= 0) & valid[i] & valid[j]
            shared += int(both.sum())
            assert ((want["with"][i][both] >> j) & 1).all() and ((want["with"][j][both] >> i) & 1).all()
    print(f"{shared} leg pairs share a foothold")
    assert shared == 59  # measured on this seeded scene; another count means the scene changed


def test_hit_decisions_against_float64(lrm, main):
    """the library's float32 decisions against the float64 brute force: wherever the float64 gap d - rr is further than BAND
    from 0, the pair distance lrm_dbg_link_pair_dist_host decides d < rr as float64 does, and the host loop's `with` bit of a
    leg pair none of whose nine link pairs is in doubt is float64's; at most 1 % of the pairs is left out"""
    quats, _, _, legs, ang, _, _ = main
    total = out = legpairs = 0
    for angles in (ang, lc.random_angles(len(quats), 6, seed=6)):
        J = sc.joints_of_sets(lrm, angles, quats, legs, sc.TIP_CLEAR)
        b64 = sc.brute_np(J, sc.RADIUS, 0.0, T=np.float64, detail=True)
        want = sc.host(lrm, quats, legs, angles, sc.RADIUS, 0.0, sc.TIP_CLEAR)
        sure, hit64 = {}, {}
        for i, j, _, _, d64, ok, rr64, segs in b64["pairs"]:
            d = lrm.dbg_link_pair_dist_host(segs[ok])  # the library's float32 distance of the scene's own link pairs
            clear = np.abs(d64[ok] - rr64) > BAND
            assert np.array_equal((d < F(rr64))[clear], (d64[ok] < rr64)[clear])  # rr64 holds the float32 sum exactly
            total += int(ok.sum())
            out += int((~clear).sum())
            sure[i, j] = sure.get((i, j), True) & (~ok | (np.abs(d64 - rr64) > BAND))
            hit64[i, j] = hit64.get((i, j), False) | (ok & (d64 < rr64))
        for (i, j), s in sure.items():
            assert np.array_equal(((want["with"][i] >> j) & 1).astype(bool)[s], hit64[i, j][s])
            assert np.array_equal(((want["with"][j] >> i) & 1).astype(bool)[s], hit64[i, j][s])
            legpairs += int(s.sum())
        assert np.array_equal(want["free"].astype(bool)[np.all(list(sure.values()), 0)], (b64["hits"] == 0).all(0)[np.all(list(sure.values()), 0)])
    print(f"{out} of {total} pairs within {BAND} mm of the decision; {legpairs} leg pairs compared")
    assert total > 20000 and out <= 0.01 * total and legpairs > 4000


# ---- consequences and forms ----

def test_live_in_forms(lrm, main):
    quats, body, targets, legs, ang, _, _ = main
    for name, lv in lc.live_forms(lrm, targets, quats, body, legs).items():
        want = check(lrm, quats, legs, ang, live_in=lv)
        if name == "zeros":
            assert (want["free"] == 0).all() and (want["worst"] == 255).all()
    threes = np.full(len(quats), 3, np.uint8)
    sc.assert_same(tuple(sc.host(lrm, quats, legs, ang, live_in=threes)[k] for k in sc.KEYS), sc.host(lrm, quats, legs, ang))


def test_pose_idx_forms(lrm, main):
    quats, _, _, legs, ang, _, _ = main
    n = len(quats)
    rng = np.random.default_rng(3)
    base = sc.host(lrm, quats, legs, ang)
    ident = check(lrm, quats, legs, ang, pose_idx=np.arange(n, dtype=np.int32))
    sc.assert_same(tuple(ident[k] for k in sc.KEYS), base)
    rnd = lc.random_angles(n, 6, seed=8)
    check(lrm, quats, legs, rnd, pose_idx=rng.permutation(n).astype(np.int32))
    check(lrm, quats, legs, rnd, pose_idx=rng.integers(0, n, n).astype(np.int32))
    check(lrm, quats, legs, rnd, pose_idx=np.full(n, 17, np.int32))
    more = lc.random_angles(400, 6, seed=9)  # more sets than poses
    check(lrm, quats, legs, more, pose_idx=rng.integers(0, n, 400).astype(np.int32))
    for bad in (-1, n, np.iinfo(np.int32).min, np.iinfo(np.int32).max):
        pi = rng.permutation(n).astype(np.int32)
        at = [0, n // 2, n - 1]
        pi[at] = bad
        want = check(lrm, quats, legs, rnd, pose_idx=pi)
        assert (want["free"][at] == 0).all() and (want["worst"][:, at] == 255).all() and (np.delete(want["hits"], at, 1) > 0).any()
    # every set dead: no pose at all
    none = sc.host(lrm, np.zeros((0, 4), F), legs, more, pose_idx=np.zeros(400, np.int32))
    assert (none["free"] == 0).all() and (none["hits"] == 0).all() and (none["worst"] == 255).all() and np.isneginf(none["pen"]).all()


def test_invalid_legs_take_part_in_no_pair(lrm, main):
    quats, _, _, legs, ang, st, _ = main
    n = len(quats)
    assert (st == 0).any() and np.isnan(ang[st == 0]).all()  # the stance angles hold legs without a foothold already
    a = lc.random_angles(n, 6, seed=10).reshape(6, n, 3)
    a[0, ::3, 0], a[2, 1::4, 1], a[5, ::5, 2] = np.nan, 120.0, -500.0
    a[3, 7], a[1, 9, 1] = np.inf, -120.0
    a[:, 11] = np.nan  # no valid leg
    want = check(lrm, quats, legs, a.reshape(-1, 3))
    bad = ~np.isfinite(sc.joints_of_sets(lrm, a.reshape(-1, 3), quats, legs, sc.TIP_CLEAR)).all((2, 3))
    assert bad[0, ::3].all() and bad[2, 1::4].all() and bad[5, ::5].all() and bad[3, 7] and bad[1, 9] and bad[:, 11].all()
    assert (want["hits"][bad] == 0).all() and (want["worst"][bad] == 255).all() and want["free"][11] == 1
    for l in range(6):  # nobody has an invalid leg's bit
        assert (((want["with"] >> l) & 1)[:, bad[l]] == 0).all()
    assert (want["hits"][~bad] > 0).any()


def test_radius_zero_switches_a_link_off(lrm, main):
    quats, _, _, legs, ang, _, _ = main
    rnd = lc.random_angles(len(quats), 6, seed=12)
    full = check(lrm, quats, legs, rnd, sc.RADIUS_COXA)
    for k in range(3):
        r = list(sc.RADIUS_COXA)
        r[k] = 0.0
        want = check(lrm, quats, legs, rnd, r)
        assert ((want["links"] >> k) & 1 == 0).all() and ((want["worst"] != 255) <= ((want["worst"] % 9) // 3 != k)).all()
        assert (want["hits"] <= full["hits"]).all() and (want["hits"] > 0).any()
    none = check(lrm, quats, legs, rnd, (0.0, 0.0, 0.0))
    assert (none["free"] == 1).all() and (none["worst"] == 255).all()
    check(lrm, quats, legs, ang, (0.0, 0.0, 16.0))


def test_tip_clear_beyond_the_tibia(lrm, main):
    """T' = 0: the tibia link shrinks to the knee, a degenerate segment in every pair it takes part in"""
    quats, _, _, legs, ang, _, _ = main
    want = check(lrm, quats, legs, lc.random_angles(len(quats), 6, seed=13), tip_clear=1e4)
    assert (want["hits"] > 0).any()
    check(lrm, quats, legs, ang, tip_clear=1e4)


@pytest.mark.parametrize("nlegs", range(1, 9))
def test_leg_counts(lrm, nlegs):
    legs = sc.legs_n(lrm, nlegs)
    n = 60
    quats = posed_cases.random_unit_quats(n, np.random.default_rng(nlegs))
    want = check(lrm, quats, legs, lc.random_angles(n, nlegs, seed=20 + nlegs), sc.RADIUS_COXA)
    if nlegs == 1:
        assert (want["free"] == 1).all()
        lv = (np.arange(n) % 3 != 0).astype(np.uint8)
        assert np.array_equal(check(lrm, quats, legs, lc.random_angles(n, 1, seed=2), live_in=lv)["free"], lv)
    else:
        assert (want["hits"] > 0).any()


def test_nonunit_and_nan_quaternions(lrm, main):
    _, _, _, legs, _, _, _ = main
    n = 90
    rng = np.random.default_rng(14)
    quats = (posed_cases.random_unit_quats(n, rng) * rng.uniform(0.5, 2.0, (n, 1))).astype(F)
    quats[5, 1], quats[40], quats[77, 3] = np.nan, np.nan, np.inf
    want = check(lrm, quats, legs, lc.random_angles(n, 6, seed=15))
    assert (want["free"][[5, 40, 77]] == 1).all() and (want["worst"][:, [5, 40, 77]] == 255).all()  # no valid leg, the set stays live
    assert (want["hits"] > 0).any()


def test_every_einval_and_the_null_forms(lrm, main):
    quats, _, _, legs, ang, _, _ = main
    n = len(quats)
    base = sc.host(lrm, quats, legs, ang)
    for kw in ({"want_pen": False}, {"want_free": False}, {"want_pen": False, "want_free": False}):
        got = sc.host(lrm, quats, legs, ang, **kw)
        assert got["pen"] is None or "want_pen" not in kw
        assert got["free"] is None or "want_free" not in kw
        sc.assert_same(tuple(got[k] for k in sc.KEYS), base)
    for kw in ({"radius": (1.0, -1.0, 1.0)}, {"radius": (np.nan, 1.0, 1.0)}, {"radius": (1.0, 1.0, np.inf)}, {"margin": -1.0},
               {"margin": np.nan}, {"margin": np.inf}, {"tip_clear": -0.5}, {"tip_clear": np.nan}, {"tip_clear": np.inf}):
        with pytest.raises(lrm.LrmError):
            sc.host(lrm, quats, legs, ang, **kw)
    with pytest.raises(lrm.LrmError):  # without pose_idx a set is a pose
        sc.host(lrm, quats[:100], legs, ang)
    for bad in (dict(pose_idx=np.zeros(n - 1, np.int32)), dict(live_in=np.zeros(n + 1, np.uint8))):
        with pytest.raises(ValueError):
            sc.host(lrm, quats, legs, ang, **bad)
    with pytest.raises(ValueError):
        lrm.self_clearance_posed_cpu(quats, legs, ang[:-1], sc.RADIUS)
    # the C ABI's own checks, in its order
    L = lrm.load()
    q, lg, a, r = (np.ascontiguousarray(x, F) for x in (quats, legs, ang, sc.RADIUS))
    hits = np.zeros((6, n), np.int32)
    w, lk, ws = (np.zeros((6, n), np.uint8) for _ in range(3))
    ptr = lambda x: None if x is None else x.ctypes.data
    ok = dict(quats=q, nposes=n, legs=lg, nl=6, pose_idx=None, ns=n, angles=a, radius=r, hits=hits, with_=w, links=lk, worst=ws)

    def rc(**kw):
        v = dict(ok, **kw)
        return L.lrm_self_clearance_posed_cpu(ptr(v["quats"]), v["nposes"], ptr(v["legs"]), v["nl"], ptr(v["pose_idx"]), v["ns"], ptr(v["angles"]),
                                              ptr(v["radius"]), 0.0, 0.0, None, ptr(v["hits"]), ptr(v["with_"]), ptr(v["links"]), ptr(v["worst"]),
                                              None, None, None)

    assert rc() == 0
    big = 2 ** 31
    for kw in (dict(nl=0), dict(nl=9), dict(ns=big), dict(nposes=big), dict(ns=2 ** 30, nposes=2 ** 30, nl=8), dict(radius=None), dict(ns=n + 1),
               dict(quats=None), dict(legs=None), dict(angles=None), dict(hits=None), dict(with_=None), dict(links=None), dict(worst=None)):
        assert rc(**kw) == -1, kw
    assert rc(ns=0, angles=None, hits=None) == 0  # nsets == 0 is a no-op
    assert L.lrm_dbg_link_pair_dist_host(None, 3, None) == -1 and L.lrm_dbg_link_pair_dist_host(None, 0, None) == 0


def test_symbols_are_declared_and_exported(lrm):
    names = {"lrm_self_clearance_posed_dev", "lrm_self_clearance_posed_cpu", "lrm_dbg_link_pair_dist_host", "lrm_dbg_link_pair_dist_dev"}
    assert names <= set(lrm.declared_symbols()) and names <= set(lrm.exported_symbols())
    for name in ("self_clearance_posed_cpu", "dbg_link_pair_dist_host", "dbg_link_pair_dist"):
        assert callable(getattr(lrm, name))
    assert callable(lrm.PoseSet.self_clearance) and callable(lrm.device.dbg_link_pair_dist)
