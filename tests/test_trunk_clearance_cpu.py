"""Trunk-leg clearance on the host (no GPU): lrm_dbg_trunk_link_dist_host against trunk_clearance_cases.link_dist_np, the
numpy float32 restatement of include/lrm.h's link-to-cylinder distance, bit for bit; hand-made links whose distance has a
closed form; the float32 distance against tests/trunk_model64.py, the true minimum in float64 (checked on its own against a
4097-point grid), measured below and above per kind and asserted at four times the measured worst; the host loop
lrm_trunk_clearance_posed_cpu -- the reference of tests/test_gpu_trunk_clearance.py -- against trunk_clearance_cases.brute_np
bit for bit on every output and against the float64 model's rows wherever no decision lies inside the band; the consequences,
forms and refusals of the contract."""
import os
import re

import numpy as np
import pytest

import leg_clearance_cases as lc
import pair_cases as pc
import posed_cases
import self_clearance_cases as sc
import trunk_clearance_cases as tc
import trunk_model64 as t64

F = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged-robot-movability-cuda_amd", "csrc")


def legs6(lrm):
    return sc.legs_n(lrm, 6)


@pytest.fixture(scope="module")
def kinds():
    hm = tc.hand_made_links()
    A, B = tc.random_links()
    hm["random"] = (A, B, np.full(len(A), np.nan))
    return hm


@pytest.fixture(scope="module")
def d64(kinds):
    """the model's distance of every kind's links, computed once"""
    return {kind: t64.link_cyl_dist64(A, B, tc.CYL) for kind, (A, B, _) in kinds.items()}


@pytest.fixture(scope="module")
def main(lrm):
    """(quats, body, targets, legs, stance angles, IK status, trunk): leg_clearance_cases.main_scene under the chain's own
    choice, the trunk a cylinder a little beyond the legs' mounts"""
    legs = legs6(lrm)
    quats, body, targets = lc.main_scene(lrm)
    ang, st, _ = lc.stance_angles(lrm, targets, quats, body, legs)
    return quats, body, targets, legs, ang, st, tc.trunk_of(legs)


def check(lrm, quats, legs, angles, trunk, radius=tc.RADIUS, margin=tc.MARGIN, tip_clear=tc.TIP_CLEAR, links=tc.LINKS, pose_idx=None,
          live_in=None):
    """the host loop against the brute force, bit for bit, and the consequences -> the host's answer"""
    want = tc.host(lrm, quats, legs, angles, trunk, radius, margin, tip_clear, links, pose_idx, live_in)
    ns = want["links"].shape[1]
    _, live = sc.set_poses(len(quats), ns, pose_idx, live_in)
    brute = tc.brute_np(sc.joints_of_sets(lrm, angles, quats, legs, tip_clear, pose_idx), quats, radius, margin, trunk, links, pose_idx, live)
    tc.assert_same(tuple(want[k] for k in tc.KEYS), brute)
    tc.assert_consequences(want, margin, links, live)
    return want


def dist(lrm, A, B, cyl=tc.CYL):
    return lrm.dbg_trunk_link_dist_host(np.concatenate([A, B], 1), *cyl)


# ---- the link distance ----

def test_the_rounds_are_the_headers():
    src = open(os.path.join(CSRC, "lrm_trunk_clearance.h")).read()
    assert int(re.search(r"#define LRM_TRUNK_ROUNDS (\d+)", src).group(1)) == tc.ROUNDS == 32


def test_link_distance_is_the_contracts_bit_for_bit(lrm, kinds):
    which = np.zeros(3, int)
    for kind, (A, B, _) in kinds.items():
        d, w = tc.link_dist_np(A, B, tc.CYL, detail=True)
        assert np.array_equal(pc.bits(dist(lrm, A, B)), pc.bits(d)), kind
        assert (d >= 0).all() and max(np.abs(A).max(), np.abs(B).max()) <= 600.0
        which += np.bincount(w, minlength=3)
    # the least h is h(A), h(B) and a point of the search, each in thousands of links
    assert (which > 1000).all(), which
    A, B, _ = kinds["random"]
    other = (97.5, 12.0, -3.25)  # another cylinder: the scalars are read, not assumed
    assert np.array_equal(pc.bits(dist(lrm, A[:5000], B[:5000], other)), pc.bits(tc.link_dist_np(A[:5000], B[:5000], other)))


def test_link_distance_special_values(lrm):
    """exact answers about the cylinder R 150, z in [-30, 40]: inside 0, 3-4-5 to the rim, a side gap, a cap gap, a point"""
    g = np.array([[0, 0, 0, 10, 0, 0], [153, 0, 44, 153, 50, 44], [160, -50, 0, 160, 50, 0], [0, 0, 47, 100, 0, 47], [0, 0, -42, 0, 0, -42],
                  [-300, 0, 10, 300, 0, 10], [150, 0, 40, 200, 0, 90], [200, 0, 40, 150, 0, 40]], F)
    assert lrm.dbg_trunk_link_dist_host(g, *tc.CYL).tolist() == [0.0, 5.0, 10.0, 7.0, 12.0, 0.0, 0.0, 0.0]
    # a nan coordinate fails every comparison of h, so its term counts 0 (include/lrm.h says so; the posed call screens non-finite
    # joints before): whatever comes out is the restatement's, bit for bit
    bad = np.tile(g[1], (4, 1))
    bad[0, 0], bad[1, 4], bad[2, 2], bad[3, 5] = np.nan, np.nan, np.inf, -np.inf
    d = lrm.dbg_trunk_link_dist_host(bad, *tc.CYL)
    assert np.array_equal(pc.bits(d), pc.bits(tc.link_dist_np(bad[:, :3], bad[:, 3:], tc.CYL))) and d[0] == 4.0
    assert len(lrm.dbg_trunk_link_dist_host(np.zeros((0, 6), F), *tc.CYL)) == 0
    L = lrm.load()
    assert L.lrm_dbg_trunk_link_dist_host(None, 3, 1.0, 1.0, 0.0, None) == -1 and L.lrm_dbg_trunk_link_dist_host(None, 0, 1.0, 1.0, 0.0, None) == 0


def test_the_model_against_a_dense_grid_and_closed_forms(kinds, d64):
    """tests/trunk_model64.py on its own, before anything is measured with it: d64 <= the minimum over 4097 points of the
    link <= d64 + |B - A| / 4096 on every kind; and the hand-made kinds with a closed form -- which says which term of h
    decides (trunk_clearance_cases.hand_made_links) -- have that distance"""
    closed = 0
    for kind, (A, B, expect) in kinds.items():
        n = 200 if kind != "random" else 1000
        worst = t64.check_link_cyl_dist64(A[:n], B[:n], tc.CYL)
        have = np.isfinite(expect)
        err = float(np.abs(d64[kind] - expect)[have].max()) if have.any() else 0.0
        closed += int(have.sum())
        print(f"{kind}: grid minimum above the model's by at most {worst:.3g} mm; {int(have.sum())} closed forms, worst |d64 - closed| {err:.3g} mm")
        assert err <= 1e-7, kind
        assert have.all() == (kind in ("through_axis", "tangent_side", "crossing_cap", "parallel_inside", "parallel_outside", "in_cap_plane",
                                       "wholly_inside")), kind
    assert closed == 7 * 1500
    # each kind is what its name says, in the model's own terms
    d = d64
    assert (d["through_axis"] == 0).all() and (d["crossing_cap"] == 0).all() and (d["wholly_inside"] == 0).all()
    assert (d["tangent_side"] > 0).mean() > 0.95 and d["tangent_side"].max() < 61.0
    assert (d["nearest_rim"] > 0).mean() > 0.9
    assert 0.2 < (d["parallel_inside"] == 0).mean() < 0.8  # through the slab, and above or below it
    assert (d["parallel_outside"] > 0).mean() > 0.99
    assert 0.2 < (d["in_cap_plane"] == 0).mean() < 0.8
    A, B, _ = kinds["degenerate"]
    assert np.array_equal(A, B) and np.allclose(d["degenerate"], np.sqrt(t64.h64(A, tc.CYL)), rtol=0, atol=1e-12)


def test_link_distance_against_float64(lrm, kinds, d64):
    """d32 - d64 on the same float32 links, measured below (what float32 under-reports: the header's "never under-reports"
    holds up to rounding) and above (rounding, and what 32 rounds of the search leave) per kind; asserted at four times the
    measured worst, to one digit (DESIGN.md 3.21 has the table)"""
    for kind, (A, B, _) in kinds.items():
        e = dist(lrm, A, B).astype(np.float64) - d64[kind]
        above, below = float(e.max()), float((-e).max())
        print(f"{kind}: {len(A)} links, d32 - d64 above {max(above, 0.0):.3g} below {max(below, 0.0):.3g} mm "
              f"(bands {t64.BAND_KIND[kind][0]:g} / {t64.BAND_KIND[kind][1]:g})")
        assert above <= t64.BAND_KIND[kind][0] and below <= t64.BAND_KIND[kind][1], (kind, above, below)
        assert t64.BAND_KIND[kind][1] <= t64.BAND_LOW
    # the search itself, apart from float32: the same 32 rounds in float64 stay within 1e-7 mm of the true minimum
    A, B, _ = kinds["random"]
    e = tc.link_dist_np(A, B, tc.CYL, np.float64) - d64["random"]
    print(f"the search in float64: above {e.max():.3g} below {(-e).max():.3g} mm")
    assert e.max() <= 1e-7 and (-e).max() <= 1e-9


# ---- the host loop against the brute force ----

@pytest.mark.parametrize("links", [0b110, 0b111, 0])
@pytest.mark.parametrize("margin", [0.0, 10.0])
@pytest.mark.parametrize("angles", ["stance", "random"])
def test_host_loop_is_the_brute_force(lrm, main, angles, margin, links):
    quats, _, _, legs, ang, _, trunk = main
    if angles == "random":
        ang = lc.random_angles(len(quats), 6, seed=6)
    want = check(lrm, quats, legs, ang, trunk, tc.RADIUS, margin, tc.TIP_CLEAR, links)
    valid = np.isfinite(sc.joints_of_sets(lrm, ang, quats, legs, tc.TIP_CLEAR)).all((2, 3))
    if links == 0:
        assert (want["free"] == 1).all() and (want["worst"] == 255).all()
        return
    if links & 1:  # every coxa link starts on the trunk: d = 0, pen = its radius, and only a set without a valid leg is free
        assert np.array_equal((want["links"] & 1).astype(bool), valid) and np.array_equal(want["free"].astype(bool), ~valid.any(0))
        assert (want["worst"][valid] == 0).all() and (want["pen"][valid] == F(tc.RADIUS[0])).all()
    else:
        assert 0 < want["free"].sum() < len(quats)  # free and blocked sets both occur
        assert (want["links"] & 1 == 0).all()
        if margin:
            assert ((want["worst"] != 255) & (want["links"] == 0)).any()  # near without a hit
    assert ((want["links"] >> 1) & 1).any()  # a femur hit


def test_the_chain_calls_stances_through_the_trunk_feasible(lrm, main):
    """non-vacuity on the chain's own scene (the counts are in DESIGN.md 3.21): the chain's angles alone give free and blocked
    poses, femur hits and a tibia hit; the random family gives tens of tibia hits"""
    quats, _, _, legs, ang, st, trunk = main
    want = check(lrm, quats, legs, ang, trunk)
    rnd = check(lrm, quats, legs, lc.random_angles(len(quats), 6, seed=6), trunk)
    for name, w in (("chain", want), ("random", rnd)):
        print(f"{name}: {int((w['free'] == 0).sum())} of {len(quats)} poses have a leg in the trunk; femur hits "
              f"{int(((w['links'] >> 1) & 1).sum())}, tibia hits {int(((w['links'] >> 2) & 1).sum())}, near legs {int((w['worst'] != 255).sum())}")
        assert 0 < (w["free"] == 0).sum() < len(quats)
        assert ((w["links"] >> 1) & 1).any() and ((w["links"] >> 2) & 1).any()
    assert ((rnd["links"] >> 2) & 1).sum() >= 10
    # these stances passed the chain: the IK solved them
    assert np.isin(st.reshape(6, -1)[want["links"] != 0], (1, 2)).all()


def test_rows_against_the_float64_model(lrm, main):
    """the host loop's rows against trunk_model64 on joints from the leg's geometry: links, worst, pen and free are the model's
    wherever no float64 distance lies within BAND_TRUNK of a decision; at most 1 % of the links is left out (counted from the
    model alone); the distances themselves (numpy restatement on the library's joints) stay within BAND_TRUNK"""
    quats, _, _, legs, ang, _, trunk = main
    total = out = rows = 0
    worst = 0.0
    for angles in (ang, lc.random_angles(len(quats), 6, seed=6)):
        J64 = t64.body_joints64(angles, legs, quats, tc.TIP_CLEAR)
        for margin in (0.0, 10.0):
            m = t64.trunk_clearance64(J64, tc.RADIUS, margin, trunk, 0b111)
            tested = np.isfinite(m["d"])
            with np.errstate(invalid="ignore"):
                doubt = tested & ((np.abs(m["d"] - m["radius"]) <= t64.BAND_TRUNK) | (np.abs(m["d"] - m["reach"]) <= t64.BAND_TRUNK))
            total += int(tested.sum())
            out += int(doubt.sum())
            got = tc.host(lrm, quats, legs, angles, trunk, tc.RADIUS, margin, tc.TIP_CLEAR, 0b111)
            rows += t64.check_trunk_rows(got, m, t64.BAND_TRUNK)[0]
            assert ((m["links"] >> 1) & 1).any() and ((m["links"] >> 2) & 1).sum() >= (10 if angles is not ang else 1)
        b = tc.brute_np(sc.joints_of_sets(lrm, angles, quats, legs, tc.TIP_CLEAR), quats, tc.RADIUS, 0.0, trunk, 0b111, detail=True)
        ok = np.isfinite(b["d"])
        assert np.array_equal(np.isfinite(b["d"]), np.isfinite(m["d"]))
        worst = max(worst, float(np.abs(b["d"][ok].astype(np.float64) - m["d"][ok]).max()))
    print(f"{out} of {total} links within {t64.BAND_TRUNK} mm of a decision; {rows} rows compared; worst |d32 - d64| on the scene {worst:.3g} mm")
    assert total > 7000 and out <= 0.01 * total and rows > 3000
    assert worst <= t64.BAND_TRUNK


# ---- consequences and forms ----

def test_free_is_the_next_calls_live_in(lrm, main):
    """... -> ik -> trunk_clearance -> self_clearance(live_in = free): the sets the trunk blocks are dead there, the others
    have self_clearance's own answer"""
    quats, _, _, legs, ang, _, trunk = main
    free = check(lrm, quats, legs, ang, trunk)["free"]
    chained = sc.host(lrm, quats, legs, ang, live_in=free)
    alone = sc.host(lrm, quats, legs, ang)
    assert np.array_equal(chained["free"], alone["free"] & free) and (chained["worst"][:, free == 0] == 255).all()
    assert np.array_equal(chained["hits"][:, free == 1], alone["hits"][:, free == 1]) and 0 < chained["free"].sum() < free.sum()


def test_live_in_forms(lrm, main):
    quats, body, targets, legs, ang, _, trunk = main
    for name, lv in lc.live_forms(lrm, targets, quats, body, legs).items():
        want = check(lrm, quats, legs, ang, trunk, live_in=lv)
        if name == "zeros":
            assert (want["free"] == 0).all() and (want["worst"] == 255).all()
    threes = np.full(len(quats), 3, np.uint8)
    tc.assert_same(tuple(tc.host(lrm, quats, legs, ang, trunk, live_in=threes)[k] for k in tc.KEYS), tc.host(lrm, quats, legs, ang, trunk))
    lv = (np.arange(len(quats)) % 3 != 0).astype(np.uint8)
    assert np.array_equal(check(lrm, quats, legs, ang, trunk, links=0, live_in=lv)["free"], lv)  # links == 0: free = live


def test_pose_idx_forms(lrm, main):
    quats, _, _, legs, ang, _, trunk = main
    n = len(quats)
    rng = np.random.default_rng(3)
    base = tc.host(lrm, quats, legs, ang, trunk)
    ident = check(lrm, quats, legs, ang, trunk, pose_idx=np.arange(n, dtype=np.int32))
    tc.assert_same(tuple(ident[k] for k in tc.KEYS), base)
    rnd = lc.random_angles(n, 6, seed=8)
    check(lrm, quats, legs, rnd, trunk, pose_idx=rng.permutation(n).astype(np.int32))
    check(lrm, quats, legs, rnd, trunk, pose_idx=rng.integers(0, n, n).astype(np.int32))
    check(lrm, quats, legs, rnd, trunk, pose_idx=np.full(n, 17, np.int32))
    more = lc.random_angles(400, 6, seed=9)  # more sets than poses
    check(lrm, quats, legs, more, trunk, pose_idx=rng.integers(0, n, 400).astype(np.int32))
    for bad in (-1, n, np.iinfo(np.int32).min, np.iinfo(np.int32).max):
        pi = rng.permutation(n).astype(np.int32)
        at = [0, n // 2, n - 1]
        pi[at] = bad
        want = check(lrm, quats, legs, rnd, trunk, pose_idx=pi)
        assert (want["free"][at] == 0).all() and (want["worst"][:, at] == 255).all() and (np.delete(want["links"], at, 1) != 0).any()
    none = tc.host(lrm, np.zeros((0, 4), F), legs, more, trunk, pose_idx=np.zeros(400, np.int32))  # every set dead: no pose at all
    assert (none["free"] == 0).all() and (none["links"] == 0).all() and (none["worst"] == 255).all() and np.isneginf(none["pen"]).all()


def test_invalid_legs_get_the_empty_answer(lrm, main):
    quats, _, _, legs, ang, st, trunk = main
    n = len(quats)
    assert (st == 0).any() and np.isnan(ang[st == 0]).all()  # the stance angles hold legs without a foothold already
    a = lc.random_angles(n, 6, seed=10).reshape(6, n, 3)
    a[0, ::3, 0], a[2, 1::4, 1], a[5, ::5, 2] = np.nan, 120.0, -500.0
    a[3, 7], a[1, 9, 1], a[4, 13, 0] = np.inf, -120.0, 120.0
    a[:, 11] = np.nan  # no valid leg
    want = check(lrm, quats, legs, a.reshape(-1, 3), trunk, links=0b111)
    bad = ~np.isfinite(sc.joints_of_sets(lrm, a.reshape(-1, 3), quats, legs, tc.TIP_CLEAR)).all((2, 3))
    assert bad[0, ::3].all() and bad[2, 1::4].all() and bad[5, ::5].all() and bad[3, 7] and bad[1, 9] and bad[4, 13] and bad[:, 11].all()
    assert (want["links"][bad] == 0).all() and (want["worst"][bad] == 255).all() and want["free"][11] == 1
    assert (want["links"][~bad] & 1 == 1).all()
    # angles just inside +-120 are inside the sincos range: valid legs
    edge = lc.random_angles(n, 6, seed=11).reshape(6, n, 3)
    edge[1, ::2, 0], edge[2, ::3, 0], edge[4, ::5, 1] = 119.99, -119.99, 117.0
    w = check(lrm, quats, legs, edge.reshape(-1, 3), trunk, links=0b111)
    assert (w["links"] & 1 == 1).all()


def test_radius_zero_and_the_link_mask_switch_a_link_off(lrm, main):
    quats, _, _, legs, _, _, trunk = main
    rnd = lc.random_angles(len(quats), 6, seed=12)
    full = check(lrm, quats, legs, rnd, trunk, links=0b111)
    for k in range(3):
        r = list(tc.RADIUS)
        r[k] = 0.0
        by_radius = check(lrm, quats, legs, rnd, trunk, r, links=0b111)
        by_mask = check(lrm, quats, legs, rnd, trunk, links=0b111 & ~(1 << k))
        tc.assert_same(tuple(by_radius[key] for key in tc.KEYS), by_mask)
        assert ((by_mask["links"] >> k) & 1 == 0).all() and (by_mask["worst"] != k).all()
        assert np.array_equal(by_mask["links"], full["links"] & ~np.uint8(1 << k))
    none = check(lrm, quats, legs, rnd, trunk, (0.0, 0.0, 0.0), links=0b111)
    assert (none["free"] == 1).all() and (none["worst"] == 255).all()


def test_tip_clear_beyond_the_tibia_and_a_thin_or_flat_trunk(lrm, main):
    """T' = 0: the tibia link is a point at the knee; trunk_radius 0: the cylinder is a piece of the axis; a slab 1e-3 mm thick"""
    quats, _, _, legs, ang, _, trunk = main
    rnd = lc.random_angles(len(quats), 6, seed=13)
    check(lrm, quats, legs, rnd, trunk, tip_clear=1e4, links=0b111)
    check(lrm, quats, legs, ang, trunk, tip_clear=0.0)
    thin = check(lrm, quats, legs, rnd, (0.0, 40.0, -80.0), links=0b111)
    assert (thin["links"] == 0).all()
    check(lrm, quats, legs, rnd, (trunk[0], 0.001, 0.0), links=0b111)
    check(lrm, quats, legs, rnd, (300.0, 200.0, -200.0), margin=0.0)


@pytest.mark.parametrize("nlegs", range(1, 9))
def test_leg_counts(lrm, nlegs):
    legs = sc.legs_n(lrm, nlegs)
    n = 60
    quats = posed_cases.random_unit_quats(n, np.random.default_rng(nlegs))
    trunk = tc.trunk_of(legs)
    want = check(lrm, quats, legs, lc.random_angles(n, nlegs, seed=20 + nlegs), trunk, links=0b111)
    assert (want["links"] & 1 == 1).all()
    check(lrm, quats, legs, lc.random_angles(n, nlegs, seed=40 + nlegs), trunk)


def test_nonunit_and_nan_quaternions(lrm, main):
    _, _, _, legs, _, _, trunk = main
    n = 90
    rng = np.random.default_rng(14)
    quats = (posed_cases.random_unit_quats(n, rng) * rng.uniform(0.5, 2.0, (n, 1))).astype(F)
    quats[5, 1], quats[40], quats[77, 3] = np.nan, np.nan, np.inf
    want = check(lrm, quats, legs, lc.random_angles(n, 6, seed=15), trunk)
    assert (want["free"][[5, 40, 77]] == 1).all() and (want["worst"][:, [5, 40, 77]] == 255).all()  # no valid leg, the set stays live
    assert (want["links"] != 0).any()


def test_every_einval_and_the_null_forms(lrm, main):
    quats, _, _, legs, ang, _, trunk = main
    n = len(quats)
    base = tc.host(lrm, quats, legs, ang, trunk)
    for kw in ({"want_pen": False}, {"want_free": False}, {"want_pen": False, "want_free": False}):
        got = tc.host(lrm, quats, legs, ang, trunk, **kw)
        assert got["pen"] is None or "want_pen" not in kw
        assert got["free"] is None or "want_free" not in kw
        tc.assert_same(tuple(got[k] for k in tc.KEYS), base)
    for kw in ({"radius": (1.0, -1.0, 1.0)}, {"radius": (np.nan, 1.0, 1.0)}, {"radius": (1.0, 1.0, np.inf)}, {"margin": -1.0},
               {"margin": np.nan}, {"margin": np.inf}, {"tip_clear": -0.5}, {"tip_clear": np.nan}, {"tip_clear": np.inf},
               {"links": 8}, {"links": 0b1110}, {"links": 255}):
        with pytest.raises(lrm.LrmError):
            tc.host(lrm, quats, legs, ang, trunk, **kw)
    for bad in ((np.nan, 40.0, -80.0), (np.inf, 40.0, -80.0), (186.0, np.nan, -80.0), (186.0, np.inf, -80.0), (186.0, 40.0, np.nan),
                (186.0, 40.0, -np.inf), (-1.0, 40.0, -80.0), (186.0, -80.0, -80.0), (186.0, -80.0, 40.0)):
        with pytest.raises(lrm.LrmError):
            tc.host(lrm, quats, legs, ang, bad)
    with pytest.raises(lrm.LrmError):  # without pose_idx a set is a pose
        tc.host(lrm, quats[:100], legs, ang, trunk)
    for bad in (dict(pose_idx=np.zeros(n - 1, np.int32)), dict(live_in=np.zeros(n + 1, np.uint8)), dict(links=-1), dict(links=256)):
        with pytest.raises(ValueError):
            tc.host(lrm, quats, legs, ang, trunk, **bad)
    with pytest.raises(ValueError):
        lrm.trunk_clearance_posed_cpu(quats, legs, ang[:-1], tc.RADIUS, *trunk)
    # the C ABI's own checks, in its order
    L = lrm.load()
    q, lg, a, r = (np.ascontiguousarray(x, F) for x in (quats, legs, ang, tc.RADIUS))
    lk, ws = (np.zeros((6, n), np.uint8) for _ in range(2))
    ptr = lambda x: None if x is None else x.ctypes.data
    ok = dict(quats=q, nposes=n, legs=lg, nl=6, pose_idx=None, ns=n, angles=a, radius=r, R=186.0, pz=40.0, mz=-80.0, mask=6, links=lk, worst=ws)

    def rc(**kw):
        v = dict(ok, **kw)
        return L.lrm_trunk_clearance_posed_cpu(ptr(v["quats"]), v["nposes"], ptr(v["legs"]), v["nl"], ptr(v["pose_idx"]), v["ns"], ptr(v["angles"]),
                                               ptr(v["radius"]), 0.0, 0.0, v["R"], v["pz"], v["mz"], v["mask"], None, ptr(v["links"]),
                                               ptr(v["worst"]), None, None, None)

    assert rc() == 0
    big = 2 ** 31
    for kw in (dict(nl=0), dict(nl=9), dict(ns=big), dict(nposes=big), dict(ns=2 ** 30, nposes=2 ** 30, nl=8), dict(radius=None), dict(ns=n + 1),
               dict(R=float("nan")), dict(R=-0.5), dict(pz=-80.0), dict(mz=float("inf")), dict(mask=8),
               dict(quats=None), dict(legs=None), dict(angles=None), dict(links=None), dict(worst=None)):
        assert rc(**kw) == -1, kw
    assert rc(ns=0, angles=None, links=None) == 0  # nsets == 0 is a no-op
    assert rc(ns=0, mask=8) == -1 and rc(ns=0, pz=-80.0) == -1  # the scalars are checked before the no-op
    assert rc(R=0.0) == 0 and rc(mask=0) == 0


def test_symbols_are_declared_and_exported(lrm):
    names = {"lrm_trunk_clearance_posed_dev", "lrm_trunk_clearance_posed_cpu", "lrm_dbg_trunk_link_dist_host", "lrm_dbg_trunk_link_dist_dev"}
    assert names <= set(lrm.declared_symbols()) and names <= set(lrm.exported_symbols())
    for name in ("trunk_clearance_posed_cpu", "dbg_trunk_link_dist_host", "dbg_trunk_link_dist"):
        assert callable(getattr(lrm, name))
    assert callable(lrm.PoseSet.trunk_clearance) and callable(lrm.device.dbg_trunk_link_dist)
