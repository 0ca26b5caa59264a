"""The host side of the pair tests (tests/pair_cases.py): lrm_footholds_cpu against the brute force over the oracle on
every leg family, orientation and scene, so that the host loop is a trusted intermediate for the GPU cases too large
for the oracle; and the two culling bounds of the pair kernels (per-leg bounding sphere, body reach radius) against the
oracle's reachable set, wide coxa ranges and non-unit quaternions included.  Everything is exact: integers equal,
best_d2 equal bit for bit."""
import numpy as np
import pytest

import pair_cases as pc
from footholds_cases import oracle_reachable

FAMILIES = ["m2_1_identity", "m2_2_tilted", "m2_3_nonunit", "m2_5_identity", "m2_6_tilted", "m2_7_nonunit",
            "m2_8_identity", "moonbot_6_identity", "moonbot_3_tilted", "moonbot_5_nonunit", "random_8_identity",
            "random_7_tilted", "random_wide_3_nonunit", "random_2_tilted", "mixed_5_tilted", "mixed_2_identity"]


def assert_host_equals_brute(lrm, oracle, bodies, targets, legs, quat, nominal, both=True):
    want = pc.brute(oracle, bodies, targets, legs, quat, nominal)
    if both:
        pc.assert_both_outcomes(want)
    count, best, best_d2, _ = lrm.footholds_cpu(bodies, targets, legs, quat, nominal)
    assert np.array_equal(count, want["count"])
    assert np.array_equal(best, want["best"])
    assert np.array_equal(pc.bits(best_d2), pc.bits(want["best_d2"]))
    return want


def test_family_list_is_complete(lrm):
    assert sorted(FAMILIES) == sorted(pc.leg_families(lrm))
    assert {len(legs) for legs, _ in pc.leg_families(lrm).values()} >= {1, 2, 3, 5, 7, 8}


def test_reach_pairs_is_the_oracles_pair_test(oracle, lrm):
    """orc_reach_pairs = orc_reachable_rotate_leg per triple = orc_reach_any's any"""
    legs, q = pc.leg_families(lrm)["mixed_5_tilted"]
    bodies, targets = pc.rough(9, 700, seed=2)
    got = oracle.reach_pairs(bodies, targets, legs, q)
    assert np.array_equal(got.astype(bool), oracle_reachable(oracle, bodies, targets, legs, q))
    assert np.array_equal(got.max(-1), oracle.reach_any(bodies, targets, legs, q))
    assert 0 < got.mean() < 1


@pytest.mark.parametrize("family", FAMILIES)
def test_host_loop_matches_bruteforce_for_every_leg_family(lrm, oracle, family):
    legs, q = pc.leg_families(lrm)[family]
    bodies, targets = pc.rough(64, 4000, seed=len(family) + len(legs), density_half=700.0)
    for nominal in (None, pc.nominal_for(len(legs))):
        assert_host_equals_brute(lrm, oracle, bodies, targets, legs, q, nominal)


def test_mixed_family_holds_an_ineligible_leg_among_eligible_ones(lrm):
    fam = pc.leg_families(lrm)
    legs, q = fam["mixed_5_tilted"]
    ok = [pc.filter_eligible(lrm, leg, q) for leg in legs]
    assert not all(ok) and sum(ok) >= 3, ok
    assert not all(pc.filter_eligible(lrm, leg, fam["random_8_identity"][1]) for leg in fam["random_8_identity"][0])
    r2 = [float(pc.body_radius(leg)) for leg in legs]
    assert max(r2) > 4 * min(r2)  # short and long: the shared r2max is far from the short leg's own radius


@pytest.mark.parametrize("scene", ["dense_cluster", "sparse_tiles", "raster", "shuffled", "morton", "repeated",
                                   "duplicates"])
def test_host_loop_matches_bruteforce_on_every_scene(lrm, oracle, scene):
    legs, q = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6, seed=5)
    if scene == "dense_cluster":
        bodies, targets = pc.dense_cluster(40, 6000, seed=1)
        d2 = ((targets[None, :2048] - bodies[:, None]) ** 2).sum(-1)
        assert (d2[:, np.arange(2048) != 5] <= min(pc.body_radius(l) for l in legs)).all()  # all survive the radius test
    elif scene == "sparse_tiles":
        bodies, targets = pc.sparse_tiles(40, 9, seed=2)
    elif scene in ("raster", "shuffled", "morton"):
        bodies, clouds = pc.raster(lrm, 96, 60)
        targets = clouds[scene][0]
    else:
        bodies, base = pc.rough(40, 2500, seed=4, density_half=600.0)
        one = pc.brute(oracle, bodies, base, legs, q, nominal)
        if scene == "repeated":
            targets = pc.repeated(base, 3)
        else:
            targets, twin = pc.with_spread_duplicates(base, seed=6)
    want = assert_host_equals_brute(lrm, oracle, bodies, targets, legs, q, nominal)
    if scene == "repeated":
        assert np.array_equal(want["count"], 3 * one["count"]) and np.array_equal(want["best"], one["best"])
    if scene == "duplicates":
        assert np.array_equal(want["count"], 2 * one["count"])
        has = want["best"] >= 0
        assert (want["best"][has] < twin[want["best"][has]]).all()  # the smaller index of the two equal d2


def test_host_loop_on_bad_and_extreme_input(lrm, oracle):
    legs, q = pc.leg_families(lrm)["m2_5_identity"]
    bodies, targets = pc.rough(40, 3000, seed=8, density_half=600.0)
    nominal = pc.nominal_for(5)
    bad_t = targets.copy()
    bad_t[::7] = np.nan
    bad_t[3::11, 1] = np.inf
    bad_t[5::13] = -np.inf
    bad_t[1024:1088] = np.nan
    assert_host_equals_brute(lrm, oracle, bodies, bad_t, legs, q, nominal)
    bad_b = bodies.copy()
    bad_b[1] = np.nan
    bad_b[2, 0] = np.inf
    bad_b[3] = -np.inf
    bad_b[4, 2] = np.nan
    want = assert_host_equals_brute(lrm, oracle, bad_b, targets, legs, q, nominal)
    assert (want["count"][:, 1:5] == 0).all()
    # a nominal point 1e30 mm away: d2 = +inf for every target, the choice is the smallest reachable index
    huge = np.full((5, 3), 1e30, np.float32)
    want = assert_host_equals_brute(lrm, oracle, bodies, targets, legs, q, huge)
    has = want["count"] > 0
    assert np.isposinf(want["best_d2"]).all() and (want["best"][has] >= 0).all()
    first = pc.brute(oracle, bodies, targets, legs, q, None)
    assert np.array_equal(has, first["count"] > 0)
    reach = oracle.reach_pairs(bodies, targets, legs, q)
    assert np.array_equal(want["best"][has], np.argmax(reach, -1)[has])


@pytest.mark.parametrize("offset", [1e4, 1e5, 1e6, 4e6])
def test_host_loop_far_from_the_origin(lrm, oracle, offset):
    legs, q = pc.leg_families(lrm)["m2_6_tilted"]
    bodies, targets = pc.translated(*pc.rough(48, 4000, seed=9, density_half=700.0), offset)
    assert_host_equals_brute(lrm, oracle, bodies, targets, legs, q, pc.nominal_for(6))


# ---- the culling bounds ---------------------------------------------------------------------------------------------
def _bound_legs(lrm):
    """(leg, quat as the calls take them): the committed robots, narrow and wide random legs, the mixed set; identity,
    random non-unit and fixture non-unit quaternions"""
    rng = np.random.default_rng(78)
    legs = [lrm.get_M2_leg(a) for a in (0.0, 2.0943952, -1.0471976)] + [lrm.get_moonbot_leg(a) for a in (0.0, 1.5707964)]
    for k in range(12):
        coxa_deg = rng.uniform(95, 150) if k % 2 else rng.uniform(30, 94)
        legs.append(lrm.leg_factory(rng.uniform(-3, 3), rng.uniform(80, 250), rng.uniform(-60, 30), rng.uniform(30, 90),
                                    rng.uniform(90, 160), rng.uniform(90, 170), coxa_deg, rng.uniform(60, 100),
                                    rng.uniform(90, 140), rng.uniform(-20, 10), rng.uniform(-20, 10)))
    legs += [pc.short_leg(lrm, 0.4), pc.long_leg(lrm, -2.0), pc.wide_leg(lrm, 1.0), pc.wide_leg(lrm, -0.3, 175.0)]
    nonunit = pc.quats()["nonunit"]
    out = []
    for i, leg in enumerate(legs):
        q = (np.array([1, 0, 0, 0], np.float32), (rng.normal(size=4) + [3, 0, 0, 0]).astype(np.float32), nonunit)[i % 3]
        out.append((leg, q))
        out.append((lrm.rotate_leg_data(q, leg), q))  # as the footholds tests pass their legs
    return out


def test_pair_sphere_and_body_radius_contain_every_reachable_pair(lrm, oracle):
    """No (foothold - body) the oracle accepts lies outside the leg's bounding sphere (lrm_dbg_pair_sphere) or outside
    the body radius body + coxa + femur + tibia + 1 mm with its 1e-4 slack: dense samples of the radius' cube, coxa
    half-ranges up to 175 degrees (the whole-ball fallback), non-unit quaternions."""
    rng = np.random.default_rng(79)
    seen = wide_seen = 0
    for i, (leg, q) in enumerate(_bound_legs(lrm)):
        centre, r2 = lrm.dbg_pair_sphere(leg, q)
        rmax2 = float(pc.body_radius(leg))
        side = 1.15 * np.sqrt(rmax2)
        rel = rng.uniform(-side, side, (120_000, 3)).astype(np.float32)
        # reach(body, target) depends on target - body only: one target at the origin, bodies at -rel
        hit = oracle.reach_any(-rel, np.zeros((1, 3), np.float32), [leg], q)[0].astype(bool)
        r = rel[hit].astype(np.float64)
        assert (((r - centre) ** 2).sum(1) <= r2).all(), (i, "pair sphere")
        # the kernels' own float32 statement of the radius test
        d2 = rel[hit, 2] * rel[hit, 2] + (rel[hit, 1] * rel[hit, 1] + rel[hit, 0] * rel[hit, 0])
        assert (d2 <= np.float32(rmax2)).all(), (i, "body radius")
        seen += int(hit.sum())
        half_range = 0.5 * (float(leg[8]) - float(leg[9]))
        if half_range > np.deg2rad(87):
            wide_seen += int(hit.sum())
    assert seen > 20000 and wide_seen > 5000
