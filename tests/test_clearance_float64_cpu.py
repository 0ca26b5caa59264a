"""Leg and self clearance on the host (no GPU) against tests/leg_model64.py, a float64 model written from the leg's geometry
and not from the library: where the four joints are (lrm_leg_joints_posed_cpu against joints64), that d is the distance from a
target to a link and that the link-pair distance is the distance between two links (true minima, the latter checked on its own
against a dense grid), and that the rows of lrm_leg_clearance_posed_cpu and lrm_self_clearance_posed_cpu are the model's
wherever no decision lies inside the measured band.  Every test prints what it measured; the bands asserted are the constants of
leg_model64 (four times the measured worst, one significant digit), shared with tests/test_gpu_clearance_float64.py.

Domain: unit quaternions (ik_cases.is_unit); a non-unit quaternion scales lengths, and the bit-for-bit tests cover those.
The caps on what doubt may hide -- at most 1 % of the decisions and 2 % of the rows -- and the non-vacuity counts are taken
from the float64 model alone, before the library is consulted."""
import numpy as np
import pytest

import ik_cases
import leg_clearance_cases as lc
import leg_model64 as m64
import posed_cases
import self_clearance_cases as sc

F = np.float32
TIP_CLEARS = (0.0, 30.0, 1e4)  # none, the scenes', beyond every tibia (T' = 0)
SELF_MARGIN_WIDE = 40.0  # legs stand further from each other than from the terrain: the margin under which a tenth of the main
#                          scene's legs is near another leg without touching it


def cap(name, skipped, total, share):
    print(f"{name}: {skipped} of {total} in doubt ({100.0 * skipped / max(total, 1):.3f} %, cap {100 * share:g} %)")
    assert total > 0 and skipped <= share * total, (name, skipped, total)


def assert_not_vacuous(name, hit, near, min_rows=400):
    """of the live valid rows at least 10 % have hits, 10 % are near without a hit, 10 % have nothing near"""
    n = len(hit)
    shares = float(hit.mean()), float((near & ~hit).mean()), float((~near).mean())
    print(f"{name}: {n} live valid rows: {100 * shares[0]:.1f} % hit, {100 * shares[1]:.1f} % near only, {100 * shares[2]:.1f} % clear")
    assert n >= min_rows and min(shares) >= 0.10, (name, n, shares)


# ---- the model's own distance functions ----

def test_point_link_dist64_special_values():
    A, B = np.array([0.0, 0, 0]), np.array([10.0, 0, 0])
    q = np.array([[5, 3, 4], [-3, 4, 0], [13, 0, 4], [0, 0, 0], [10, 0, 0], [2, 0, 0]], float)
    assert np.allclose(m64.point_link_dist64(q, A, B), [5, 5, 5, 0, 0, 0], rtol=0, atol=1e-15)
    assert np.allclose(m64.point_link_dist64(q, A, A), np.linalg.norm(q, axis=1), rtol=0, atol=1e-15)  # a link that is a point


def test_link_link_dist64_against_a_dense_grid():
    """the model's segment-segment distance is checked on its own, before anything is measured with it: exact answers, and
    every kind of pair against the minimum over a 257 x 257 grid of both parameters, the grid's gap bounded by its spacing"""
    g = np.array([[0, 0, 0, 100, 0, 0, 0, 0, 0, 100, 0, 0], [0, 0, 0, 100, 0, 0, 20, 3, 4, 80, 3, 4], [1, 2, 3, 1, 2, 3, 1, 2, 15, 1, 2, 15],
                  [0, 0, 0, 10, 0, 0, 13, 4, 0, 50, 4, 0], [0, 0, 0, 0, 0, 100, -50, 0, 50, 50, 0, 50], [0, 0, 0, 0, 0, 100, -50, 6, 50, 50, 6, 50],
                  [0, 0, 0, 10, 0, 0, 12, 0, 0, 20, 0, 0], [0, 0, 0, 10, 0, 0, 5, 0, 0, 20, 0, 0], [0, 0, 0, 10, 0, 0, 10, 0, 0, 10, 7, 0]], float)
    d = m64.link_link_dist64(g[:, 0:3], g[:, 3:6], g[:, 6:9], g[:, 9:12])
    assert np.allclose(d, [0, 5, 12, 5, 0, 6, 2, 0, 0], rtol=0, atol=1e-13)
    kinds = sc.hand_made_pairs(n=60, seed=17)
    kinds["random"] = sc.random_pairs(n=120, seed=19)
    assert {"crossing", "parallel", "nearly_parallel", "collinear", "touching", "one_degenerate", "both_degenerate"} <= set(kinds)
    for kind, segs in kinds.items():
        worst = m64.check_link_link_dist64(segs)
        # symmetric in the two links and in each link's direction
        a, b, c, e = segs[:, 0:3], segs[:, 3:6], segs[:, 6:9], segs[:, 9:12]
        d = m64.link_link_dist64(a, b, c, e)
        assert np.allclose(d, m64.link_link_dist64(c, e, b, a), rtol=1e-12, atol=1e-10)
        print(f"{kind}: {len(segs)} pairs, grid minimum above the model's by at most {worst:.3g} mm")


# ---- the joints ----

def joint_cases(lrm):
    return ik_cases.standard_cases(lrm) + ik_cases.random_legs(lrm)


def stance_angles_of(lrm, leg, quat, n, seed):
    """angles from the host IK on a cloud round the leg: the rows the IK solved (reached, or nearest within the limits)"""
    pts = ik_cases.random_cloud(n, seed)
    ang, st, _ = lrm.apply_ik_cpu(pts, leg, quat)
    ok = np.isin(st, (1, 2)) & np.isfinite(ang).all(1)
    return np.ascontiguousarray(ang[ok], F)


@pytest.mark.parametrize("tip_clear", TIP_CLEARS)
def test_joints_against_the_float64_model(lrm, tip_clear):
    """lrm_leg_joints_posed_cpu against joints64 (+ body), each of J0..J3 on its own: the coxa end and the knee are where a leg
    of these dimensions has them, and T' shortens the leg along the tibia"""
    worst = np.zeros(4)
    rows = 0
    rng = np.random.default_rng(5)
    for k, (name, leg, quat) in enumerate(joint_cases(lrm)):
        assert ik_cases.is_unit(quat), name
        legs = np.asarray(leg, F).reshape(1, 14)
        stance = stance_angles_of(lrm, leg, quat, 300, seed=k)
        assert len(stance) > 50, name
        for ang in (stance, lc.random_angles(200, 1, seed=k)):
            n = len(ang)
            quats = np.tile(np.asarray(quat, F), (n, 1))
            body = rng.uniform(-1500.0, 1500.0, (n, 3)).astype(F)
            want = m64.joints64(ang, leg, quat, tip_clear)
            for b in (None, body):
                got = lrm.leg_joints_posed_cpu(ang, quats, b, legs, tip_clear)[0][0].astype(np.float64)
                ref = want if b is None else want + body.astype(np.float64)[:, None, :]
                worst = np.maximum(worst, np.abs(got - ref).max((0, 2)))
            rows += n
        if tip_clear >= 1e4:  # the tibia link is a point at the knee
            assert np.array_equal(want[:, 3], want[:, 2])
    print(f"tip_clear {tip_clear:g}: {rows} (angle, leg) rows; worst |J_host - J64| per joint J0..J3 = "
          + ", ".join(f"{w:.3g}" for w in worst) + f" mm (band {m64.BAND_J:g})")
    assert m64.BAND_J <= ik_cases.TOL
    assert (worst <= m64.BAND_J).all(), worst


def test_the_tibia_is_what_tip_clear_shortens(lrm):
    """geometry, from the library's joints alone: |J1 - J0| = coxa, |J2 - J1| = femur, |J3 - J2| = T', and J3 lies on the line
    from the knee to the foot"""
    for k, (name, leg, quat) in enumerate(joint_cases(lrm)[::5]):
        legs = np.asarray(leg, F).reshape(1, 14)
        ang = lc.random_angles(100, 1, seed=40 + k)
        quats = np.tile(np.asarray(quat, F), (100, 1))
        foot = lrm.leg_joints_posed_cpu(ang, quats, None, legs, 0.0)[0][0].astype(np.float64)
        J = lrm.leg_joints_posed_cpu(ang, quats, None, legs, 30.0)[0][0].astype(np.float64)
        T = float(legs[0, ik_cases.TIBIA_LEN])
        lens = np.linalg.norm(np.diff(J, axis=1), axis=2)
        want = [float(legs[0, ik_cases.COXA_LEN]), float(legs[0, ik_cases.FEMUR_LEN]), m64.tibia_short(leg, 30.0)]
        assert np.abs(lens - want).max() <= 2 * m64.BAND_J, (name, np.abs(lens - want).max())
        assert np.abs(J[:, :3] - foot[:, :3]).max() <= 2 * m64.BAND_J  # coxa, femur and knee do not move
        on_line = foot[:, 2] + (foot[:, 3] - foot[:, 2]) * (want[2] / T)
        assert np.abs(J[:, 3] - on_line).max() <= 3 * m64.BAND_J, (name, np.abs(J[:, 3] - on_line).max())


# ---- point to link: the decisions and the rows of lrm_leg_clearance_posed_cpu ----

@pytest.fixture(scope="module")
def main(lrm):
    """leg_clearance_cases.main_scene under the chain's own choice, and under angles from no IK"""
    legs = sc.legs_n(lrm, 6)
    quats, body, targets = lc.main_scene(lrm)
    assert all(ik_cases.is_unit(q) for q in quats)
    stance = lc.stance_angles(lrm, targets, quats, body, legs)[0]
    return {"legs": legs, "quats": quats, "body": body, "targets": targets,
            "angles": {"stance": stance, "random": lc.random_angles(len(quats), 6, seed=6)}}


@pytest.fixture(scope="module")
def leg_models(main):
    """(angles, margin) -> the float64 model on joints64, computed once and left unchanged"""
    cache = {}

    def get(angles, margin, tip_clear=lc.TIP_CLEAR):
        key = (angles, margin, tip_clear)
        if key not in cache:
            J = m64.joints64_posed(main["angles"][angles], main["legs"], main["quats"], tip_clear)
            cache[key] = m64.leg_clearance64(main["targets"], main["body"], J, lc.RADIUS, margin)
        return cache[key]
    return get


@pytest.mark.parametrize("angles", ["stance", "random"])
def test_point_link_decisions_against_float64(lrm, main, leg_models, angles):
    """brute_np's float32 d of every (leg, pose, link, target) against the true point-segment distance, on the same float32
    joints and on joints64; outside BAND_D of r_k and of r_k + margin the hit and near decisions are float64's"""
    model = leg_models(angles, lc.MARGIN)
    doubt = m64.leg_doubt(model, m64.BAND_D)
    tested = np.broadcast_to(model["valid"][:, :, None, None], doubt.shape)
    cap(f"decisions[{angles}]", int((doubt & tested).sum()), int(tested.sum()), 0.01)
    J32 = lc.joints_from_fk(lrm, main["angles"][angles], main["quats"], None, main["legs"], lc.TIP_CLEAR)
    assert np.array_equal(np.isfinite(J32).all((2, 3)), model["valid"])
    brute = lc.brute_np(main["targets"], main["body"], J32, lc.RADIUS, lc.MARGIN, detail=True)
    same = m64.leg_clearance64(main["targets"], main["body"], J32, lc.RADIUS, lc.MARGIN)
    d32 = brute["d"].astype(np.float64)
    assert np.array_equal(np.isinf(d32), np.isinf(model["d"]))  # inf marks what was not computed, in both
    e_same, e_model = np.abs(d32[tested] - same["d"][tested]), np.abs(d32[tested] - model["d"][tested])
    close = model["d"][tested] < 2 * model["reach"].max()
    print(f"[{angles}] {int(tested.sum())} decisions: worst |d32 - d64| on the same float32 joints {e_same.max():.3g} mm, on joints64 "
          f"{e_model.max():.3g} mm ({e_model[close].max():.3g} within twice the reach); band {m64.BAND_D:g}")
    assert e_same.max() <= m64.BAND_D and e_model.max() <= m64.BAND_D
    r, reach = model["radius"].astype(F)[None, None, :, None], model["reach"].astype(F)[None, None, :, None]
    sure = tested & ~doubt
    assert np.array_equal((brute["d"] < r)[sure], model["hit"][sure])
    assert np.array_equal((brute["d"] < reach)[sure], model["near"][sure])


@pytest.mark.parametrize("margin", [0.0, lc.MARGIN])
@pytest.mark.parametrize("angles", ["stance", "random"])
def test_leg_clearance_rows_against_float64(lrm, main, leg_models, angles, margin):
    model = leg_models(angles, margin)
    v = model["valid"]
    if angles == "stance" and margin > 0:
        assert_not_vacuous("leg_clearance main scene", (model["hits"] > 0)[v], model["near_any"][v])
    rows_in_doubt = int((v & m64.leg_doubt(model, m64.BAND_D).any((2, 3))).sum())
    cap(f"rows[{angles}, margin {margin:g}]", rows_in_doubt, int(v.sum()), 0.02)
    got = lc.host(lrm, main["targets"], main["quats"], main["body"], main["legs"], main["angles"][angles], lc.RADIUS, margin, lc.TIP_CLEAR)
    compared, skipped = m64.check_leg_rows(got, model, m64.BAND_D)
    assert skipped == rows_in_doubt and compared + skipped == int(v.sum())


@pytest.mark.parametrize("tip_clear", [0.0, 1e4])
def test_leg_clearance_rows_under_other_tip_clear(lrm, main, leg_models, tip_clear):
    """tip_clear 0: the stance's own foothold touches the tibia's end; beyond the tibia: the tibia link is the knee"""
    model = leg_models("stance", lc.MARGIN, tip_clear)
    cap(f"rows[tip_clear {tip_clear:g}]", int((model["valid"] & m64.leg_doubt(model, m64.BAND_D).any((2, 3))).sum()), int(model["valid"].sum()), 0.02)
    got = lc.host(lrm, main["targets"], main["quats"], main["body"], main["legs"], main["angles"]["stance"], lc.RADIUS, lc.MARGIN, tip_clear)
    m64.check_leg_rows(got, model, m64.BAND_D)
    assert (model["hits"] > 0).any()


# ---- link to link: the pair distance and the rows of lrm_self_clearance_posed_cpu ----

def test_all_pairs_is_the_kinds():
    hm = sc.hand_made_pairs()
    assert set(hm) | {"random"} == set(m64.BAND_KIND)
    assert len(sc.all_pairs()) == sum(len(g) for g in hm.values()) + len(sc.random_pairs())


def test_pair_distance_against_the_true_minimum(lrm):
    """lrm_dbg_link_pair_dist_host on self_clearance_cases.all_pairs() against link_link_dist64 on the same float32 segments:
    never below the true minimum by more than BAND_PAIR_LOW (the header's one-sided promise), and above it by at most the
    kind's band (what the clamped step over-reports after the four folds)"""
    kinds = sc.hand_made_pairs()
    kinds["random"] = sc.random_pairs()
    allp = sc.all_pairs()
    d32 = lrm.dbg_link_pair_dist_host(allp).astype(np.float64)
    at = 0
    for kind, g in kinds.items():
        assert np.array_equal(allp[at:at + len(g)], g)
        d = d32[at:at + len(g)]
        at += len(g)
        d64 = m64.link_link_dist64(g[:, 0:3], g[:, 3:6], g[:, 6:9], g[:, 9:12])
        under, over = float((d64 - d).max()), float((d - d64).max())
        print(f"{kind}: {len(g)} pairs; d32 below the true minimum by at most {max(under, 0.0):.3g} mm (band {m64.BAND_PAIR_LOW:g}), above by at most "
              f"{max(over, 0.0):.3g} mm (band {m64.BAND_KIND[kind]:g})")
        assert under <= m64.BAND_PAIR_LOW, (kind, under)
        assert over <= m64.BAND_KIND[kind], (kind, over)
    assert at == len(allp)
    assert max(m64.BAND_KIND.values()) <= ik_cases.TOL and m64.BAND_SELF <= ik_cases.TOL and m64.BAND_D <= ik_cases.TOL


def self_scene(lrm, main, angles, margin, tip_clear=sc.TIP_CLEAR, radius=sc.RADIUS):
    ang = main["angles"][angles]
    model = m64.self_clearance64(m64.joints64_posed(ang, main["legs"], main["quats"], tip_clear), radius, margin)
    return ang, model


@pytest.mark.parametrize("angles", ["stance", "random"])
def test_pair_decisions_on_the_scene_against_float64(lrm, main, angles):
    """the library's distance of the scene's own link pairs (its float32 joints) against the model's (joints64)"""
    ang, model = self_scene(lrm, main, angles, sc.MARGIN)
    J32 = sc.joints_of_sets(lrm, ang, main["quats"], main["legs"], sc.TIP_CLEAR)
    total = out = 0
    worst = 0.0
    for i, j, ka, kb, d64, ok, rr, reach in model["pairs"]:
        doubt = (np.abs(d64 - rr) <= m64.BAND_SELF) | (np.abs(d64 - reach) <= m64.BAND_SELF)
        total += int(ok.sum())
        out += int((ok & doubt).sum())
    cap(f"pair decisions[{angles}]", out, total, 0.01)
    for i, j, ka, kb, d64, ok, rr, reach in model["pairs"]:
        segs = np.concatenate([J32[i, :, ka], J32[i, :, ka + 1], J32[j, :, kb], J32[j, :, kb + 1]], 1)[ok]
        d = lrm.dbg_link_pair_dist_host(segs)
        worst = max(worst, float(np.abs(d.astype(np.float64) - d64[ok]).max()))
        sure = ~((np.abs(d64 - rr) <= m64.BAND_SELF) | (np.abs(d64 - reach) <= m64.BAND_SELF))[ok]
        assert np.array_equal((d < F(rr))[sure], (d64[ok] < rr)[sure])
        assert np.array_equal((d < F(reach))[sure], (d64[ok] < reach)[sure])
    print(f"[{angles}] {total} link pairs: worst |d32 on the library's joints - d64 on joints64| = {worst:.3g} mm (band {m64.BAND_SELF:g})")
    assert total > 10000 and worst <= m64.BAND_SELF


@pytest.mark.parametrize("margin", [0.0, sc.MARGIN, SELF_MARGIN_WIDE])
@pytest.mark.parametrize("angles", ["stance", "random"])
def test_self_clearance_rows_against_float64(lrm, main, angles, margin):
    ang, model = self_scene(lrm, main, angles, margin)
    v = model["valid"]
    if angles == "stance" and margin == SELF_MARGIN_WIDE:
        assert_not_vacuous("self_clearance main scene, wide margin", (model["hits"] > 0)[v], (model["worst"] != 255)[v])
    in_doubt = int((v & m64.self_doubt(model, m64.BAND_SELF)).sum())
    cap(f"self rows[{angles}, margin {margin:g}]", in_doubt, int(v.sum()), 0.02)
    got = sc.host(lrm, main["quats"], main["legs"], ang, sc.RADIUS, margin, sc.TIP_CLEAR)
    compared, skipped = m64.check_self_rows(got, model, m64.BAND_SELF)
    assert skipped == in_doubt and (model["hits"] > 0).any() and (model["free"] == 1).any()


@pytest.mark.parametrize("nlegs", [2, 8])
def test_self_clearance_rows_with_a_thick_coxa_and_other_leg_counts(lrm, nlegs):
    """coxa links in hits, two and eight legs (random legs of ik_cases beyond six), sets through pose_idx, dead sets"""
    n, ns = 40, 130
    legs = sc.legs_n(lrm, nlegs)
    quats = posed_cases.random_unit_quats(n, np.random.default_rng(nlegs))
    assert all(ik_cases.is_unit(q) for q in quats)
    rng = np.random.default_rng(9)
    pi = rng.integers(0, n, ns).astype(np.int32)
    live = (rng.uniform(size=ns) < 0.9).astype(np.uint8)
    ang = lc.random_angles(ns, nlegs, seed=50 + nlegs)
    model = m64.self_clearance64(m64.joints64_posed(ang, legs, quats, sc.TIP_CLEAR, pose_of=pi), sc.RADIUS_COXA, sc.MARGIN, live != 0)
    cap(f"self rows[{nlegs} legs]", int((model["valid"] & m64.self_doubt(model, m64.BAND_SELF)).sum()), int(model["valid"].sum()), 0.02)
    got = sc.host(lrm, quats, legs, ang, sc.RADIUS_COXA, sc.MARGIN, sc.TIP_CLEAR, pi, live)
    m64.check_self_rows(got, model, m64.BAND_SELF)
    assert (model["links"] & 1).any() and (model["hits"] > 0).any()
