"""Foothold counts and choice per (pose, leg) on the host (lrm_footholds_posed_cpu, lrm_dbg_pose_footholds_compile_host,
include/lrm.h): the host loop against a brute force over the oracle's reachability_global that skips nothing, the
nominal point's rotation against the project's own FK, the cull sphere against the oracle's reachable set, the identity
pose against lrm_footholds_cpu, and the argument checks and conventions.  Everything but the FK bound is exact:
integers equal, best_d2 equal bit for bit."""
import ctypes as C

import numpy as np
import pytest

import footholds_posed_cases as fc
import pair_cases as pc
import posed_cases
from test_pair_cpu import FAMILIES, _bound_legs

LRM_EINVAL = -1


def check_host_equals_brute(lrm, oracle, targets, quats, body, legs, nominal, both=True):
    nw = fc.nominal_w_of(lrm, quats, legs, nominal)
    want = fc.brute(oracle, targets, quats, body, legs, nw)
    if both:
        pc.assert_both_outcomes(want)  # by the oracle alone
    got = fc.host(lrm, targets, quats, body, legs, nominal)
    fc.assert_same((got["count"], got["best"], got["best_d2"], got["all_legs"]), want)
    return want


def test_pose_quats_hold_every_kind(lrm):
    q = fc.pose_quats(lrm, 40)
    n = np.linalg.norm(q.astype(np.float64), axis=1)
    assert np.array_equal(q[0], [1, 0, 0, 0]) and np.isnan(n).sum() >= 1
    assert (np.abs(n - 1) < 1e-6).sum() >= 20 and ((n > 0.45) & (n < 0.95)).any() and ((n > 1.1) & (n < 2.05)).any()
    assert {len(legs) for legs, _ in pc.leg_families(lrm).values()} >= {1, 2, 3, 5, 6, 7, 8}


@pytest.mark.parametrize("family", FAMILIES)
def test_host_loop_matches_bruteforce_for_every_leg_family(lrm, oracle, family):
    legs, _ = pc.leg_families(lrm)[family]
    quats, body, targets = fc.scene(lrm, 48, 4000, seed=len(family) + len(legs))
    for nominal in (None, pc.nominal_for(len(legs))):
        want = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, nominal)
    bad = ~(np.abs(np.linalg.norm(quats.astype(np.float64), axis=1) - 1) < 1e-3)
    assert (want["count"][:, np.isnan(quats).any(1)] == 0).all() and bad.sum() >= 7


@pytest.mark.parametrize("kind", ["dense_cluster", "sparse_tiles", "duplicates"])
def test_host_loop_matches_bruteforce_on_every_scene(lrm, oracle, kind):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6, seed=5)
    if kind == "duplicates":
        quats, body, base = fc.scene(lrm, 40, 2500, seed=4)
        targets, twin = pc.with_spread_duplicates(base, seed=6)
        one = fc.brute(oracle, base, quats, body, legs, fc.nominal_w_of(lrm, quats, legs, nominal))
    else:
        quats, body, targets = fc.scene(lrm, 40, 6000 if kind == "dense_cluster" else 9 * 1024, seed=2, kind=kind)
    want = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, nominal)
    if kind == "duplicates":
        assert np.array_equal(want["count"], 2 * one["count"])
        has = want["best"] >= 0
        assert has.any() and (want["best"][has] < twin[want["best"][has]]).all()  # the smaller index of two equal d2


@pytest.mark.parametrize("offset", [1e4, 1e6, 4e6])
def test_host_loop_far_from_the_origin(lrm, oracle, offset):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fc.scene(lrm, 48, 4000, seed=9)
    body, targets = pc.translated(body, targets, offset)
    check_host_equals_brute(lrm, oracle, targets, quats, body, legs, pc.nominal_for(6))


def test_host_loop_on_bad_and_extreme_input(lrm, oracle):
    legs, _ = pc.leg_families(lrm)["m2_5_identity"]
    quats, body, targets = fc.scene(lrm, 40, 3000, seed=8)
    nominal = pc.nominal_for(5)
    bad_t = targets.copy()
    bad_t[::7] = np.nan
    bad_t[3::11, 1] = np.inf
    bad_t[5::13] = -np.inf
    bad_t[1024:1088] = np.nan
    check_host_equals_brute(lrm, oracle, bad_t, quats, body, legs, nominal)
    bad_b = body.copy()
    bad_b[1] = np.nan
    bad_b[2, 0] = np.inf
    bad_b[5] = -np.inf
    want = check_host_equals_brute(lrm, oracle, targets, quats, bad_b, legs, nominal)
    assert (want["count"][:, [1, 2, 5]] == 0).all()
    # a nominal point 1e30 mm away: d2 = +inf for every target, the choice is the smallest reachable index
    huge = np.full((5, 3), 1e30, np.float32)
    want = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, huge)
    has = want["count"] > 0
    assert np.isposinf(want["best_d2"]).all() and has.any()
    for l, p in zip(*np.nonzero(has)):
        r = oracle.reach((targets - body[p]).astype(np.float32), legs[l], quats[p])
        assert want["best"][l, p] == np.argmax(r)


def test_nominal_w_is_the_body_to_caller_rotation(lrm):
    """With nominal = a body-frame FK tip (lrm_fk_cpu, identity quaternion), body + nominal_w is the posed FK tip of the
    same angles: within 2.5e-3 mm + 2^-22 |x| per component, the project's own FK bound.  Unit
    quaternions only: for the others qtRotate is not the inverse of qtInvRotate."""
    legs = posed_cases.leg_table(lrm)
    quats, body = posed_cases.pose_table(lrm, 37)
    unit = np.abs(np.linalg.norm(quats.astype(np.float64), axis=1) - 1) < 1e-6
    quats, body = quats[unit], body[unit]
    assert len(quats) >= 20
    rng = np.random.default_rng(3)
    for trial in range(3):
        ang = np.stack([[rng.uniform(l[9], l[8]), rng.uniform(l[13], l[12]), rng.uniform(l[11], l[10])] for l in legs]).astype(np.float32)
        nominal = np.stack([lrm.apply_fk_cpu(ang[k:k + 1], legs[k], (1, 0, 0, 0))[0][0] for k in range(len(legs))])
        assert np.abs(nominal).max() > 100
        tab = lrm.dbg_pose_footholds_compile_host(quats, legs, nominal)
        assert (tab[:, :, 7] == 0).all()
        npz, nl = len(quats), len(legs)
        pose_idx, leg_idx = np.repeat(np.arange(npz), nl), np.tile(np.arange(nl), npz)
        tip, _ = lrm.apply_fk_posed_cpu(ang[leg_idx], pose_idx, leg_idx, quats, body, legs)
        mine = (body[:, None, :] + tab[:, :, 4:7]).astype(np.float32).reshape(-1, 3)
        assert (np.abs(mine.astype(np.float64) - tip) <= 2.5e-3 + 2.0 ** -22 * np.abs(tip)).all()
    # no nominal: exactly zero, whatever the quaternion (non-unit and nan ones included)
    mixed = fc.pose_quats(lrm, 40)
    assert np.isnan(mixed).any()
    for q in (quats, mixed):
        assert (lrm.dbg_pose_footholds_compile_host(q, legs, None)[:, :, 4:8] == 0).all()
        assert (lrm.dbg_pose_footholds_compile_host(q, legs, np.zeros((len(legs), 3), np.float32))[:, :, 4:8] == 0).all()


def test_cull_sphere_contains_every_reachable_pair(lrm, oracle):
    """No p = target - body the oracle's reachability_global accepts lies outside the entry's sphere, in float64 and in
    the kernel's own float32 statement, nor (unit quaternions) outside the body radius the tile cull uses: dense samples
    of the scaled radius' cube, coxa half-ranges up to 175 degrees, unit, near-unit and non-unit quaternions, every leg
    family.  A quaternion that is not unit or not finite must get the sphere that excludes nothing."""
    rng = np.random.default_rng(80)
    cases = [(leg, q) for leg, q in _bound_legs(lrm)]
    for name in FAMILIES:
        legs, q = pc.leg_families(lrm)[name]
        cases.append((legs[len(name) % len(legs)], q))
    pool = fc.pose_quats(lrm, 60, seed=11)
    seen = wide_seen = finite = near_seen = 0
    for i, (leg, q0) in enumerate(cases):
        u = posed_cases.random_unit_quats(1, rng)[0].astype(np.float64)
        near = (u * np.sqrt(1.0 + rng.choice([-1.0, 1.0]) * rng.uniform(2e-6, 8e-6))).astype(np.float32)  # finite sphere, off unit
        for q in (q0, pool[(3 * i) % 60], posed_cases.random_unit_quats(1, rng)[0], near):
            q = np.asarray(q, np.float32)
            e = lrm.dbg_pose_footholds_compile_host(q[None], leg[None], None)[0, 0]
            centre, r2 = e[:3], e[3]
            n2 = float((q.astype(np.float64) ** 2).sum())
            if not abs(n2 - 1) < 2e-5:  # the code's gate is 1e-5 on the float32 sum; beyond 2e-5 it cannot pass
                assert np.isposinf(r2) and (centre == 0).all(), (i, q)
            if np.isnan(q).any():
                continue
            scale = max(1.0, 1.0 / n2) if np.isposinf(r2) else 1.0  # qtInvRotate of a small q shrinks p: the set grows
            side = 1.15 * np.sqrt(float(pc.body_radius(leg))) * scale
            rel = rng.uniform(-side, side, (60_000, 3)).astype(np.float32)
            hit = oracle.reach(rel, leg, q).astype(bool)
            r = rel[hit]
            assert (((r.astype(np.float64) - centre) ** 2).sum(1) <= r2).all(), (i, q, "sphere, float64")
            ex, ey, ez = r[:, 0] - centre[0], r[:, 1] - centre[1], r[:, 2] - centre[2]
            d2 = ez * ez + (ey * ey + ex * ex)
            assert (d2 <= r2).all(), (i, q, "sphere, float32")
            if np.isfinite(r2):
                finite += 1
                near_seen += int(q is near and 1e-6 < abs(n2 - 1) < 1e-5)
                b2 = r[:, 2] * r[:, 2] + (r[:, 1] * r[:, 1] + r[:, 0] * r[:, 0])
                assert (b2 <= pc.body_radius(leg)).all(), (i, q, "body radius")
                seen += int(hit.sum())
                if 0.5 * (float(leg[8]) - float(leg[9])) > np.deg2rad(87):
                    wide_seen += int(hit.sum())
    assert finite > 60 and seen > 20000 and wide_seen > 3000 and near_seen > 30, (finite, seen, wide_seen, near_seen)


def test_identity_pose_equals_the_existing_call(lrm, oracle):
    """With the identity quaternion in every pose and no nominal, (leg, pose) gets lrm_footholds_cpu's count, best and
    best_d2 on the same bodies with lrm_rotate_leg_data(identity) legs -- wherever the gravity gate of
    reachable_rotate_leg passes, i.e. wherever no target that reachability_global accepts lies behind the leg's mount
    direction (gx < 0, several_leg.cu:56-59).  reachability_global has no such gate, so elsewhere the posed count is
    the larger one: by exactly the targets the oracle's two tests disagree on."""
    ident = np.array([1, 0, 0, 0], np.float32)
    for name in ("m2_6_tilted", "moonbot_6_identity", "mixed_5_tilted"):
        raw, _ = pc.leg_families(lrm)[name]
        legs = np.stack([lrm.rotate_leg_data(ident, leg) for leg in raw]).astype(np.float32)
        assert np.array_equal(legs, raw)  # the identity leaves the limits alone
        body, targets = pc.rough(60, 3000, seed=12)
        quats = np.tile(ident, (len(body), 1))
        got = fc.host(lrm, targets, quats, body, legs, None)
        count, best, best_d2, _ = lrm.footholds_cpu(body, targets, legs, ident, None)
        gated = oracle.reach_pairs(body, targets, legs, ident).astype(bool)  # [L, B, T]
        free = np.stack([[oracle.reach((targets - b).astype(np.float32), leg, ident).astype(bool) for b in body] for leg in legs])
        assert not (gated & ~free).any()
        extra = (free & ~gated).sum(-1)
        same = extra == 0
        assert same.sum() > same.size // 2 and (count[same] > 0).any()
        assert np.array_equal(got["count"], count + extra)
        assert np.array_equal(got["count"][same], count[same]) and np.array_equal(got["best"][same], best[same])
        assert np.array_equal(pc.bits(got["best_d2"][same]), pc.bits(best_d2[same]))


def test_argument_checks_and_conventions(lrm):
    L = lrm.load()
    p = lrm._capi._ptr
    legs = np.stack([lrm.get_M2_leg(0.3 * k) for k in range(9)]).astype(np.float32)
    f = np.zeros(64, np.float32)
    i = np.zeros(64, np.int32)
    u = np.zeros(64, np.uint8)
    d = C.c_void_p(16)  # never dereferenced: every call below returns before its launch
    q = np.array([[1, 0, 0, 0]], np.float32)
    for nt, nlegs in ((2 ** 31, 6), (4, 0), (4, 9)):
        assert L.lrm_footholds_posed_cpu(p(f), nt, p(q), None, 0, p(legs), nlegs, None, p(i), p(i), p(f), p(u), None) == LRM_EINVAL
        assert L.lrm_footholds_posed_dev(d, d, d, nt, d, d, 0, nlegs, d, d, d, d, None) == LRM_EINVAL
    assert L.lrm_footholds_posed_dev(d, d, d, 4, d, d, 2 ** 31, 2, d, d, d, d, None) == LRM_EINVAL
    assert L.lrm_footholds_posed_dev(d, d, d, 4, d, d, 2 ** 30, 8, d, d, d, d, None) == LRM_EINVAL
    # nposes == 0: a no-op after the checks
    assert L.lrm_footholds_posed_cpu(p(f), 2 ** 31 - 1, p(q), None, 0, p(legs), 8, None, p(i), p(i), p(f), p(u), None) == 0
    assert L.lrm_footholds_posed_dev(None, None, None, 2 ** 31 - 1, None, None, 0, 8, None, None, None, None, None) == 0
    # null or misaligned tables, missing outputs
    assert L.lrm_footholds_posed_dev(d, d, d, 4, None, d, 1, 2, d, d, d, d, None) == LRM_EINVAL
    assert L.lrm_footholds_posed_dev(d, d, d, 4, d, None, 1, 2, d, d, d, d, None) == LRM_EINVAL
    assert L.lrm_footholds_posed_dev(d, d, d, 4, d, C.c_void_p(24), 1, 2, d, d, d, d, None) == LRM_EINVAL
    assert L.lrm_footholds_posed_dev(d, d, d, 4, d, d, 1, 2, None, d, d, d, None) == LRM_EINVAL
    assert L.lrm_footholds_posed_dev(None, d, d, 4, d, d, 1, 2, d, d, d, d, None) == LRM_EINVAL
    assert L.lrm_pose_footholds_compile_dev(d, 4, p(legs), 9, None, d, None) == LRM_EINVAL
    assert L.lrm_pose_footholds_compile_dev(d, 4, p(legs), 2, None, None, None) == LRM_EINVAL
    assert L.lrm_pose_footholds_compile_dev(d, 4, p(legs), 2, None, C.c_void_p(8), None) == LRM_EINVAL
    assert L.lrm_pose_footholds_compile_dev(d, 0, p(legs), 2, None, d, None) == 0
    assert L.lrm_dbg_pose_footholds_compile_host(p(q), 1, p(legs), 9, None, p(f)) == LRM_EINVAL
    assert L.lrm_posed_footholds_workspace_bytes(3, 5) == 3 * 5 * 32 == 15 * lrm.POSE_FOOTHOLD_BYTES
    # nt == 0: count 0, best -1, d2 +inf, all_legs 0 everywhere; best_d2 and all_legs may be NULL
    quats = fc.pose_quats(lrm, 7)
    body = np.zeros((7, 3), np.float32)
    count, best, best_d2, all_legs, _ = lrm.footholds_posed_cpu(np.zeros((0, 3), np.float32), quats, body, legs[:3])
    assert (count == 0).all() and (best == -1).all() and np.isposinf(best_d2).all() and (all_legs == 0).all()
    cnt, bst = np.full((3, 7), 9, np.int32), np.full((3, 7), 9, np.int32)
    assert L.lrm_footholds_posed_cpu(None, 0, p(quats), None, 7, p(legs), 3, None, p(cnt), p(bst), None, None, None) == 0
    assert (cnt == 0).all() and (bst == -1).all()
    # all_legs is the AND over the legs; a pose whose every leg reaches the same single target
    leg = lrm.get_M2_leg(0.0)
    tip = lrm.apply_fk_cpu(np.array([[0.0, 0.2, 0.3]], np.float32), leg, (1, 0, 0, 0))[0]
    q2 = np.array([[1, 0, 0, 0], [1, 0, 0, 0]], np.float32)
    b2 = np.array([[0, 0, 0], [5000, 0, 0]], np.float32)
    count, best, best_d2, all_legs, _ = lrm.footholds_posed_cpu(tip, q2, b2, np.stack([leg, leg]))
    assert count.tolist() == [[1, 0], [1, 0]] and best.tolist() == [[0, -1], [0, -1]] and all_legs.tolist() == [1, 0]
    assert np.isfinite(best_d2[:, 0]).all() and np.isposinf(best_d2[:, 1]).all()


def test_symbols_are_declared_and_exported(lrm):
    names = {"lrm_posed_footholds_workspace_bytes", "lrm_pose_footholds_compile_dev", "lrm_dbg_pose_footholds_compile_host",
             "lrm_footholds_posed_dev", "lrm_footholds_posed_cpu"}
    assert names <= set(lrm.declared_symbols())
    assert names <= set(lrm.exported_symbols())
