"""Common-foothold counts and choice per pose transition on the host (lrm_foothold_edges_posed_cpu, include/lrm.h): the
host loop against a brute force over the oracle's reachability_global that skips nothing (tests/foothold_edges_cases.py),
the stated consequences (a == b against lrm_footholds_posed_cpu with best_d2 exactly doubled, swap symmetry bit for bit),
bad indices, and the argument checks and conventions.  Everything is exact: integers equal, best_d2 equal bit for bit."""
import ctypes as C

import numpy as np
import pytest

import foothold_edges_cases as fe
import footholds_posed_cases as fc
import pair_cases as pc
from test_pair_cpu import FAMILIES

LRM_EINVAL = -1


def check_host_equals_brute(lrm, oracle, targets, quats, body, legs, nominal, ea, eb, both=True):
    nw = fc.nominal_w_of(lrm, quats, legs, nominal)
    want = fe.brute(oracle, targets, quats, body, legs, nw, ea, eb)
    if both:
        pc.assert_both_outcomes(want)  # by the oracle alone
    got = fe.host(lrm, targets, quats, body, legs, nominal, ea, eb)
    fe.assert_same((got["count"], got["best"], got["best_d2"], got["all_legs"]), want)
    return want


def test_main_scene_is_not_vacuous(lrm, oracle):
    """the neighbour edges of the main scene, on the host loop's own output: at least a quarter of the (edge, leg) entries
    have 0 < common < min(count_a, count_b), some edge is feasible with all feet planted and some is not"""
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6)
    quats, body, targets, ea, eb = fe.scene(lrm, 48, 4000, seed=13, extra=False)
    got = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, nominal, ea, eb)
    single = fc.host(lrm, targets, quats, body, legs, nominal)["count"]
    fe.assert_not_vacuous(got["count"], single[:, ea], single[:, eb], got["all_legs"])
    # the pool holds every kind of pair: unit-unit, unit with non-unit or nan, two non-unit
    unit = np.abs(np.linalg.norm(quats.astype(np.float64), axis=1) - 1) < 1e-3
    kinds = {(bool(unit[a]), bool(unit[b])) for a, b in zip(ea, eb)}
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    d = np.linalg.norm(body[ea].astype(np.float64) - body[eb], axis=1)
    assert (d >= 49.9).all() and (d <= 154.0).all()  # 150 mm horizontally, up to a fifth of it vertically


@pytest.mark.parametrize("family", FAMILIES)
def test_host_loop_matches_bruteforce_for_every_leg_family(lrm, oracle, family):
    legs, _ = pc.leg_families(lrm)[family]
    quats, body, targets, ea, eb = fe.scene(lrm, 48, 4000, seed=len(family) + len(legs))
    for nominal in (None, pc.nominal_for(len(legs))):
        want = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, nominal, ea, eb)
    nan = np.isnan(quats).any(1)
    assert nan.any() and (want["count"][:, nan[ea] | nan[eb]] == 0).all()


@pytest.mark.parametrize("kind", ["dense_cluster", "sparse_tiles"])
def test_host_loop_matches_bruteforce_on_every_scene(lrm, oracle, kind):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets, ea, eb = fe.scene(lrm, 40, 6000 if kind == "dense_cluster" else 9 * 1024, seed=2, kind=kind)
    check_host_equals_brute(lrm, oracle, targets, quats, body, legs, pc.nominal_for(6, seed=5), ea, eb)


def test_host_loop_on_sweep_and_random_unit_quaternions(lrm, oracle):
    import posed_cases
    legs, _ = pc.leg_families(lrm)["moonbot_6_identity"]
    quats, body, targets, ea, eb = fe.scene(lrm, 48, 4000, seed=17)
    n = len(quats)
    quats[: n // 2] = fc.sweep_pose_quats(lrm, n // 2)
    quats[n // 2:] = posed_cases.random_unit_quats(n - n // 2, np.random.default_rng(4))
    check_host_equals_brute(lrm, oracle, targets, quats, body, legs, pc.nominal_for(6), ea, eb)


def test_host_loop_on_bad_and_extreme_input(lrm, oracle):
    legs, _ = pc.leg_families(lrm)["m2_5_identity"]
    quats, body, targets, ea, eb = fe.scene(lrm, 40, 3000, seed=8)
    nominal = pc.nominal_for(5)
    bad_t = targets.copy()
    bad_t[::7] = np.nan
    bad_t[3::11, 1] = np.inf
    bad_t[5::13] = -np.inf
    bad_t[1024:1088] = np.nan
    check_host_equals_brute(lrm, oracle, bad_t, quats, body, legs, nominal, ea, eb)
    bad_b = body.copy()
    bad_b[1] = np.nan
    bad_b[2, 0] = np.inf
    bad_b[45] = -np.inf
    want = check_host_equals_brute(lrm, oracle, targets, quats, bad_b, legs, nominal, ea, eb)
    hit = np.isin(ea, (1, 2, 45)) | np.isin(eb, (1, 2, 45))
    assert hit.sum() >= 3 and (want["count"][:, hit] == 0).all()
    # a nominal point 1e30 mm away: d2 = +inf for every target, the choice is the smallest common index
    huge = np.full((5, 3), 1e30, np.float32)
    want = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, huge, ea, eb)
    has = want["count"] > 0
    assert np.isposinf(want["best_d2"]).all() and has.any()
    for l, e in zip(*np.nonzero(has)):
        ra = oracle.reach((targets - body[ea[e]]).astype(np.float32), legs[l], quats[ea[e]]).astype(bool)
        rb = oracle.reach((targets - body[eb[e]]).astype(np.float32), legs[l], quats[eb[e]]).astype(bool)
        assert want["best"][l, e] == np.argmax(ra & rb)


def test_same_pose_twice_is_the_single_pose_call_with_d2_doubled(lrm):
    for name in ("m2_6_tilted", "mixed_5_tilted", "random_8_identity"):
        legs, _ = pc.leg_families(lrm)[name]
        nominal = pc.nominal_for(len(legs))
        quats, body, targets = fc.scene(lrm, 60, 4000, seed=21)
        one = fc.host(lrm, targets, quats, body, legs, nominal)
        pc.assert_both_outcomes(one)
        e = np.arange(60, dtype=np.int32)
        got = fe.host(lrm, targets, quats, body, legs, nominal, e, e)
        assert np.array_equal(got["count"], one["count"]) and np.array_equal(got["best"], one["best"])
        assert np.array_equal(got["all_legs"], one["all_legs"])
        twice = one["best_d2"] + one["best_d2"]  # exact in float32
        assert np.array_equal(pc.bits(got["best_d2"]), pc.bits(twice)) and np.isfinite(twice).any()


def test_swapping_the_ends_changes_no_bit(lrm):
    legs, _ = pc.leg_families(lrm)["m2_7_nonunit"]
    nominal = pc.nominal_for(7)
    quats, body, targets, ea, eb = fe.scene(lrm, 48, 4000, seed=23)
    fwd = fe.host(lrm, targets, quats, body, legs, nominal, ea, eb)
    pc.assert_both_outcomes(fwd)
    rev = fe.host(lrm, targets, quats, body, legs, nominal, eb, ea)
    fe.assert_same((rev["count"], rev["best"], rev["best_d2"], rev["all_legs"]), fwd)


def test_out_of_range_and_negative_indices(lrm, oracle):
    legs, _ = pc.leg_families(lrm)["m2_3_nonunit"]
    nominal = pc.nominal_for(3)
    quats, body, targets, ea, eb = fe.scene(lrm, 24, 2000, seed=5, extra=False)
    npz = len(quats)
    ea, eb = ea.copy(), eb.copy()
    ea[0], ea[3], eb[5], eb[7] = -1, npz, npz + 1000, np.iinfo(np.int32).min
    ea[9], eb[9] = np.iinfo(np.int32).max, -7
    want = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, nominal, ea, eb)
    bad = [0, 3, 5, 7, 9]
    assert (want["count"][:, bad] == 0).all() and (want["best"][:, bad] == -1).all()
    assert np.isposinf(want["best_d2"][:, bad]).all() and (want["all_legs"][bad] == 0).all()


def test_argument_checks_and_conventions(lrm):
    L = lrm.load()
    p = lrm._capi._ptr
    legs = np.stack([lrm.get_M2_leg(0.3 * k) for k in range(9)]).astype(np.float32)
    f = np.zeros(64, np.float32)
    i = np.zeros(64, np.int32)
    u = np.zeros(64, np.uint8)
    d = C.c_void_p(16)  # never dereferenced: every call below returns before its launch
    q = np.array([[1, 0, 0, 0]], np.float32)

    def cpu(nt, nposes, nlegs, nedges, ea=p(i), eb=p(i), cnt=p(i), bst=p(i)):
        return L.lrm_foothold_edges_posed_cpu(p(f), nt, p(q), None, nposes, p(legs), nlegs, None, ea, eb, nedges, cnt, bst, p(f), p(u), None)

    def gpu(nt, nposes, nlegs, nedges, ea=d, eb=d, cnt=d, bst=d, ws=d, fh=d, tx=d):
        return L.lrm_foothold_edges_posed_dev(tx, d, d, nt, ws, fh, nposes, nlegs, ea, eb, nedges, cnt, bst, d, d, None)

    # the range checks come first, before nedges == 0 returns
    for nt, nposes, nlegs, nedges in ((2 ** 31, 1, 6, 0), (4, 1, 0, 0), (4, 1, 9, 0), (4, 2 ** 31, 2, 0), (4, 2 ** 30, 8, 0),
                                      (4, 1, 6, (2 ** 32 - 1) // 6 + 1), (4, 1, 1, 2 ** 32)):
        assert cpu(nt, nposes, nlegs, nedges) == LRM_EINVAL, (nt, nposes, nlegs, nedges)
        assert gpu(nt, nposes, nlegs, nedges) == LRM_EINVAL, (nt, nposes, nlegs, nedges)
    # nedges == 0: a no-op after the checks, whatever the pointers
    assert L.lrm_foothold_edges_posed_cpu(None, 2 ** 31 - 1, None, None, 1, p(legs), 8, None, None, None, 0, None, None, None, None, None) == 0
    assert L.lrm_foothold_edges_posed_dev(None, None, None, 2 ** 31 - 1, None, None, 1, 8, None, None, 0, None, None, None, None, None) == 0
    # NULL edges or required outputs, NULL or misaligned tables, missing clouds
    for kw in ({"ea": None}, {"eb": None}, {"cnt": None}, {"bst": None}):
        assert cpu(4, 1, 2, 1, **kw) == LRM_EINVAL and gpu(4, 1, 2, 1, **kw) == LRM_EINVAL, kw
    for kw in ({"ws": None}, {"fh": None}, {"fh": C.c_void_p(24)}, {"tx": None}):
        assert gpu(4, 1, 2, 1, **kw) == LRM_EINVAL, kw
    # nt == 0: count 0, best -1, d2 +inf, all_legs 0 everywhere; best_d2 and all_legs may be NULL
    quats = fc.pose_quats(lrm, 7)
    body = np.zeros((7, 3), np.float32)
    ea, eb = np.arange(7, dtype=np.int32), np.arange(7, dtype=np.int32)[::-1].copy()
    count, best, best_d2, all_legs, _ = lrm.foothold_edges_posed_cpu(np.zeros((0, 3), np.float32), quats, body, legs[:3], ea, eb)
    assert (count == 0).all() and (best == -1).all() and np.isposinf(best_d2).all() and (all_legs == 0).all()
    cnt, bst = np.full((3, 7), 9, np.int32), np.full((3, 7), 9, np.int32)
    assert L.lrm_foothold_edges_posed_cpu(None, 0, p(quats), None, 7, p(legs), 3, None, p(ea), p(eb), 7, p(cnt), p(bst), None, None, None) == 0
    assert (cnt == 0).all() and (bst == -1).all()


def test_null_outputs_and_sentinels_outside_the_outputs(lrm):
    """the C ABI writes nlegs * nedges (and nedges) entries and nothing behind them; NULL best_d2 / all_legs are skipped"""
    L = lrm.load()
    p = lrm._capi._ptr
    legs, _ = pc.leg_families(lrm)["m2_5_identity"]
    nominal = pc.nominal_for(5)
    quats, body, targets, ea, eb = fe.scene(lrm, 20, 2000, seed=3)
    ne, nl = len(ea), 5
    want = fe.host(lrm, targets, quats, body, legs, nominal, ea, eb)
    pc.assert_both_outcomes(want)
    for d2, al in ((True, True), (False, True), (True, False), (False, False)):
        cnt, bst = np.full(nl * ne + 8, -7, np.int32), np.full(nl * ne + 8, -7, np.int32)
        bd2, alv = np.full(nl * ne + 8, -7.0, np.float32), np.full(ne + 8, 9, np.uint8)
        rc = L.lrm_foothold_edges_posed_cpu(p(targets), len(targets), p(quats), p(body), len(quats), p(legs), nl, p(nominal), p(ea), p(eb),
                                            ne, p(cnt), p(bst), p(bd2) if d2 else None, p(alv) if al else None, None)
        assert rc == 0
        got = (cnt[:nl * ne].reshape(nl, ne), bst[:nl * ne].reshape(nl, ne), bd2[:nl * ne].reshape(nl, ne) if d2 else None,
               alv[:ne] if al else None)
        fe.assert_same(got, want)
        assert (cnt[nl * ne:] == -7).all() and (bst[nl * ne:] == -7).all()
        assert (bd2[nl * ne if d2 else 0:] == -7.0).all() and (alv[ne if al else 0:] == 9).all()


def test_symbols_are_declared_and_exported(lrm):
    names = {"lrm_foothold_edges_posed_dev", "lrm_foothold_edges_posed_cpu"}
    assert names <= set(lrm.declared_symbols())
    assert names <= set(lrm.exported_symbols())
