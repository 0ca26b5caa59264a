"""Nearest-miss footholds per (pose, leg) on the host (lrm_foothold_misses_posed_cpu, include/lrm.h): the host loop
against a brute force built from the oracle alone (tests/foothold_misses_cases.py: the oracle's reachability_global mask
and distance_global vector, the candidate rule and m2 restated in float32 numpy), the stated consequences (the per-query
call returns mask 0 and the shift bits, margin = +inf is the plain minimum over all targets, a larger margin never gives a
larger m2), the count_in forms, and the argument checks and conventions.  Everything is exact: integers equal, m2 and
shift equal bit for bit."""
import ctypes as C

import numpy as np
import pytest

import foothold_misses_cases as fm
import footholds_posed_cases as fc
import pair_cases as pc
from test_pair_cpu import FAMILIES

LRM_EINVAL = -1


def check_host_equals_brute(lrm, oracle, targets, quats, body, legs, margin, count_in=None):
    want = fm.brute(oracle, targets, quats, body, legs, fm.spheres_of(lrm, quats, legs), margin, count_in)
    got = fm.host(lrm, targets, quats, body, legs, margin, count_in)
    fm.assert_same((got["miss"], got["m2"], got["shift"], got["near"]), want)
    return want


def oracle_counts(lrm, oracle, targets, quats, body, legs):
    return fc.brute(oracle, targets, quats, body, legs, fc.nominal_w_of(lrm, quats, legs, None))["count"]


def test_main_scene_is_not_vacuous(lrm, oracle):
    """from the oracle alone: at least a quarter of the (pose, leg) entries are footless with a miss inside margin 25,
    some are footless with no candidate at all, some have a foothold; unit, non-unit and nan quaternions all occur"""
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fm.scene(lrm, 48, 4000, seed=13)
    count = oracle_counts(lrm, oracle, targets, quats, body, legs)
    want = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, 25.0)
    fm.assert_not_vacuous(count, want)
    r2 = fm.spheres_of(lrm, quats, legs)[:, 0, 3]
    assert np.isposinf(r2).any() and np.isfinite(r2).sum() > 30 and np.isnan(quats).any()
    # with the counts as count_in only the footless entries are answered, and those answers do not change
    skip = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, 25.0, count)
    assert (skip["miss"][count > 0] == -1).all() and (skip["near"][count > 0] == 0).all()
    assert np.array_equal(skip["miss"][count == 0], want["miss"][count == 0])


@pytest.mark.parametrize("family", FAMILIES)
def test_host_loop_matches_bruteforce_for_every_leg_family(lrm, oracle, family):
    legs, _ = pc.leg_families(lrm)[family]
    quats, body, targets = fm.scene(lrm, 36, 3000, seed=len(family) + len(legs))
    prev = None
    for margin in fm.MARGINS:
        want = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, margin)
        if prev is not None:  # a larger margin only adds candidates
            assert (want["m2"] <= prev["m2"]).all() and (want["near"] >= prev["near"]).all()
        prev = want
    assert (want["miss"] >= 0).any()
    count = fc.host(lrm, targets, quats, body, legs, None)["count"]
    for name, cin in fm.count_forms(count).items():
        got = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, 25.0, cin)
        if cin is not None:
            assert (got["miss"][cin > 0] == -1).all(), name
    # every target is a candidate of a non-unit pose, at margin 0 too
    inf = np.isposinf(fm.spheres_of(lrm, quats, legs)[:, :, 3]).T
    assert inf.any()
    zero = fm.host(lrm, targets, quats, body, legs, 0.0)
    assert np.array_equal(zero["miss"][inf], want["miss"][inf]) and np.array_equal(zero["near"][inf], want["near"][inf])


@pytest.mark.parametrize("kind", ["dense_cluster", "sparse_tiles"])
def test_host_loop_matches_bruteforce_on_every_scene(lrm, oracle, kind):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fm.scene(lrm, 40, 6000 if kind == "dense_cluster" else 9 * 1024, seed=2, kind=kind)
    for margin in (0.0, 400.0):
        want = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, margin)
    assert (want["miss"] >= 0).any() and (want["miss"] < 0).any()


def test_host_loop_on_sweep_and_random_unit_quaternions(lrm, oracle):
    import posed_cases
    legs, _ = pc.leg_families(lrm)["moonbot_6_identity"]
    quats, body, targets = fm.scene(lrm, 48, 4000, seed=17)
    n = len(quats)
    quats[: n // 2] = fc.sweep_pose_quats(lrm, n // 2)
    quats[n // 2:] = posed_cases.random_unit_quats(n - n // 2, np.random.default_rng(4))
    for margin in (0.0, 25.0):
        want = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, margin)
    assert (want["miss"] >= 0).mean() > 0.2


def test_host_loop_on_bad_and_extreme_input(lrm, oracle):
    legs, _ = pc.leg_families(lrm)["m2_5_identity"]
    quats, body, targets = fm.scene(lrm, 40, 3000, seed=8)
    bad_t = targets.copy()
    bad_t[::7] = np.nan
    bad_t[3::11, 1] = np.inf
    bad_t[5::13] = -np.inf
    bad_t[1024:1088] = np.nan
    for margin in (25.0, np.inf):
        check_host_equals_brute(lrm, oracle, bad_t, quats, body, legs, margin)
    bad_b = body.copy()
    bad_b[1] = np.nan
    bad_b[2, 0] = np.inf
    bad_b[35] = -np.inf
    for margin in (25.0, np.inf):
        want = check_host_equals_brute(lrm, oracle, targets, quats, bad_b, legs, margin)
        assert (want["miss"][:, [1, 2, 35]] == -1).all()


def test_the_per_query_call_returns_mask_zero_and_the_shift_bits(lrm):
    for name, margin in (("m2_6_tilted", 25.0), ("mixed_5_tilted", 400.0), ("random_8_identity", np.inf)):
        legs, _ = pc.leg_families(lrm)[name]
        quats, body, targets = fm.scene(lrm, 48, 4000, seed=21)
        got = fm.host(lrm, targets, quats, body, legs, margin)
        l, p = np.nonzero(got["miss"] >= 0)
        assert len(l) > 40
        mask, _, field, _ = lrm.apply_reach_dist_posed_cpu(targets[got["miss"][l, p]], p, l, quats, body, legs)
        assert (mask == 0).all()
        assert np.array_equal(pc.bits(field.T), pc.bits(got["shift"][:, l, p]))
        m2 = (field[:, 0] * field[:, 0] + field[:, 1] * field[:, 1]) + field[:, 2] * field[:, 2]
        assert np.array_equal(pc.bits(m2), pc.bits(got["m2"][l, p]))


def test_infinite_margin_is_the_plain_minimum_over_all_targets(lrm):
    legs, _ = pc.leg_families(lrm)["m2_3_nonunit"]
    quats, body, targets = fm.scene(lrm, 24, 1500, seed=5)
    got = fm.host(lrm, targets, quats, body, legs, np.inf)
    nt = len(targets)
    with np.errstate(over="ignore", invalid="ignore"):
        for p in range(len(quats)):
            for l in range(len(legs)):
                mask, _, d, _ = lrm.apply_reach_dist_posed_cpu(targets, np.full(nt, p), np.full(nt, l), quats, body, legs)
                v = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                ok = (mask == 0) & (v < np.inf) & ~np.isnan(targets - body[p]).any(1)
                assert got["near"][l, p] == ((mask == 0) & ~np.isnan((targets - body[p]).astype(np.float32)).any(1)).sum()
                if ok.any():
                    k = int(np.argmax(ok & (v == v[ok].min())))
                    assert got["miss"][l, p] == k and pc.bits(got["m2"][l, p]) == pc.bits(v[k])
                else:
                    assert got["miss"][l, p] == -1
    assert (got["miss"] >= 0).any()


def test_argument_checks_and_conventions(lrm):
    L = lrm.load()
    p = lrm._capi._ptr
    legs = np.stack([lrm.get_M2_leg(0.3 * k) for k in range(9)]).astype(np.float32)
    f = np.zeros(64, np.float32)
    i = np.zeros(64, np.int32)
    d = C.c_void_p(16)  # never dereferenced: every call below returns before its launch
    q = np.array([[1, 0, 0, 0]], np.float32)

    def cpu(nt, nposes, nlegs, margin=0.0, miss=p(i), sx=p(f), sy=p(f), sz=p(f), quats=p(q)):
        return L.lrm_foothold_misses_posed_cpu(p(f), nt, quats, None, nposes, p(legs), nlegs, margin, None, miss, p(f), sx, sy, sz, p(i), None)

    def gpu(nt, nposes, nlegs, margin=0.0, miss=d, sx=d, sy=d, sz=d, ws=d, fh=d, tx=d):
        return L.lrm_foothold_misses_posed_dev(tx, d, d, nt, ws, fh, nposes, nlegs, margin, None, miss, d, sx, sy, sz, d, None)

    # the range checks come first, then the margin's, all before nposes == 0 returns
    for nt, nposes, nlegs in ((2 ** 31, 0, 6), (4, 0, 0), (4, 0, 9), (4, 2 ** 31, 2), (4, 2 ** 30, 8)):
        assert cpu(nt, nposes, nlegs) == LRM_EINVAL and gpu(nt, nposes, nlegs) == LRM_EINVAL, (nt, nposes, nlegs)
    for margin in (-1.0, -1e-30, float("nan"), float("-inf")):
        assert cpu(4, 0, 2, margin) == LRM_EINVAL and gpu(4, 0, 2, margin) == LRM_EINVAL, margin
    # nposes == 0: a no-op after the checks, whatever the pointers
    for margin in (0.0, 25.0, float("inf")):
        assert L.lrm_foothold_misses_posed_cpu(None, 2 ** 31 - 1, None, None, 0, p(legs), 8, margin, None, None, None, None, None, None, None, None) == 0
        assert L.lrm_foothold_misses_posed_dev(None, None, None, 2 ** 31 - 1, None, None, 0, 8, margin, None, None, None, None, None, None, None, None) == 0
    # NULL miss_out, one or two shift arrays, NULL or misaligned tables, missing clouds
    for kw in ({"miss": None}, {"sx": None}, {"sy": None, "sz": None}, {"sz": None}):
        assert cpu(4, 1, 2, **kw) == LRM_EINVAL and gpu(4, 1, 2, **kw) == LRM_EINVAL, kw
    assert cpu(4, 1, 2, quats=None) == LRM_EINVAL
    for kw in ({"ws": None}, {"fh": None}, {"fh": C.c_void_p(24)}, {"tx": None}):
        assert gpu(4, 1, 2, **kw) == LRM_EINVAL, kw
    # nt == 0: the empty answer everywhere
    quats = fc.pose_quats(lrm, 7)
    body = np.zeros((7, 3), np.float32)
    miss, m2, shift, near, _ = lrm.foothold_misses_posed_cpu(np.zeros((0, 3), np.float32), quats, body, legs[:3], np.inf)
    assert (miss == -1).all() and np.isposinf(m2).all() and (pc.bits(shift) == 0x7FC00000).all() and (near == 0).all()


def test_null_outputs_and_sentinels_outside_the_outputs(lrm):
    """the C ABI writes nlegs * nposes entries per output and nothing behind them; NULL m2 / shift / near are skipped"""
    L = lrm.load()
    p = lrm._capi._ptr
    legs, _ = pc.leg_families(lrm)["m2_5_identity"]
    quats, body, targets = fm.scene(lrm, 20, 2000, seed=3)
    n = 5 * len(quats)
    want = fm.host(lrm, targets, quats, body, legs, 25.0)
    assert (want["miss"] >= 0).any() and (want["miss"] < 0).any()
    for w_m2, w_sh, w_near in ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        miss, near = np.full(n + 8, -7, np.int32), np.full(n + 8, -7, np.int32)
        m2, sh = np.full(n + 8, -7.0, np.float32), np.full((3, n + 8), -7.0, np.float32)
        rc = L.lrm_foothold_misses_posed_cpu(p(targets), len(targets), p(quats), p(body), len(quats), p(legs), 5, 25.0, None, p(miss),
                                             p(m2) if w_m2 else None, p(sh[0]) if w_sh else None, p(sh[1]) if w_sh else None,
                                             p(sh[2]) if w_sh else None, p(near) if w_near else None, None)
        assert rc == 0
        shape = want["miss"].shape
        fm.assert_same((miss[:n].reshape(shape), m2[:n].reshape(shape) if w_m2 else None,
                        sh[:, :n].reshape((3,) + shape) if w_sh else None, near[:n].reshape(shape) if w_near else None), want)
        assert (miss[n:] == -7).all() and (near[n if w_near else 0:] == -7).all()
        assert (m2[n if w_m2 else 0:] == -7.0).all() and (sh[:, n if w_sh else 0:] == -7.0).all()


def test_symbols_are_declared_and_exported(lrm):
    names = {"lrm_foothold_misses_posed_dev", "lrm_foothold_misses_posed_cpu"}
    assert names <= set(lrm.declared_symbols())
    assert names <= set(lrm.exported_symbols())
