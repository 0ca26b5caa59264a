"""Per-target foothold support on the host (lrm_foothold_support_posed_cpu, include/lrm.h): the host loop against a brute
force built from the oracle alone (tests/foothold_support_cases.py), the consequences the header states (column sums
against lrm_footholds_posed_cpu, membership and d2 bits against lrm_foothold_lists_posed_cpu, lrm_ik_posed_cpu at the best
pose, legs_mask against the counts), the pose_live forms, and the argument checks and conventions.  Everything is exact:
integers equal, d2 equal bit for bit."""
import ctypes as C

import numpy as np
import pytest

import foothold_support_cases as fs
import footholds_posed_cases as fc
import pair_cases as pc
from test_pair_cpu import FAMILIES

LRM_EINVAL = -1
MAIN = dict(nposes=128, nt=3000, seed=13, dup=32)


def check_host_equals_brute(lrm, oracle, targets, quats, body, legs, nominal=None, pose_live=None):
    want = fs.brute(oracle, targets, quats, body, legs, fc.nominal_w_of(lrm, quats, legs, nominal), pose_live)
    got = fs.host(lrm, targets, quats, body, legs, nominal, pose_live)
    fs.assert_same((got["count"], got["best_pose"], got["best_d2"], got["legs_mask"]), want)
    return want


def test_main_scene_is_not_vacuous(lrm, oracle):
    """from the oracle alone: at least a quarter of the (target, leg) entries have two or more reaching poses, some have
    none and some exactly one, duplicated poses tie exactly and the smaller index wins; unit, non-unit and nan
    quaternions all occur"""
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fs.scene(lrm, MAIN["nposes"], MAIN["nt"], MAIN["seed"], dup=MAIN["dup"])
    want = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, pc.nominal_for(6))
    fs.assert_not_vacuous(want, MAIN["nposes"], MAIN["dup"])
    r2 = lrm.dbg_pose_footholds_compile_host(quats, legs, None)[:, 0, 3]
    assert np.isposinf(r2).any() and np.isfinite(r2).sum() > 30 and np.isnan(quats).any()


def test_pose_live_forms(lrm, oracle):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6)
    quats, body, targets = fs.scene(lrm, MAIN["nposes"], MAIN["nt"], MAIN["seed"], dup=MAIN["dup"])
    forms = fs.live_forms(lrm, targets, quats, body, legs, nominal)
    res = {name: check_host_equals_brute(lrm, oracle, targets, quats, body, legs, nominal, live) for name, live in forms.items()}
    for k in ("count", "best_pose", "best_d2", "legs_mask"):
        assert np.array_equal(res["null"][k], res["ones"][k])
    assert (res["zeros"]["count"] == 0).all() and (res["zeros"]["best_pose"] == -1).all() and (res["zeros"]["legs_mask"] == 0).all()
    al = forms["all_legs"].astype(bool)
    assert al.any() and (~al).any()
    # only positionable bodies count: never more than with every pose, strictly fewer somewhere, and no dead pose wins
    assert (res["all_legs"]["count"] <= res["null"]["count"]).all() and (res["all_legs"]["count"] < res["null"]["count"]).any()
    won = res["all_legs"]["best_pose"]
    assert al[won[won >= 0]].all()
    # bytes other than 0 and 1 are live too
    odd = forms["all_legs"] * np.uint8(37)
    got = fs.host(lrm, targets, quats, body, legs, nominal, odd)
    assert np.array_equal(got["count"], res["all_legs"]["count"]) and np.array_equal(got["best_pose"], res["all_legs"]["best_pose"])


@pytest.mark.parametrize("family", FAMILIES)
def test_host_loop_matches_bruteforce_for_every_leg_family(lrm, oracle, family):
    legs, _ = pc.leg_families(lrm)[family]
    quats, body, targets = fs.scene(lrm, 60, 2000, seed=len(family) + len(legs), dup=12)
    nominal = pc.nominal_for(len(legs), seed=len(family))
    want = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, nominal)
    assert (want["count"] > 0).any() and (want["count"] == 0).any()
    want0 = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, None)
    assert np.array_equal(want0["count"], want["count"])  # the nominal point moves the choice, never the counts


@pytest.mark.parametrize("kind", ["dense_cluster", "sparse_tiles"])
def test_host_loop_matches_bruteforce_on_every_scene(lrm, oracle, kind):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fs.scene(lrm, 40, 6000 if kind == "dense_cluster" else 9 * 1024, seed=2, kind=kind, dup=8)
    want = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, pc.nominal_for(6))
    assert (want["count"] >= 2).any() and (want["count"] == 0).any()


def test_host_loop_on_sweep_and_random_unit_quaternions(lrm, oracle):
    import posed_cases
    legs, _ = pc.leg_families(lrm)["moonbot_6_identity"]
    quats, body, targets = fs.scene(lrm, 64, 3000, seed=17)
    n = len(quats)
    quats[: n // 2] = fc.sweep_pose_quats(lrm, n // 2)
    quats[n // 2:] = posed_cases.random_unit_quats(n - n // 2, np.random.default_rng(4))
    want = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, pc.nominal_for(6))
    assert (want["count"] > 0).mean() > 0.2


def test_host_loop_on_bad_and_extreme_input(lrm, oracle):
    legs, _ = pc.leg_families(lrm)["m2_5_identity"]
    quats, body, targets = fs.scene(lrm, 40, 3000, seed=8, dup=6)
    bad_t = targets.copy()
    bad_t[::7] = np.nan
    bad_t[3::11, 1] = np.inf
    bad_t[5::13] = -np.inf
    bad_t[1024:1088] = np.nan
    want = check_host_equals_brute(lrm, oracle, bad_t, quats, body, legs, pc.nominal_for(5))
    assert (want["count"][:, ~np.isfinite(bad_t).all(1)] == 0).all() and (want["count"] > 0).any()  # nan / inf targets reach nothing
    bad_b = body.copy()
    bad_b[1] = np.nan
    bad_b[2, 0] = np.inf
    bad_b[35] = -np.inf
    want = check_host_equals_brute(lrm, oracle, targets, quats, bad_b, legs, pc.nominal_for(5))
    assert not np.isin(want["best_pose"], [1, 2, 35]).any() and (want["count"] > 0).any()
    # a nominal point 1e30 away: every d2 overflows to +inf, all reaching poses tie, the smallest index wins
    far = np.full((5, 3), 1e30, np.float32)
    want = check_host_equals_brute(lrm, oracle, targets, quats, body, legs, far)
    have = want["count"] > 0
    assert have.any() and np.isposinf(want["best_d2"][have]).all()
    plain = fs.host(lrm, targets, quats, body, legs, None)
    assert np.array_equal(plain["count"], want["count"])


def test_consequences_against_the_pose_first_calls(lrm):
    """column sums equal lrm_footholds_posed_cpu's; count > 0 iff the target occurs in a list of that leg; the list of the
    best pose holds the target with best_d2's bits; legs_mask restates the counts"""
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6)
    quats, body, targets = fs.scene(lrm, MAIN["nposes"], MAIN["nt"], MAIN["seed"], dup=MAIN["dup"])
    nl, npz, nt = 6, len(quats), len(targets)
    got = fs.host(lrm, targets, quats, body, legs, nominal)
    count = lrm.footholds_posed_cpu(targets, quats, body, legs, nominal)[0]
    assert np.array_equal(got["count"].sum(1, dtype=np.int64), count.sum(1, dtype=np.int64))
    offsets = np.concatenate([[0], np.cumsum(count.reshape(-1), dtype=np.int64)])
    idx, d2, written, _ = lrm.foothold_lists_posed_cpu(targets, quats, body, legs, offsets, nominal=nominal)
    assert np.array_equal(written, count)
    seen = np.zeros((nl, nt), np.int32)
    for l in range(nl):
        seg = idx[offsets[l * npz]:offsets[(l + 1) * npz]]
        seen[l] = np.bincount(seg, minlength=nt)
    assert np.array_equal(seen, got["count"])  # every (pose, leg) list holds a target at most once
    ls, ts = np.nonzero(got["count"] > 0)
    assert len(ls) > 1000
    for l, t in zip(ls[::37], ts[::37]):
        o = l * npz + got["best_pose"][l, t]
        seg = slice(offsets[o], offsets[o + 1])
        k = np.nonzero(idx[seg] == t)[0]
        assert len(k) == 1 and pc.bits(d2[seg][k[0]]) == pc.bits(got["best_d2"][l, t])
    want_mask = np.zeros(nt, np.uint8)
    for l in range(nl):
        want_mask |= ((got["count"][l] > 0).astype(np.uint8) << l).astype(np.uint8)
    assert np.array_equal(got["legs_mask"], want_mask)


def test_ik_at_the_best_pose_reports_reached(lrm):
    """lrm_ik_posed_cpu on (t, best_pose[l, t], l) answers with a mask-1 status wherever count > 0.  The reach test this call
    is defined by is the circle model's; the IK reports LRM_IK_REACHED where the joint model agrees within 2e-3 mm and
    LRM_IK_MODEL_GAP where it does not (include/lrm.h, the IK section: a property of the two models at the workspace
    boundary, the same for every foothold call -- tests/test_gpu_footholds_posed.py accepts both as well).  Measured on
    these three scenes: 14 261 of 14 299 entries REACHED, 38 MODEL_GAP, all at unit quaternions.  So: every status is one
    of the two, never NONE / NEAREST / FAR_GAP, and REACHED is the rule."""
    total = gaps = 0
    for name in ("m2_6_tilted", "mixed_5_tilted", "random_8_identity"):
        legs, _ = pc.leg_families(lrm)[name]
        quats, body, targets = fs.scene(lrm, 64, 2000, seed=21, dup=10)
        got = fs.host(lrm, targets, quats, body, legs, pc.nominal_for(len(legs)))
        l, t = np.nonzero(got["count"] > 0)
        assert len(l) > 200
        _, status, _ = lrm.apply_ik_posed_cpu(targets, got["best_pose"][l, t], l.astype(np.uint8), quats, body, legs, target_idx=t)
        assert np.isin(status, (lrm.IK_REACHED, lrm.IK_MODEL_GAP)).all(), np.bincount(status, minlength=5)
        # the per-query reach call agrees: mask 1 at every best pose
        mask, _, _, _ = lrm.apply_reach_dist_posed_cpu(targets[t], got["best_pose"][l, t], l.astype(np.uint8), quats, body, legs)
        assert (mask == 1).all()
        total += len(status)
        gaps += int((status == lrm.IK_MODEL_GAP).sum())
        # and where no pose reaches there is nothing to solve: best_pose is -1
        assert (got["best_pose"][got["count"] == 0] == -1).all()
    print(f"ik at the best pose: {total - gaps} REACHED, {gaps} MODEL_GAP of {total}")
    assert gaps * 100 < total  # a boundary effect, not the rule: the boundary shell is thin against the workspace


def test_argument_checks_and_conventions(lrm):
    L = lrm.load()
    p = lrm._capi._ptr
    legs = np.stack([lrm.get_M2_leg(0.3 * k) for k in range(9)]).astype(np.float32)
    f = np.zeros(64, np.float32)
    i = np.zeros(64, np.int32)
    d = C.c_void_p(16)  # never dereferenced: every call below returns before its launch
    q = np.array([[1, 0, 0, 0]], np.float32)

    def cpu(nt, nposes, nlegs, count=p(i), best=p(i), quats=p(q), targets=p(f), lg=p(legs)):
        return L.lrm_foothold_support_posed_cpu(targets, nt, quats, None, nposes, lg, nlegs, None, None, count, best, p(f), None, None)

    def gpu(nt, nposes, nlegs, count=d, best=d, ws=d, fh=d, sw=d, tx=d):
        return L.lrm_foothold_support_posed_dev(tx, d, d, nt, ws, fh, nposes, nlegs, None, sw, count, best, d, d, None)

    # the range checks come first, in lrm_footholds_posed_dev's order, before nt == 0 returns
    for nt, nposes, nlegs in ((2 ** 31, 0, 6), (0, 0, 0), (0, 0, 9), (0, 2 ** 31, 2), (0, 2 ** 30, 8), (4, 2 ** 31, 2)):
        assert cpu(nt, nposes, nlegs) == LRM_EINVAL and gpu(nt, nposes, nlegs) == LRM_EINVAL, (nt, nposes, nlegs)
    # nt == 0: a no-op after the checks, whatever the pointers
    assert L.lrm_foothold_support_posed_cpu(None, 0, None, None, 2 ** 31 - 1, p(legs), 2, None, None, None, None, None, None, None) == 0
    assert L.lrm_foothold_support_posed_dev(None, None, None, 0, None, None, 2 ** 31 - 1, 2, None, None, None, None, None, None, None) == 0
    # NULL count_out, best_pose_out, support_workspace; NULL or misaligned tables, missing clouds
    for kw in ({"count": None}, {"best": None}):
        assert cpu(4, 1, 2, **kw) == LRM_EINVAL and gpu(4, 1, 2, **kw) == LRM_EINVAL, kw
    for kw in ({"quats": None}, {"targets": None}, {"lg": None}):
        assert cpu(4, 1, 2, **kw) == LRM_EINVAL, kw
    for kw in ({"sw": None}, {"sw": C.c_void_p(24)}, {"ws": None}, {"fh": None}, {"fh": C.c_void_p(24)}, {"tx": None}):
        assert gpu(4, 1, 2, **kw) == LRM_EINVAL, kw
    assert gpu(4, 0, 2, sw=None) == LRM_EINVAL  # also without poses
    # nposes == 0: 0 / -1 / +inf / 0 everywhere
    targets = np.random.default_rng(1).uniform(-300, 300, (37, 3)).astype(np.float32)
    count, best, d2, mask, _ = lrm.foothold_support_posed_cpu(targets, np.zeros((0, 4), np.float32), None, legs[:3])
    assert count.shape == (3, 37) and (count == 0).all() and (best == -1).all() and np.isposinf(d2).all() and (mask == 0).all()
    # the workspace size grows with every argument and is a multiple of 16
    wb = L.lrm_foothold_support_workspace_bytes
    assert wb(100, 6, 1000) % 16 == 0 and wb(100, 6, 1000) >= 12 * 6 * 1000 + 16 * 600
    assert wb(101, 6, 1000) >= wb(100, 6, 1000) and wb(100, 7, 1000) > wb(100, 6, 1000) and wb(100, 6, 1001) > wb(100, 6, 1000)


def test_null_outputs_and_sentinels_outside_the_outputs(lrm):
    """the C ABI writes nlegs * nt entries per output and nt mask bytes and nothing behind them; NULL best_d2 / legs_mask
    are skipped"""
    L = lrm.load()
    p = lrm._capi._ptr
    legs, _ = pc.leg_families(lrm)["m2_5_identity"]
    quats, body, targets = fs.scene(lrm, 30, 1500, seed=3, dup=5)
    nt = len(targets)
    n = 5 * nt
    want = fs.host(lrm, targets, quats, body, legs)
    assert (want["count"] > 0).any() and (want["count"] == 0).any()
    for w_d2, w_mask in ((True, True), (False, True), (True, False), (False, False)):
        count, best = np.full(n + 8, -7, np.int32), np.full(n + 8, -7, np.int32)
        d2, mask = np.full(n + 8, -7.0, np.float32), np.full(nt + 8, 0xA5, np.uint8)
        rc = L.lrm_foothold_support_posed_cpu(p(targets), nt, p(quats), p(body), len(quats), p(legs), 5, None, None, p(count), p(best),
                                              p(d2) if w_d2 else None, p(mask) if w_mask else None, None)
        assert rc == 0
        fs.assert_same((count[:n].reshape(5, nt), best[:n].reshape(5, nt), d2[:n].reshape(5, nt) if w_d2 else None,
                        mask[:nt] if w_mask else None), want)
        assert (count[n:] == -7).all() and (best[n:] == -7).all()
        assert (d2[n if w_d2 else 0:] == -7.0).all() and (mask[nt if w_mask else 0:] == 0xA5).all()


def test_grid_is_a_function_of_the_sizes_alone(lrm):
    """lrm_dbg_foothold_support_grid: host only; the slices never exceed the pose chunks, every pose chunk has a slice,
    and the grid holds one wave per (target chunk, slice)"""
    for nt, nposes in ((1, 1), (64, 64), (64, 65), (65, 4096), (64, 3000), (4096, 500), (65536, 89600), (2 ** 21, 1000), (100, 0)):
        g = lrm.dbg_foothold_support_grid(nt, nposes)
        chunks = -(-nposes // g["pose_chunk"])
        assert g["pose_chunk"] == 64 and 1 <= g["slices"] <= max(chunks, 1)
        assert g["poses_per_slice"] * g["slices"] >= nposes and g["poses_per_slice"] == -(-chunks // g["slices"]) * 64
        assert g["blocks"] == -(-(-(-nt // 64) * g["slices"]) // 4)
    assert lrm.dbg_foothold_support_grid(64, 64)["slices"] == 1 and lrm.dbg_foothold_support_grid(64, 3000)["slices"] >= 2


def test_symbols_are_declared_and_exported(lrm):
    names = {"lrm_foothold_support_posed_dev", "lrm_foothold_support_posed_cpu", "lrm_foothold_support_workspace_bytes",
             "lrm_dbg_foothold_support_grid"}
    assert names <= set(lrm.declared_symbols())
    assert names <= set(lrm.exported_symbols())
