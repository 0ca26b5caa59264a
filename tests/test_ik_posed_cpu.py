"""Joint angles per (target, pose, leg) on the host (lrm_ik_posed_cpu, lrm_fk_posed_cpu, lrm_dbg_pose_ik_compile_host):
bit-identical to the single-pose calls lrm_ik_cpu / lrm_fk_cpu per (pose, leg) group on p = target - body, the
out-of-range rule, the contract of include/lrm.h per group, and the foothold pipeline lrm_footholds_cpu -> posed IK."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits_equal
from footholds_cases import QUATS, legs_for, nominal_for, scene
from ik_cases import AZIMUTHS, check_contract, fixture_quats, random_legs, unit
from posed_cases import queries, random_unit_quats

INT32_MIN = np.iinfo(np.int32).min
IDENTITY = np.array([1, 0, 0, 0], np.float32)


def pose_quats(rng, n_random=4):
    """the fixture quaternions normalised, one kept non-unit, random unit ones"""
    fq = fixture_quats()
    return np.concatenate([[unit(q) for q in fq], fq[1:2], random_unit_quats(n_random, rng)]).astype(np.float32)


def leg_tables(lrm):
    std = np.stack([make(az) for make in (lrm.get_M2_leg, lrm.get_moonbot_leg) for az in AZIMUTHS]).astype(np.float32)
    rnd = np.stack([leg for _, leg, _ in random_legs(lrm)[:8]]).astype(np.float32)
    return {"standard": std, "random": rnd}


def bad_seeds(n, rng):
    """the seed families of test_gpu_ik.py: finite, nan, inf, -inf, 1e20"""
    seed = (rng.random((n, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
    seed[::7, 0] = np.nan
    seed[3::11] = np.inf
    seed[5::13, 2] = -np.inf
    seed[6::17] = 1e20
    return seed


def groups(pose, leg, nlegs):
    key = pose.astype(np.int64) * nlegs + leg
    order = np.argsort(key, kind="stable")
    keys, starts = np.unique(key[order], return_index=True)
    for k, sel in zip(keys, np.split(order, starts[1:])):
        yield int(k) // nlegs, int(k) % nlegs, sel


def single_pose_ik(lrm, xyz, pose, leg, quats, body, legs, seed):
    """the yardstick: lrm_ik_cpu per (pose, leg) group on p = target - body formed in numpy float32"""
    n = len(pose)
    ang, st = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    p_all = (xyz - body[pose]).astype(np.float32) if body is not None else xyz
    for pi, li, sel in groups(pose, leg, len(legs)):
        a, s, _ = lrm.apply_ik_cpu(np.ascontiguousarray(p_all[sel]), legs[li], quats[pi],
                                   seed=None if seed is None else np.ascontiguousarray(seed[sel]))
        ang[sel], st[sel] = a, s
    return ang, st, p_all


def single_pose_fk(lrm, ang, pose, leg, quats, body, legs):
    out = np.zeros((len(pose), 3), np.float32)
    for pi, li, sel in groups(pose, leg, len(legs)):
        p, _ = lrm.apply_fk_cpu(np.ascontiguousarray(ang[sel]), legs[li], quats[pi])
        out[sel] = p if body is None else (p + body[pi]).astype(np.float32)
    return out


@pytest.mark.parametrize("family", ["standard", "random"])
@pytest.mark.parametrize("with_body", [True, False])
@pytest.mark.parametrize("with_seed", [False, True])
def test_posed_cpu_equals_single_pose_calls(lrm, family, with_body, with_seed):
    rng = np.random.default_rng(17)
    quats = pose_quats(rng)
    legs = leg_tables(lrm)[family]
    body = (rng.random((len(quats), 3), dtype=np.float32) * 4000 - 2000).astype(np.float32)
    xyz, pose, leg = queries(len(quats), len(legs), body if with_body else np.zeros_like(body), 23, rng, "shuffled")
    xyz[::501] = np.nan
    n = len(xyz)
    b = body if with_body else None
    seed = bad_seeds(n, rng) if with_seed else None
    want_a, want_s, _ = single_pose_ik(lrm, xyz, pose, leg, quats, b, legs, seed)
    ang, st, ms = lrm.apply_ik_posed_cpu(xyz, pose, leg, quats, b, legs, seed=seed)
    assert ms >= 0 and np.array_equal(st, want_s) and bits_equal(ang, want_a).all()
    assert len(np.unique(st)) >= 3
    # target_idx: a permutation with repeats of the same targets
    ti = rng.integers(0, n, n).astype(np.int32)
    ti[: n // 2] = rng.permutation(n)[: n // 2]
    want_a2, want_s2, _ = single_pose_ik(lrm, xyz[ti], pose, leg, quats, b, legs, seed)
    ang2, st2, _ = lrm.apply_ik_posed_cpu(xyz, pose, leg, quats, b, legs, target_idx=ti, seed=seed)
    assert np.array_equal(st2, want_s2) and bits_equal(ang2, want_a2).all()
    # FK of the angles (finite ones; the nan rows stay nan on both sides)
    got_p, ms = lrm.apply_fk_posed_cpu(ang, pose, leg, quats, b, legs)
    assert ms >= 0 and bits_equal(got_p, single_pose_fk(lrm, ang, pose, leg, quats, b, legs)).all()


def test_null_indices_mean_pose_0_leg_0_target_i(lrm):
    rng = np.random.default_rng(3)
    quats = pose_quats(rng)[:3]
    legs = leg_tables(lrm)["standard"]
    body = (rng.random((3, 3), dtype=np.float32) * 100).astype(np.float32)
    xyz, _, _ = queries(1, 1, body[:1], 500, rng, "pair_major")
    ang, st, _ = lrm.apply_ik_posed_cpu(xyz, None, None, quats, body, legs)
    a, s, _ = lrm.apply_ik_cpu((xyz - body[0]).astype(np.float32), legs[0], quats[0])
    assert np.array_equal(st, s) and bits_equal(ang, a).all()
    got, _ = lrm.apply_fk_posed_cpu(ang, None, None, quats, body, legs)
    p, _ = lrm.apply_fk_cpu(a, legs[0], quats[0])
    assert bits_equal(got, (p + body[0]).astype(np.float32)).all()


def test_out_of_range_indices_and_bad_arguments(lrm):
    rng = np.random.default_rng(8)
    quats = pose_quats(rng)[:4]
    legs = leg_tables(lrm)["standard"]
    nl = len(legs)
    body = (rng.random((4, 3), dtype=np.float32) * 2000 - 1000).astype(np.float32)
    xyz, pose, leg = queries(4, nl, body, 20, rng, "shuffled")
    n = len(xyz)
    ti = rng.permutation(n).astype(np.int32)
    clean_a, clean_s, _ = lrm.apply_ik_posed_cpu(xyz, pose, leg, quats, body, legs, target_idx=ti)
    clean_p, _ = lrm.apply_fk_posed_cpu(clean_a, pose, leg, quats, body, legs)
    pose2, leg2, ti2 = pose.copy(), leg.copy(), ti.copy()
    kind = rng.integers(0, 8, n)
    pose2[kind == 1] = rng.choice(np.array([-1, 4, 1000, INT32_MIN], np.int32), (kind == 1).sum())
    leg2[kind == 2] = rng.choice(np.array([nl, nl + 1, 255], np.uint8), (kind == 2).sum())
    ti2[kind == 3] = rng.choice(np.array([-1, n, n + 7, INT32_MIN], np.int32), (kind == 3).sum())
    oob = np.isin(kind, (1, 2, 3))
    assert oob.sum() > 30 and (~oob).sum() > 30
    ang, st, _ = lrm.apply_ik_posed_cpu(xyz, pose2, leg2, quats, body, legs, target_idx=ti2)
    assert (st[oob] == 0).all() and np.isnan(ang[oob]).all()
    assert np.array_equal(st[~oob], clean_s[~oob]) and bits_equal(ang[~oob], clean_a[~oob]).all()
    got_p, _ = lrm.apply_fk_posed_cpu(clean_a, pose2, leg2, quats, body, legs)
    fk_oob = np.isin(kind, (1, 2))
    assert np.isnan(got_p[fk_oob]).all() and bits_equal(got_p[~fk_oob], clean_p[~fk_oob]).all()
    # arguments
    L = lrm.lib()
    p = lrm._capi._ptr
    a, s = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    nine = np.concatenate([legs, legs[:3]])
    assert len(nine) == 9
    ik = lambda nt, tidx, nq, nlegs, lg, ao, so: L.lrm_ik_posed_cpu(p(xyz), nt, tidx, nq, p(pose), p(leg), p(quats), p(body), 4,
                                                                      p(lg), nlegs, None, ao, so, None)
    assert ik(n, None, n, nl, legs, p(a), p(s)) == 0
    for bad in (ik(n - 1, None, n, nl, legs, p(a), p(s)),   # n > nt without target_idx
                ik(n, None, n, 0, legs, p(a), p(s)), ik(n, None, n, 9, nine, p(a), p(s)),
                ik(n, None, n, nl, legs, None, p(s)), ik(n, None, n, nl, legs, p(a), None)):
        assert bad == -1 and L.lrm_last_error()
    assert L.lrm_fk_posed_cpu(p(a), n, p(pose), p(leg), p(quats), p(body), 4, p(legs), nl, None, None) == -1
    assert L.lrm_fk_posed_cpu(p(a), n, p(pose), p(leg), p(quats), p(body), 4, p(nine), 9, p(a), None) == -1
    assert L.lrm_fk_posed_cpu(p(a), n, p(pose), p(leg), p(quats), p(body), 4, p(legs), 0, p(a), None) == -1
    # the device entry points refuse the same before anything is launched
    d = C.c_void_p(0x1000)
    dev = lambda nt, tidx, nq, nlegs, ws, iws, out: L.lrm_ik_posed_dev(d, d, d, nt, tidx, nq, None, None, ws, iws, 4, nlegs, None,
                                                                       None, None, out, d, d, d, None)
    for bad in (dev(15, None, 16, 6, d, d, d), dev(16, None, 16, 0, d, d, d), dev(16, None, 16, 9, d, d, d),
                dev(16, None, 16, 6, None, d, d), dev(16, None, 16, 6, d, None, d), dev(16, None, 16, 6, d, d, None)):
        assert bad == -1 and L.lrm_last_error()
    assert L.lrm_ik_posed_dev(d, d, d, 16, None, 16, None, None, d, d, 4, 6, d, None, None, d, d, d, d, None) == -1  # partial seed
    assert L.lrm_fk_posed_dev(d, d, d, 16, None, None, d, None, 4, 6, d, d, d, None) == -1
    assert L.lrm_fk_posed_dev(d, d, d, 16, None, None, d, d, 4, 9, d, d, d, None) == -1
    assert L.lrm_pose_ik_compile_dev(d, 4, p(nine), 9, d, None) == -1
    assert L.lrm_pose_ik_compile_dev(d, 4, p(legs), nl, None, None) == -1
    assert L.lrm_ik_posed_dev(None, None, None, 0, None, 0, None, None, None, None, 0, 0, None, None, None, None, None, None,
                              None, None) == 0
    assert L.lrm_posed_ik_workspace_bytes(4096, 6) == 4096 * 6 * lrm.POSE_IK_RECORD_BYTES


def test_contract_per_pose_and_leg(lrm, oracle):
    rng = np.random.default_rng(29)
    quats = np.concatenate([[unit(q) for q in fixture_quats()], random_unit_quats(3, rng)]).astype(np.float32)
    legs = leg_tables(lrm)["standard"]
    body = (rng.random((len(quats), 3), dtype=np.float32) * 3000 - 1500).astype(np.float32)
    xyz, pose, leg = queries(len(quats), len(legs), body, 400, rng, "interleaved")
    ang, st, _ = lrm.apply_ik_posed_cpu(xyz, pose, leg, quats, body, legs)
    p_all = (xyz - body[pose]).astype(np.float32)
    seen = np.zeros(5, np.int64)
    for pi, li, sel in groups(pose, leg, len(legs)):
        seen += check_contract(oracle, p_all[sel], legs[li], quats[pi], ang[sel], st[sel], clean=True)["counts"]
    assert seen[1] > 500 and seen[2] > 5000


@pytest.mark.parametrize("qname", sorted(QUATS))
def test_footholds_to_joint_angles_on_the_host(lrm, qname):
    """lrm_footholds_cpu's best[l*nb + b] is the target_idx of the posed IK as it stands: one pose per body with the
    IDENTITY quaternion and the body position, the legs as the foothold call got them (already rotated)."""
    quat = np.asarray(QUATS[qname], np.float32)
    nb, nl = 120, 6
    bodies, targets = scene(nb, 3000, seed=7)
    legs = legs_for(lrm, nl, quat)
    # the premise: the identity pose leaves these legs as they are
    for l in legs:
        assert lrm.rotate_leg_data(IDENTITY, l).tobytes() == np.asarray(l, np.float32).tobytes()
    count, best, _, _ = lrm.footholds_cpu(bodies, targets, legs, quat, nominal_for(nl))
    assert (best == -1).any() and (best >= 0).sum() > 50
    pose = np.tile(np.arange(nb, dtype=np.int32), nl)
    leg = np.repeat(np.arange(nl, dtype=np.uint8), nb)
    quats = np.tile(IDENTITY, (nb, 1))
    ti = best.reshape(-1)
    ang, st, _ = lrm.apply_ik_posed_cpu(targets, pose, leg, quats, bodies, legs, target_idx=ti)
    assert np.array_equal(st == 0, ti == -1)
    assert np.isin(st[ti >= 0], (1, 3)).all(), np.bincount(st, minlength=5)
    assert (st[ti >= 0] == 1).all(), np.bincount(st, minlength=5)  # M2 legs: no model gap
    ok = ti >= 0
    tip, _ = lrm.apply_fk_posed_cpu(ang[ok], pose[ok], leg[ok], quats, bodies, legs)
    want = targets[ti[ok]].astype(np.float64)
    miss = np.linalg.norm(tip.astype(np.float64) - want, axis=1)
    bound = 2.5e-3 + 2.0 ** -22 * np.linalg.norm(want, axis=1)
    print(f"{qname}: max miss {miss.max():.3e} mm, min slack {(bound - miss).min():.3e} mm")
    assert (miss <= bound).all(), f"max miss {miss.max():.3e} mm"


def test_host_ik_table_equals_the_single_pose_compile(lrm):
    """the struct is not reachable from Python: compare through FK outputs and default-seed IK outputs, which read every
    field (lengths, limits, f_lo / f_hi, seed, back); and the table's size and determinism"""
    rng = np.random.default_rng(5)
    quats = pose_quats(rng, n_random=20)
    legs = np.concatenate(list(leg_tables(lrm).values()))[:8]
    recs = lrm.dbg_pose_ik_compile_host(quats, legs)
    assert recs.shape == (len(quats), len(legs), 128) and not recs[:, :, 112:].any()  # pad_ stays zero
    assert np.array_equal(recs, lrm.dbg_pose_ik_compile_host(quats, legs))
    f = recs.view(np.float32).reshape(len(quats), len(legs), 32)
    for pi in range(len(quats)):
        for li in range(len(legs)):
            r = lrm.rotate_leg_data(quats[pi], legs[li])
            k = f[pi, li]
            # C, F, T, the six joint limits and the rotated absolute limits are the rotated leg's floats
            want = [r[3], r[5], r[4], r[9], r[8], r[13], r[12], r[11], r[10], r[7], r[6]]
            assert k[[0, 1, 2, 6, 7, 8, 9, 10, 11, 12, 13]].tobytes() == np.array(want, np.float32).tobytes(), (pi, li)
    xyz, pose, leg = queries(len(quats), len(legs), np.zeros((len(quats), 3), np.float32), 9, rng, "pair_major")
    ang, st, _ = lrm.apply_ik_posed_cpu(xyz, pose, leg, quats, None, legs)
    want_a, want_s, _ = single_pose_ik(lrm, xyz, pose, leg, quats, None, legs, None)
    assert np.array_equal(st, want_s) and bits_equal(ang, want_a).all()
    tip, _ = lrm.apply_fk_posed_cpu(ang, pose, leg, quats, None, legs)
    assert bits_equal(tip, single_pose_fk(lrm, ang, pose, leg, quats, None, legs)).all()


def test_symbols_are_declared_and_exported(lrm):
    names = {"lrm_posed_ik_workspace_bytes", "lrm_pose_ik_compile_dev", "lrm_dbg_pose_ik_compile_host", "lrm_ik_posed_dev",
             "lrm_fk_posed_dev", "lrm_ik_posed_cpu", "lrm_fk_posed_cpu"}
    assert names <= set(lrm.declared_symbols())
    assert names <= set(lrm.exported_symbols())
