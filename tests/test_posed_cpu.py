"""Batched multi-pose queries on the host (lrm_reach_dist_posed_cpu, lrm_dbg_pose_compile_host): the same per-point code
and the same records as the device path, checked against the oracle per (pose, leg); the shared strict head of the leg
compiler; the device pose compiler's libm (lrm_sincosf) against glibc's separate cosf / sinf."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

from conftest import bits_equal
from posed_cases import leg_table, oracle_answer, pose_table, queries, random_unit_quats


def test_cpu_entry_matches_oracle_per_pose_and_leg(lrm, oracle):
    quats, body = pose_table(lrm)
    legs = leg_table(lrm)
    assert len(quats) == 37 and len(legs) == 7
    rng = np.random.default_rng(11)
    xyz, pose, leg = queries(len(quats), len(legs), body, 61, rng, "shuffled")
    keep = rng.permutation(len(xyz))[:15_797]  # a ragged count, shuffled order, every (pose, leg) still present
    xyz, pose, leg = xyz[keep], pose[keep], leg[keep]
    m, v, d, ms = lrm.apply_reach_dist_posed_cpu(xyz, pose, leg, quats, body, legs)
    wm, wv, wd = oracle_answer(oracle, xyz, pose, leg, quats, body, legs)
    assert ms >= 0
    assert np.array_equal(m, wm) and np.array_equal(v, wv)
    assert bits_equal(d, wd).all()
    assert wm.sum() > 100  # the cloud does reach the legs


def test_cpu_entry_without_body_and_without_indices(lrm, oracle):
    quats, _ = pose_table(lrm, n=5)
    legs = leg_table(lrm)
    rng = np.random.default_rng(3)
    xyz, pose, leg = queries(len(quats), len(legs), np.zeros((5, 3), np.float32), 40, rng, "interleaved")
    m, v, d, _ = lrm.apply_reach_dist_posed_cpu(xyz, pose, leg, quats, None, legs)
    wm, wv, wd = oracle_answer(oracle, xyz, pose, leg, quats, None, legs)
    assert np.array_equal(m, wm) and np.array_equal(v, wv) and bits_equal(d, wd).all()
    # NULL indices: pose 0 and leg 0 for every query
    m, v, d, _ = lrm.apply_reach_dist_posed_cpu(xyz, None, None, quats, None, legs)
    assert np.array_equal(m, oracle.reach(xyz, legs[0], quats[0]))
    wd, wv = oracle.dist(xyz, legs[0], quats[0])
    assert np.array_equal(v, wv) and bits_equal(d, wd).all()


def test_out_of_range_indices_and_bad_arguments(lrm, oracle):
    quats, body = pose_table(lrm, n=4)
    legs = leg_table(lrm)
    rng = np.random.default_rng(8)
    xyz, pose, leg = queries(4, len(legs), body, 10, rng, "shuffled")
    bad = rng.random(len(xyz)) < 0.3
    pose = pose.copy()
    leg = leg.copy()
    pose[bad & (rng.random(len(xyz)) < 0.5)] = rng.choice(np.array([-1, 4, 1000, np.iinfo(np.int32).min], np.int32))
    leg[bad & (pose >= 0) & (pose < 4)] = rng.choice(np.array([7, 8, 255], np.uint8))
    oob = (pose < 0) | (pose >= 4) | (leg >= len(legs))
    assert oob.sum() > 10
    m, v, d, _ = lrm.apply_reach_dist_posed_cpu(xyz, pose, leg, quats, body, legs)
    assert not m[oob].any() and not v[oob].any() and np.isnan(d[oob]).all()
    ok = ~oob
    wm, wv, wd = oracle_answer(oracle, xyz[ok], pose[ok], leg[ok], quats, body, legs)
    assert np.array_equal(m[ok], wm) and np.array_equal(v[ok], wv) and bits_equal(d[ok], wd).all()
    # nine legs: more than LRM_MAX_LEGS
    nine = np.concatenate([legs, legs[:2]])
    with pytest.raises(lrm.LrmError, match="LRM_MAX_LEGS"):
        lrm.apply_reach_dist_posed_cpu(xyz, pose, leg, quats, body, nine)
    with pytest.raises(lrm.LrmError, match="LRM_MAX_LEGS"):
        lrm.dbg_pose_compile_host(quats, body, nine)
    L = lrm.lib()
    # no pose for n > 0 queries, a null workspace, nine legs: errors before anything is launched
    assert L.lrm_reach_dist_posed_cpu(lrm._capi._ptr(xyz), len(xyz), None, None, lrm._capi._ptr(quats), None, 0,
                                      lrm._capi._ptr(legs), len(legs), lrm._capi._ptr(m), None, None, None) == -1
    assert L.lrm_last_error()
    dummy = 0x1000
    assert L.lrm_reach_dist_posed_dev(dummy, dummy, dummy, 16, None, None, None, 4, 7, dummy, None, None, None, None, None) == -1
    assert b"workspace" in L.lrm_last_error()
    assert L.lrm_reach_dist_posed_dev(dummy, dummy, dummy, 16, None, None, dummy, 0, 7, dummy, None, None, None, None, None) == -1
    assert L.lrm_reach_dist_posed_dev(dummy, dummy, dummy, 16, None, None, dummy, 4, 9, dummy, None, None, None, None, None) == -1
    assert L.lrm_pose_compile_dev(dummy, None, 4, lrm._capi._ptr(nine), 9, dummy, None) == -1
    assert L.lrm_reach_dist_posed_dev(None, None, None, 0, None, None, None, 0, 0, None, None, None, None, None, None) == 0
    assert L.lrm_posed_workspace_bytes(4096, 6) == 4096 * 6 * lrm.POSE_RECORD_BYTES


def test_pose_records_are_the_compiled_leg_head(lrm):
    """Every record = the first 480 bytes of lrm_compile_leg(leg, quat, 1) (the shared strict head), then the body
    position and zero padding."""
    quats, body = pose_table(lrm)
    rng = np.random.default_rng(2)
    quats = np.concatenate([quats, random_unit_quats(20, rng), (rng.standard_normal((5, 4)) * 2).astype(np.float32)])
    body = np.concatenate([body, rng.standard_normal((25, 3)).astype(np.float32) * 500])
    legs = leg_table(lrm)
    recs = lrm.dbg_pose_compile_host(quats, body, legs)
    assert recs.shape == (len(quats), len(legs), 512)
    for p in range(len(quats)):
        for k in range(len(legs)):
            assert recs[p, k, :480].tobytes() == lrm.dbg_compile_leg_head(legs[k], quats[p]).tobytes(), (p, k)
    assert recs[:, :, 480:492].view(np.float32).reshape(len(quats), len(legs), 3).tobytes() == \
        np.repeat(body[:, None, :], len(legs), axis=1).tobytes()
    assert not recs[:, :, 492:].any()
    none = lrm.dbg_pose_compile_host(quats, None, legs)
    assert np.array_equal(none[:, :, :480], recs[:, :, :480]) and not none[:, :, 480:].any()


def _glibc():
    m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.cosf.argtypes = m.sinf.argtypes = [C.c_float]
    m.cosf.restype = m.sinf.restype = C.c_float
    return m


def _compile_arguments(lrm, quats, legs):
    """every argument the leg compiler's head passes to cosf / sinf / sincosf, for these (quat, leg) pairs (f32 as the
    compiler forms them)"""
    f = np.float32
    out = []
    for leg in legs:
        out += [f(-leg[0]), f(leg[2]), f(-leg[2]), f(leg[0] / f(2))]  # -body_angle, +-coxa_pitch, body_angle / 2
        for q in quats:
            r = lrm.rotate_leg_data(q, leg)
            tp, tn, mxt, mnt, mxf, mnf = r[6], r[7], r[10], r[11], r[12], r[13]
            fem = [mnf, mnf, mnf, f(tn - mnt), f(tn - mxt), mxf, mxf, mxf, f(tp - mnt), f(tp - mnt)]
            tib = [mxt, mnt, f(tn - fem[2]), f(tn - fem[3]), f(tn - fem[4]), mnt, mxt, f(tp - fem[7]), f(tp - fem[8]), f(tp - fem[9])]
            out += [mnt, tp, tn, mnf, mxf] + fem + [f(a + b) for a, b in zip(fem, tib)]
    return np.array(out, np.float32)


def test_device_libm_equals_glibc_cosf_sinf(lrm):
    """The device pose compiler takes cosf / sinf / sincosf from lrm_sincosf (lrm_exact_math.h); the host compiler calls
    glibc's cosf and sinf.  They must be the same functions on the compile's arguments and on a large random sample."""
    libm = _glibc()
    quats, _ = pose_table(lrm)
    rng = np.random.default_rng(4)
    from lrm_amd import workloads
    quats = np.concatenate([quats, workloads.reference_sweep_quats(), random_unit_quats(200, rng)])
    args = _compile_arguments(lrm, quats, leg_table(lrm))
    sample = np.concatenate([args, (rng.random(400_000) * 4 * np.pi - 2 * np.pi).astype(np.float32),
                             (rng.random(100_000) * 239.9 - 119.95).astype(np.float32),
                             rng.standard_normal(100_000).astype(np.float32) * 1e-3])
    n = len(sample)
    at2, sn, cs = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    lrm._capi.check(lrm.lib().lrm_dbg_exact_math_host(lrm._capi._ptr(sample), lrm._capi._ptr(np.ones(n, np.float32)), n,
                                                      lrm._capi._ptr(at2), lrm._capi._ptr(sn), lrm._capi._ptr(cs)))
    want_c = np.array([libm.cosf(float(a)) for a in sample], np.float32)
    want_s = np.array([libm.sinf(float(a)) for a in sample], np.float32)
    bad = ~(bits_equal(cs, want_c) & bits_equal(sn, want_s))
    assert not bad.any(), sample[bad][:10]
