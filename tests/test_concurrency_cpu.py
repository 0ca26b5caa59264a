"""The library called from several host threads at once, without a GPU (include/lrm.h, "Threading").

ctypes drops the GIL around every library call, so the calls of these threads really overlap.  Each thread works on inputs of
its own and every result must equal, byte for byte, what the same call returns when it runs alone: the host table builder,
the host reach / distance / IK / posed entry points.  lrm_last_error() is per thread.  Without a device, the *_dev calls of
every thread report LRM_ENODEV; lrm_release_workspaces may be called again and again, with or without a device."""
import ctypes as C
import threading

import numpy as np

from conftest import bits_equal, random_cloud
from posed_cases import leg_table, pose_table, queries

NTHREADS = 8
LRM_EINVAL, LRM_ENODEV = -1, -2


def run_threads(fns):
    """fns[i]() on thread i, all released at once by a barrier -> their results (the first exception is raised here)"""
    barrier = threading.Barrier(len(fns))
    out, errs = [None] * len(fns), []

    def body(i):
        try:
            barrier.wait()
            out[i] = fns[i]()
        except BaseException as e:  # noqa: BLE001 -- re-raised on the main thread
            errs.append(e)

    ts = [threading.Thread(target=body, args=(i,)) for i in range(len(fns))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if errs:
        raise errs[0]
    return out


def legs_and_quats(lrm):
    """one (leg, orientation) per thread, all different"""
    out = []
    for k in range(NTHREADS):
        leg = lrm.get_M2_leg(-2.5 + 0.7 * k) if k % 2 == 0 else lrm.get_moonbot_leg(-2.0 + 0.6 * k)
        a = 0.05 + 0.04 * k
        q = np.array([np.cos(a), 0.3 * np.sin(a), np.sin(a), -0.2 * np.sin(a)], np.float64)
        out.append((leg, (q / np.linalg.norm(q)).astype(np.float32)))
    return out


def work(lrm, k, leg, q):
    """every host entry point the threads share, on inputs of thread k"""
    pts = random_cloud(60_000 + 1_001 * k, seed=100 + k)
    tab, _ = lrm.dbg_toltab_build(leg, q, device=False)
    m, _ = lrm.apply_reach_cpu(pts, leg, q)
    d, v, _ = lrm.apply_dist_cpu(pts, leg, q)
    ang, st, _ = lrm.apply_ik_cpu(pts[:20_000], leg, q)
    quats, body = pose_table(lrm, n=9, seed=k)
    legs = leg_table(lrm)
    xyz, pose, li = queries(len(quats), len(legs), body, 211, np.random.default_rng(k), "shuffled")
    pm, pv, pd, _ = lrm.apply_reach_dist_posed_cpu(xyz, pose, li, quats, body, legs)
    return dict(tab=tab, m=m, d=d, v=v, ang=ang, st=st, pm=pm, pv=pv, pd=pd)


def same(a, b):
    return (a["tab"].size == b["tab"].size and np.array_equal(a["tab"], b["tab"]) and np.array_equal(a["m"], b["m"])
            and bits_equal(a["d"], b["d"]).all() and np.array_equal(a["v"], b["v"]) and bits_equal(a["ang"], b["ang"]).all()
            and np.array_equal(a["st"], b["st"]) and np.array_equal(a["pm"], b["pm"]) and np.array_equal(a["pv"], b["pv"])
            and bits_equal(a["pd"], b["pd"]).all())


def test_host_entry_points_from_eight_threads_equal_serial_calls(lrm):
    cases = legs_and_quats(lrm)
    serial = [work(lrm, k, leg, q) for k, (leg, q) in enumerate(cases)]
    assert len({s["tab"].tobytes() for s in serial}) == NTHREADS  # eight different tables: a mix-up would show
    for _ in range(2):
        got = run_threads([lambda k=k, c=c: work(lrm, k, *c) for k, c in enumerate(cases)])
        for k in range(NTHREADS):
            assert same(got[k], serial[k]), f"thread {k}: a result differs from the same call run alone"


def test_last_error_is_per_thread(lrm):
    """two threads fail with different messages over and over while six succeed: each sees its own lrm_last_error()"""
    L = lrm.load()
    leg = lrm.get_M2_leg(0.0)
    lo, hi = C.c_size_t(0), C.c_size_t(0)

    def null_arg():
        seen = set()
        for _ in range(400):
            assert L.lrm_reach_cpu(None, 4, None, None, None, None) == LRM_EINVAL
            seen.add(L.lrm_last_error())
        return seen

    def bad_shard():
        seen = set()
        for _ in range(400):
            assert L.lrm_shard_bounds(100, 0, 0, 64, C.byref(lo), C.byref(hi)) == LRM_EINVAL
            seen.add(L.lrm_last_error())
        return seen

    def succeed(k):
        pts = random_cloud(5_000, seed=k)
        for _ in range(20):
            lrm.apply_reach_cpu(pts, leg)
            lrm.apply_ik_cpu(pts[:500], leg)
        return {L.lrm_last_error()}

    got = run_threads([null_arg, bad_shard] + [lambda k=k: succeed(k) for k in range(NTHREADS - 2)])
    assert got[0] == {b"null argument"}, got[0]
    assert got[1] == {b"bad shard arguments"}, got[1]
    for s in got[2:]:
        assert s == {b""}, s  # a thread that never failed has no message, whatever the others did


def test_device_calls_from_threads_without_a_device_report_enodev(lrm):
    """no CPU fallback, from any thread; on a machine with a GPU the same calls on empty clouds succeed"""
    L = lrm.load()
    legs = [np.ascontiguousarray(lrm.get_M2_leg(0.3 * k), np.float32) for k in range(NTHREADS)]
    have_dev = lrm.device_count() > 0
    one = C.c_void_p(16)

    def calls(k):
        lp = legs[k].ctypes.data_as(C.c_void_p)
        n = 0 if have_dev else 4
        p = None if have_dev else one
        rcs = [L.lrm_reach_bits_dev(p, p, p, n, lp, None, p, p, None),
               L.lrm_dist_dev(p, p, p, n, lp, None, p, p, p, p, None),
               L.lrm_reach_dist_bits_dev(p, p, p, n, lp, None, p, p, p, p, p, None),
               L.lrm_reach_aos_dev(p, n, lp, None, p, None),
               L.lrm_dist_aos_dev(p, n, lp, None, p, p, None)]
        if not have_dev:
            rcs.append(L.lrm_tol_prepare(lp, None, 250_000, None))
            rcs.append(L.lrm_reach_any_dev(one, one, one, 4, one, one, one, 4, lp, 1, None, one, one, None))
        return rcs, L.lrm_last_error()

    saved = lrm.get_mode()
    try:
        for mode in (lrm.MODE_STRICT, lrm.MODE_FAST, lrm.MODE_TOL, lrm.MODE_TOL_REL):
            lrm.set_mode(mode)
            for rcs, msg in run_threads([lambda k=k: calls(k) for k in range(NTHREADS)]):
                if have_dev:
                    assert rcs == [0] * len(rcs), rcs
                else:
                    assert rcs == [LRM_ENODEV] * len(rcs), (mode, rcs)
                    assert msg, "LRM_ENODEV without a message"
    finally:
        lrm.set_mode(saved)


def test_release_workspaces_can_be_called_repeatedly(lrm):
    for _ in range(3):
        lrm.release_workspaces()
    pts = random_cloud(1_000, seed=3)
    leg = lrm.get_moonbot_leg(0.4)
    m0, _ = lrm.apply_reach_cpu(pts, leg)
    lrm.release_workspaces()
    m1, _ = lrm.apply_reach_cpu(pts, leg)
    lrm.release_workspaces()
    assert np.array_equal(m0, m1)
