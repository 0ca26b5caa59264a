"""Stance stability on the device (run with -m gpu on an MI355X): device.stance_stability / PoseSet.stance_stability /
lrm_stance_stability_dev against the host loop lrm_stance_stability_cpu bit for bit (margin bits, edge, stable, feet) over
stance counts around the wave, block and grid-stride boundaries, lift-set counts around the 64-set rounds of the kernel's
second phase, 1, 3, 6 and 8 legs, every bad-foot, bad-pose, dead-stance and live_in form at the first, second, middle and last
positions of a 64-stance group, the hand-made stances, plane forms, clouds of 0 and 1 targets, 4e6 mm from the origin and the
NULL forms of the C ABI (tests/test_stance_cpu.py ties that host loop to a numpy restatement of include/lrm.h); the edge form
and the chain update -> footholds -> stance_stability -> body_clearance on ONE PoseSet against the host chains; a graph
replay; two streams.  Every output is prefilled with a sentinel, so an unwritten entry fails too."""
import os
import re

import numpy as np
import pytest

import pair_cases as pc
import stance_cases as sc

pytestmark = pytest.mark.gpu

F = np.float32
SENT_F, SENT_B = -7.0, 0xA5
GRID_STANCES = 65536  # kMaxGrid workgroups of four waves, one stance per wave
WAVES = 4
SPOTS = (0, 1, 31, 32, 62, 63)
COM = [30.0, 10.0, -5.0]


def test_the_constants_are_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged-robot-movability-cuda_amd", "csrc",
                            "lrm_stance.hip")).read()
    assert int(re.search(r"constexpr unsigned kMaxGrid = (\d+);", src).group(1)) * WAVES == GRID_STANCES
    assert int(re.search(r"constexpr int kBlock = (\d+);", src).group(1)) == 64 * WAVES
    assert int(re.search(r"m0 < P\.nmasks; m0 \+= (\d+)\)", src).group(1)) == 64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def soa(torch, pts):
    pts = np.asarray(pts, F).reshape(-1, 3)
    t = dev(torch, pts.T) if len(pts) else torch.empty((3, 0), dtype=torch.float32, device="cuda")
    return t[0], t[1], t[2]


def outputs(torch, nm, ns):
    return (torch.full((nm, ns), SENT_F, dtype=torch.float32, device="cuda"), torch.full((nm, ns), SENT_B, dtype=torch.uint8, device="cuda"),
            torch.full((nm, ns), SENT_B, dtype=torch.uint8, device="cuda"), torch.full((ns,), SENT_B, dtype=torch.uint8, device="cuda"))


def run(lrm, torch, targets, foot, quats, body=None, pose_idx=None, com=None, plane=None, lift=None, min_margin=0.0, live_in=None, edge=True,
        feet=True):
    """device.stance_stability into sentinel-filled outputs -> numpy (margin, edge or None, stable, feet or None)"""
    nl, ns = foot.shape
    lf = lrm.stance_lift(lift, nl)
    m, e, st, ft = outputs(torch, len(lf), ns)
    tx, ty, tz = soa(torch, targets)
    q, b, fo = dev(torch, np.asarray(quats, F)), dev(torch, None if body is None else np.asarray(body, F)), dev(torch, np.asarray(foot, np.int32))
    pi = dev(torch, None if pose_idx is None else np.asarray(pose_idx, np.int32))
    lv = dev(torch, None if live_in is None else np.asarray(live_in, np.uint8))
    if edge and feet:
        lrm.device.stance_stability(tx, ty, tz, fo, q, b, pi, com, plane, lift, min_margin, lv, m, e, st, ft)
    else:  # the NULL forms of the C ABI
        dp = lambda t: None if t is None else t.data_ptr()
        hp = lambda a: None if a is None else a.ctypes.data
        cm, pl = None if com is None else np.ascontiguousarray(com, F), None if plane is None else np.ascontiguousarray(plane, F).reshape(6)
        rc = lrm.load().lrm_stance_stability_dev(dp(tx), dp(ty), dp(tz), tx.numel(), dp(q), dp(b), len(quats), dp(pi), dp(fo), ns, nl, hp(cm), hp(pl),
                                                 hp(lf), len(lf), float(min_margin), dp(lv), dp(m), dp(e if edge else None), dp(st),
                                                 dp(ft if feet else None), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    if not edge:
        assert (e == SENT_B).all()
    if not feet:
        assert (ft == SENT_B).all()
    return m.cpu().numpy(), e.cpu().numpy() if edge else None, st.cpu().numpy(), ft.cpu().numpy() if feet else None


def check(lrm, torch, targets, foot, quats, body=None, pose_idx=None, com=None, plane=None, lift=None, min_margin=0.0, live_in=None, mixed=True,
          **kw):
    want = sc.host(lrm, targets, foot, quats, body, pose_idx, com, plane, lift, min_margin, live_in)
    if mixed:  # stable, unstable and -inf answers
        assert min(sc.kinds(want)) > 0, sc.kinds(want)
    sc.assert_same(run(lrm, torch, targets, foot, quats, body, pose_idx, com, plane, lift, min_margin, live_in, **kw), want)
    sc.assert_consequences(want, min_margin)
    return want


@pytest.mark.parametrize("ns", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257])
def test_stance_counts(lrm, torch_cuda, ns):
    targets, foot, quats, body = sc.synthetic(ns, 6, seed=ns)
    check(lrm, torch_cuda, targets, foot, quats, body, com=COM, lift="each", mixed=ns >= 63)


def test_stance_count_past_the_grid_stride(lrm, torch_cuda):
    """kMaxGrid workgroups hold 65 536 stances; a workgroup and one more make the first five waves take a second stance"""
    ns = GRID_STANCES + WAVES + 1
    targets, foot, quats, body = sc.synthetic(ns, 6, seed=3)
    want = check(lrm, torch_cuda, targets, foot, quats, body, com=COM, lift=[0, 0b000101])
    assert (want["stable"][:, GRID_STANCES:] == 1).any() and (want["feet"][GRID_STANCES:] != 0).all()


@pytest.mark.parametrize("nm", [1, 7, 63, 64, 65, 128, 255, 256])
def test_lift_set_counts(lrm, torch_cuda, nm):
    """the lift sets of eight legs in a shuffled order, cut to nm: 64 sets fill a round of the second phase, 65 start another"""
    targets, foot, quats, body = sc.synthetic(70, 8, seed=nm, missing=0.15)
    lift = np.random.default_rng(nm).permutation(256)[:nm].astype(np.uint8)
    if nm >= 7:
        lift[:7] = [0, 1, 2, 4, 0x55, 0xAA, 0xFF]
    check(lrm, torch_cuda, targets, foot, quats, body, com=COM, lift=lift, mixed=nm >= 7)


@pytest.mark.parametrize("nlegs", [1, 3, 6, 8])
def test_leg_counts(lrm, torch_cuda, nlegs):
    targets, foot, quats, body = sc.synthetic(130, nlegs, seed=20 + nlegs)
    want = check(lrm, torch_cuda, targets, foot, quats, body, com=[20.0, -10.0, 5.0], lift=sc.lift_all(nlegs), mixed=nlegs >= 3)
    if nlegs == 1:
        assert np.isneginf(want["margin"]).all()


def spots(ns):
    return np.array([g + s for g in range(0, ns, 64) for s in SPOTS if g + s < ns])


def test_bad_feet_and_targets_at_the_ends_of_a_group(lrm, torch_cuda):
    ns = 192
    at = spots(ns)
    imin, imax = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    for k, bad in enumerate((-1, "nt", imin, imax, "nan", "inf")):
        targets, foot, quats, body = sc.synthetic(ns, 6, seed=40 + k, missing=0.0)
        nt = len(targets)
        leg = k % 6
        if bad == "nan":
            targets = np.concatenate([targets, np.array([[np.nan, 0, 0]], F)])
            foot[leg, at] = nt
        elif bad == "inf":
            targets = np.concatenate([targets, np.array([[0, -np.inf, 0]], F), np.array([[0, 0, np.inf]], F)])
            foot[leg, at[::2]], foot[leg, at[1::2]] = nt, nt + 1
        else:
            foot[leg, at] = nt if bad == "nt" else bad
        want = check(lrm, torch_cuda, targets, foot, quats, body, com=COM, lift="each", mixed=False)
        assert (want["feet"][at] == 63 & ~(1 << leg)).all() and (np.delete(want["feet"], at) == 63).all()
    # all six legs bad at the spots: no foot, -inf
    foot[:, at] = -1
    want = check(lrm, torch_cuda, targets, foot, quats, body, com=COM, lift="each", mixed=False)
    assert (want["feet"][at] == 0).all() and np.isneginf(want["margin"][:, at]).all()


def test_bad_poses_dead_stances_and_live_in_at_the_ends_of_a_group(lrm, torch_cuda):
    ns = 192
    at = spots(ns)
    targets, foot, quats, body = sc.synthetic(ns, 6, seed=50, missing=0.25)
    q = quats.copy()
    q[at[0::3], 2], q[at[1::3], 0], q[at[2::3]] = np.nan, np.inf, q[at[2::3]] * F(0.6)
    want = check(lrm, torch_cuda, targets, foot, q, body, lift="each")  # a zero com: every stance stays live
    assert (want["feet"][at] != 0).any()
    want = check(lrm, torch_cuda, targets, foot, q, body, com=COM, lift="each")
    assert (want["feet"][at[0::3]] == 0).all() and (want["feet"][at[1::3]] == 0).all() and (want["feet"][at[2::3]] != 0).any()
    b = body.copy()
    b[at[0::3]], b[at[1::3], 1], b[at[2::3], 2] = np.nan, np.inf, -np.inf
    want = check(lrm, torch_cuda, targets, foot, quats, b, com=COM, lift="each")
    assert (want["feet"][at] == 0).all()
    check(lrm, torch_cuda, targets, foot, quats, None, com=COM, lift="each", mixed=False)  # body NULL
    rng = np.random.default_rng(5)
    for pose_idx in (rng.permutation(ns), rng.integers(0, ns, ns), np.full(ns, 17)):
        check(lrm, torch_cuda, targets, foot, quats, body, pose_idx.astype(np.int32), com=COM, lift="each", mixed=False)
    pi = rng.permutation(ns).astype(np.int32)
    pi[at[0::3]], pi[at[1::3]], pi[at[2::3]] = -1, ns, np.iinfo(np.int32).min
    want = check(lrm, torch_cuda, targets, foot, quats, body, pi, com=COM, lift="each")
    assert (want["feet"][at] == 0).all() and (np.delete(want["feet"], at) != 0).any()
    t2, f2, _, _ = sc.synthetic(500, 6, seed=51)  # more stances than poses
    check(lrm, torch_cuda, t2, f2, quats, body, rng.integers(0, ns, 500).astype(np.int32), com=COM, lift="each")
    live = np.ones(ns, np.uint8)
    live[at] = 0
    live[5], live[64:128] = 3, 0  # the four waves of sixteen whole blocks
    for lv in (np.ones(ns, np.uint8), np.zeros(ns, np.uint8), live):
        want = check(lrm, torch_cuda, targets, foot, quats, body, com=COM, lift="each", live_in=lv, mixed=lv.any())
        assert (want["feet"][lv == 0] == 0).all()


@pytest.mark.parametrize("name", sorted(sc.hand_made()))
def test_hand_made_stances(lrm, torch_cuda, name):
    targets, foot, com, expect = sc.hand_made()[name]
    want = check(lrm, torch_cuda, targets, foot, sc.IDENTITY, None, com=com, mixed=False)
    assert float(want["margin"][0, 0]) == expect["margin"] and int(want["edge"][0, 0]) == expect["edge"]
    check(lrm, torch_cuda, targets, foot, sc.IDENTITY, None, com=com, lift=sc.lift_all(len(foot)), mixed=False)


def test_plane_forms_and_min_margin(lrm, torch_cuda):
    targets, foot, quats, body = sc.synthetic(140, 6, seed=15)
    com = [25.0, -15.0, 10.0]
    a = check(lrm, torch_cuda, targets, foot, quats, body, com=com, lift="each")
    b = check(lrm, torch_cuda, targets, foot, quats, body, com=com, lift="each", plane=[[1, 0, 0], [0, 1, 0]])
    assert np.array_equal(pc.bits(a["margin"]), pc.bits(b["margin"]))
    t = np.deg2rad(20.0)
    check(lrm, torch_cuda, targets, foot, quats, body, com=com, lift="each", plane=[[1, 0, 0], [0, np.cos(t), np.sin(t)]])
    check(lrm, torch_cuda, targets, foot, quats, body, com=com, lift="each", plane=[[0, 1, 0], [1, 0, 0]])
    c = check(lrm, torch_cuda, targets, foot, quats, body, com=com, lift="each", min_margin=25.0)
    assert (a["stable"] != c["stable"]).any()


def test_clouds_of_zero_and_one_target(lrm, torch_cuda):
    _, foot, quats, body = sc.synthetic(70, 6, seed=16)
    want = check(lrm, torch_cuda, np.zeros((0, 3), F), foot, quats, body, com=COM, lift="each", mixed=False)
    assert (want["feet"] == 0).all() and np.isneginf(want["margin"]).all()
    foot = np.where(foot >= 0, foot % 2, foot).astype(np.int32)  # 0 is the one target, 1 is past the cloud
    want = check(lrm, torch_cuda, np.array([[120.0, -40.0, 3.0]], F), foot, quats, body, com=COM, lift="each", mixed=False)
    assert (want["feet"] != 0).any() and np.isneginf(want["margin"]).all()  # coincident feet


def test_far_from_the_origin(lrm, torch_cuda):
    """cloud and bodies 4e6 mm from the origin, where the float32 grid is 0.25-0.5 mm: the feet are few-grid-step multiples and
    many cross products are exactly 0"""
    targets, foot, quats, body = sc.synthetic(256, 6, seed=9, offset=4e6)
    want = check(lrm, torch_cuda, targets, foot, quats, body, com=COM, lift="each")
    assert (want["stable"] == 1).sum() > 40


def test_null_outputs(lrm, torch_cuda):
    targets, foot, quats, body = sc.synthetic(100, 6, seed=12)
    for kw in ({"edge": False}, {"feet": False}, {"edge": False, "feet": False}):
        check(lrm, torch_cuda, targets, foot, quats, body, com=COM, lift="each", **kw)


def test_refused_views_and_every_einval(lrm, torch_cuda):
    torch = torch_cuda
    targets, foot, quats, body = sc.synthetic(64, 6, seed=13)
    tx, ty, tz = soa(torch, targets)
    q, b, fo = dev(torch, quats), dev(torch, body), dev(torch, foot)
    call = lambda **kw: lrm.device.stance_stability(tx, ty, tz, kw.pop("foot", fo), kw.pop("quats", q), kw.pop("body", b), **kw)
    call()
    wide_f, wide_q = dev(torch, np.repeat(foot, 2, 1)), dev(torch, np.repeat(quats, 2, 0))
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device="cuda")
    for kw in ({"foot": wide_f[:, ::2]}, {"foot": fo.long()}, {"foot": fo.cpu()}, {"foot": fo.view(-1)}, {"foot": dev(torch, np.zeros((9, 64), np.int32))},
               {"quats": wide_q[::2]}, {"quats": q.double()}, {"quats": q[:, :3]}, {"quats": q[:63]}, {"body": b[:63]}, {"body": b.double()},
               {"body": dev(torch, np.repeat(body, 2, 0))[::2]}, {"pose_idx": torch.zeros(64, dtype=torch.int64, device="cuda")},
               {"pose_idx": torch.zeros(128, dtype=torch.int32, device="cuda")[::2]}, {"pose_idx": torch.zeros(63, dtype=torch.int32, device="cuda")},
               {"live_in": u8(128)[::2]}, {"live_in": u8(63)}, {"live_in": torch.empty(64, dtype=torch.uint8)},
               {"margin": torch.empty((1, 64), dtype=torch.float64, device="cuda")}, {"margin": torch.empty((1, 63), dtype=torch.float32, device="cuda")},
               {"edge": u8(1, 128)[:, ::2]}, {"stable": u8(1, 32)}, {"feet": torch.empty(64, dtype=torch.int32, device="cuda")},
               {"stable": u8(3, 64), "lift": "each"}, {"lift": "all"}, {"lift": [256]}, {"lift": np.zeros(257, np.uint8)}, {"lift": []},
               {"com": [1.0, 2.0]}, {"plane": [1.0, 0.0, 0.0]}):
        with pytest.raises(ValueError):
            call(**kw)
    for kw in ({"lift": [64]}, {"lift": [0, 128]}, {"min_margin": -1.0}, {"min_margin": float("nan")}, {"min_margin": float("inf")},
               {"com": [np.nan, 0, 0]}, {"com": [0, 0, np.inf]}, {"plane": [[1, 0, 0], [0, np.nan, 0]]}, {"plane": [[np.inf, 0, 0], [0, 1, 0]]}):
        with pytest.raises(lrm.LrmError):
            call(**kw)
    # the C ABI's own checks, in its order; nothing is launched
    L, dp = lrm.load(), lambda t: t.data_ptr()
    m, e, st, ft = outputs(torch, 1, 64)
    lf = np.zeros(256, np.uint8)
    big = 2 ** 31
    ok = dict(nt=len(targets), nposes=64, pose_idx=None, foot=dp(fo), ns=64, nl=6, lift=lf.ctypes.data, nm=1, quats=dp(q), margin=dp(m), stable=dp(st))

    def rc(**kw):
        a = dict(ok, **kw)
        return L.lrm_stance_stability_dev(dp(tx), dp(ty), dp(tz), a["nt"], a["quats"], dp(b), a["nposes"], a["pose_idx"], a["foot"], a["ns"], a["nl"],
                                          None, None, a["lift"], a["nm"], 0.0, None, a["margin"], dp(e), a["stable"], dp(ft),
                                          torch.cuda.current_stream().cuda_stream)

    assert rc() == 0
    for kw in (dict(nl=0), dict(nl=9), dict(nm=0), dict(nm=257), dict(nt=big), dict(nposes=big), dict(ns=big), dict(ns=2 ** 24, nposes=2 ** 24, nm=256),
               dict(lift=None), dict(nposes=63), dict(foot=None), dict(quats=None), dict(margin=None), dict(stable=None)):
        assert rc(**kw) == -1, kw
    assert rc(ns=0, foot=None, margin=None) == 0  # nstances == 0 is a no-op
    torch.cuda.synchronize()
    # a PoseSet checks the poses and legs against its own
    ps = lrm.PoseSet(sc.legs_n(lrm, 6), 64, footholds=True)
    with pytest.raises(ValueError):
        ps.stance_stability(tx, ty, tz, fo, q, b)  # before update()
    ps.update(q, b)
    ps.stance_stability(tx, ty, tz, fo, q, b)
    for args in ((fo[:5], q, b), (fo, q[:60], b[:60]), (fo.view(-1), q, b)):
        with pytest.raises(ValueError):
            ps.stance_stability(tx, ty, tz, *args)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def main(lrm):
    return sc.main_scene(lrm, nposes=192, nt=3000, seed=2)


def test_edge_form_against_the_host_chain(lrm, torch_cuda, main):
    """foot = foothold_edges()'s best, pose_idx = edge_a, then edge_b: can the robot stand in either pose on the common feet"""
    torch = torch_cuda
    targets, _, quats, body, legs = main
    n = len(quats)
    rng = np.random.default_rng(7)
    ea = rng.integers(0, n, 300).astype(np.int32)
    eb = np.clip(ea + rng.integers(-2, 3, 300), 0, n - 1).astype(np.int32)
    ps = lrm.PoseSet(legs, n, footholds=True, nominal=sc.nominal_ring(6))
    q, b = dev(torch, quats), dev(torch, body)
    ps.update(q, b)
    tx, ty, tz = soa(torch, targets)
    da, db = dev(torch, ea), dev(torch, eb)
    best = ps.foothold_edges(tx, ty, tz, da, db)[1]
    h_best = lrm.foothold_edges_posed_cpu(targets, quats, body, legs, ea, eb, sc.nominal_ring(6))[1]
    assert np.array_equal(best.cpu().numpy(), h_best)
    for pose_idx, dpi in ((ea, da), (eb, db)):
        got = ps.stance_stability(tx, ty, tz, best, q, b, pose_idx=dpi, com=sc.COM, lift="each")
        torch.cuda.synchronize()
        want = sc.host(lrm, targets, h_best, quats, body, pose_idx, com=sc.COM, lift="each")
        sc.assert_same(tuple(t.cpu().numpy() for t in got), want)
        assert min(sc.kinds(want)) > 0


def test_chain_on_one_pose_set(lrm, torch_cuda, main):
    """update -> footholds -> stance_stability(lift="each") -> body_clearance(live_in = stable[0]) on ONE PoseSet"""
    torch = torch_cuda
    targets, h_foot, quats, body, legs = main
    n = len(quats)
    cyl = (120.0, 60.0, -40.0, -400.0)
    ps = lrm.PoseSet(legs, n, footholds=True, nominal=sc.nominal_ring(6))
    q, b = dev(torch, quats), dev(torch, body)
    ps.update(q, b)
    tx, ty, tz = soa(torch, targets)
    best = ps.footholds(tx, ty, tz)[1]
    margin, edge, stable, feet = ps.stance_stability(tx, ty, tz, best, q, b, com=sc.COM, lift="each")
    hits, top, height, free = ps.body_clearance(tx, ty, tz, *cyl, live_in=stable[0])
    torch.cuda.synchronize()
    assert np.array_equal(best.cpu().numpy(), h_foot)
    want = sc.host(lrm, targets, h_foot, quats, body, com=sc.COM, lift="each")
    sc.assert_same((margin.cpu().numpy(), edge.cpu().numpy(), stable.cpu().numpy(), feet.cpu().numpy()), want)
    h = lrm.body_clearance_posed_cpu(targets, quats, body, legs, *cyl, live_in=want["stable"][0])
    assert np.array_equal(hits.cpu().numpy(), h[0]) and np.array_equal(top.cpu().numpy(), h[1]) and np.array_equal(free.cpu().numpy(), h[3])
    assert np.array_equal(pc.bits(height.cpu().numpy()), pc.bits(h[2]))
    assert 0 < want["stable"][0].sum() < n and (h[3] <= want["stable"][0]).all()


def test_chain_replays_from_a_graph(lrm, torch_cuda):
    """update(), footholds() and stance_stability() only launch once the box buffer holds the cloud's size: captured on ONE side
    stream after a warm call, replayed after new quaternions, bodies and targets were copied into the captured tensors"""
    torch = torch_cuda
    t0, _, q0, b0, legs = sc.main_scene(lrm, nposes=128, nt=4500, seed=41)
    t1, f1, q1, b1, _ = sc.main_scene(lrm, nposes=128, nt=4500, seed=42)
    qt, bt, tt = dev(torch, q0), dev(torch, b0), dev(torch, t0.T.copy())
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
    cnt, bst, bd, al = i32(6, 128), i32(6, 128), torch.empty((6, 128), dtype=torch.float32, device="cuda"), torch.empty(128, dtype=torch.uint8, device="cuda")
    m, e, st, ft = outputs(torch, 7, 128)
    ps = lrm.PoseSet(legs, 128, footholds=True, nominal=sc.nominal_ring(6))

    def work():
        ps.update(qt, bt)
        ps.footholds(tt[0], tt[1], tt[2], cnt, bst, bd, al)
        ps.stance_stability(tt[0], tt[1], tt[2], bst, qt, bt, None, sc.COM, None, "each", 0.0, None, m, e, st, ft)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the warm call outside the capture: the box buffer grows here
        work()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            work()
        qt.copy_(dev(torch, q1))
        bt.copy_(dev(torch, b1))
        tt.copy_(dev(torch, t1.T.copy()))
        for t, v in ((m, SENT_F), (e, SENT_B), (st, SENT_B), (ft, SENT_B)):
            t.fill_(v)
        g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bst.cpu().numpy(), f1)
    want = sc.host(lrm, t1, f1, q1, b1, com=sc.COM, lift="each")
    assert min(sc.kinds(want)) > 0
    sc.assert_same((m.cpu().numpy(), e.cpu().numpy(), st.cpu().numpy(), ft.cpu().numpy()), want)
    del g


def test_two_streams_next_to_footholds(lrm, torch_cuda, main):
    """stance_stability uses no shared buffer: on a second stream it runs while footholds() of another cloud size walks its cloud
    on the first; both answers are the host's"""
    torch = torch_cuda
    targets, h_foot, quats, body, legs = main
    n = len(quats)
    t2, _, q2, b2, _ = sc.main_scene(lrm, nposes=n, nt=6000, seed=8)
    ps = lrm.PoseSet(legs, n, footholds=True, nominal=sc.nominal_ring(6))
    q, b, fo = dev(torch, quats), dev(torch, body), dev(torch, h_foot)
    dq2, db2 = dev(torch, q2), dev(torch, b2)
    tx, ty, tz = soa(torch, targets)
    ux, uy, uz = soa(torch, t2)
    ps.update(dq2, db2)
    ps.footholds(ux, uy, uz)  # warm: the box buffer holds the larger cloud
    m, e, st, ft = outputs(torch, 7, n)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(s1):
            best = ps.footholds(ux, uy, uz)[1]
        with torch.cuda.stream(s2):
            lrm.device.stance_stability(tx, ty, tz, fo, q, b, None, sc.COM, None, "each", 0.0, None, m, e, st, ft)
    torch.cuda.synchronize()
    want = sc.host(lrm, targets, h_foot, quats, body, com=sc.COM, lift="each")
    sc.assert_same((m.cpu().numpy(), e.cpu().numpy(), st.cpu().numpy(), ft.cpu().numpy()), want)
    assert np.array_equal(best.cpu().numpy(), lrm.footholds_posed_cpu(t2, q2, b2, legs, sc.nominal_ring(6))[1])
