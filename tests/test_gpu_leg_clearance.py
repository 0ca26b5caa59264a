"""Leg link clearance on the device (run with -m gpu on an MI355X): PoseSet.leg_clearance / lrm_leg_clearance_posed_dev
against the host loop lrm_leg_clearance_posed_cpu bit for bit (hits, links, worst, pen bits, free) over cloud sizes around
the wave, chunk, tile, box-threshold and 64-tile-group boundaries, pose counts around the block and grid-stride
boundaries, 1, 6 and 8 legs, live_in forms, skipped legs, quaternion kinds, an inflation that culls nothing, the cull
scenes, 4e6 mm from the origin, four clouds through the shared box buffer and the NULL forms of the C ABI
(tests/test_leg_clearance_cpu.py ties that host loop to a numpy restatement of include/lrm.h); PoseSet.leg_joints against
its host form; the chain update -> footholds -> ik -> leg_clearance on ONE PoseSet against the host chain; a graph replay.
Every output is prefilled with a sentinel, so an unwritten entry fails too."""
import numpy as np
import pytest

import footholds_posed_cases as fc
import leg_clearance_cases as lc
import pair_cases as pc

pytestmark = pytest.mark.gpu

SENTINEL = -7
KEYS = ("hits", "links", "worst", "pen", "free")
FLT_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def soa(torch, pts):
    t = dev(torch, np.asarray(pts, np.float32).reshape(-1, 3).T)
    return t[0], t[1], t[2]


def legs_n(lrm, n):
    return pc.leg_families(lrm)[{1: "m2_1_identity", 6: "m2_6_tilted", 8: "m2_8_identity"}[n]][0]


def outputs(torch, nl, npz):
    return (torch.full((nl, npz), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((nl, npz), 0xA5, dtype=torch.uint8, device="cuda"),
            torch.full((nl, npz), SENTINEL, dtype=torch.int32, device="cuda"),
            torch.full((nl, npz), float(SENTINEL), dtype=torch.float32, device="cuda"), torch.full((npz,), 0xA5, dtype=torch.uint8, device="cuda"))


def run(lrm, torch, targets, quats, body, legs, ang, radius=lc.RADIUS, margin=lc.MARGIN, tip_clear=lc.TIP_CLEAR, live_in=None, pen=True,
        free=True, ps=None):
    """PoseSet.leg_clearance into sentinel-filled outputs -> numpy (hits, links, worst, pen or None, free or None)"""
    npz, nl = len(quats), len(legs)
    if ps is None:
        ps = lrm.PoseSet(legs, npz, ik=True)
    ps.update(dev(torch, quats), dev(torch, body))
    hits, links, worst, pn, fre = outputs(torch, nl, npz)
    live = None if live_in is None else dev(torch, np.asarray(live_in, np.uint8))
    tx, ty, tz = soa(torch, targets)
    a = dev(torch, np.asarray(ang, np.float32).reshape(-1, 3).T)
    if pen and free:
        ps.leg_clearance(tx, ty, tz, a, radius, margin, tip_clear, live, hits, links, worst, pn, fre)
    else:  # the NULL forms of the C ABI
        L, dp = lrm.load(), lambda t: None if t is None else t.data_ptr()
        r = np.array(radius, np.float32)
        rc = L.lrm_leg_clearance_posed_dev(dp(tx), dp(ty), dp(tz), len(targets), dp(ps.workspace), dp(ps.ik_workspace), npz, nl, dp(a[0]),
                                           dp(a[1]), dp(a[2]), r.ctypes.data, margin, tip_clear, dp(live), dp(hits), dp(links), dp(worst),
                                           dp(pn if pen else None), dp(fre if free else None), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    if not pen:
        assert (pn == float(SENTINEL)).all()
    if not free:
        assert (fre == 0xA5).all()
    return hits.cpu().numpy(), links.cpu().numpy(), worst.cpu().numpy(), pn.cpu().numpy() if pen else None, fre.cpu().numpy() if free else None


def check(lrm, torch, targets, quats, body, legs, ang, margin=lc.MARGIN, live_in=None, mixed=True, radius=lc.RADIUS, tip_clear=lc.TIP_CLEAR, **kw):
    want = lc.host(lrm, targets, quats, body, legs, ang, radius, margin, tip_clear, live_in)
    if mixed:  # hit legs, legs near without a hit or clear, and legs with no near target
        assert (want["hits"] > 0).any() and ((want["hits"] == 0) & (want["worst"] >= 0)).any() and (want["worst"] < 0).any()
    lc.assert_same(run(lrm, torch, targets, quats, body, legs, ang, radius, margin, tip_clear, live_in, **kw), want)
    lc.assert_consequences(want, margin, live_in)
    return want


def picked(lrm, nposes, nt, seed):
    """nt targets drawn (in order) from a scene of at least 600, so that a few targets still meet many legs"""
    quats, body, targets = lc.scene(lrm, nposes, max(nt, 600), seed)
    pick = np.sort(np.random.default_rng(seed).permutation(len(targets))[:nt])
    return quats, body, np.ascontiguousarray(targets[pick])


@pytest.mark.parametrize("nt", [1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025])
def test_cloud_sizes_without_boxes(lrm, torch_cuda, nt):
    quats, body, targets = picked(lrm, 150, nt, seed=nt % 89)
    check(lrm, torch_cuda, targets, quats, body, legs_n(lrm, 6), lc.random_angles(150, 6, seed=nt), mixed=nt >= 127)


@pytest.mark.parametrize("nt", [4095, 4096, 4097, 65 * 1024 + 77])
def test_cloud_sizes_around_the_box_threshold_and_past_a_tile_group(lrm, torch_cuda, nt):
    """4096 targets switch the box culls on; 65 tiles and a ragged 66th take a second lane = tile round"""
    legs = legs_n(lrm, 6)[:2]
    if nt <= 65 * 1024:
        quats, body, targets = lc.scene(lrm, 180, nt, seed=nt % 83)
    else:  # pair_cases.sized: the targets behind the first 64 tiles form a patch of their own with a third of the bodies
        body, targets = pc.sized(180, nt, 64 * 1024, seed=5)
        quats = fc.pose_quats(lrm, 180, seed=5)
        body[:, 2] += lc.OFFSETS[np.arange(180) % len(lc.OFFSETS)] - np.float32(60.0)
    want = check(lrm, torch_cuda, targets, quats, body, legs, lc.random_angles(180, 2, seed=3))
    if nt > 65 * 1024:  # some winners lie behind the first 64 tiles
        assert (want["worst"] >= 64 * 1024).sum() > 5 and (want["hits"][want["worst"] >= 64 * 1024] > 0).any()


@pytest.mark.parametrize("nposes", [1, 2, 3, 4, 5, 255, 256, 257])
def test_pose_counts(lrm, torch_cuda, nposes):
    quats, body, targets = lc.scene(lrm, 257, 5000, seed=nposes + 1)
    ang = lc.random_angles(nposes, 2, seed=nposes)
    check(lrm, torch_cuda, targets, quats[:nposes], body[:nposes], legs_n(lrm, 6)[:2], ang, mixed=nposes >= 255)


def test_pose_count_past_the_grid_stride(lrm, torch_cuda):
    """16384 workgroups x 4 waves hold 65 536 poses; 65 536 + 9 make the first waves take a second pose.  Almost all poses
    hover 1e6 mm away from the cloud, the first and the last 300 stand in it"""
    n = 65536 + 9
    legs = legs_n(lrm, 1)
    quats, body, targets = lc.scene(lrm, 600, 700, seed=17)
    q = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
    b = np.tile(np.array([1e6, -1e6, 5e5], np.float32), (n, 1))
    q[:300], b[:300], q[-300:], b[-300:] = quats[:300], body[:300], quats[300:], body[300:]
    want = check(lrm, torch_cuda, targets, q, b, legs, lc.random_angles(n, 1, seed=2))
    assert (want["hits"][:, 65536:] > 0).any() and (want["worst"][:, 300:-300] == -1).all()


@pytest.mark.parametrize("nlegs", [1, 6, 8])
def test_leg_counts_with_stance_angles(lrm, torch_cuda, nlegs):
    """angles from the host IK on the host foothold choice: legs that reach nothing carry nan angles and are skipped inside
    live poses; pose_quats holds non-unit and nan quaternions"""
    legs = legs_n(lrm, nlegs)
    quats, body, targets = lc.scene(lrm, 130, 4600, seed=30 + nlegs)
    ang, st, _ = lc.stance_angles(lrm, targets, quats, body, legs)
    assert (st == 0).any() and (st != 0).any()
    want = check(lrm, torch_cuda, targets, quats, body, legs, ang)
    skipped = (st == 0).reshape(nlegs, 130)
    assert (want["hits"][skipped] == 0).all() and (want["worst"][skipped] == -1).all()


def test_live_in_forms_dead_blocks_and_refused_views(lrm, torch_cuda):
    torch = torch_cuda
    legs = legs_n(lrm, 6)
    quats, body, targets = lc.scene(lrm, 200, 5000, seed=33)
    ang = lc.stance_angles(lrm, targets, quats, body, legs)[0]
    forms = lc.live_forms(lrm, targets, quats, body, legs)
    assert 0 < forms["all_legs"].sum() < 200
    for name, live in forms.items():
        want = check(lrm, torch, targets, quats, body, legs, ang, live_in=live, mixed=name != "zeros")
        if name == "zeros":
            assert (want["free"] == 0).all() and (want["worst"] == -1).all()
    live = np.ones(200, np.uint8)
    live[64:128] = 0  # the four waves of sixteen whole blocks
    live[130] = 0
    live[150] = 3
    check(lrm, torch, targets, quats, body, legs, ang, live_in=live)
    # refused by the binding, not read with the wrong stride, size, type or device
    ps = lrm.PoseSet(legs, 200, ik=True).update(dev(torch, quats), dev(torch, body))
    tx, ty, tz = soa(torch, targets)
    a = dev(torch, ang.T)
    wide = dev(torch, np.repeat(forms["all_legs"], 2))
    for kw in ({"live_in": wide[::2]}, {"live_in": wide[:100]}, {"hits": torch.empty((6, 200), dtype=torch.int64, device="cuda")},
               {"links": torch.empty((6, 100), dtype=torch.uint8, device="cuda")}, {"pen": torch.empty((6, 400), dtype=torch.float32, device="cuda")[:, ::2]},
               {"free": torch.empty(200, dtype=torch.uint8)}, {"worst": torch.empty((6, 200), dtype=torch.float32, device="cuda")}):
        with pytest.raises(ValueError):
            ps.leg_clearance(tx, ty, tz, a, lc.RADIUS, **kw)
    for bad in (a[:, :-1], a.double(), dev(torch, np.repeat(ang, 2, 0).T)[:, ::2], a.cpu(), a.reshape(-1)):
        with pytest.raises(ValueError):
            ps.leg_clearance(tx, ty, tz, bad, lc.RADIUS)
        with pytest.raises(ValueError):
            ps.leg_joints(bad)
    with pytest.raises(ValueError):
        ps.leg_clearance(tx, ty, tz, a, (1.0, 2.0))
    with pytest.raises(ValueError):  # a PoseSet without the IK table refuses
        lrm.PoseSet(legs, 200).update(dev(torch, quats), dev(torch, body)).leg_clearance(tx, ty, tz, a, lc.RADIUS)
    for kw in ({"margin": -1.0}, {"margin": float("nan")}, {"margin": float("inf")}, {"tip_clear": -1.0}, {"tip_clear": float("inf")}):
        with pytest.raises(lrm.LrmError):
            ps.leg_clearance(tx, ty, tz, a, lc.RADIUS, **kw)
    for r in ((-1.0, 1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0, float("inf"))):
        with pytest.raises(lrm.LrmError):
            ps.leg_clearance(tx, ty, tz, a, r)


def test_non_unit_and_nan_quaternions_in_single_poses(lrm, torch_cuda):
    import posed_cases
    legs = legs_n(lrm, 6)
    quats, body, targets = lc.scene(lrm, 160, 9000, seed=14)
    quats[:] = posed_cases.random_unit_quats(160, np.random.default_rng(3))
    quats[70] *= np.float32(1.3)   # the leg shrinks
    quats[71] *= np.float32(0.6)   # the leg grows far beyond a unit pose's reach
    quats[100, 2] = np.nan
    body[[70, 71]] = body[[2, 2]]
    want = check(lrm, torch_cuda, targets, quats, body, legs, lc.random_angles(160, 6, seed=5))
    assert (want["worst"][:, 100] == -1).all() and want["free"][100] == 1  # nan joints: every leg skipped


@pytest.mark.parametrize("margin", [FLT_MAX, 1e30])
def test_an_inflation_that_culls_nothing(lrm, torch_cuda, margin):
    """margin FLT_MAX: (radius + margin) * 1.0001 overflows, the inflation is +inf and no box is skipped; every finite target
    is near every tested link of every valid leg, so worst is the deepest target of the whole cloud"""
    quats, body, targets = lc.scene(lrm, 90, 6000, seed=6)
    targets[5::17] = np.nan
    want = check(lrm, torch_cuda, targets, quats, body, legs_n(lrm, 6), lc.random_angles(90, 6, seed=6), margin=margin, mixed=False)
    valid = np.isfinite(quats).all(1)
    assert (want["worst"][:, valid] >= 0).all() and (want["hits"] > 0).any()


@pytest.mark.parametrize("kind,nt", [("dense_cluster", 6000), ("sparse_tiles", 9 * 1024)])
def test_cull_scenes(lrm, torch_cuda, kind, nt):
    """sparse_tiles: every tile box is huge and touches every leg's box, while at most one of its chunk boxes does"""
    quats, body, targets = lc.scene(lrm, 160, nt, seed=2, kind=kind)
    if kind == "dense_cluster":
        body[:, 2] -= np.float32(60.0)
    check(lrm, torch_cuda, targets, quats, body, legs_n(lrm, 6), lc.random_angles(160, 6, seed=7), margin=15.0)


def test_bad_targets_and_bodies(lrm, torch_cuda):
    quats, body, targets = lc.scene(lrm, 100, 6000, seed=8)
    ang = lc.random_angles(100, 6, seed=8)
    bad_t = targets.copy()
    bad_t[::7] = np.nan
    bad_t[3::11, 1] = np.inf
    bad_t[5::13] = -np.inf
    bad_t[1024:1088] = np.nan  # a whole chunk of nan targets: an empty box
    check(lrm, torch_cuda, bad_t, quats, body, legs_n(lrm, 6), ang)
    bad_b = body.copy()
    bad_b[1] = np.nan
    bad_b[2, 0] = np.inf
    bad_b[35] = -np.inf
    bad_b[70, 2] = np.nan
    check(lrm, torch_cuda, targets, quats, bad_b, legs_n(lrm, 6), ang)


def test_far_from_the_origin(lrm, torch_cuda):
    """a cloud and bodies 4e6 mm from the origin, where the float32 grid is 0.25-0.5 mm: no box cull may drop a near target
    of the host loop.  The first half of the cloud is in x order: thin slabs whose faces decide"""
    quats, body, targets = lc.scene(lrm, 256, 8000, seed=9)
    body, targets = pc.translated(body, targets, 4e6)
    want = check(lrm, torch_cuda, targets, quats, body, legs_n(lrm, 6), lc.random_angles(256, 6, seed=9))
    assert (want["hits"] > 0).sum() > 40


def test_four_clouds_through_the_shared_box_buffer(lrm, torch_cuda):
    """clouds of different size on ONE PoseSet, larger, smaller, larger again, then one below the box threshold"""
    legs = legs_n(lrm, 6)
    ps = lrm.PoseSet(legs, 128, ik=True)
    for k, nt in enumerate((9000, 4500, 12000, 700)):
        quats, body, targets = lc.scene(lrm, 128, nt, seed=20 + k)
        ang = lc.random_angles(128, 6, seed=k)
        want = lc.host(lrm, targets, quats, body, legs, ang)
        assert (want["hits"] > 0).any() and (want["worst"] < 0).any()
        lc.assert_same(run(lrm, torch_cuda, targets, quats, body, legs, ang, ps=ps), want)


def test_null_outputs_zero_radii_and_tip_clear(lrm, torch_cuda):
    quats, body, targets = lc.scene(lrm, 90, 5000, seed=12)
    legs = legs_n(lrm, 6)
    ang = lc.random_angles(90, 6, seed=12)
    check(lrm, torch_cuda, targets, quats, body, legs, ang, pen=False)
    check(lrm, torch_cuda, targets, quats, body, legs, ang, free=False)
    check(lrm, torch_cuda, targets, quats, body, legs, ang, pen=False, free=False, margin=0.0, mixed=False)  # margin 0: near is hit
    check(lrm, torch_cuda, targets, quats, body, legs, ang, radius=(0.0, 22.0, 0.0))
    want = check(lrm, torch_cuda, targets, quats, body, legs, ang, radius=(0.0, 0.0, 0.0), mixed=False)
    assert (want["free"] == 1).all()
    check(lrm, torch_cuda, targets, quats, body, legs, ang, tip_clear=1e4)
    check(lrm, torch_cuda, targets, quats, body, legs, ang, tip_clear=0.0)
    got = run(lrm, torch_cuda, np.zeros((0, 3), np.float32), quats, body, legs, ang)  # nt == 0: the empty answer
    assert (got[0] == 0).all() and (got[1] == 0).all() and (got[2] == -1).all() and np.isneginf(got[3]).all() and (got[4] == 1).all()


@pytest.mark.parametrize("nposes", [1, 63, 64, 65, 255, 256, 257])
def test_leg_joints_against_the_host_form(lrm, torch_cuda, nposes):
    torch = torch_cuda
    legs = legs_n(lrm, 6)[:1 if nposes != 65 else 6]  # one leg: nposes entries; six: a leg's entries straddle waves
    quats, body, _ = lc.scene(lrm, 257, 600, seed=3)
    ang = lc.random_angles(nposes, len(legs), seed=nposes)
    ang[::9] = np.nan
    ps = lrm.PoseSet(legs, 257, ik=True).update(dev(torch, quats[:nposes]), dev(torch, body[:nposes]))
    for tc in (0.0, 30.0):
        out = torch.full((len(legs), nposes, 4, 3), float(SENTINEL), dtype=torch.float32, device="cuda")
        ps.leg_joints(dev(torch, ang.T), tc, out)
        torch.cuda.synchronize()
        want = lrm.leg_joints_posed_cpu(ang, quats[:nposes], body[:nposes], legs, tc)[0]
        assert np.array_equal(pc.bits(out.cpu().numpy()), pc.bits(want))


def test_chain_on_one_pose_set(lrm, torch_cuda):
    """update -> footholds -> ik -> leg_clearance(live_in=all_legs) on the SAME PoseSet against the host chain"""
    torch = torch_cuda
    legs = legs_n(lrm, 6)
    quats, body, targets = lc.main_scene(lrm, 256, 4600, seed=51)
    ps = lrm.PoseSet(legs, 256, ik=True, footholds=True).update(dev(torch, quats), dev(torch, body))
    tx, ty, tz = soa(torch, targets)
    count, best, best_d2, all_legs = ps.footholds(tx, ty, tz)
    pi, li = lrm.device.footholds_layout(256, 6, "cuda")
    ang, st = ps.ik(tx, ty, tz, pi, li, target_idx=best.view(-1))
    hits, links, worst, pen, free = ps.leg_clearance(tx, ty, tz, ang, lc.RADIUS, lc.MARGIN, lc.TIP_CLEAR, live_in=all_legs)
    torch.cuda.synchronize()
    h_ang, h_st, h_best = lc.stance_angles(lrm, targets, quats, body, legs)
    al = lrm.footholds_posed_cpu(targets, quats, body, legs, None)[3]
    assert np.array_equal(best.cpu().numpy(), h_best) and np.array_equal(all_legs.cpu().numpy(), al)
    assert np.array_equal(pc.bits(ang.cpu().numpy().T), pc.bits(h_ang)) and np.array_equal(st.cpu().numpy(), h_st)
    want = lc.host(lrm, targets, quats, body, legs, h_ang, live_in=al)
    lc.assert_same((hits.cpu().numpy(), links.cpu().numpy(), worst.cpu().numpy(), pen.cpu().numpy(), free.cpu().numpy()), want)
    assert 0 < want["free"].sum() < al.sum() < 256  # some poses that stand have a leg inside the terrain


def test_chain_replays_from_a_graph(lrm, torch_cuda):
    """update(), footholds(), ik() and leg_clearance() only launch once the box buffer holds the cloud's size: captured on ONE
    side stream after a warm call, replayed after new quaternions, bodies and targets were copied into the captured tensors"""
    torch = torch_cuda
    legs = legs_n(lrm, 6)
    q0, b0, t0 = lc.main_scene(lrm, 192, 5000, seed=41)
    q1, b1, t1 = lc.main_scene(lrm, 192, 5000, seed=42)
    qt, bt, tt = dev(torch, q0), dev(torch, b0), dev(torch, t0.T.copy())
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
    cnt, bst, bd, al = i32(6, 192), i32(6, 192), torch.empty((6, 192), dtype=torch.float32, device="cuda"), torch.empty(192, dtype=torch.uint8, device="cuda")
    ang, st = torch.empty((3, 6 * 192), dtype=torch.float32, device="cuda"), torch.empty(6 * 192, dtype=torch.uint8, device="cuda")
    hits, links, worst, pen, fre = outputs(torch, 6, 192)
    pi, li = lrm.device.footholds_layout(192, 6, "cuda")
    ps = lrm.PoseSet(legs, 256, ik=True, footholds=True)

    def work():
        ps.update(qt, bt)
        ps.footholds(tt[0], tt[1], tt[2], cnt, bst, bd, al)
        ps.ik(tt[0], tt[1], tt[2], pi, li, target_idx=bst.view(-1), out=ang, status=st, check=False)
        ps.leg_clearance(tt[0], tt[1], tt[2], ang, lc.RADIUS, lc.MARGIN, lc.TIP_CLEAR, al, hits, links, worst, pen, fre)

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
        for t, v in ((hits, SENTINEL), (links, 0xA5), (worst, SENTINEL), (pen, SENTINEL), (fre, 0xA5)):
            t.fill_(v)
        g.replay()
    torch.cuda.synchronize()
    h_ang = lc.stance_angles(lrm, t1, q1, b1, legs)[0]
    live = lrm.footholds_posed_cpu(t1, q1, b1, legs, None)[3]
    assert np.array_equal(al.cpu().numpy(), live) and 0 < live.sum() < 192
    want = lc.host(lrm, t1, q1, b1, legs, h_ang, live_in=live)
    assert (want["hits"] > 0).any() and (want["free"] == 1).any()
    lc.assert_same((hits.cpu().numpy(), links.cpu().numpy(), worst.cpu().numpy(), pen.cpu().numpy(), fre.cpu().numpy()), want)
    del g
