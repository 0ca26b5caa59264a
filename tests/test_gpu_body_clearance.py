"""Body clearance on the device (run with -m gpu on an MI355X): PoseSet.body_clearance / lrm_body_clearance_posed_dev
against the host loop lrm_body_clearance_posed_cpu bit for bit (hits, top, height bits, free) over cloud sizes around the
wave, chunk, tile, box-threshold and 64-tile-group boundaries, pose counts around the block and grid-stride boundaries,
live_in forms, quaternion kinds, the uncullable scalars, the box-slack case 4e6 mm from the origin, two clouds through the
shared box buffer and the NULL forms of the C ABI (tests/test_body_clearance_cpu.py ties that host loop to a brute force
over the oracle); free against any_in_cylinder under the identity quaternion; the chain update -> footholds ->
body_clearance(all_legs) -> foothold_support(free) -> ik on ONE PoseSet; a graph replay; and one scale case against the
oracle's arithmetic on an eighth of the reference terrain.  Every output is prefilled with a sentinel, so an unwritten
entry fails too."""
import numpy as np
import pytest

import body_clearance_cases as bc
import footholds_posed_cases as fc
import pair_cases as pc

pytestmark = pytest.mark.gpu

SENTINEL = -7
CYL = (181.0, bc.PLUS_Z, -110.0, -410.0)  # radius, plus_z, minus_z, floor_z


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


def run(lrm, torch, targets, quats, body, legs, cyl=CYL, live_in=None, height=True, free=True, ps=None):
    """PoseSet.body_clearance into sentinel-filled outputs -> numpy (hits, top, height or None, free or None)"""
    npz = len(quats)
    if ps is None:
        ps = lrm.PoseSet(legs, npz, footholds=True)
    ps.update(dev(torch, quats), dev(torch, body))
    hits = torch.full((npz,), SENTINEL, dtype=torch.int32, device="cuda")
    top = torch.full((npz,), SENTINEL, dtype=torch.int32, device="cuda")
    hgt = torch.full((npz,), float(SENTINEL), dtype=torch.float32, device="cuda")
    fre = torch.full((npz,), 0xA5, dtype=torch.uint8, device="cuda")
    live = None if live_in is None else dev(torch, np.asarray(live_in, np.uint8))
    tx, ty, tz = soa(torch, targets)
    if height and free:
        ps.body_clearance(tx, ty, tz, cyl[0], cyl[1], cyl[2], cyl[3], live, hits, top, hgt, fre)
    else:  # the NULL forms of the C ABI
        L, dp = lrm.load(), lambda t: None if t is None else t.data_ptr()
        rc = L.lrm_body_clearance_posed_dev(dp(tx), dp(ty), dp(tz), len(targets), dp(ps.workspace), dp(ps.fh_workspace), npz, len(legs),
                                            cyl[0], cyl[1], cyl[2], cyl[3], dp(live), dp(hits), dp(top), dp(hgt if height else None),
                                            dp(fre if free else None), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    if not height:
        assert (hgt == float(SENTINEL)).all()
    if not free:
        assert (fre == 0xA5).all()
    return hits.cpu().numpy(), top.cpu().numpy(), hgt.cpu().numpy() if height else None, fre.cpu().numpy() if free else None


def check(lrm, torch, targets, quats, body, legs, cyl=CYL, live_in=None, mixed=True, **kw):
    want = bc.host(lrm, targets, quats, body, legs, cyl[0], cyl[1], cyl[2], cyl[3], live_in)
    if mixed:  # colliding poses, free ones over terrain, and empty columns
        assert (want["hits"] > 0).any() and ((want["hits"] == 0) & (want["top"] >= 0)).any() and (want["top"] < 0).any()
    bc.assert_same(run(lrm, torch, targets, quats, body, legs, cyl, live_in, **kw), want)
    bc.assert_consequences(want, live_in)
    return want


def legs6(lrm):
    return pc.leg_families(lrm)["m2_6_tilted"][0]


def picked(lrm, nposes, nt, seed):
    """nt targets drawn (in order) from a scene of at least 600, so that a few targets still meet many bodies"""
    quats, body, targets = bc.scene(lrm, nposes, max(nt, 600), seed)
    pick = np.sort(np.random.default_rng(seed).permutation(len(targets))[:nt])
    return quats, body, np.ascontiguousarray(targets[pick])


@pytest.mark.parametrize("nt", [0, 1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025])
def test_cloud_sizes_without_boxes(lrm, torch_cuda, nt):
    quats, body, targets = picked(lrm, 150, nt, seed=nt % 89)
    check(lrm, torch_cuda, targets, quats, body, legs6(lrm), mixed=nt >= 63)


@pytest.mark.parametrize("nt", [4095, 4096, 4097, 65 * 1024 + 77])
def test_cloud_sizes_around_the_box_threshold_and_past_a_tile_group(lrm, torch_cuda, nt):
    """4096 targets switch the box culls on; 65 tiles and a ragged 66th take a second lane = tile round"""
    if nt <= 65 * 1024:
        quats, body, targets = bc.scene(lrm, 180, nt, seed=nt % 83)
    else:  # pair_cases.sized: the targets behind the first 64 tiles form a patch of their own with a third of the bodies
        body, targets = pc.sized(180, nt, 64 * 1024, seed=5)
        quats = fc.pose_quats(lrm, 180, seed=5)
        body[:, 2] += bc.OFFSETS[np.arange(180) % len(bc.OFFSETS)]
    want = check(lrm, torch_cuda, targets, quats, body, legs6(lrm))
    if nt > 65 * 1024:  # some winners lie behind the first 64 tiles
        assert (want["top"] >= 64 * 1024).sum() > 5 and (want["hits"][want["top"] >= 64 * 1024] > 0).any()


@pytest.mark.parametrize("nposes", [1, 2, 3, 4, 5, 255, 256, 257])
def test_pose_counts(lrm, torch_cuda, nposes):
    quats, body, targets = bc.scene(lrm, 257, 5000, seed=nposes + 1)
    check(lrm, torch_cuda, targets, quats[:nposes], body[:nposes], legs6(lrm)[:2], mixed=nposes >= 255)


def test_pose_count_past_the_grid_stride(lrm, torch_cuda):
    """16384 workgroups x 4 waves hold 65 536 poses; 65 536 + 9 make the first waves take a second pose.  Almost all poses
    hover 1e6 mm away from the cloud, the first and the last 300 stand in it"""
    n = 65536 + 9
    legs = legs6(lrm)[:1]
    quats, body, targets = bc.scene(lrm, 600, 700, seed=17)
    q = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
    b = np.tile(np.array([1e6, -1e6, 5e5], np.float32), (n, 1))
    q[:300], b[:300], q[-300:], b[-300:] = quats[:300], body[:300], quats[300:], body[300:]
    want = check(lrm, torch_cuda, targets, q, b, legs)
    assert (want["hits"][65536:] > 0).any() and (want["top"][300:-300] == -1).all()


def test_live_in_forms_and_a_dead_table(lrm, torch_cuda):
    torch = torch_cuda
    legs = legs6(lrm)
    quats, body, targets = bc.scene(lrm, 200, 5000, seed=33)
    forms = bc.live_forms(lrm, targets, quats, body, legs)
    assert 0 < forms["all_legs"].sum() < 200
    for name, live in forms.items():
        want = check(lrm, torch, targets, quats, body, legs, live_in=live, mixed=name != "zeros")
        if name == "zeros":
            assert (want["free"] == 0).all() and (want["top"] == -1).all()
    live = np.ones(200, np.uint8)
    live[64:128] = 0  # the four waves of sixteen whole blocks
    live[130] = 0
    live[150] = 3
    check(lrm, torch, targets, quats, body, legs, live_in=live)
    # a non-contiguous or short live_in is refused by the binding, not read with the wrong stride
    ps = lrm.PoseSet(legs, 200, footholds=True).update(dev(torch, quats), dev(torch, body))
    tx, ty, tz = soa(torch, targets)
    wide = dev(torch, np.repeat(forms["all_legs"], 2))
    with pytest.raises(ValueError):
        ps.body_clearance(tx, ty, tz, *CYL, live_in=wide[::2])
    with pytest.raises(ValueError):
        ps.body_clearance(tx, ty, tz, *CYL, live_in=wide[:100])
    with pytest.raises(ValueError):  # a PoseSet without the foothold table refuses
        lrm.PoseSet(legs, 8).update(dev(torch, quats[:8]), dev(torch, body[:8])).body_clearance(tx, ty, tz, *CYL)


def test_a_non_unit_quaternion_in_one_pose(lrm, torch_cuda):
    """unit quaternions everywhere but in pose 70 (|q| = 1.3: lengths shrink, targets far outside the cull sphere of a
    unit pose fall into the column) and pose 100 (a nan): their entries carry cull_r2 = +inf and nothing is culled"""
    import posed_cases
    legs = legs6(lrm)
    quats, body, targets = bc.scene(lrm, 160, 9000, seed=14)
    quats[:] = posed_cases.random_unit_quats(160, np.random.default_rng(3))
    quats[70] *= np.float32(1.3)
    quats[71] *= np.float32(0.6)
    quats[100, 2] = np.nan
    r2 = lrm.dbg_pose_footholds_compile_host(quats, legs, None)[:, 0, 3]
    assert np.isposinf(r2[[70, 71, 100]]).all() and np.isfinite(np.delete(r2, [70, 71, 100])).all()
    body[[70, 71]] = body[[2, 2]]  # standing poses: their columns hold terrain
    want = check(lrm, torch_cuda, targets, quats, body, legs, cyl=(181.0, 250.0, -110.0, -900.0))
    assert want["hits"][70] > 500 and want["top"][100] == -1  # pose 70 takes in terrain far outside a unit pose's sphere


@pytest.mark.parametrize("radius,plus_z", [(np.inf, bc.PLUS_Z), (181.0, np.inf), (np.inf, np.inf)])
def test_uncullable_scalars(lrm, torch_cuda, radius, plus_z):
    quats, body, targets = bc.scene(lrm, 90, 6000, seed=6)
    check(lrm, torch_cuda, targets, quats, body, legs6(lrm), cyl=(radius, plus_z, -110.0, -410.0))


@pytest.mark.parametrize("kind,nt", [("dense_cluster", 6000), ("sparse_tiles", 9 * 1024)])
def test_cull_scenes(lrm, torch_cuda, kind, nt):
    quats, body, targets = bc.scene(lrm, 160, nt, seed=2, kind=kind)
    check(lrm, torch_cuda, targets, quats, body, legs6(lrm), cyl=(181.0, bc.PLUS_Z, -45.0, -345.0))


def test_bad_targets_and_bodies(lrm, torch_cuda):
    quats, body, targets = bc.scene(lrm, 100, 6000, seed=8)
    bad_t = targets.copy()
    bad_t[::7] = np.nan
    bad_t[3::11, 1] = np.inf
    bad_t[5::13] = -np.inf
    bad_t[1024:1088] = np.nan  # a whole chunk of nan targets: an empty box
    check(lrm, torch_cuda, bad_t, quats, body, legs6(lrm))
    bad_b = body.copy()
    bad_b[1] = np.nan
    bad_b[2, 0] = np.inf
    bad_b[35] = -np.inf
    bad_b[70, 2] = np.nan
    check(lrm, torch_cuda, targets, quats, bad_b, legs6(lrm))


def test_far_from_the_origin(lrm, torch_cuda):
    """the box-slack case: a cloud and bodies 4e6 mm from the origin, where the float32 grid is 0.25-0.5 mm: no box cull
    may drop a column target of the host loop.  The first half of the cloud is in x order: thin slabs whose faces decide"""
    quats, body, targets = bc.scene(lrm, 256, 8000, seed=9)
    body, targets = pc.translated(body, targets, 4e6)
    want = check(lrm, torch_cuda, targets, quats, body, legs6(lrm))
    assert (want["hits"] > 0).sum() > 40


def test_two_clouds_through_the_shared_box_buffer(lrm, torch_cuda):
    """clouds of different size on ONE PoseSet, larger, smaller, larger again: every call refills the per-device boxes"""
    legs = legs6(lrm)
    ps = lrm.PoseSet(legs, 128, footholds=True)
    for k, nt in enumerate((9000, 4500, 12000, 700)):
        quats, body, targets = bc.scene(lrm, 128, nt, seed=20 + k)
        want = bc.host(lrm, targets, quats, body, legs, *CYL)
        assert (want["hits"] > 0).any() and (want["top"] < 0).any()
        bc.assert_same(run(lrm, torch_cuda, targets, quats, body, legs, ps=ps), want)


def test_null_outputs_and_mode(lrm, torch_cuda):
    quats, body, targets = bc.scene(lrm, 90, 5000, seed=12)
    legs = legs6(lrm)
    check(lrm, torch_cuda, targets, quats, body, legs, height=False)
    check(lrm, torch_cuda, targets, quats, body, legs, free=False)
    lrm.set_mode(lrm.MODE_STRICT)  # the answers do not depend on the mode
    try:
        check(lrm, torch_cuda, targets, quats, body, legs, height=False, free=False)
    finally:
        lrm.set_mode(lrm.MODE_FAST)  # the library default


def test_free_is_the_negation_of_any_in_cylinder_under_the_identity(lrm, torch_cuda):
    torch = torch_cuda
    legs = legs6(lrm)
    quats, body, targets = bc.scene(lrm, 300, 8000, seed=21)
    quats[:] = [1, 0, 0, 0]
    ps = lrm.PoseSet(legs, 300, footholds=True).update(dev(torch, quats), dev(torch, body))
    tx, ty, tz = soa(torch, targets)
    bx, by, bz = soa(torch, body)
    for minus_z in bc.MINUS_Z:
        free = ps.body_clearance(tx, ty, tz, 181.0, bc.PLUS_Z, minus_z, bc.floor_of(minus_z))[3]
        coll = lrm.device.any_in_cylinder(bx, by, bz, tx, ty, tz, 181.0, bc.PLUS_Z, minus_z)
        torch.cuda.synchronize()
        f, c = free.cpu().numpy(), coll.cpu().numpy()
        assert 0 < c.sum() < 300 and np.array_equal(f, 1 - c)


def test_chain_on_one_pose_set(lrm, torch_cuda):
    """update -> footholds -> body_clearance(live_in=all_legs) -> foothold_support(pose_live=free) -> ik on the SAME
    PoseSet: only poses that stand and fit support a foothold, and IK solves every supported one"""
    import foothold_support_cases as fs
    torch = torch_cuda
    legs = legs6(lrm)
    quats, body, targets = bc.scene(lrm, 256, 4000, seed=51)
    nl, nt = 6, len(targets)
    ps = lrm.PoseSet(legs, 256, ik=True, footholds=True).update(dev(torch, quats), dev(torch, body))
    tx, ty, tz = soa(torch, targets)
    all_legs = ps.footholds(tx, ty, tz)[3]
    hits, top, height, free = ps.body_clearance(tx, ty, tz, 181.0, bc.PLUS_Z, -45.0, -345.0, live_in=all_legs)
    count, best_pose, best_d2, legs_mask = ps.foothold_support(tx, ty, tz, pose_live=free)
    ti, pi, li, valid = lrm.device.foothold_support_layout(nt, nl, "cuda", best_pose)
    ang, st = ps.ik(tx, ty, tz, pi, li, target_idx=ti)
    torch.cuda.synchronize()
    al = all_legs.cpu().numpy()
    assert np.array_equal(al, lrm.footholds_posed_cpu(targets, quats, body, legs, None)[3])
    want = bc.host(lrm, targets, quats, body, legs, 181.0, bc.PLUS_Z, -45.0, -345.0, al)
    bc.assert_same((hits.cpu().numpy(), top.cpu().numpy(), height.cpu().numpy(), free.cpu().numpy()), want)
    fr = want["free"]
    assert 0 < fr.sum() < al.sum() < 256  # some positionable poses are buried
    fs.assert_same((count.cpu().numpy(), best_pose.cpu().numpy(), best_d2.cpu().numpy(), legs_mask.cpu().numpy()),
                   fs.host(lrm, targets, quats, body, legs, None, fr))
    s, v, bp = st.cpu().numpy(), valid.cpu().numpy(), best_pose.cpu().numpy().reshape(-1)
    assert v.sum() > 100 and fr[bp[v]].all()
    assert np.array_equal(np.isin(s, (lrm.IK_REACHED, lrm.IK_MODEL_GAP)), v) and np.array_equal(s == 0, ~v)


def test_update_footholds_and_clearance_replay_from_a_graph(lrm, torch_cuda):
    """update(), footholds() and body_clearance() only launch once the box buffer holds the cloud's size: captured on ONE
    side stream after a warm-up call, replayed after new quaternions, bodies and targets were copied into the captured
    tensors"""
    torch = torch_cuda
    legs = legs6(lrm)
    q0, b0, t0 = bc.scene(lrm, 192, 5000, seed=41)
    q1, b1, t1 = bc.scene(lrm, 192, 5000, seed=42)
    qt, bt, tt = dev(torch, q0), dev(torch, b0), dev(torch, t0.T.copy())
    cnt, bst = torch.empty((6, 192), dtype=torch.int32, device="cuda"), torch.empty((6, 192), dtype=torch.int32, device="cuda")
    bd, al = torch.empty((6, 192), dtype=torch.float32, device="cuda"), torch.empty(192, dtype=torch.uint8, device="cuda")
    hits, top = torch.empty(192, dtype=torch.int32, device="cuda"), torch.empty(192, dtype=torch.int32, device="cuda")
    hgt, fre = torch.empty(192, dtype=torch.float32, device="cuda"), torch.empty(192, dtype=torch.uint8, device="cuda")
    ps = lrm.PoseSet(legs, 256, footholds=True)

    def work():
        ps.update(qt, bt)
        ps.footholds(tt[0], tt[1], tt[2], cnt, bst, bd, al)
        ps.body_clearance(tt[0], tt[1], tt[2], *CYL, al, hits, top, hgt, fre)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture: the box buffer grows here
        work()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            work()
        qt.copy_(dev(torch, q1))
        bt.copy_(dev(torch, b1))
        tt.copy_(dev(torch, t1.T.copy()))
        hits.fill_(SENTINEL)
        top.fill_(SENTINEL)
        hgt.fill_(SENTINEL)
        fre.fill_(0xA5)
        g.replay()
    torch.cuda.synchronize()
    live = lrm.footholds_posed_cpu(t1, q1, b1, legs, None)[3]
    assert np.array_equal(al.cpu().numpy(), live) and 0 < live.sum() < 192
    want = bc.host(lrm, t1, q1, b1, legs, *CYL, live)
    assert (want["hits"] > 0).any() and (want["free"] == 1).any()
    bc.assert_same((hits.cpu().numpy(), top.cpu().numpy(), hgt.cpu().numpy(), fre.cpu().numpy()), want)
    del g


def scale_scene(lrm):
    """an eighth of the reference terrain (the first 8192 points along the Morton curve) under the lattice poses over it,
    in Morton order, with the reference's sweep orientations; every third body is lowered into the ground"""
    from lrm_amd import workloads
    ground = workloads.terrain(256)
    targets = np.ascontiguousarray(ground[lrm.morton_order(ground)][:8192])
    bodies = workloads.body_lattice(ground, 20000, seed=3)
    lo, hi = targets.min(0) - 300.0, targets.max(0) + 300.0
    bodies = bodies[((bodies[:, :2] >= lo[:2]) & (bodies[:, :2] <= hi[:2])).all(1)][::2]
    bodies = np.ascontiguousarray(bodies[lrm.morton_order(bodies)])
    bodies[::3, 2] -= np.float32(150.0)
    return fc.sweep_pose_quats(lrm, len(bodies)), bodies, targets


def test_reference_terrain_against_the_oracle(lrm, oracle, torch_cuda):
    """one scale case: the device against the oracle's arithmetic directly.  Every (pose, target) pair goes through
    body_clearance_cases.brute_np, the numpy restatement the CPU tests hold to the oracle bit for bit; every 40th pose
    also goes through the oracle's own functions pair by pair"""
    quats, bodies, targets = scale_scene(lrm)
    assert 2000 < len(bodies) < 4000
    legs = np.stack([lrm.get_M2_leg(np.float32(2 * np.pi * k / 6)) for k in range(6)]).astype(np.float32)
    cyl = (float(legs[0][bc.BODY]), bc.PLUS_Z, -110.0, -410.0)
    want = bc.brute_np(targets, quats, bodies, *cyl)
    some = np.arange(0, len(bodies), 40)
    assert len(some) * len(targets) <= bc.MAX_PAIRS
    part = bc.brute(oracle, targets, quats[some], bodies[some], *cyl)
    bc.assert_same(tuple(want[k][some] for k in ("hits", "top", "height", "free")), part)
    assert (want["hits"] > 0).mean() > 0.1 and ((want["hits"] == 0) & (want["top"] >= 0)).mean() > 0.1
    bc.assert_same(run(lrm, torch_cuda, targets, quats, bodies, legs, cyl), want)
