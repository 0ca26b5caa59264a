"""Per-target foothold support on the device (run with -m gpu on an MI355X): PoseSet.foothold_support /
lrm_foothold_support_posed_dev against the host loop lrm_foothold_support_posed_cpu bit for bit (count, best_pose, best_d2
bits, legs_mask) over cloud sizes, pose counts around every boundary lrm_dbg_foothold_support_grid reports, leg counts,
pose_live forms, quaternion kinds, the cull scenes, NULL outputs and the box-slack case 4e6 mm from the origin
(tests/test_foothold_support_cpu.py ties that host loop to a brute force over the oracle); workspace regrowth and reuse;
the chain update -> footholds -> foothold_support(all_legs) -> ik on ONE PoseSet; a graph replay; and one scale case
against the oracle on the reference terrain.  Every output is prefilled with a sentinel, so an unwritten entry fails too."""
import numpy as np
import pytest

import foothold_support_cases as fs
import footholds_posed_cases as fc
import pair_cases as pc

pytestmark = pytest.mark.gpu

SENTINEL = -7


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


def run(lrm, torch, targets, quats, body, legs, nominal=None, pose_live=None, d2=True, mask=True, ps=None):
    """PoseSet.foothold_support into sentinel-filled outputs -> numpy (count, best_pose, best_d2 or None, legs_mask or None)"""
    npz, nl, nt = len(quats), len(legs), len(targets)
    if ps is None:
        ps = lrm.PoseSet(legs, npz, footholds=True, nominal=nominal)
    ps.update(dev(torch, quats), dev(torch, body))
    count = torch.full((nl, nt), SENTINEL, dtype=torch.int32, device="cuda")
    best = torch.full((nl, nt), SENTINEL, dtype=torch.int32, device="cuda")
    bd2 = torch.full((nl, nt), float(SENTINEL), dtype=torch.float32, device="cuda")
    lm = torch.full((nt,), 0xA5, dtype=torch.uint8, device="cuda")
    live = None if pose_live is None else dev(torch, np.asarray(pose_live, np.uint8))
    tx, ty, tz = soa(torch, targets)
    if d2 and mask:
        ps.foothold_support(tx, ty, tz, live, count, best, bd2, lm)
    else:  # the NULL forms of the C ABI, on a workspace of exactly the size the library asks for
        L, dp = lrm.load(), lambda t: None if t is None else t.data_ptr()
        sw = torch.empty(L.lrm_foothold_support_workspace_bytes(npz, nl, nt), dtype=torch.uint8, device="cuda")
        rc = L.lrm_foothold_support_posed_dev(dp(tx), dp(ty), dp(tz), nt, dp(ps.workspace), dp(ps.fh_workspace), npz, nl, dp(live),
                                              dp(sw), dp(count), dp(best), dp(bd2 if d2 else None), dp(lm if mask else None),
                                              torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    if not d2:
        assert (bd2 == float(SENTINEL)).all()
    if not mask:
        assert (lm == 0xA5).all()
    return count.cpu().numpy(), best.cpu().numpy(), bd2.cpu().numpy() if d2 else None, lm.cpu().numpy() if mask else None


def check(lrm, torch, targets, quats, body, legs, nominal=None, pose_live=None, both=True, **kw):
    want = fs.host(lrm, targets, quats, body, legs, nominal, pose_live)
    if both:
        assert (want["count"] > 0).any() and (want["count"] == 0).any()
    fs.assert_same(run(lrm, torch, targets, quats, body, legs, nominal, pose_live, **kw), want)
    return want


def small_scene(lrm, nposes, nt, seed, dup=0):
    """a scene in which a few targets meet many poses: the cloud of nt targets and the bodies of a 400-target scene"""
    quats, body, targets = fs.scene(lrm, nposes, max(nt, 400), seed, dup=dup)
    pick = np.random.default_rng(seed).permutation(len(targets))[:nt]
    return quats, body, np.ascontiguousarray(targets[np.sort(pick)])


@pytest.mark.parametrize("nt", [1, 63, 64, 65, 127, 128, 129, 5 * 64 + 17])
def test_every_cloud_size(lrm, torch_cuda, nt):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = small_scene(lrm, 200, nt, seed=nt % 97, dup=20)
    check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(6), both=nt >= 63)


@pytest.mark.parametrize("nposes", [1, 2, 3, 4, 5, 63, 64, 65])
def test_every_small_pose_count(lrm, torch_cuda, nposes):
    legs, _ = pc.leg_families(lrm)["mixed_5_tilted"]
    quats, body, targets = fs.scene(lrm, 65, 700, seed=nposes + 3)
    g = lrm.dbg_foothold_support_grid(700, nposes)
    assert g["slices"] == (1 if nposes <= g["pose_chunk"] else 2)  # one pose chunk: S = 1; one more pose: two slices
    check(lrm, torch_cuda, targets, quats[:nposes], body[:nposes], legs, pc.nominal_for(5), both=nposes > 5)


def boundaries(lrm, nt):
    """pose counts around every boundary the grid reports for nt targets: the first pose count at which a slice walks a
    second and a third pose chunk (the slice count is capped there), each -1 / +0 / +1"""
    chunk = lrm.dbg_foothold_support_grid(nt, 1)["pose_chunk"]
    out, n = [], chunk
    for want in (2, 3):
        while lrm.dbg_foothold_support_grid(nt, n)["poses_per_slice"] < want * chunk:
            n += chunk
        out.append(n - chunk + 1)  # the first pose count with `want` pose chunks in some slice
    cap = lrm.dbg_foothold_support_grid(nt, out[0])["slices"]
    assert lrm.dbg_foothold_support_grid(nt, out[1])["slices"] == cap >= 2  # capped: more poses, no more slices
    return [out[0] - 2, out[0] - 1, out[0], out[1] - 1, out[1]], cap


def test_pose_counts_around_the_slice_boundaries(lrm, torch_cuda):
    """one target chunk against thousands of poses: S >= 2 slices share ONE chunk of targets, so every answer crosses the
    atomic combine; the pose counts sit where a slice gets its second and third pose chunk (past the slice cap) and at one
    slice +- 1 poses.  Duplicated poses tie across slices: a pose and its copy lie in different slices"""
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nt = 64
    counts, cap = boundaries(lrm, nt)
    nmax = max(counts)
    quats, body, targets = small_scene(lrm, nmax, nt, seed=5)
    # copies three pose chunks on: chunk c and chunk c + 3 lie in different slices (c % S) unless S divides 3
    step = 64 * 3
    assert cap > 3
    quats[step:2 * step] = quats[:step]
    body[step:2 * step] = body[:step]
    for n in counts:
        g = lrm.dbg_foothold_support_grid(nt, n)
        assert g["slices"] >= 2 and g["blocks"] == -(-g["slices"] // 4)
        want = check(lrm, torch_cuda, targets, quats[:n], body[:n], legs, pc.nominal_for(6), both=False)  # so many poses leave no target out
        assert not ((want["best_pose"] >= step) & (want["best_pose"] < 2 * step)).any()  # the original wins every tie
    assert ((want["best_pose"] >= 0) & (want["best_pose"] < step)).any() and (want["count"] >= 2).any()


@pytest.mark.parametrize("nposes", [127, 128, 129, 192, 193])
def test_pose_counts_at_which_the_slice_count_steps(lrm, torch_cuda, nposes):
    """below the cap there are as many slices as pose chunks: two slices' worth of poses - 1 / + 0 / + 1 (the third slice
    holds ONE pose) and three slices' worth + 0 / + 1, on a ragged cloud of several chunks"""
    legs, _ = pc.leg_families(lrm)["m2_5_identity"]
    nt = 4 * 64 + 29
    g = lrm.dbg_foothold_support_grid(nt, nposes)
    assert g["slices"] == -(-nposes // 64) and g["poses_per_slice"] == 64 and g["blocks"] == -(-5 * g["slices"] // 4)
    quats, body, targets = small_scene(lrm, 193, nt, seed=31, dup=40)
    check(lrm, torch_cuda, targets, quats[:nposes], body[:nposes], legs, pc.nominal_for(5))


@pytest.mark.parametrize("family", ["m2_1_identity", "m2_6_tilted", "random_7_tilted", "m2_8_identity"])
def test_leg_counts(lrm, torch_cuda, family):
    legs, _ = pc.leg_families(lrm)[family]
    quats, body, targets = fs.scene(lrm, 150, 3000, seed=len(family) + len(legs), dup=20)
    want = check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(len(legs)))
    assert want["legs_mask"].max() >= 1 << (len(legs) - 1) or len(legs) == 1


def test_pose_live_forms(lrm, torch_cuda):
    torch = torch_cuda
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6)
    quats, body, targets = fs.scene(lrm, 200, 3000, seed=33, dup=30)
    forms = fs.live_forms(lrm, targets, quats, body, legs, nominal)
    assert 0 < forms["all_legs"].sum() < 200
    for name, live in forms.items():
        want = check(lrm, torch, targets, quats, body, legs, nominal, live, both=name != "zeros")
        if name == "zeros":
            assert (want["count"] == 0).all()
    # a whole chunk of dead poses, and a chunk with one live pose
    live = np.ones(200, np.uint8)
    live[64:128] = 0
    live[137] = 1
    live[128:192] = 0
    live[150] = 3
    check(lrm, torch, targets, quats, body, legs, nominal, live)
    # a non-contiguous pose_live is refused by the binding, not read with the wrong stride
    ps = lrm.PoseSet(legs, 200, footholds=True).update(dev(torch, quats), dev(torch, body))
    tx, ty, tz = soa(torch, targets)
    wide = dev(torch, np.repeat(forms["all_legs"], 2))
    with pytest.raises(ValueError):
        ps.foothold_support(tx, ty, tz, wide[::2])
    with pytest.raises(ValueError):
        ps.foothold_support(tx, ty, tz, wide[:100])  # too short


def test_non_unit_and_nan_quaternions_in_one_pose_and_in_a_whole_chunk(lrm, torch_cuda):
    import posed_cases
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fs.scene(lrm, 192, 2500, seed=14)
    quats[:] = posed_cases.random_unit_quats(192, np.random.default_rng(3))
    quats[70] *= np.float32(1.3)         # one open sphere in chunk 1: the whole chunk's box opens
    quats[100, 2] = np.nan
    quats[128:192] *= np.float32(0.8)    # every pose of chunk 2
    quats[128:192:5, 1] = np.nan
    r2 = lrm.dbg_pose_footholds_compile_host(quats, legs, None)[:, 0, 3]
    assert np.isposinf(r2[[70, 100]]).all() and np.isposinf(r2[128:]).all() and np.isfinite(r2[:64]).all()
    want = check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(6))
    assert (want["best_pose"] >= 128).any()  # non-unit poses do reach


@pytest.mark.parametrize("kind", ["dense_cluster", "sparse_tiles"])
def test_cull_scenes(lrm, torch_cuda, kind):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fs.scene(lrm, 160, 6000 if kind == "dense_cluster" else 9 * 1024, seed=2, kind=kind, dup=16)
    want = check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(6))
    assert (want["count"] >= 2).any()


def test_bad_and_extreme_input(lrm, torch_cuda):
    legs, _ = pc.leg_families(lrm)["m2_5_identity"]
    quats, body, targets = fs.scene(lrm, 100, 3000, seed=8, dup=6)
    bad_t = targets.copy()
    bad_t[::7] = np.nan
    bad_t[3::11, 1] = np.inf
    bad_t[5::13] = -np.inf
    bad_t[1024:1088] = np.nan  # a whole chunk of nan targets: an empty box
    check(lrm, torch_cuda, bad_t, quats, body, legs, pc.nominal_for(5))
    bad_b = body.copy()
    bad_b[1] = np.nan
    bad_b[2, 0] = np.inf
    bad_b[35] = -np.inf
    bad_b[70, 2] = np.nan
    check(lrm, torch_cuda, targets, quats, bad_b, legs, pc.nominal_for(5))
    check(lrm, torch_cuda, targets, quats, body, legs, np.full((5, 3), 1e30, np.float32))  # every d2 is +inf: ties everywhere


def test_far_from_the_origin(lrm, torch_cuda):
    """the box-slack case: a cloud and bodies 4e6 mm from the origin, where the float32 grid is 0.25-0.5 mm and
    (t - body) - centre and body + centre round differently: no box cull may drop a triple of the host loop.  The cloud is
    in x order, so the target boxes are thin slabs whose faces decide"""
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fs.scene(lrm, 256, 6000, seed=9, dup=20)
    body, targets = pc.translated(body, targets, 4e6)
    want = check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(6))
    assert (want["count"] > 0).sum() > 1000


def test_null_outputs_and_mode(lrm, torch_cuda):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fs.scene(lrm, 90, 2000, seed=12, dup=10)
    check(lrm, torch_cuda, targets, quats, body, legs, None, d2=False)
    check(lrm, torch_cuda, targets, quats, body, legs, None, mask=False)
    lrm.set_mode(lrm.MODE_STRICT)  # the answers do not depend on the mode
    try:
        check(lrm, torch_cuda, targets, quats, body, legs, None, d2=False, mask=False)
    finally:
        lrm.set_mode(lrm.MODE_FAST)  # the library default


def test_workspace_regrowth_and_reuse(lrm, torch_cuda):
    """clouds of different sizes on ONE PoseSet: the support workspace grows once and is reused; two consecutive calls on
    the same workspace give identical bytes (counts and keys are reset by every call)"""
    torch = torch_cuda
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    ps = lrm.PoseSet(legs, 256, footholds=True, nominal=pc.nominal_for(6))
    sizes = []
    for k, (npz, nt) in enumerate(((128, 1500), (200, 4000), (64, 700))):
        quats, body, targets = fs.scene(lrm, npz, nt, seed=20 + k, dup=10)
        want = fs.host(lrm, targets, quats, body, legs, pc.nominal_for(6))
        assert (want["count"] > 0).any() and (want["count"] == 0).any()
        fs.assert_same(run(lrm, torch, targets, quats, body, legs, ps=ps), want)
        sizes.append(ps.support_workspace.numel())
        first = ps.support_workspace.data_ptr()
        again = run(lrm, torch, targets, quats, body, legs, ps=ps)
        fs.assert_same(again, want)
        assert ps.support_workspace.data_ptr() == first
    assert sizes[0] < sizes[1] == sizes[2]
    # a PoseSet without the foothold table refuses
    with pytest.raises(ValueError):
        lrm.PoseSet(legs, 8).update(dev(torch, quats[:8]), dev(torch, body[:8])).foothold_support(*soa(torch, targets))


def test_chain_on_one_pose_set(lrm, torch_cuda):
    """update -> footholds -> foothold_support(pose_live=all_legs) -> ik on the SAME PoseSet, through
    foothold_support_layout: mask-1 statuses exactly where a pose reaches, status 0 elsewhere, no dead pose chosen"""
    torch = torch_cuda
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6)
    quats, body, targets = fs.scene(lrm, 256, 4000, seed=51, dup=30)
    nl, nt = 6, len(targets)
    ps = lrm.PoseSet(legs, 256, ik=True, footholds=True, nominal=nominal).update(dev(torch, quats), dev(torch, body))
    tx, ty, tz = soa(torch, targets)
    all_legs = ps.footholds(tx, ty, tz)[3]
    count, best_pose, best_d2, legs_mask = ps.foothold_support(tx, ty, tz, pose_live=all_legs)
    ti, pi, li, valid = lrm.device.foothold_support_layout(nt, nl, "cuda", best_pose)
    ang, st = ps.ik(tx, ty, tz, pi, li, target_idx=ti)
    torch.cuda.synchronize()
    al = all_legs.cpu().numpy()
    assert np.array_equal(al, lrm.footholds_posed_cpu(targets, quats, body, legs, nominal)[3]) and 0 < al.sum() < 256
    want = fs.host(lrm, targets, quats, body, legs, nominal, al)
    fs.assert_same((count.cpu().numpy(), best_pose.cpu().numpy(), best_d2.cpu().numpy(), legs_mask.cpu().numpy()), want)
    s, v, bp = st.cpu().numpy(), valid.cpu().numpy(), best_pose.cpu().numpy().reshape(-1)
    assert np.array_equal(v, bp >= 0) and v.sum() > 1000 and (~v).sum() > 1000
    assert np.array_equal(np.isin(s, (lrm.IK_REACHED, lrm.IK_MODEL_GAP)), v) and np.array_equal(s == 0, ~v)
    assert (s == lrm.IK_REACHED).sum() > 0.99 * v.sum() and al[bp[v]].all()


def test_update_footholds_and_support_replay_from_a_graph(lrm, torch_cuda):
    """update(), footholds() and foothold_support() only launch once the workspaces hold the cloud's size: captured on ONE
    side stream after a warm-up call, replayed after new quaternions, bodies and targets were copied into the captured
    tensors"""
    torch = torch_cuda
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    q0, b0, t0 = fs.scene(lrm, 192, 5000, seed=41, dup=10)
    q1, b1, t1 = fs.scene(lrm, 192, 5000, seed=42, dup=10)
    qt, bt, tt = dev(torch, q0), dev(torch, b0), dev(torch, t0.T.copy())
    nl, nt = 6, 5000
    cnt, bst = torch.empty((nl, 192), dtype=torch.int32, device="cuda"), torch.empty((nl, 192), dtype=torch.int32, device="cuda")
    bd, al = torch.empty((nl, 192), dtype=torch.float32, device="cuda"), torch.empty(192, dtype=torch.uint8, device="cuda")
    count, best = torch.empty((nl, nt), dtype=torch.int32, device="cuda"), torch.empty((nl, nt), dtype=torch.int32, device="cuda")
    d2, lm = torch.empty((nl, nt), dtype=torch.float32, device="cuda"), torch.empty(nt, dtype=torch.uint8, device="cuda")
    ps = lrm.PoseSet(legs, 256, footholds=True)

    def work():
        ps.update(qt, bt)
        ps.footholds(tt[0], tt[1], tt[2], cnt, bst, bd, al)
        ps.foothold_support(tt[0], tt[1], tt[2], al, count, best, d2, lm)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture: the workspaces grow here
        work()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            work()
        qt.copy_(dev(torch, q1))
        bt.copy_(dev(torch, b1))
        tt.copy_(dev(torch, t1.T.copy()))
        count.fill_(SENTINEL)
        best.fill_(SENTINEL)
        d2.fill_(SENTINEL)
        lm.fill_(0xA5)
        g.replay()
    torch.cuda.synchronize()
    live = lrm.footholds_posed_cpu(t1, q1, b1, legs, None)[3]
    assert np.array_equal(al.cpu().numpy(), live)
    want = fs.host(lrm, t1, q1, b1, legs, None, live)
    assert (want["count"] > 0).any() and (want["count"] == 0).any()
    fs.assert_same((count.cpu().numpy(), best.cpu().numpy(), d2.cpu().numpy(), lm.cpu().numpy()), want)
    del g


def test_reference_terrain_against_the_oracle(lrm, oracle, torch_cuda):
    """one scale case: an eighth of the reference terrain (the first 8192 points along the Morton curve, every twelfth
    as a target) under a few thousand lattice poses in Morton order with the reference's sweep orientations, the device
    against the oracle brute force directly"""
    from lrm_amd import workloads
    ground = workloads.terrain(256)
    region = ground[lrm.morton_order(ground)][:8192]
    targets = np.ascontiguousarray(region[::12])
    bodies = workloads.body_lattice(ground, 20000, seed=3)
    lo, hi = region.min(0) - 300.0, region.max(0) + 300.0
    bodies = bodies[((bodies[:, :2] >= lo[:2]) & (bodies[:, :2] <= hi[:2])).all(1)][::2]
    bodies = np.ascontiguousarray(bodies[lrm.morton_order(bodies)])
    assert 2000 < len(bodies) < 4000 and lrm.dbg_foothold_support_grid(len(targets), len(bodies))["slices"] >= 2
    quats = fc.sweep_pose_quats(lrm, len(bodies))
    legs = np.stack([lrm.get_M2_leg(np.float32(2 * np.pi * k / 6)) for k in range(6)]).astype(np.float32)
    nominal = pc.nominal_for(6)
    assert 6 * len(bodies) * len(targets) <= fs.MAX_TRIPLES
    want = fs.brute(oracle, targets, quats, bodies, legs, fc.nominal_w_of(lrm, quats, legs, nominal))
    assert (want["count"] >= 2).mean() > 0.25 and (want["count"] == 0).any()
    fs.assert_same(run(lrm, torch_cuda, targets, quats, bodies, legs, nominal), want)
