"""Nearest-miss footholds per (pose, leg) on the device (run with -m gpu on an MI355X): PoseSet.foothold_misses /
lrm_foothold_misses_posed_dev against the host loop lrm_foothold_misses_posed_cpu bit for bit (miss, m2 bits, shift bits,
near) over cloud sizes, pose counts, leg counts, count_in forms, margins, quaternion kinds, NULL outputs, the box-slack
case 4e6 mm from the origin and two clouds through the shared box buffer (tests/test_foothold_misses_cpu.py ties that host
loop to a brute force over the oracle); the chain update -> footholds -> foothold_misses -> reach_dist on ONE PoseSet; and
a graph capture of the chain.  Every output is prefilled with a sentinel, so an unwritten entry fails too."""
import numpy as np
import pytest

import foothold_misses_cases as fm
import footholds_posed_cases as fc
import pair_cases as pc

pytestmark = pytest.mark.gpu

SENTINEL = -7
TILE, GROUP, GRID_POSES = 1024, 64, 16384 * 4  # targets per tile, tiles per outer iteration, poses per grid stride


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def test_constants_match_the_kernel():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged-robot-movability-cuda_amd",
                            "csrc", "lrm_foothold_misses.hip")).read()
    assert int(re.search(r"constexpr int kTargetTile = (\d+);", src).group(1)) == TILE
    assert int(re.search(r"tw0 < ntiles; tw0 \+= (\d+)\)", src).group(1)) == GROUP
    assert int(re.search(r"constexpr unsigned kMaxGrid = (\d+);", src).group(1)) * 4 == GRID_POSES


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def soa(torch, pts):
    t = dev(torch, np.asarray(pts, np.float32).reshape(-1, 3).T)
    return t[0], t[1], t[2]


def run(lrm, torch, targets, quats, body, legs, margin, count_in=None, m2=True, shift=True, near=True, ps=None):
    """PoseSet.foothold_misses into sentinel-filled outputs -> numpy (miss, m2 or None, shift or None, near or None)"""
    npz, nl = len(quats), len(legs)
    if ps is None:
        ps = lrm.PoseSet(legs, npz, footholds=True)
    ps.update(dev(torch, quats), dev(torch, body))
    miss = torch.full((nl, npz), SENTINEL, dtype=torch.int32, device="cuda")
    nr = torch.full((nl, npz), SENTINEL, dtype=torch.int32, device="cuda")
    mm = torch.full((nl, npz), float(SENTINEL), dtype=torch.float32, device="cuda")
    sh = torch.full((3, nl, npz), float(SENTINEL), dtype=torch.float32, device="cuda")
    cin = None if count_in is None else dev(torch, np.asarray(count_in, np.int32).reshape(nl, npz))
    tx, ty, tz = soa(torch, targets)
    if m2 and shift and near:
        ps.foothold_misses(tx, ty, tz, margin, cin, miss, mm, sh, nr)
    else:  # the NULL forms of the C ABI
        L, dp = lrm.load(), lambda t: None if t is None else t.data_ptr()
        rc = L.lrm_foothold_misses_posed_dev(dp(tx), dp(ty), dp(tz), len(targets), dp(ps.workspace), dp(ps.fh_workspace), npz, nl,
                                             float(margin), dp(cin), dp(miss), dp(mm if m2 else None), dp(sh[0] if shift else None),
                                             dp(sh[1] if shift else None), dp(sh[2] if shift else None), dp(nr if near else None),
                                             torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    if not m2:
        assert (mm == float(SENTINEL)).all()
    if not shift:
        assert (sh == float(SENTINEL)).all()
    if not near:
        assert (nr == SENTINEL).all()
    return (miss.cpu().numpy(), mm.cpu().numpy() if m2 else None, sh.cpu().numpy() if shift else None,
            nr.cpu().numpy() if near else None)


def check(lrm, torch, targets, quats, body, legs, margin, count_in=None, both=True, **kw):
    want = fm.host(lrm, targets, quats, body, legs, margin, count_in)
    if both:
        assert (want["miss"] >= 0).any() and (want["miss"] < 0).any()
    fm.assert_same(run(lrm, torch, targets, quats, body, legs, margin, count_in, **kw), want)
    return want


@pytest.mark.parametrize("nt", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 4095, 4096, 4097, (GROUP + 1) * TILE + 1])
def test_every_cloud_size(lrm, torch_cuda, nt):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fm.scene(lrm, 16 if nt > 20000 else 64, nt, seed=nt % 97)
    for margin in (0.0, 25.0):
        check(lrm, torch_cuda, targets, quats, body, legs, margin, both=nt >= TILE - 1)


@pytest.mark.parametrize("nposes", [1, 2, 3, 4, 5, 255, 257])
@pytest.mark.parametrize("nt", [3000, 5000])
def test_every_pose_count(lrm, torch_cuda, nposes, nt):
    legs, _ = pc.leg_families(lrm)["mixed_5_tilted"]
    quats, body, targets = fm.scene(lrm, 257, nt, seed=nposes + nt)
    check(lrm, torch_cuda, targets, quats[:nposes], body[:nposes], legs, 25.0, both=nposes > 100)


def test_poses_past_the_grid_stride(lrm, torch_cuda):
    """more poses than one pass of the grid holds: a wave walks on to pose + GRID_POSES"""
    legs, _ = pc.leg_families(lrm)["m2_1_identity"]
    n = GRID_POSES + 777
    quats, body, targets = fm.scene(lrm, 300, 200, seed=3)
    targets = targets * np.float32(0.25)  # 200 targets within 230 mm of the origin
    body[:, :2] = body[:, :2] * np.float32(0.1)
    pick = np.random.default_rng(8).integers(0, 300, n)
    want = check(lrm, torch_cuda, targets, quats[pick], body[pick], legs, 25.0)
    tail = want["miss"][:, GRID_POSES:]
    assert (tail >= 0).sum() > 20 and (tail < 0).sum() > 20


@pytest.mark.parametrize("family", ["m2_1_identity", "m2_6_tilted", "m2_8_identity", "random_7_tilted"])
def test_leg_counts_and_margins(lrm, torch_cuda, family):
    legs, _ = pc.leg_families(lrm)[family]
    quats, body, targets = fm.scene(lrm, 64, 5000, seed=len(family) + len(legs))
    for margin in (0.0, np.inf):
        check(lrm, torch_cuda, targets, quats, body, legs, margin)


def test_count_in_forms(lrm, torch_cuda):
    """NULL, all zero, footholds()'s counts, negative entries (not skipped), every leg skipped (the early exit) and one
    non-skipped leg in an otherwise skipped pose"""
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fm.scene(lrm, 96, 6000, seed=33)
    count = fc.host(lrm, targets, quats, body, legs, None)["count"]
    for name, cin in fm.count_forms(count).items():
        want = check(lrm, torch_cuda, targets, quats, body, legs, 25.0, cin)
        if cin is not None:
            assert (want["miss"][cin > 0] == -1).all() and (want["near"][cin > 0] == 0).all(), name
    ones = np.ones_like(count)
    want = check(lrm, torch_cuda, targets, quats, body, legs, 25.0, ones, both=False)
    assert (want["miss"] == -1).all() and (want["near"] == 0).all()
    one = ones.copy()
    one[np.arange(96) % 6, np.arange(96)] = 0  # leg p % 6 of pose p alone
    want = check(lrm, torch_cuda, targets, quats, body, legs, 400.0, one)
    assert (want["miss"][one > 0] == -1).all() and (want["miss"][one == 0] >= 0).sum() > 20


def test_non_unit_quaternions(lrm, torch_cuda):
    """a +inf sphere makes every target a candidate of that pose, whatever the margin, and nothing is culled for it"""
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fm.scene(lrm, 60, 6000, seed=14)
    inf = np.isposinf(fm.spheres_of(lrm, quats, legs)[:, 0, 3])
    assert 3 <= inf.sum() < 30
    want = check(lrm, torch_cuda, targets, quats, body, legs, 0.0)
    assert (want["near"][:, inf] > 3000).any()


def test_null_outputs_and_mode(lrm, torch_cuda):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fm.scene(lrm, 45, 5000, seed=12)
    check(lrm, torch_cuda, targets, quats, body, legs, 25.0, m2=False)
    check(lrm, torch_cuda, targets, quats, body, legs, 25.0, shift=False)
    check(lrm, torch_cuda, targets, quats, body, legs, 25.0, near=False)
    lrm.set_mode(lrm.MODE_STRICT)  # the answers do not depend on the mode
    try:
        check(lrm, torch_cuda, targets, quats, body, legs, 25.0, m2=False, shift=False, near=False)
    finally:
        lrm.set_mode(lrm.MODE_FAST)  # the library default


@pytest.mark.parametrize("kind", ["dense_cluster_boxes", "dense_cluster_plain", "sparse_tiles"])
def test_scenes_against_each_cull(lrm, torch_cuda, kind):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    if kind == "sparse_tiles":
        quats, body, targets = fm.scene(lrm, 80, 9 * 1024, seed=2, kind="sparse_tiles")
    else:
        quats, body, targets = fm.scene(lrm, 80, 6000 if kind.endswith("boxes") else 3500, seed=1, kind="dense_cluster")
    for margin in (0.0, 400.0):
        check(lrm, torch_cuda, targets, quats, body, legs, margin)


def test_bad_and_extreme_input(lrm, torch_cuda):
    legs, _ = pc.leg_families(lrm)["m2_5_identity"]
    quats, body, targets = fm.scene(lrm, 40, 5000, seed=8)
    bad_t = targets.copy()
    bad_t[::7] = np.nan
    bad_t[3::11, 1] = np.inf
    bad_t[5::13] = -np.inf
    bad_t[1024:1088] = np.nan
    for margin in (25.0, np.inf):
        check(lrm, torch_cuda, bad_t, quats, body, legs, margin)
    bad_b = body.copy()
    bad_b[1] = np.nan
    bad_b[2, 0] = np.inf
    bad_b[35] = -np.inf
    for margin in (25.0, np.inf):
        check(lrm, torch_cuda, targets, quats, bad_b, legs, margin)


@pytest.mark.parametrize("margin", [0.0, 25.0])
def test_far_from_the_origin(lrm, torch_cuda, margin):
    """the box-slack case: a cloud and bodies 4e6 mm from the origin, where the float32 grid is 0.25-0.5 mm and
    (t - body) - centre and body + centre round differently: no box cull may drop a candidate of the host loop.  The
    cloud is in x order, so the chunk boxes are thin slabs whose faces decide"""
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fm.scene(lrm, 192, 12000, seed=9)
    body, targets = pc.translated(body, targets, 4e6)
    want = check(lrm, torch_cuda, targets, quats, body, legs, margin)
    assert (want["miss"] >= 0).sum() > 100


def test_two_clouds_share_the_box_buffer(lrm, torch_cuda):
    """a large cloud, then a smaller one, then one below the box threshold, on one PoseSet: no box of an earlier cloud
    leaks into a later answer"""
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    ps = lrm.PoseSet(legs, 128, footholds=True)
    for k, nt in enumerate((30_000, 6_000, 3_000)):
        quats, body, targets = fm.scene(lrm, 64, nt, seed=20 + k)
        want = fm.host(lrm, targets, quats, body, legs, 25.0)
        assert (want["miss"] >= 0).any() and (want["miss"] < 0).any()
        fm.assert_same(run(lrm, torch_cuda, targets, quats, body, legs, 25.0, ps=ps), want)


def test_chain_on_one_pose_set(lrm, torch_cuda):
    """update -> footholds -> foothold_misses(count=...) on the SAME PoseSet; reach_dist on the chosen targets then returns
    mask 0 and the same shift bits, and moving the body by the shift brings the target within reach or onto the boundary"""
    torch = torch_cuda
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fm.scene(lrm, 256, 9000, seed=51)
    nl, npz = 6, 256
    ps = lrm.PoseSet(legs, npz, footholds=True, nominal=pc.nominal_for(6)).update(dev(torch, quats), dev(torch, body))
    tx, ty, tz = soa(torch, targets)
    count = ps.footholds(tx, ty, tz)[0]
    miss, m2, shift, near = ps.foothold_misses(tx, ty, tz, 100.0, count=count)
    torch.cuda.synchronize()
    want = fm.host(lrm, targets, quats, body, legs, 100.0, count.cpu().numpy())
    fm.assert_same((miss.cpu().numpy(), m2.cpu().numpy(), shift.cpu().numpy(), near.cpu().numpy()), want)
    have = (miss >= 0).view(-1)
    assert int(have.sum()) > 100 and not bool(((count > 0).view(-1) & have).any())
    pi, li = lrm.device.footholds_layout(npz, nl, "cuda")
    idx = miss.view(-1)[have].long()
    mask, field, _ = ps.reach_dist(tx[idx].contiguous(), ty[idx].contiguous(), tz[idx].contiguous(), pi[have].contiguous(),
                                   li[have].contiguous())
    torch.cuda.synchronize()
    assert int(mask.sum()) == 0
    assert torch.equal(field.view(torch.int32), shift.view(3, -1)[:, have].contiguous().view(torch.int32))


def test_update_footholds_and_misses_replay_from_a_graph(lrm, torch_cuda):
    """update(), footholds() and foothold_misses() only launch once the box buffer holds the cloud's size: captured on ONE
    side stream after a warm-up call, replayed after new quaternions, bodies and targets were copied into the captured
    tensors"""
    torch = torch_cuda
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    q0, b0, t0 = fm.scene(lrm, 128, 9000, seed=41)
    q1, b1, t1 = fm.scene(lrm, 128, 9000, seed=42)
    qt, bt, tt = dev(torch, q0), dev(torch, b0), dev(torch, t0.T.copy())
    shape = (6, 128)
    count, best = torch.empty(shape, dtype=torch.int32, device="cuda"), torch.empty(shape, dtype=torch.int32, device="cuda")
    bd2, al = torch.empty(shape, dtype=torch.float32, device="cuda"), torch.empty(128, dtype=torch.uint8, device="cuda")
    miss, near = torch.empty(shape, dtype=torch.int32, device="cuda"), torch.empty(shape, dtype=torch.int32, device="cuda")
    m2, sh = torch.empty(shape, dtype=torch.float32, device="cuda"), torch.empty((3,) + shape, dtype=torch.float32, device="cuda")
    ps = lrm.PoseSet(legs, 256, footholds=True)

    def work():
        ps.update(qt, bt)
        ps.footholds(tt[0], tt[1], tt[2], count, best, bd2, al)
        ps.foothold_misses(tt[0], tt[1], tt[2], 25.0, count, miss, m2, sh, near)

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
        miss.fill_(SENTINEL)
        near.fill_(SENTINEL)
        m2.fill_(SENTINEL)
        sh.fill_(SENTINEL)
        g.replay()
    torch.cuda.synchronize()
    cnt = fc.host(lrm, t1, q1, b1, legs, None)["count"]
    assert np.array_equal(count.cpu().numpy(), cnt)
    want = fm.host(lrm, t1, q1, b1, legs, 25.0, cnt)
    assert (want["miss"] >= 0).any() and (want["miss"] < 0).any()
    fm.assert_same((miss.cpu().numpy(), m2.cpu().numpy(), sh.cpu().numpy(), near.cpu().numpy()), want)
    del g
