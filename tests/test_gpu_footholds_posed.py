"""Foothold counts and choice per (pose, leg) on the device (run with -m gpu on an MI355X): the device table against the
host table byte for byte; lrm_footholds_posed_dev against the host loop lrm_footholds_posed_cpu bit for bit on the leg
families, cloud sizes, pose counts and bad input of the pair tests (tests/test_footholds_posed_cpu.py ties that host
loop to a brute force over the oracle); one scale case against the oracle directly; the chain update -> footholds -> ik
-> fk on ONE PoseSet; and a graph capture of update() + footholds().  Every output is prefilled with a sentinel, so an
unwritten entry fails too."""
import numpy as np
import pytest

import footholds_posed_cases as fc
import pair_cases as pc
import posed_cases
from conftest import reference_terrain
from test_pair_cpu import FAMILIES

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
                            "csrc", "lrm_footholds_posed.hip")).read()
    assert int(re.search(r"constexpr int kTargetTile = (\d+);", src).group(1)) == TILE
    assert int(re.search(r"tw0 < ntiles; tw0 \+= (\d+)\)", src).group(1)) == GROUP
    assert int(re.search(r"constexpr unsigned kMaxGrid = (\d+);", src).group(1)) * 4 == GRID_POSES


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def soa(torch, pts):
    t = dev(torch, np.asarray(pts, np.float32).reshape(-1, 3).T)
    return t[0], t[1], t[2]


def run(lrm, torch, targets, quats, body, legs, nominal, d2=True, all_legs=True, ps=None):
    """PoseSet.footholds into sentinel-filled outputs -> numpy (count, best, best_d2 or None, all_legs or None)"""
    npz, nl = len(quats), len(legs)
    if ps is None:
        ps = lrm.PoseSet(legs, npz, footholds=True, nominal=nominal)
    ps.update(dev(torch, quats), dev(torch, body))
    count = torch.full((nl, npz), SENTINEL, dtype=torch.int32, device="cuda")
    best = torch.full((nl, npz), SENTINEL, dtype=torch.int32, device="cuda")
    bd2 = torch.full((nl, npz), float(SENTINEL), dtype=torch.float32, device="cuda")
    al = torch.full((npz,), 9, dtype=torch.uint8, device="cuda")
    tx, ty, tz = soa(torch, targets)
    if d2 and all_legs:
        ps.footholds(tx, ty, tz, count, best, bd2, al)
    else:  # the NULL forms of the C ABI
        L, dp = lrm.load(), lambda t: None if t is None else t.data_ptr()
        rc = L.lrm_footholds_posed_dev(dp(tx), dp(ty), dp(tz), len(targets), dp(ps.workspace), dp(ps.fh_workspace), npz, nl,
                                       dp(count), dp(best), dp(bd2 if d2 else None), dp(al if all_legs else None),
                                       torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    if not d2:
        assert (bd2 == float(SENTINEL)).all()
    if not all_legs:
        assert (al == 9).all()
    return count.cpu().numpy(), best.cpu().numpy(), bd2.cpu().numpy() if d2 else None, al.cpu().numpy() if all_legs else None


def check(lrm, torch, targets, quats, body, legs, nominal, both=True, **kw):
    want = fc.host(lrm, targets, quats, body, legs, nominal)
    if both:
        pc.assert_both_outcomes(want)
    fc.assert_same(run(lrm, torch, targets, quats, body, legs, nominal, **kw), want)
    return want


def test_device_table_equals_host_table(lrm, torch_cuda):
    """every fixture and sweep quaternion, the mixed pose pool, and 1e5 random (quat, leg) pairs, byte for byte"""
    from lrm_amd import workloads
    torch = torch_cuda
    rng = np.random.default_rng(31)
    fam = pc.leg_families(lrm)
    quats = np.concatenate([posed_cases.fixture_quats(), np.asarray(workloads.reference_sweep_quats(), np.float32),
                            fc.pose_quats(lrm, 60, seed=2)]).astype(np.float32)
    for name in ("m2_8_identity", "random_8_identity", "random_7_tilted", "mixed_5_tilted", "moonbot_6_identity"):
        legs, _ = fam[name]
        nominal = pc.nominal_for(len(legs), seed=len(name))
        ps = lrm.PoseSet(legs, len(quats), footholds=True, nominal=nominal).update(dev(torch, quats))
        torch.cuda.synchronize()
        got = ps.fh_workspace.cpu().numpy().view(np.float32).reshape(len(quats), len(legs), 8)
        want = lrm.dbg_pose_footholds_compile_host(quats, legs, nominal)
        diff = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert len(diff) == 0, (name, len(diff), [(tuple(d), quats[d[0]], got[tuple(d)], want[tuple(d)]) for d in diff[:4]])
        assert np.isfinite(want[..., 3]).any() and np.isposinf(want[..., 3]).any()
    # 1e5 random pairs: 12 500 random unit quaternions (a few scaled off unit) x 8 random legs
    from ik_cases import random_legs
    legs = np.stack([leg for _, leg, _ in random_legs(lrm)][:8]).astype(np.float32)
    q = posed_cases.random_unit_quats(12_500, rng)
    q[::97] *= rng.uniform(0.5, 2.0, (len(q[::97]), 1)).astype(np.float32)
    nominal = pc.nominal_for(8, seed=1)
    ps = lrm.PoseSet(legs, len(q), footholds=True, nominal=nominal).update(dev(torch, q))
    torch.cuda.synchronize()
    got = ps.fh_workspace.cpu().numpy().view(np.uint32).reshape(len(q), 8, 8)
    want = lrm.dbg_pose_footholds_compile_host(q, legs, nominal).view(np.uint32)
    bad = np.nonzero((got != want).any(-1))
    assert len(bad[0]) == 0, (len(bad[0]), q[bad[0][:3]], bad[1][:3])


@pytest.mark.parametrize("family", FAMILIES)
def test_every_leg_family(lrm, torch_cuda, family):
    legs, _ = pc.leg_families(lrm)[family]
    quats, body, targets = fc.scene(lrm, 96, 6000, seed=len(family) + len(legs))
    for nominal in (None, pc.nominal_for(len(legs))):
        check(lrm, torch_cuda, targets, quats, body, legs, nominal)


@pytest.mark.parametrize("nt", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 4095, 4096, 4097, GROUP * TILE - 1, GROUP * TILE + 1,
                                (GROUP + 1) * TILE + 1])
def test_every_cloud_size(lrm, torch_cuda, nt):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    npz = 64 if nt > 20000 else 128
    quats, body, targets = fc.scene(lrm, npz, nt, seed=nt % 97)
    check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(6), both=nt >= TILE - 1)


@pytest.mark.parametrize("nposes", [1, 2, 3, 4, 5, 255, 257])
@pytest.mark.parametrize("nt", [3000, 5000])
def test_every_pose_count(lrm, torch_cuda, nposes, nt):
    legs, _ = pc.leg_families(lrm)["mixed_5_tilted"]
    quats, body, targets = fc.scene(lrm, nposes, nt, seed=nposes + nt)
    check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(5), both=nposes > 100)


def test_poses_past_the_grid_stride(lrm, torch_cuda):
    """more poses than one pass of the grid holds: a wave walks on to pose + GRID_POSES"""
    legs, _ = pc.leg_families(lrm)["m2_2_tilted"]
    n = GRID_POSES + 777
    quats, body, targets = fc.scene(lrm, n, 64, seed=3)
    targets = targets * np.float32(0.05)  # 64 targets within 50 mm of the origin
    body[:, :2] = body[:, :2] * np.float32(0.02)
    want = check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(2))
    tail = want["count"][:, GRID_POSES:]
    assert (tail > 0).sum() > 20 and (tail == 0).sum() > 20


@pytest.mark.parametrize("kind", ["dense_cluster_boxes", "dense_cluster_plain", "sparse_tiles", "duplicates"])
def test_scenes_against_each_cull(lrm, torch_cuda, kind):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    if kind == "duplicates":
        quats, body, base = fc.scene(lrm, 80, 5000, seed=4)
        targets, _ = pc.with_spread_duplicates(base, seed=6)
    elif kind == "sparse_tiles":
        quats, body, targets = fc.scene(lrm, 80, 9 * 1024, seed=2, kind="sparse_tiles")
    else:
        quats, body, targets = fc.scene(lrm, 80, 6000 if kind.endswith("boxes") else 3500, seed=1, kind="dense_cluster")
    check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(6, seed=5))


@pytest.mark.parametrize("nt", [3000, 20000])
def test_bad_and_extreme_input(lrm, torch_cuda, nt):
    legs, _ = pc.leg_families(lrm)["m2_5_identity"]
    quats, body, targets = fc.scene(lrm, 80, nt, seed=8)
    bad_t = targets.copy()
    bad_t[::7] = np.nan
    bad_t[3::11, 1] = np.inf
    bad_t[5::13] = -np.inf
    bad_t[1024:1088] = np.nan
    check(lrm, torch_cuda, bad_t, quats, body, legs, pc.nominal_for(5))
    bad_b = body.copy()
    bad_b[1] = np.nan
    bad_b[2, 0] = np.inf
    bad_b[5] = -np.inf
    check(lrm, torch_cuda, targets, quats, bad_b, legs, pc.nominal_for(5))
    want = check(lrm, torch_cuda, targets, quats, body, legs, np.full((5, 3), 1e30, np.float32))
    assert np.isposinf(want["best_d2"]).all()


@pytest.mark.parametrize("offset", [1e4, 1e6, 4e6])
def test_far_from_the_origin(lrm, torch_cuda, offset):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fc.scene(lrm, 96, 6000, seed=9)
    body, targets = pc.translated(body, targets, offset)
    check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(6))


def test_null_outputs(lrm, torch_cuda):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fc.scene(lrm, 45, 5000, seed=12)
    check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(6), d2=False)
    check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(6), all_legs=False)
    lrm.set_mode(lrm.MODE_STRICT)  # the answers do not depend on the mode
    try:
        check(lrm, torch_cuda, targets, quats, body, legs, None, d2=False, all_legs=False)
    finally:
        lrm.set_mode(lrm.MODE_FAST)  # the library default


def test_four_clouds_share_the_box_buffer(lrm, torch_cuda):
    """four clouds of different size, large, small, below the box threshold and large again, in one process on one
    PoseSet: no box of an earlier cloud leaks into a later answer"""
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6)
    ps = lrm.PoseSet(legs, 64, footholds=True, nominal=nominal)
    for k, nt in enumerate((40_000, 6_000, 3_000, 23_000)):
        quats, body, targets = fc.scene(lrm, 64, nt, seed=20 + k)
        want = fc.host(lrm, targets, quats, body, legs, nominal)
        pc.assert_both_outcomes(want)
        fc.assert_same(run(lrm, torch_cuda, targets, quats, body, legs, nominal, ps=ps), want)


def test_scale_against_the_oracle(lrm, oracle, torch_cuda):
    """the reference terrain (65 536 targets), 24 000 poses with a sweep orientation each, 6 M2 legs; a fixed sample of 64
    poses against the oracle brute force (64 x 6 x 65 536 = 2.5e7 evaluations)"""
    from lrm_amd import workloads
    t = reference_terrain()
    ground = np.ascontiguousarray(t["ground"], np.float32)
    assert len(ground) == 65536
    n = 24_000
    body = np.ascontiguousarray(t["bodies"][np.random.default_rng(5).choice(len(t["bodies"]), n, replace=False)], np.float32)
    quats = fc.sweep_pose_quats(lrm, n)
    legs = workloads.hexapod(lrm.get_M2_leg, 6)
    nominal = pc.nominal_for(6, seed=7)
    got = run(lrm, torch_cuda, ground, quats, body, legs, nominal)
    pick = np.sort(np.random.default_rng(21).choice(n, 64, replace=False))
    want = fc.brute(oracle, ground, quats, body, legs, fc.nominal_w_of(lrm, quats, legs, nominal), pick)
    assert (want["count"] > 0).any() and (want["count"] == 0).any()
    fc.assert_same((got[0][:, pick], got[1][:, pick], got[2][:, pick], got[3][pick]), want)
    assert 0.01 < got[3].mean() < 1.0 and np.array_equal(got[3], (got[0] > 0).all(0))


def test_chain_on_one_pose_set(lrm, torch_cuda):
    """update -> footholds -> ik -> fk on the SAME PoseSet: status in {1, 3} exactly where best >= 0 and 0 where best is
    -1; for status 1 the FK tip is within 2.5e-3 mm + 2^-22 |target| of the chosen target (the FK bound of DESIGN.md 3.10)"""
    from lrm_amd import workloads
    torch = torch_cuda
    t = reference_terrain()
    ground = np.ascontiguousarray(t["ground"], np.float32)
    n, nl = 20_000, 6
    body = np.ascontiguousarray(t["bodies"][np.random.default_rng(6).choice(len(t["bodies"]), n, replace=False)], np.float32)
    quats = fc.sweep_pose_quats(lrm, n, seed=8)
    legs = workloads.hexapod(lrm.get_M2_leg, nl)
    nominal = np.stack([lrm.apply_fk_cpu(np.array([[0.0, 0.3, -1.2]], np.float32), leg, (1, 0, 0, 0))[0][0] for leg in legs])
    ps = lrm.PoseSet(legs, n, ik=True, footholds=True, nominal=nominal).update(dev(torch, quats), dev(torch, body))
    tx, ty, tz = soa(torch, ground)
    count, best, best_d2, all_legs = ps.footholds(tx, ty, tz)
    pi, li = lrm.device.footholds_layout(ps.nposes, ps.nlegs, "cuda")
    ang, st = ps.ik(tx, ty, tz, pi, li, target_idx=best.view(-1))
    tip = ps.fk(ang[0], ang[1], ang[2], pi, li)
    torch.cuda.synchronize()
    ti, s = best.cpu().numpy().reshape(-1), st.cpu().numpy()
    assert (ti == -1).any() and (ti >= 0).sum() > 5_000
    assert np.array_equal(np.isin(s, (1, 3)), ti >= 0) and np.array_equal(s == 0, ti == -1)
    ok = s == 1
    assert ok.sum() > 5_000
    chosen = ground[ti[ok]].astype(np.float64)
    err = np.abs(tip.cpu().numpy().T[ok].astype(np.float64) - chosen)
    assert (err <= 2.5e-3 + 2.0 ** -22 * np.abs(chosen)).all(), float(err.max())


def test_update_and_footholds_replay_from_a_graph(lrm, torch_cuda):
    """update() and footholds() only launch once the box buffer holds the cloud's size: captured on ONE side stream after
    a warm-up call, replayed after new quaternions, bodies and targets were copied into the captured tensors"""
    torch = torch_cuda
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6)
    q0, b0, t0 = fc.scene(lrm, 256, 9000, seed=41)
    q1, b1, t1 = fc.scene(lrm, 256, 9000, seed=42)
    q1 = q1[::-1].copy()
    qt, bt, tt = dev(torch, q0), dev(torch, b0), dev(torch, t0.T.copy())
    count = torch.empty((6, 256), dtype=torch.int32, device="cuda")
    best = torch.empty((6, 256), dtype=torch.int32, device="cuda")
    bd2 = torch.empty((6, 256), dtype=torch.float32, device="cuda")
    al = torch.empty(256, dtype=torch.uint8, device="cuda")
    ps = lrm.PoseSet(legs, 256, footholds=True, nominal=nominal)

    def work():
        ps.update(qt, bt)
        ps.footholds(tt[0], tt[1], tt[2], count, best, bd2, al)

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
        count.fill_(SENTINEL)
        best.fill_(SENTINEL)
        bd2.fill_(SENTINEL)
        al.fill_(9)
        g.replay()
    torch.cuda.synchronize()
    want = fc.host(lrm, t1, q1, b1, legs, nominal)
    pc.assert_both_outcomes(want)
    fc.assert_same((count.cpu().numpy(), best.cpu().numpy(), bd2.cpu().numpy(), al.cpu().numpy()), want)
    del g
