"""Joint angles per (target, pose, leg) on the MI355X (run with -m gpu): the device IK table against the host's, PoseSet.ik /
PoseSet.fk against the posed CPU calls bit for bit in every query order, against the single-pose device call, at scale, fed
from lrm_footholds_dev, with out-of-range indices, and captured in a graph."""
import numpy as np
import pytest

from conftest import bits_equal, random_cloud
from footholds_cases import QUATS, legs_for, nominal_for, scene
from posed_cases import fixture_quats, leg_table, pose_table, queries, random_unit_quats

pytestmark = pytest.mark.gpu

INT32_MIN = np.iinfo(np.int32).min


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the gpu tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def soa(torch, a):
    t = dev(torch, np.asarray(a, np.float32).T)
    return t[0], t[1], t[2]


def seeds(n, rng):
    seed = (rng.random((n, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
    seed[::7, 0] = np.nan
    seed[3::11] = np.inf
    seed[5::13, 2] = -np.inf
    seed[6::17] = 1e20
    return seed


def check_ik(ang, st, want_a, want_s):
    assert np.array_equal(st.cpu().numpy(), want_s)
    assert bits_equal(ang.cpu().numpy().T, want_a).all()


def test_device_ik_table_equals_the_host_table(lrm, torch_cuda):
    """the quaternion families of test_gpu_posed.py's record test: the device entries are the host's, byte for byte (the
    only device-side libm call is the double asin of rotate_leg_data's pitch: DESIGN.md 3.7, 3.10)"""
    torch = torch_cuda
    from lrm_amd import workloads
    rng = np.random.default_rng(21)
    quats = np.concatenate([fixture_quats(), workloads.reference_sweep_quats(), random_unit_quats(131_072, rng)])
    legs = np.concatenate([leg_table(lrm), lrm.get_M2_leg(-2.1)[None]])
    assert len(quats) * len(legs) >= 1_000_000
    ps = lrm.PoseSet(legs, len(quats), ik=True)
    ps.update(dev(torch, quats))
    torch.cuda.synchronize()
    got = ps.ik_workspace.cpu().numpy().reshape(len(quats), len(legs), lrm.POSE_IK_RECORD_BYTES)
    want = lrm.dbg_pose_ik_compile_host(quats, legs)
    bad = np.nonzero((got != want).any(axis=2))
    assert len(bad[0]) == 0, f"{len(bad[0])} entries differ, first (pose, leg) {bad[0][0], bad[1][0]}: quat {quats[bad[0][0]]}"


@pytest.mark.parametrize("order", ["pair_major", "interleaved", "shuffled"])
def test_posed_ik_fk_equal_the_cpu_calls(lrm, torch_cuda, order):
    """three query orders, ragged n, seeds, target_idx, 4-byte-offset views and caller outputs with a guard past n"""
    torch = torch_cuda
    quats, body = pose_table(lrm)
    legs = leg_table(lrm)
    rng = np.random.default_rng(31)
    xyz, pose, leg = queries(len(quats), len(legs), body, 197, rng, order)
    n = len(xyz) - 37  # ragged: not a multiple of 64 or 256
    assert n % 64 and n % 256
    xyz, pose, leg = xyz[:n], pose[:n], leg[:n]
    xyz[::4001] = np.nan
    ps = lrm.PoseSet(legs, 64, ik=True).update(dev(torch, quats), dev(torch, body))
    x, y, z = soa(torch, xyz)
    pi, li = dev(torch, pose), dev(torch, leg)
    want_a, want_s, _ = lrm.apply_ik_posed_cpu(xyz, pose, leg, quats, body, legs)
    ang, st = ps.ik(x, y, z, pi, li)
    tip = ps.fk(ang[0], ang[1], ang[2], pi, li)
    torch.cuda.synchronize()
    check_ik(ang, st, want_a, want_s)
    want_p, _ = lrm.apply_fk_posed_cpu(want_a, pose, leg, quats, body, legs)
    assert bits_equal(tip.cpu().numpy().T, want_p).all()
    # seeds and a target_idx with repeats
    seed = seeds(n, rng)
    ti = rng.integers(0, n, n).astype(np.int32)
    want_a2, want_s2, _ = lrm.apply_ik_posed_cpu(xyz, pose, leg, quats, body, legs, target_idx=ti, seed=seed)
    ang2, st2 = ps.ik(x, y, z, pi, li, target_idx=dev(torch, ti), seed=soa(torch, seed))
    torch.cuda.synchronize()
    check_ik(ang2, st2, want_a2, want_s2)
    # views that start 1 element in (4-byte aligned only), outputs into views of wider buffers, guards past n
    big = torch.zeros((3, n + 1), dtype=torch.float32, device="cuda")
    big[:, 1:] = torch.stack([x, y, z])
    pib = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    pib[1:] = pi
    lib_ = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
    lib_[1:] = li
    out = torch.full((3, n + 5), 7.0, dtype=torch.float32, device="cuda")[:, 1:]
    stb = torch.full((n + 4,), 9, dtype=torch.uint8, device="cuda")[1:]
    ang3, st3 = ps.ik(big[0, 1:], big[1, 1:], big[2, 1:], pib[1:], lib_[1:], out=out, status=stb)
    pout = torch.full((3, n + 5), 7.0, dtype=torch.float32, device="cuda")[:, 1:]
    tip3 = ps.fk(ang3[0, :n], ang3[1, :n], ang3[2, :n], pib[1:], lib_[1:], out=pout)
    torch.cuda.synchronize()
    check_ik(ang3[:, :n], st3[:n], want_a, want_s)
    assert bits_equal(tip3[:, :n].cpu().numpy().T, want_p).all()
    assert (ang3[:, n:] == 7.0).all() and (st3[n:] == 9).all() and (tip3[:, n:] == 7.0).all()


def test_one_query_and_none(lrm, torch_cuda):
    torch = torch_cuda
    quats, body = pose_table(lrm, n=3)
    legs = leg_table(lrm)
    ps = lrm.PoseSet(legs, 3, ik=True).update(dev(torch, quats), dev(torch, body))
    xyz = (body[2:3] + np.array([[300, 40, -120]], np.float32)).astype(np.float32)
    pose, leg = np.array([2], np.int32), np.array([6], np.uint8)
    x, y, z = soa(torch, xyz)
    ang, st = ps.ik(x, y, z, dev(torch, pose), dev(torch, leg))
    tip = ps.fk(ang[0], ang[1], ang[2], dev(torch, pose), dev(torch, leg))
    torch.cuda.synchronize()
    want_a, want_s, _ = lrm.apply_ik_posed_cpu(xyz, pose, leg, quats, body, legs)
    check_ik(ang, st, want_a, want_s)
    assert bits_equal(tip.cpu().numpy().T, lrm.apply_fk_posed_cpu(want_a, pose, leg, quats, body, legs)[0]).all()
    e = torch.empty(0, dtype=torch.float32, device="cuda")
    ang, st = ps.ik(e, e, e)
    assert tuple(ang.shape) == (3, 0) and st.numel() == 0 and tuple(ps.fk(e, e, e).shape) == (3, 0)
    with pytest.raises(ValueError):
        lrm.PoseSet(legs, 3).update(dev(torch, quats)).ik(x, y, z)  # built without ik=True


def test_single_pose_equals_the_single_pose_device_call(lrm, torch_cuda):
    torch = torch_cuda
    pts = random_cloud(1_000_000, seed=5)
    leg = lrm.get_moonbot_leg(0.9)
    q = np.array([0.95, 0.1, -0.2, 0.2], np.float32)
    q /= np.float32(np.linalg.norm(q))
    x, y, z = soa(torch, pts)
    wa, ws = lrm.device.ik(x, y, z, leg, q)
    wp = lrm.device.fk(wa[0], wa[1], wa[2], leg, q)
    ps = lrm.PoseSet([leg], 1, ik=True).update(dev(torch, q[None]))
    ang, st = ps.ik(x, y, z)
    tip = ps.fk(ang[0], ang[1], ang[2])
    torch.cuda.synchronize()
    assert torch.equal(st, ws) and torch.equal(ang.view(torch.int32), wa.view(torch.int32))
    assert torch.equal(tip.view(torch.int32), wp.view(torch.int32))
    assert len(torch.unique(st)) >= 2


def test_scale_4096_poses_6_legs_pair_major(lrm, torch_cuda):
    torch = torch_cuda
    from lrm_amd import workloads
    rng = np.random.default_rng(41)
    B, K = 4096, 64
    legs = workloads.hexapod(lrm.get_moonbot_leg).astype(np.float32)
    quats = random_unit_quats(B, rng)
    body = (rng.random((B, 3), dtype=np.float32) * 8000 - 4000).astype(np.float32)
    xyz, pose, leg = queries(B, len(legs), body, K, rng, "pair_major")
    ps = lrm.PoseSet(legs, B, ik=True).update(dev(torch, quats), dev(torch, body))
    x, y, z = soa(torch, xyz)
    ang, st = ps.ik(x, y, z, dev(torch, pose), dev(torch, leg))
    torch.cuda.synchronize()
    want_a, want_s, _ = lrm.apply_ik_posed_cpu(xyz, pose, leg, quats, body, legs)
    check_ik(ang, st, want_a, want_s)


def test_scale_footholds_feed_the_posed_ik(lrm, torch_cuda):
    """100 000 bodies x 6 legs in lrm_footholds_dev's [l*nb + b] order through footholds_layout: the status rule on every
    query, a fixed sample of 2^16 queries against the CPU call"""
    torch = torch_cuda
    nb, nl = 100_000, 6
    quat = np.asarray(QUATS["tilted"], np.float32)
    bodies, targets = scene(nb, 20_000, seed=13, half=3000.0)
    legs = legs_for(lrm, nl, quat)
    bx, by, bz = soa(torch, bodies)
    tx, ty, tz = soa(torch, targets)
    count, best, _ = lrm.device.footholds(bx, by, bz, tx, ty, tz, legs, quat, nominal_for(nl))
    ident = np.tile(np.array([1, 0, 0, 0], np.float32), (nb, 1))
    ps = lrm.PoseSet(legs, nb, ik=True).update(dev(torch, ident), dev(torch, bodies))
    pi, li = lrm.device.footholds_layout(nb, nl, "cuda")
    ang, st = ps.ik(tx, ty, tz, pi, li, target_idx=best.view(-1))
    torch.cuda.synchronize()
    ti = best.cpu().numpy().reshape(-1)
    s = st.cpu().numpy()
    assert (ti == -1).any() and (ti >= 0).sum() > 10_000
    assert np.array_equal(s == 0, ti == -1)
    assert (s[ti >= 0] == 1).all(), np.bincount(s, minlength=5)  # M2 legs: {1, 3} and no model gap
    sel = np.sort(np.random.default_rng(0).choice(nb * nl, 1 << 16, replace=False))
    pose = np.tile(np.arange(nb, dtype=np.int32), nl)
    leg = np.repeat(np.arange(nl, dtype=np.uint8), nb)
    assert np.array_equal(pi.cpu().numpy(), pose) and np.array_equal(li.cpu().numpy(), leg)
    want_a, want_s, _ = lrm.apply_ik_posed_cpu(targets, pose[sel], leg[sel], ident, bodies, legs, target_idx=ti[sel])
    assert np.array_equal(s[sel], want_s) and bits_equal(ang.cpu().numpy().T[sel], want_a).all()


def test_out_of_range_indices_on_the_device(lrm, torch_cuda):
    """workspaces sized exactly (nposes, nlegs): an unclamped index would leave them; the check is the outputs"""
    torch = torch_cuda
    rng = np.random.default_rng(8)
    quats, body = pose_table(lrm, n=4)
    legs = leg_table(lrm)
    nl = len(legs)
    xyz, pose, leg = queries(4, nl, body, 300, rng, "shuffled")
    n = len(xyz)
    ti = rng.permutation(n).astype(np.int32)
    kind = rng.integers(0, 8, n)
    pose[kind == 1] = rng.choice(np.array([-1, 4, 1000, INT32_MIN], np.int32), (kind == 1).sum())
    leg[kind == 2] = rng.choice(np.array([nl, nl + 1, 255], np.uint8), (kind == 2).sum())
    ti[kind == 3] = rng.choice(np.array([-1, n, n + 7, INT32_MIN], np.int32), (kind == 3).sum())
    oob = np.isin(kind, (1, 2, 3))
    ps = lrm.PoseSet(legs, 4, ik=True).update(dev(torch, quats), dev(torch, body))
    assert ps.workspace.numel() == 4 * nl * 512 and ps.ik_workspace.numel() == 4 * nl * 128
    x, y, z = soa(torch, xyz)
    pi, li = dev(torch, pose), dev(torch, leg)
    with pytest.raises(ValueError):
        ps.ik(x, y, z, pi, li, target_idx=dev(torch, ti))  # check=True refuses the pose / leg indices on the host
    ang, st = ps.ik(x, y, z, pi, li, target_idx=dev(torch, ti), check=False)
    torch.cuda.synchronize()
    want_a, want_s, _ = lrm.apply_ik_posed_cpu(xyz, pose, leg, quats, body, legs, target_idx=ti)
    assert (want_s[oob] == 0).all() and (want_s[~oob] != 0).all()
    check_ik(ang, st, want_a, want_s)
    a = np.nan_to_num(want_a)
    tip = ps.fk(*soa(torch, a), pi, li, check=False)
    torch.cuda.synchronize()
    want_p, _ = lrm.apply_fk_posed_cpu(a, pose, leg, quats, body, legs)
    assert np.isnan(want_p[np.isin(kind, (1, 2))]).all() and bits_equal(tip.cpu().numpy().T, want_p).all()


def test_update_ik_fk_replay_from_a_graph(lrm, torch_cuda):
    """update() (with the IK table), ik() and fk() only launch: captured on ONE side stream, no parallel branches, replayed
    after new quaternions, bodies and targets were copied into the captured tensors"""
    torch = torch_cuda
    legs = leg_table(lrm)[:6]
    B = 256
    rng = np.random.default_rng(51)
    q0, q1 = random_unit_quats(B, rng), random_unit_quats(B, rng)
    b0 = (rng.random((B, 3), dtype=np.float32) * 2000 - 1000).astype(np.float32)
    b1 = (rng.random((B, 3), dtype=np.float32) * 2000 - 1000).astype(np.float32)
    xyz0, pose, leg = queries(B, len(legs), b0, 64, rng, "interleaved")
    xyz1, _, _ = queries(B, len(legs), b1, 64, rng, "interleaved")
    n = len(xyz0)
    qt, bt = dev(torch, q0), dev(torch, b0)
    inp = dev(torch, xyz0.T.copy())
    pi, li = dev(torch, pose), dev(torch, leg)
    ang = torch.empty((3, n), dtype=torch.float32, device="cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    tip = torch.empty((3, n), dtype=torch.float32, device="cuda")
    ps = lrm.PoseSet(legs, B, ik=True)

    def work():
        ps.update(qt, bt)
        ps.ik(inp[0], inp[1], inp[2], pi, li, out=ang, status=st, check=False)
        ps.fk(ang[0], ang[1], ang[2], pi, li, out=tip, check=False)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture
        work()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            work()
        qt.copy_(dev(torch, q1))
        bt.copy_(dev(torch, b1))
        inp.copy_(dev(torch, xyz1.T.copy()))
        ang.zero_()
        st.zero_()
        tip.zero_()
        g.replay()
    torch.cuda.synchronize()
    want_a, want_s, _ = lrm.apply_ik_posed_cpu(xyz1, pose, leg, q1, b1, legs)
    want_p, _ = lrm.apply_fk_posed_cpu(want_a, pose, leg, q1, b1, legs)
    check_ik(ang, st, want_a, want_s)
    assert bits_equal(tip.cpu().numpy().T, want_p).all()
    del g
