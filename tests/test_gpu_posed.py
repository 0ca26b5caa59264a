"""Batched multi-pose queries on the MI355X (run with -m gpu): the device pose compiler against the host's, the posed kernel
against the oracle per (pose, leg) in every index order, against the reference fixtures and against the single-pose strict
call, at scale, and captured in a graph.  Every output bit must be equal.  Out-of-range indices reach the kernel in
tests/test_gpu_query_shapes.py, next to its wave, block and pass boundaries (tests/test_posed_cpu.py covers that rule on the
host)."""
import numpy as np
import pytest

from conftest import bits_equal, golden_cases, load_case, random_cloud
from posed_cases import fixture_quats, leg_table, oracle_answer, pose_table, queries, random_unit_quats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the gpu tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def soa(torch, xyz):
    t = dev(torch, xyz.T)
    return t[0], t[1], t[2]


def check(got_m, got_d, got_v, want):
    wm, wv, wd = want
    assert np.array_equal(got_m.cpu().numpy(), wm)
    assert np.array_equal(got_v.cpu().numpy(), wv)
    assert bits_equal(got_d.cpu().numpy().T, wd).all()


def test_device_pose_records_equal_the_host_compiler(lrm, torch_cuda):
    """>= 1e6 (quat, leg) pairs plus every fixture and sweep quaternion: the device records are the host's, byte for byte
    (the device takes sincosf from lrm_sincosf and asin from the device libm: see DESIGN.md)"""
    torch = torch_cuda
    from lrm_amd import workloads
    rng = np.random.default_rng(21)
    quats = np.concatenate([fixture_quats(), workloads.reference_sweep_quats(), random_unit_quats(131_072, rng)])
    body = (rng.standard_normal((len(quats), 3)) * 800).astype(np.float32)
    legs = np.concatenate([leg_table(lrm), lrm.get_M2_leg(-2.1)[None]])
    assert len(quats) * len(legs) >= 1_000_000
    ps = lrm.PoseSet(legs, len(quats))
    ps.update(dev(torch, quats), dev(torch, body))
    got = ps.workspace.cpu().numpy().reshape(len(quats), len(legs), lrm.POSE_RECORD_BYTES)
    want = lrm.dbg_pose_compile_host(quats, body, legs)
    bad = np.nonzero((got != want).any(axis=2))
    assert len(bad[0]) == 0, f"{len(bad[0])} records differ, first (pose, leg) {bad[0][0], bad[1][0]}: quat {quats[bad[0][0]]}"


@pytest.mark.parametrize("order", ["pair_major", "interleaved", "shuffled"])
@pytest.mark.parametrize("mode", ["strict", "fast"])
def test_posed_call_matches_oracle(lrm, oracle, torch_cuda, order, mode):
    """three index orders, a ragged n, aligned and unaligned views; the arithmetic mode does not matter"""
    torch = torch_cuda
    lrm.set_mode(lrm.MODE_STRICT if mode == "strict" else lrm.MODE_FAST)
    try:
        quats, body = pose_table(lrm)
        legs = leg_table(lrm)
        rng = np.random.default_rng(31)
        xyz, pose, leg = queries(len(quats), len(legs), body, 197, rng, order)
        n = len(xyz) - 37  # ragged
        xyz, pose, leg = xyz[:n], pose[:n], leg[:n]
        want = oracle_answer(oracle, xyz, pose, leg, quats, body, legs)
        ps = lrm.PoseSet(legs, 64).update(dev(torch, quats), dev(torch, body))
        x, y, z = soa(torch, xyz)
        pi, li = dev(torch, pose), dev(torch, leg)
        m, d, v = ps.reach_dist(x, y, z, pi, li)
        torch.cuda.synchronize()
        check(m, d, v, want)
        # reach only: the same mask
        m2, d2, v2 = ps.reach_dist(x, y, z, pi, li, want_dist=False)
        torch.cuda.synchronize()
        assert d2 is None and v2 is None and torch.equal(m2, m)
        # views that start 1 element in (4-byte aligned only), outputs into views of wider buffers
        big = torch.zeros((3, n + 1), dtype=torch.float32, device="cuda")
        big[:, 1:] = torch.stack([x, y, z])
        pib = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        pib[1:] = pi
        lib_ = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
        lib_[1:] = li
        mb = torch.zeros(n + 3, dtype=torch.uint8, device="cuda")
        vb = torch.zeros(n + 3, dtype=torch.uint8, device="cuda")
        fb = torch.zeros((3, n + 5), dtype=torch.float32, device="cuda")
        m3, d3, v3 = ps.reach_dist(big[0, 1:], big[1, 1:], big[2, 1:], pib[1:], lib_[1:], mask=mb[3:], out=fb[:, 5:], valid=vb[3:])
        torch.cuda.synchronize()
        check(m3, d3, v3, want)
        assert not mb[:3].any() and not vb[:3].any() and not fb[:, :5].any()
    finally:
        lrm.set_mode(lrm.MODE_FAST)


@pytest.mark.parametrize("name", golden_cases())
def test_each_fixture_as_one_pose(lrm, torch_cuda, name):
    torch = torch_cuda
    c = load_case(name)
    ps = lrm.PoseSet([c["leg"]], 1).update(dev(torch, np.asarray(c["quat"], np.float32).reshape(1, 4)))
    x, y, z = soa(torch, c["points"])
    m, d, v = ps.reach_dist(x, y, z)
    torch.cuda.synchronize()
    check(m, d, v, (c["mask"], c["valid"], c["dist"]))


def test_single_pose_equals_the_strict_single_pose_call(lrm, torch_cuda):
    torch = torch_cuda
    pts = random_cloud(1_000_000, seed=5)
    leg = lrm.get_moonbot_leg(0.9)
    q = np.array([0.95, 0.1, -0.2, 0.2], np.float32)
    x, y, z = soa(torch, pts)
    lrm.set_mode(lrm.MODE_STRICT)
    try:
        wm, wd = lrm.device.reach_dist(x, y, z, leg, q)
        wd2, wv = lrm.device.dist(x, y, z, leg, q)
    finally:
        lrm.set_mode(lrm.MODE_FAST)
    ps = lrm.PoseSet([leg], 1).update(dev(torch, q[None]))
    m, d, v = ps.reach_dist(x, y, z)
    torch.cuda.synchronize()
    assert torch.equal(m, wm) and torch.equal(v, wv)
    assert torch.equal(d.view(torch.int32), wd.view(torch.int32)) and torch.equal(wd.view(torch.int32), wd2.view(torch.int32))


def test_scale_4096_poses_6_legs(lrm, oracle, torch_cuda):
    """4096 poses x 6 legs x 400 targets (~1e7 queries, pair-major): a 2e5-query sample and 8 whole (pose, leg) pairs
    against the oracle"""
    torch = torch_cuda
    from lrm_amd import workloads
    rng = np.random.default_rng(41)
    B, K = 4096, 400
    legs = workloads.hexapod(lrm.get_moonbot_leg).astype(np.float32)
    quats = random_unit_quats(B, rng)
    body = (rng.random((B, 3), dtype=np.float32) * 8000 - 4000).astype(np.float32)
    xyz, pose, leg = queries(B, len(legs), body, K, rng, "pair_major")
    ps = lrm.PoseSet(legs, B).update(dev(torch, quats), dev(torch, body))
    x, y, z = soa(torch, xyz)
    m, d, v = ps.reach_dist(x, y, z, dev(torch, pose), dev(torch, leg))
    torch.cuda.synchronize()
    m, d, v = m.cpu().numpy(), d.cpu().numpy().T, v.cpu().numpy()
    sample = np.sort(rng.choice(len(xyz), 200_000, replace=False))
    pairs = rng.choice(B * len(legs), 8, replace=False)
    whole = np.concatenate([np.arange(p * K, (p + 1) * K) for p in pairs])
    for sel in (sample, whole):
        wm, wv, wd = oracle_answer(oracle, xyz[sel], pose[sel], leg[sel], quats, body, legs)
        assert np.array_equal(m[sel], wm) and np.array_equal(v[sel], wv) and bits_equal(d[sel], wd).all()


def test_update_and_queries_replay_from_a_graph(lrm, oracle, torch_cuda):
    """PoseSet.update + reach_dist(check=False) only launch: captured in a graph on a side stream and replayed after new
    quaternions were copied into the captured tensor, they answer for the NEW poses, and device memory does not move"""
    torch = torch_cuda
    legs = leg_table(lrm)[:6]
    B = 256
    rng = np.random.default_rng(51)
    q0, q1 = random_unit_quats(B, rng), random_unit_quats(B, rng)
    body = (rng.random((B, 3), dtype=np.float32) * 2000 - 1000).astype(np.float32)
    xyz, pose, leg = queries(B, len(legs), body, 64, rng, "interleaved")
    n = len(xyz)
    qt, bt = dev(torch, q0), dev(torch, body)
    x, y, z = soa(torch, xyz)
    pi, li = dev(torch, pose), dev(torch, leg)
    mask = torch.empty(n, dtype=torch.uint8, device="cuda")
    valid = torch.empty(n, dtype=torch.uint8, device="cuda")
    field = torch.empty((3, n), dtype=torch.float32, device="cuda")
    ps = lrm.PoseSet(legs, B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture
        ps.update(qt, bt)
        ps.reach_dist(x, y, z, pi, li, mask=mask, out=field, valid=valid, check=False)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ps.update(qt, bt)
            ps.reach_dist(x, y, z, pi, li, mask=mask, out=field, valid=valid, check=False)
        qt.copy_(dev(torch, q1))
        mask.zero_()
        valid.zero_()
        field.zero_()
        g.replay()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (8 << 20)  # nothing but the graph's own bookkeeping
    check(mask, field, valid, oracle_answer(oracle, xyz, pose, leg, q1, body, legs))
    del g
