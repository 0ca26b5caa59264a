"""Joint angles on the device (lrm_ik_dev, lrm_fk_dev): bit-identical to the CPU entry points (angles, status bytes, FK
positions) on standard and random legs, with and without a seed, ragged counts and unaligned views; the contract on the
config-2 cloud; one capture and replay in a graph."""
import numpy as np
import pytest

from conftest import bits_equal
from ik_cases import check_contract, fixture_quats, random_cloud, random_legs, unit

pytestmark = pytest.mark.gpu


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


def cases(lrm):
    qs = [unit(q) for q in fixture_quats()]
    out = [(lrm.get_M2_leg(0.4), qs[0]), (lrm.get_moonbot_leg(-1.3), qs[1]), (lrm.get_M2_leg(2.0), qs[4]),
           (lrm.get_moonbot_leg(0.0), fixture_quats()[1])]  # the last one keeps the fixture's non-unit quaternion
    return out + [(leg, q) for _, leg, q in random_legs(lrm)[::3]]


def test_device_equals_cpu(lrm, torch_cuda):
    torch = torch_cuda
    n = 1_000_003  # ragged
    pts = random_cloud(n, seed=11)
    pts[::99_991] = np.nan
    rng = np.random.default_rng(2)
    for k, (leg, q) in enumerate(cases(lrm)):
        x, y, z = soa(torch, pts)
        seed = None
        if k % 2:
            seed = (rng.random((n, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
            seed[::7, 0] = np.nan  # non-finite and far seeds: no seed / the best-residual candidate
            seed[3::11] = np.inf
            seed[5::13, 2] = -np.inf
            seed[6::17] = 1e20
        sd = None if seed is None else soa(torch, seed)
        ang, st = lrm.device.ik(x, y, z, leg, q, seed=sd)
        xyz = lrm.device.fk(ang[0], ang[1], ang[2], leg, q)
        torch.cuda.synchronize()
        want_a, want_s, _ = lrm.apply_ik_cpu(pts, leg, q, seed=seed)
        want_p, _ = lrm.apply_fk_cpu(want_a, leg, q)
        assert np.array_equal(st.cpu().numpy(), want_s)
        assert bits_equal(ang.cpu().numpy().T, want_a).all()
        assert bits_equal(xyz.cpu().numpy().T, want_p).all()


def test_unaligned_views_and_caller_outputs(lrm, torch_cuda):
    torch = torch_cuda
    n = 77_777
    pts = random_cloud(n + 3, seed=5)
    leg, q = lrm.get_moonbot_leg(0.9), unit(fixture_quats()[2])
    big = dev(torch, pts.T.copy())
    x, y, z = big[0, 1:n + 1], big[1, 2:n + 2], big[2, 3:n + 3]  # 4-byte offsets
    out = torch.full((3, n + 5), 7.0, dtype=torch.float32, device="cuda")[:, 1:]  # rows of a wider buffer, offset
    status = torch.full((n + 1,), 9, dtype=torch.uint8, device="cuda")[1:]
    ang, st = lrm.device.ik(x, y, z, leg, q, out=out, status=status)
    torch.cuda.synchronize()
    host = np.stack([pts[1:n + 1, 0], pts[2:n + 2, 1], pts[3:n + 3, 2]], 1)
    want_a, want_s, _ = lrm.apply_ik_cpu(host, leg, q)
    assert np.array_equal(st.cpu().numpy(), want_s)
    assert bits_equal(ang[:, :n].cpu().numpy().T, want_a).all()
    assert (ang[:, n:].cpu().numpy() == 7.0).all()  # nothing written past n


def test_config2_cloud_contract(lrm, oracle, torch_cuda):
    """1e7 config-2 points: status in {1, 3} equals strict lrm_reach_dev's mask; items 2-5 on a fixed 2^20 sample"""
    torch = torch_cuda
    n = 10_000_000
    pts = random_cloud(n, seed=42)
    leg = lrm.get_M2_leg(0.0)
    x, y, z = soa(torch, pts)
    ang, st = lrm.device.ik(x, y, z, leg)
    prev = lrm.get_mode()
    lrm.set_mode(lrm.MODE_STRICT)
    try:
        mask = lrm.device.reach(x, y, z, leg)
    finally:
        lrm.set_mode(prev)
    torch.cuda.synchronize()
    s = st.cpu().numpy()
    assert np.array_equal(np.isin(s, (1, 3)), mask.cpu().numpy().astype(bool))
    sel = np.sort(np.random.default_rng(0).choice(n, 1 << 20, replace=False))
    a = ang.cpu().numpy().T[sel]
    check_contract(oracle, pts[sel], leg, (1, 0, 0, 0), a, s[sel])


def test_graph_capture_and_replay(lrm, oracle, torch_cuda):
    """lrm_ik_dev and lrm_fk_dev only launch: captured in one graph on a single stream (no parallel branches), replayed
    after new points were copied into the captured input"""
    torch = torch_cuda
    n = 300_000
    p0, p1 = random_cloud(n, seed=1), random_cloud(n, seed=2)
    leg, q = lrm.get_M2_leg(0.5), unit(fixture_quats()[3])
    inp = dev(torch, p0.T.copy())
    ang = torch.empty((3, n), dtype=torch.float32, device="cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    xyz = torch.empty((3, n), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture
        lrm.device.ik(inp[0], inp[1], inp[2], leg, q, out=ang, status=st)
        lrm.device.fk(ang[0], ang[1], ang[2], leg, q, out=xyz)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            lrm.device.ik(inp[0], inp[1], inp[2], leg, q, out=ang, status=st)
            lrm.device.fk(ang[0], ang[1], ang[2], leg, q, out=xyz)
        inp.copy_(dev(torch, p1.T.copy()))
        ang.zero_()
        st.zero_()
        xyz.zero_()
        g.replay()
    torch.cuda.synchronize()
    want_a, want_s, _ = lrm.apply_ik_cpu(p1, leg, q)
    want_p, _ = lrm.apply_fk_cpu(want_a, leg, q)
    assert np.array_equal(st.cpu().numpy(), want_s)
    assert bits_equal(ang.cpu().numpy().T, want_a).all()
    assert bits_equal(xyz.cpu().numpy().T, want_p).all()
    check_contract(oracle, p1, leg, q, want_a, want_s)
    del g
