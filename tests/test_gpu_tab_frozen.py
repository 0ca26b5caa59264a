"""The table kernels after the cut of their per-point instruction count (run with -m gpu): on the seeded config-2 cloud at 1e6
points and at the 2e5 dispatch threshold, in LRM_MODE_TOL and LRM_MODE_TOL_REL, the device mask and ballot words are the
oracle's bit for bit, the field meets the mode's contract exactly as tests/test_gpu_tol.py states it, and the doubt count
(dbg_tol_queue_counts) stays inside the bounds tests/test_gpu_tol.py sets for such clouds, with no overflowed segment (that the
doubt SET did not move is shown on the host, bit for bit, by tests/test_tab_point_frozen_cpu.py: one source for host and device).  One more case lies beyond the inner grid, so that the instance of
the look-up for waves with outer-grid lanes runs.  No timing here."""
import numpy as np
import pytest

from conftest import bits_equal, random_cloud
from tolcheck import TOL, field_error

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the gpu tests need a GPU"
    return torch


def packed(mask):
    n = len(mask)
    return np.packbits(np.pad(mask, (0, (-n) % 64)), bitorder="little").view(np.uint64)


def run(lrm, torch, pts, leg, mode):
    n = len(pts)
    x, y, z = (torch.from_numpy(np.ascontiguousarray(pts[:, k])).cuda() for k in range(3))
    lrm.set_mode(lrm.MODE_TOL if mode == "tol" else lrm.MODE_TOL_REL)
    try:
        bits = torch.empty((n + 63) // 64, dtype=torch.int64, device="cuda")
        m, d, bits = lrm.device.reach_dist(x, y, z, leg, None, mask=torch.empty(n, dtype=torch.uint8, device="cuda"), bits=bits)
        torch.cuda.synchronize()
        counts = lrm.dbg_tol_queue_counts()
    finally:
        lrm.set_mode(lrm.MODE_FAST)
    return m.cpu().numpy(), d.cpu().numpy().T, bits.cpu().numpy(), counts


def check(lrm, oracle, pts, leg, mode, max_queued, m, d, bits, counts):
    n = len(pts)
    want_m = oracle.reach(pts, leg)
    want_d, _ = oracle.dist(pts, leg)
    assert np.array_equal(m, want_m), "reach mask must be bit-exact"
    assert np.array_equal(bits.view(np.uint64), packed(want_m))
    if mode == "tol":
        e = field_error(pts, d, want_d, leg)
        assert e["metric"].max(initial=0.0) <= TOL
    else:
        err = np.linalg.norm(d.astype(np.float64) - want_d.astype(np.float64), axis=1)
        nref = np.linalg.norm(want_d.astype(np.float64), axis=1)
        assert (err <= TOL * nref).all(), float((err / np.maximum(nref, 1e-300)).max())
        assert bits_equal(d[nref < 16.0], want_d[nref < 16.0]).all()
    _, _, doubt, _ = lrm.dbg_toltab_host(pts, leg)
    npts, nq, nover = counts
    # reported, not asserted: the host build of the same source rounds 1 / sqrt differently from v_rsq_f32, so a point on the edge
    # of a band may fall on either side
    print(f"{mode}, {n} points: {nq} queued, host evaluation: {int(((doubt & 0xffff) != 0).sum())} in doubt")
    assert npts == n and nover == 0 and 0 < nq < max_queued * n, (npts, nq, nover)  # the bounds of tests/test_gpu_tol.py


@pytest.mark.parametrize("mode", ["tol", "tol_rel"])
@pytest.mark.parametrize("n", [1_000_000, 200_000])
def test_table_kernel_on_the_config2_cloud(lrm, oracle, torch_cuda, n, mode):
    pts = random_cloud(n, seed=42)
    leg = lrm.get_M2_leg(0.0)
    check(lrm, oracle, pts, leg, mode, 0.03, *run(lrm, torch_cuda, pts, leg, mode))


@pytest.mark.parametrize("mode", ["tol", "tol_rel"])
def test_table_kernel_beyond_the_inner_grid(lrm, oracle, torch_cuda, mode):
    """every wave holds lanes beyond +-1024 mm of the femur joint: lrm_toltab_lookup2<true>"""
    pts = random_cloud(400_000, seed=42)
    pts[:, 0] += np.float32(900.0)
    pts[::7, 1] *= np.float32(6.0)
    leg = lrm.get_M2_leg(0.0)
    check(lrm, oracle, pts, leg, mode, 0.05, *run(lrm, torch_cuda, pts, leg, mode))
