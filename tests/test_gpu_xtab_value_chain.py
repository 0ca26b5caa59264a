"""The exact value chain on the device, whole points: LRM_MODE_FAST (dist_xtab_kernel + fix-up) and LRM_MODE_TOL_REL (table
kernel with the replay tail + fix-up) against LRM_MODE_STRICT, on clouds of 4 097 and 65 537 points in which EVERY wave holds
twin lanes, lanes whose yaw-limit alternative is taken, lanes where it is a near tie, and lanes clamped to a yaw limit
(tests/xtab_clouds.py; tests/test_xtab_value_chain_cpu.py checks on the host that the classes are what they are named).

  LRM_MODE_FAST     every output bit equals LRM_MODE_STRICT: mask, bit words, all three floats of every vector.
  LRM_MODE_TOL_REL  mask and bit words equal; every vector shorter than 0.9 * LRM_TOL_REL_MM comes from the bit-exact code
                    (the replay tail or the fix-up) and equals bit for bit; the longer ones keep the mode's contract
                    |d - d_ref| <= 1e-5 |d_ref|.
  LRM_TOL_SELFTEST=1 (every point through the fix-up), 4 097 points: both modes equal LRM_MODE_STRICT bit for bit.

LRM_TOL_TABLE=2 makes the table kernels run at these sizes (they are the default from 2e5 points on)."""
import numpy as np
import pytest

import xtab_clouds as XC
from conftest import bits_equal

pytestmark = pytest.mark.gpu
TOL_REL_MM = 19.0  # csrc/lrm_launch.h


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def clouds(lrm):
    """{n: (points, x, y, z device arrays are made per test)}: built once, read-only"""
    leg = lrm.get_M2_leg(0.0)
    out = {}
    for n in (4_097, 65_537):
        pts, _ = XC.interleaved(lrm, leg, n)
        pts.setflags(write=False)
        out[n] = pts
    return leg, out


def run(lrm, torch, pts, leg, mode):
    n = len(pts)
    x, y, z = (torch.from_numpy(np.ascontiguousarray(pts[:, k])).cuda() for k in range(3))
    lrm.set_mode(mode)
    try:
        bits = torch.empty((n + 63) // 64, dtype=torch.int64, device="cuda")
        m, d, bits = lrm.device.reach_dist(x, y, z, leg, None, mask=torch.empty(n, dtype=torch.uint8, device="cuda"), bits=bits)
        torch.cuda.synchronize()
    finally:
        lrm.set_mode(lrm.MODE_FAST)
    return m.cpu().numpy(), d.cpu().numpy().T.copy(), bits.cpu().numpy()


@pytest.fixture(scope="module")
def strict_results(lrm, torch_cuda, clouds):
    leg, by_n = clouds
    return {n: run(lrm, torch_cuda, pts, leg, lrm.MODE_STRICT) for n, pts in by_n.items()}


def same_bits(got, want, what):
    bad = np.flatnonzero(~bits_equal(got, want).all(axis=1))
    assert len(bad) == 0, f"{what}: {len(bad)} vectors differ; first: index {bad[0]}, got {got[bad[0]]}, want {want[bad[0]]}"


@pytest.mark.parametrize("n", [4_097, 65_537])
def test_fast_equals_strict_bit_for_bit(lrm, torch_cuda, clouds, strict_results, n, monkeypatch):
    leg, by_n = clouds
    monkeypatch.setenv("LRM_TOL_TABLE", "2")
    monkeypatch.delenv("LRM_TOL_SELFTEST", raising=False)
    m0, d0, b0 = strict_results[n]
    m, d, b = run(lrm, torch_cuda, by_n[n], leg, lrm.MODE_FAST)
    assert np.array_equal(m, m0) and np.array_equal(b, b0)
    same_bits(d, d0, "LRM_MODE_FAST")


@pytest.mark.parametrize("n", [4_097, 65_537])
def test_tol_rel_short_vectors_equal_strict_bit_for_bit(lrm, torch_cuda, clouds, strict_results, n, monkeypatch):
    leg, by_n = clouds
    monkeypatch.setenv("LRM_TOL_TABLE", "2")
    monkeypatch.delenv("LRM_TOL_SELFTEST", raising=False)
    m0, d0, b0 = strict_results[n]
    m, d, b = run(lrm, torch_cuda, by_n[n], leg, lrm.MODE_TOL_REL)
    assert np.array_equal(m, m0) and np.array_equal(b, b0)
    nref = np.linalg.norm(d0.astype(np.float64), axis=1)
    short = nref < 0.9 * TOL_REL_MM
    assert short.mean() > 0.4, "the cloud is built to hold short vectors in every wave"
    same_bits(d[short], d0[short], "LRM_MODE_TOL_REL, short vectors")
    err = np.linalg.norm(d.astype(np.float64) - d0, axis=1)
    assert (err <= 1e-5 * nref).all(), f"{float((err[nref > 0] / nref[nref > 0]).max()):.3e}"


@pytest.mark.parametrize("mode", ["fast", "tol_rel"])
def test_every_point_through_the_fixup_equals_strict(lrm, torch_cuda, clouds, strict_results, mode, monkeypatch):
    leg, by_n = clouds
    monkeypatch.setenv("LRM_TOL_TABLE", "2")
    monkeypatch.setenv("LRM_TOL_SELFTEST", "1")
    m0, d0, b0 = strict_results[4_097]
    m, d, b = run(lrm, torch_cuda, by_n[4_097], leg, lrm.MODE_FAST if mode == "fast" else lrm.MODE_TOL_REL)
    assert np.array_equal(m, m0) and np.array_equal(b, b0)
    same_bits(d, d0, f"{mode}, LRM_TOL_SELFTEST=1")
