"""The exact value chain of the table-guided evaluation on the host, whole points: lrm_xtab_point (LRM_MODE_FAST) and the
tolerance evaluation + lrm_xtab_replay (LRM_MODE_TOL_REL's short vectors), against the strict host code (lrm_dist_cpu /
lrm_reach_cpu = lrm_dist_global / lrm_reach_global), BIT FOR BIT on every point the evaluation does not put in doubt:

  * the config-2 cloud, 2e6 points, seed 42;
  * a planar grid through the workspace (the reference's bench plane, y = 0);
  * a cloud of invalid points inside the yaw range in front of the coxa: every one of them has a twin candidate
    (tests/xtab_clouds.py), picked by strict norms;
  * the interleaved cloud of the GPU test (tests/test_gpu_xtab_value_chain.py), whose classes are checked here to be what
    they are named: the twins run the second chain, the alternative is taken where the yaw-limit plane is nearer.

What the chain shares between its branches (one second sincosf for the alternative and the twin, the pick of two norms from their
sums) must not show in any bit."""
import numpy as np
import pytest

import xtab_clouds as XC
from conftest import bits_equal, random_cloud


@pytest.fixture(scope="module")
def leg(lrm):
    return lrm.get_M2_leg(0.0)


def strict(lrm, pts, leg):
    d, v, _ = lrm.apply_dist_cpu(pts, leg)
    m, _ = lrm.apply_reach_cpu(pts, leg)
    return m, v, d


def check_both(lrm, pts, leg, max_doubt):
    """lrm_xtab_point and the replay against the strict code -> (doubt fraction of the first, its statistics)"""
    want_m, want_v, want_d = strict(lrm, pts, leg)
    m, d, doubt, stats = lrm.dbg_xtab_host(pts, leg)
    sure = (doubt & 0xffff) == 0
    assert np.array_equal(m[sure], want_m[sure]) and np.array_equal(m[sure], want_v[sure])
    bad = np.flatnonzero(~bits_equal(d[sure], want_d[sure]).all(axis=1))
    assert len(bad) == 0, f"lrm_xtab_point: {len(bad)} vectors differ; first: point {pts[sure][bad[0]]}, got {d[sure][bad[0]]}, want {want_d[sure][bad[0]]}"
    assert 1.0 - sure.mean() <= max_doubt, f"{1.0 - sure.mean():.4f} of the points are in doubt"
    mr, dr, doubt_r = lrm.dbg_replay_host(pts, leg)
    sure_r = (doubt_r & 0xffff) == 0
    assert np.array_equal(mr[sure_r], want_m[sure_r])
    bad = np.flatnonzero(~bits_equal(dr[sure_r], want_d[sure_r]).all(axis=1))
    assert len(bad) == 0, f"lrm_xtab_replay: {len(bad)} vectors differ; first: point {pts[sure_r][bad[0]]}, got {dr[sure_r][bad[0]]}, want {want_d[sure_r][bad[0]]}"
    assert 1.0 - sure_r.mean() <= max_doubt
    return 1.0 - sure.mean(), stats


def test_config2_cloud_of_2e6_points(lrm, leg):
    check_both(lrm, random_cloud(2_000_000, seed=42), leg, 0.02)


def test_planar_grid_through_the_workspace(lrm, leg):
    x, z = np.meshgrid(np.arange(-100.0, 601.0, 1.0), np.arange(-100.0, 51.0, 1.0))
    pts = np.stack([x.ravel(), np.zeros(x.size), z.ravel()], axis=1).astype(np.float32)
    check_both(lrm, pts, leg, 0.09)  # the plane y = 0 is the symmetry plane of the leg: more doubt than a cloud


def test_invalid_points_in_front_of_the_coxa_all_have_a_twin(lrm, leg):
    pts = XC.class_points(lrm, leg, "twin", 200_000, seed=3)
    m, v, _ = strict(lrm, pts, leg)
    assert not m.any() and not v.any(), "the twin cloud must be invalid everywhere"
    _, stats = check_both(lrm, pts, leg, 0.05)
    # (yaw -+ pi) +- pi is the yaw itself for one yaw in six: those have no twin
    assert stats["second_chains"] >= 0.8 * len(pts), stats


def test_interleaved_cloud_holds_its_classes_in_every_wave(lrm, leg):
    pts, which = XC.interleaved(lrm, leg, 65_537)
    for w in range(0, len(pts) - 63, 64):
        assert set(which[w:w + 64].tolist()) == set(range(len(XC.CLASSES)))
    # the `near` lanes (one in eight) are a tie of the yaw-limit alternative: the tolerance evaluation in front of the replay puts
    # them in doubt by design (the fix-up's filtered code takes them), lrm_xtab_point decides them with its strict norms
    check_both(lrm, pts, leg, 0.20)
    _, _, want_d = strict(lrm, pts, leg)
    n = np.linalg.norm(want_d.astype(np.float64), axis=1)
    # the in-plane boundary distance D of an alt / near point: that of its meridian point at yaw 0
    for name, factor in (("alt", 0.5), ("near", 1.0)):
        idx = np.flatnonzero(which == XC.CLASSES.index(name))
        _, _, D, _ = XC.meridian_samples(lrm, leg, len(idx), 42 + XC.CLASSES.index(name))
        assert np.mean(np.abs(n[idx] - factor * D) <= 1e-3 * D) > 0.95, name
    twin = pts[which == XC.CLASSES.index("twin")]
    assert lrm.dbg_xtab_host(twin, leg)[3]["second_chains"] >= 0.8 * len(twin)
    clamped = which == XC.CLASSES.index("clamped")
    assert not strict(lrm, pts[clamped], leg)[0].any()  # beyond the yaw limit: unreachable
