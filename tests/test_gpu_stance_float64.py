"""Stance stability on the device (run with -m gpu on an MI355X) straight against tests/stance_model64.py, the float64 model
written from geometry -- not through the host loop: device.stance_stability's margin, stable, feet and winning edge code against
stance_model64.check_stance_rows.  The bands are stance_model64.BAND, measured on the host by tests/test_stance_float64_cpu.py
(the device equals the host loop bit for bit: tests/test_gpu_stance.py); nothing is measured here.  The caps on what doubt may
hide (2 % of a scene's answers) are counted from the model alone.
Shapes: the smallest that still take each path of stance_stability_kernel -- one wave, a full workgroup of four waves and a
ragged second one, 257 stances; 1 and 7 lift sets, 64 (one round of the second phase), 65 (a second round with one live lane)
and 256; 3, 6 and 8 legs -- and 65 541 stances, past the grid cap, for the properties that need no model."""
import os
import re

import numpy as np
import pytest

import stance_cases as sc
import stance_model64 as sm

pytestmark = pytest.mark.gpu

F = np.float32
COM = [30.0, 10.0, -5.0]
TILTED = sm.gravity_basis([0.0, np.sin(np.deg2rad(20.0)), -np.cos(np.deg2rad(20.0))])
WAVES, ROUND, GRID_STANCES = 4, 64, 65536


def test_the_shapes_are_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged-robot-movability-cuda_amd", "csrc",
                            "lrm_stance.hip")).read()
    assert int(re.search(r"constexpr int kBlock = (\d+);", src).group(1)) == 64 * WAVES  # 65 stances: a full workgroup and one more wave
    assert int(re.search(r"m0 < P\.nmasks; m0 \+= (\d+)\)", src).group(1)) == ROUND  # 65 lift sets: a second round, one live lane
    assert int(re.search(r"constexpr unsigned kMaxGrid = (\d+);", src).group(1)) * WAVES == GRID_STANCES  # 65 541: a second stance per wave


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def run(lrm, torch, targets, foot, quats, body=None, pose_idx=None, com=None, plane=None, lift=None, min_margin=0.0, live_in=None):
    """device.stance_stability into sentinel-filled outputs -> dict of numpy margin, edge, stable, feet"""
    dev = lambda a, t: None if a is None else torch.from_numpy(np.ascontiguousarray(a, t)).cuda()
    nl, ns = foot.shape
    nm = len(lrm.stance_lift(lift, nl))
    t = dev(np.asarray(targets, F).reshape(-1, 3).T, F)
    m = torch.full((nm, ns), -7.0, dtype=torch.float32, device="cuda")
    e, st = (torch.full((nm, ns), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2))
    ft = torch.full((ns,), 0xA5, dtype=torch.uint8, device="cuda")
    lrm.device.stance_stability(t[0], t[1], t[2], dev(foot, np.int32), dev(quats, F), dev(body, F), dev(pose_idx, np.int32), com, plane, lift,
                                min_margin, dev(live_in, np.uint8), m, e, st, ft)
    torch.cuda.synchronize()
    return {"margin": m.cpu().numpy(), "edge": e.cpu().numpy(), "stable": st.cpu().numpy(), "feet": ft.cpu().numpy()}


def against_the_model(lrm, torch, kind, targets, foot, quats, body=None, pose_idx=None, com=None, plane=None, lift=None, min_margin=0.0,
                      live_in=None):
    lift = lrm.stance_lift(lift, len(foot))
    model = sm.stance64(targets, foot, quats, body, pose_idx, com, plane, lift, live_in)
    band = sm.BAND[kind]
    assert (model["size"] < sm.WITHIN).all()
    total, in_doubt = int(np.isfinite(model["margin64"]).sum()), int(sm.doubt(model, band, min_margin).sum())
    assert in_doubt <= 0.02 * max(total, 1), (in_doubt, total)
    got = run(lrm, torch, targets, foot, quats, body, pose_idx, com, plane, lift, min_margin, live_in)
    compared, skipped = sm.check_stance_rows(got, model, band, min_margin)
    assert skipped == in_doubt
    return model, compared


def lift_sets(nm, nlegs, seed):
    """nm lift sets of nlegs legs: nothing lifted first, then the subsets in a shuffled order, repeated where nm exceeds them"""
    lift = np.resize(np.random.default_rng(seed).permutation(1 << nlegs), nm).astype(np.uint8)
    lift[0] = 0
    return lift


@pytest.mark.parametrize("plane", ["none", "tilted"])
@pytest.mark.parametrize("ns,nm,nlegs", [(1, 1, 3), (1, 7, 6), (65, 64, 6), (65, 65, 8), (65, 256, 8), (257, 7, 3), (257, 64, 6), (257, 1, 8),
                                         (257, 65, 3)])
def test_shapes_against_the_float64_model(lrm, torch_cuda, ns, nm, nlegs, plane):
    targets, foot, quats, body = sc.synthetic(ns, nlegs, seed=ns + nm, missing=0.0 if ns == 1 else 0.1)
    model, compared = against_the_model(lrm, torch_cuda, "synthetic", targets, foot, quats, body, com=COM, plane=None if plane == "none" else TILTED,
                                        lift=lift_sets(nm, nlegs, ns + nlegs), min_margin=0.0 if nm % 2 else 25.0)
    assert compared > 0
    if ns > 1 and nm > 1:
        assert (model["margin64"] > 0).any() and np.isneginf(model["margin64"]).any()


def test_dead_entries_and_live_in_at_the_ends_of_a_wave(lrm, torch_cuda):
    ns = 65
    targets, foot, quats, body = sc.synthetic(ns, 6, seed=50)
    at = [0, 31, 32, 63]
    pi = np.random.default_rng(5).permutation(ns).astype(np.int32)
    pi[at] = [-1, ns, np.iinfo(np.int32).min, ns + 7]
    model, _ = against_the_model(lrm, torch_cuda, "synthetic", targets, foot, quats, body, pi, com=COM, lift="each")
    assert model["dead"][at].all() and model["dead"].sum() == 4
    live = np.ones(ns, np.uint8)
    live[at], live[5] = 0, 3
    model, _ = against_the_model(lrm, torch_cuda, "synthetic", targets, foot, quats, body, com=COM, plane=TILTED, lift="each", live_in=live)
    assert np.array_equal(model["dead"], live == 0)


def test_bodies_far_from_the_origin(lrm, torch_cuda):
    targets, foot, quats, body = sc.synthetic(65, 6, seed=9, offset=4e6)
    model, _ = against_the_model(lrm, torch_cuda, "far", targets, foot, quats, body, com=COM, lift=sc.lift_all(6))
    assert (model["margin64"] > 0).sum() > 40


@pytest.mark.parametrize("plane", ["none", "tilted"])
def test_near_collinear_family(lrm, torch_cuda, plane):
    """257 stances with two to five feet on one line up to rounding and c close to that side: a dropped side of the hull would show
    as a margin above margin64 + band"""
    targets, foot, quats, body, info = sm.collinear_family(257, seed=4)
    lift = np.concatenate([sc.lift_each(8), [0b00000011, 0b00010100, 0b10100000, 0b01001001]]).astype(np.uint8)
    model, compared = against_the_model(lrm, torch_cuda, "collinear", targets, foot, quats, body, com=sm.COLLINEAR_COM,
                                        plane=None if plane == "none" else TILTED, lift=lift)
    m0 = model["margin64"][0]
    assert (m0 > 0).sum() > 60 and (m0 < 0).sum() > 60 and compared > 2000
    assert set(np.unique(info["side_feet"])) >= {2, 3, 4, 5}


def test_properties_past_the_grid_cap(lrm, torch_cuda):
    """65 541 stances (a workgroup and one more past the grid's cap) under all 64 lift sets: the four properties of the library
    alone (stance_model64.check_properties), which need no model"""
    ns = GRID_STANCES + WAVES + 1
    targets, foot, quats, body = sc.synthetic(ns, 6, seed=3)
    n = sm.check_properties(lambda f, plane, lift: run(lrm, torch_cuda, targets, f, quats, body, com=COM, plane=plane, lift=lift), targets, foot, body,
                            sm.BAND["synthetic"], TILTED, sm.gravity_basis([0.0, np.sin(np.deg2rad(20.0)), -np.cos(np.deg2rad(20.0))], yaw=1.1))
    assert n > 20000
