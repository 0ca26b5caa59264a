"""Leg and self clearance on the device (run with -m gpu on an MI355X) straight against tests/leg_model64.py, the float64 model
written from the leg's geometry -- not through the host loop: PoseSet.leg_joints against joints64, PoseSet.leg_clearance and
PoseSet.self_clearance against the model's rows wherever no decision lies inside the band, and lrm_dbg_link_pair_dist_dev
against the true segment-segment distance.  The bands are leg_model64's constants, measured on the host by
tests/test_clearance_float64_cpu.py (the device equals the host loop bit for bit: tests/test_gpu_leg_clearance.py,
tests/test_gpu_self_clearance.py); nothing is measured here.  The caps on what doubt may hide (2 % of the rows) are counted from
the model alone.  A box cull that dropped a near target would show as fewer hits than float64's on a row that is not in doubt.
Shapes: the smallest that still take each path (one wave, one workgroup of four waves and a ragged second one, clouds without
and with boxes, the sparse_tiles scene where the chunk cull decides, one to four rounds of 64 pair codes)."""
import os
import re

import numpy as np
import pytest

import footholds_posed_cases as fc
import ik_cases
import leg_clearance_cases as lc
import leg_model64 as m64
import pair_cases as pc
import posed_cases
import self_clearance_cases as sc

pytestmark = pytest.mark.gpu

F = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged-robot-movability-cuda_amd", "csrc")


def test_the_shapes_are_the_kernels():
    leg = open(os.path.join(CSRC, "lrm_leg_clearance.hip")).read()
    own = open(os.path.join(CSRC, "lrm_self_clearance.hip")).read()
    capi = open(os.path.join(CSRC, "lrm_capi.cpp")).read()
    for src in (leg, own):  # four waves a workgroup, a wave per pose or set: 65 is a full workgroup and a ragged second one
        assert int(re.search(r"constexpr int kBlock = (\d+);", src).group(1)) == 256
    assert int(re.search(r"constexpr int kTargetTile = (\d+);", leg).group(1)) == 1024  # 9216 targets: nine tiles
    assert int(re.search(r"return nt >= (\d+) \? tile_boxes", capi).group(1)) == 4096  # 1000: no boxes, 4097: boxes
    assert int(re.search(r"constexpr int kRound = (\d+);", own).group(1)) == 64
    assert [-(-n * (n - 1) // 2 * 9 // 64) for n in (2, 6, 8)] == [1, 3, 4]  # pair rounds of 2, 6 and 8 legs


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def soa(torch, pts):
    t = dev(torch, np.asarray(pts, F).reshape(-1, 3).T)
    return t[0], t[1], t[2]


def unit_scene(lrm, nposes, nt, seed, kind="rough"):
    """leg_clearance_cases.scene with one unit quaternion of the reference's sweep per pose (the model's domain)"""
    _, body, targets = lc.scene(lrm, nposes, nt, seed, kind)
    return unit(fc.sweep_pose_quats(lrm, nposes, seed)), body, targets


def unit(quats):
    assert all(ik_cases.is_unit(q) for q in quats)
    return quats


def cap_rows(name, doubt_rows, rows):
    """at most 2 % of the live valid rows may be in doubt, counted from the model alone"""
    print(f"{name}: {doubt_rows} of {rows} live valid rows in doubt (cap 2 %)")
    assert rows > 0 and doubt_rows <= 0.02 * rows, (name, doubt_rows, rows)


def leg_rows_on_the_device(lrm, torch, quats, body, targets, legs, ang, margin, name):
    model = m64.leg_clearance64(targets, body, m64.joints64_posed(ang, legs, quats, lc.TIP_CLEAR), lc.RADIUS, margin)
    v = model["valid"]
    sure = v & ~m64.leg_doubt(model, m64.BAND_D).any((2, 3))
    cap_rows(name, int((v & ~sure).sum()), int(v.sum()))
    ps = lrm.PoseSet(legs, len(quats), ik=True).update(dev(torch, quats), dev(torch, body))
    tx, ty, tz = soa(torch, targets)
    out = ps.leg_clearance(tx, ty, tz, dev(torch, np.asarray(ang, F).T), lc.RADIUS, margin, lc.TIP_CLEAR)
    torch.cuda.synchronize()
    got = dict(zip(("hits", "links", "worst", "pen", "free"), (t.cpu().numpy() for t in out)))
    assert not (got["hits"][sure] < model["hits"][sure]).any(), "a near target was dropped"
    compared, _ = m64.check_leg_rows(got, model, m64.BAND_D)
    assert compared > 0
    return model


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_leg_joints_against_the_float64_model(lrm, torch_cuda, n):
    """one leg: n (pose, leg) entries, one per lane"""
    torch = torch_cuda
    legs = sc.legs_n(lrm, 6)[2:3]
    quats = unit(posed_cases.random_unit_quats(n, np.random.default_rng(n)))
    body = np.random.default_rng(n + 1).uniform(-1500.0, 1500.0, (n, 3)).astype(F)
    ang = lc.random_angles(n, 1, seed=n)
    ps = lrm.PoseSet(legs, n, ik=True).update(dev(torch, quats), dev(torch, body))
    for tip_clear in (0.0, 30.0, 1e4):
        out = torch.full((1, n, 4, 3), -7.0, dtype=torch.float32, device="cuda")
        ps.leg_joints(dev(torch, ang.T), tip_clear, out)
        torch.cuda.synchronize()
        want = m64.joints64_posed(ang, legs, quats, tip_clear) + body.astype(np.float64)[None, :, None, :]
        err = np.abs(out.cpu().numpy().astype(np.float64) - want).max((0, 1, 3))
        assert (err <= m64.BAND_J).all(), (tip_clear, err)


@pytest.mark.parametrize("margin", [0.0, 10.0])
@pytest.mark.parametrize("kind,nt", [("rough", 1000), ("rough", 4097), ("sparse_tiles", 9 * 1024)])
@pytest.mark.parametrize("nposes", [5, 65])
def test_leg_clearance_against_the_float64_model(lrm, torch_cuda, nposes, kind, nt, margin):
    quats, body, targets = unit_scene(lrm, nposes, nt, seed=3, kind=kind)
    model = leg_rows_on_the_device(lrm, torch_cuda, quats, body, targets, sc.legs_n(lrm, 6), lc.random_angles(nposes, 6, seed=nposes),
                                   margin, f"{kind}-{nt}, {nposes} poses, margin {margin:g}")
    assert (model["hits"] > 0).any() and (model["worst"] < 0).any()


def test_leg_clearance_far_from_the_origin(lrm, torch_cuda):
    """cloud and bodies 4e6 mm out, where float32 steps by 0.25 to 0.5 mm: q = t - body is still exact input of the model"""
    quats, body, targets = unit_scene(lrm, 65, 4097, seed=9)
    body, targets = pc.translated(body, targets, 4e6)
    model = leg_rows_on_the_device(lrm, torch_cuda, quats, body, targets, sc.legs_n(lrm, 6), lc.random_angles(65, 6, seed=9), lc.MARGIN,
                                   "4e6 mm from the origin")
    assert (model["hits"] > 0).sum() > 10


@pytest.mark.parametrize("nlegs", [2, 6, 8])
@pytest.mark.parametrize("ns", [1, 65, 257])
def test_self_clearance_against_the_float64_model(lrm, torch_cuda, ns, nlegs):
    """24 unit poses repeated through pose_idx, angles from no IK, a thick coxa link: every kind of link in a hit"""
    torch = torch_cuda
    legs = sc.legs_n(lrm, nlegs)
    quats = unit(posed_cases.random_unit_quats(24, np.random.default_rng(ns)))
    pi = np.random.default_rng(ns + nlegs).integers(0, 24, ns).astype(np.int32)
    ang = lc.random_angles(ns, nlegs, seed=ns + nlegs)
    model = m64.self_clearance64(m64.joints64_posed(ang, legs, quats, sc.TIP_CLEAR, pose_of=pi), sc.RADIUS_COXA, sc.MARGIN)
    cap_rows(f"{ns} sets of {nlegs} legs", int((model["valid"] & m64.self_doubt(model, m64.BAND_SELF)).sum()), int(model["valid"].sum()))
    ps = lrm.PoseSet(legs, 24, ik=True).update(dev(torch, quats))
    out = ps.self_clearance(dev(torch, ang.T), sc.RADIUS_COXA, sc.MARGIN, sc.TIP_CLEAR, dev(torch, pi))
    torch.cuda.synchronize()
    got = dict(zip(sc.KEYS, (t.cpu().numpy() for t in out)))
    compared, _ = m64.check_self_rows(got, model, m64.BAND_SELF)
    assert compared > 0
    if ns > 1:
        assert (model["hits"] > 0).any()


@pytest.mark.parametrize("n", [1, 64, 65, 8193])
def test_pair_distance_on_the_device_against_the_true_minimum(lrm, torch_cuda, n):
    """n pairs drawn evenly from every kind of self_clearance_cases.all_pairs(): never below the true minimum by more than
    BAND_PAIR_LOW, above it by at most the kind's band"""
    torch = torch_cuda
    kinds = sc.hand_made_pairs()
    kinds["random"] = sc.random_pairs(n=12000)
    segs = np.concatenate(list(kinds.values()))
    band = np.concatenate([np.full(len(g), m64.BAND_KIND[k]) for k, g in kinds.items()])
    pick = np.random.default_rng(n).permutation(len(segs))[:n]
    segs, band = np.ascontiguousarray(segs[pick]), band[pick]
    d = lrm.device.dbg_link_pair_dist(dev(torch, segs))
    torch.cuda.synchronize()
    d = d.cpu().numpy().astype(np.float64)
    d64 = m64.link_link_dist64(segs[:, 0:3], segs[:, 3:6], segs[:, 6:9], segs[:, 9:12])
    assert d.shape == (n,) and (d >= d64 - m64.BAND_PAIR_LOW).all(), float((d64 - d).max())
    assert (d <= d64 + band).all(), float((d - d64 - band).max())
