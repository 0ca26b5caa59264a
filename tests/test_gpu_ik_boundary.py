"""Joint angles ON the joint-limit faces, on the device (lrm_ik_dev, lrm_fk_dev, lrm_ik_posed_dev, lrm_fk_posed_dev): the
boundary clouds of tests/ik_boundary_cases.py, ordered so that one wave holds faces, extension, axis and far points side
by side (the re-solve branches of lrm_ik_knee diverge there), against the float64 limit model directly and against the
host loops bit for bit."""
import numpy as np
import pytest

from conftest import bits_equal
from ik_boundary_cases import (FAR, Case, assert_contract_by_class, assert_fk, assert_gaps_are_real, case_by_name,
                               seed_plan)
from ik_cases import unit
from posed_cases import fixture_quats

pytestmark = pytest.mark.gpu

# the cases with gap points on the boundary clouds
NAMES = ("m2_az0.0_q1", "m2_az-2.4_q3", "moonbot_az0.0_q4", "random0", "random10")
PREFIXES = (1, 63, 64, 65, 255, 256, 257)


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


@pytest.fixture(scope="module")
def cases(lrm, oracle):
    """mixed order, 512 far points each; 64 consecutive points hold several classes"""
    out = {}
    for name in NAMES:
        c = Case(oracle, *case_by_name(lrm, name), far=512, mixed=True)
        per_wave = [len(np.unique(c.cls[k:k + 64])) for k in range(0, len(c.pts) - 63, 64)]
        assert min(per_wave) >= 3 and (c.cls[:64] == FAR).any(), name
        out[name] = c
    return out


@pytest.mark.parametrize("name", NAMES)
def test_device_against_the_float64_model(lrm, oracle, torch_cuda, cases, name):
    """(a), (b) and (e) of tests/test_ik_boundary_cpu.py on what the device returns"""
    torch = torch_cuda
    c = cases[name]
    ang, st = lrm.device.ik(*soa(torch, c.pts), c.leg, c.quat)
    has = np.isfinite(c.src).all(1)
    xyz = lrm.device.fk(*soa(torch, c.src[has]), c.leg, c.quat)
    torch.cuda.synchronize()
    c.solve(ang.cpu().numpy().T, st.cpu().numpy())
    assert_contract_by_class(oracle, c)
    assert_gaps_are_real(c)
    full = np.full((len(c.pts), 3), np.nan)
    full[has] = xyz.cpu().numpy().T
    assert_fk(c, full)


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_cpu_on_the_faces(lrm, torch_cuda, cases, name):
    """angles, status bytes and FK positions bit for bit: the whole cloud without and with per-point seeds (source
    configuration or other knee; nan on the far points), and prefixes around the wave and block sizes"""
    torch = torch_cuda
    c = cases[name]
    seed = seed_plan(c)[0]
    x, y, z = soa(torch, c.pts)
    for sd in (None, seed):
        want_a, want_s, _ = lrm.apply_ik_cpu(c.pts, c.leg, c.quat, seed=sd)
        want_p, _ = lrm.apply_fk_cpu(want_a, c.leg, c.quat)
        ang, st = lrm.device.ik(x, y, z, c.leg, c.quat, seed=None if sd is None else soa(torch, sd))
        xyz = lrm.device.fk(ang[0], ang[1], ang[2], c.leg, c.quat)
        torch.cuda.synchronize()
        assert np.array_equal(st.cpu().numpy(), want_s)
        assert bits_equal(ang.cpu().numpy().T, want_a).all()
        assert bits_equal(xyz.cpu().numpy().T, want_p).all()
        for n in PREFIXES:
            out = torch.full((3, n + 3), 7.0, dtype=torch.float32, device="cuda")
            stb = torch.full((n + 3,), 9, dtype=torch.uint8, device="cuda")
            sn = None if sd is None else tuple(t[:n] for t in soa(torch, sd))
            a, s = lrm.device.ik(x[:n], y[:n], z[:n], c.leg, c.quat, seed=sn, out=out, status=stb)
            torch.cuda.synchronize()
            assert np.array_equal(s[:n].cpu().numpy(), want_s[:n]), n
            assert bits_equal(a[:, :n].cpu().numpy().T, want_a[:n]).all(), n
            assert (out[:, n:] == 7.0).all() and (stb[n:] == 9).all(), n  # nothing written past n


def test_posed_queries_on_the_faces(lrm, oracle, torch_cuda):
    """3 unit-quaternion poses x 2 legs: each (pose, leg) gets the boundary tips of its own limit set plus body[pose] as
    targets; the queries are shuffled, so adjacent lanes hold different (pose, leg).  Bit for bit against
    lrm_ik_posed_cpu / lrm_fk_posed_cpu; items 1-4 and the gap rule against float64 with p = float32(target - body)."""
    torch = torch_cuda
    quats = np.stack([unit(fixture_quats()[k]) for k in (1, 3, 4)]).astype(np.float32)
    body = np.array([[0, 0, 0], [256, -128, 64], [-1000.5, 730.25, 12.125]], np.float32)
    legs = np.stack([lrm.get_M2_leg(0.0), lrm.get_moonbot_leg(0.0)]).astype(np.float32)
    groups, tg, pi, li = [], [], [], []
    for p in range(3):
        for l in range(2):
            c = Case(oracle, f"pose{p}_leg{l}", legs[l], quats[p], "standard")
            groups.append((p, l, c))
            tg.append((c.pts + body[p]).astype(np.float32))
            pi.append(np.full(len(c.pts), p, np.int32))
            li.append(np.full(len(c.pts), l, np.uint8))
    tg, pi, li = np.concatenate(tg), np.concatenate(pi), np.concatenate(li)
    grp = np.concatenate([np.full(len(g[2].pts), k) for k, g in enumerate(groups)])
    o = np.random.default_rng(5).permutation(len(tg))
    tg, pi, li, grp = np.ascontiguousarray(tg[o]), pi[o], li[o], grp[o]
    assert (np.diff(grp[:4096]) != 0).mean() > 0.7
    ps = lrm.PoseSet(legs, 3, ik=True).update(dev(torch, quats), dev(torch, body))
    dpi, dli = dev(torch, pi), dev(torch, li)
    ang, st = ps.ik(*soa(torch, tg), dpi, dli)
    tip = ps.fk(ang[0], ang[1], ang[2], dpi, dli)
    torch.cuda.synchronize()
    got_a, got_s = ang.cpu().numpy().T, st.cpu().numpy()
    want_a, want_s, _ = lrm.apply_ik_posed_cpu(tg, pi, li, quats, body, legs)
    want_p, _ = lrm.apply_fk_posed_cpu(want_a, pi, li, quats, body, legs)
    assert np.array_equal(got_s, want_s)
    assert bits_equal(got_a, want_a).all()
    assert bits_equal(tip.cpu().numpy().T, want_p).all()
    inv = np.argsort(o)
    gaps = 0
    for k, (p, l, c) in enumerate(groups):
        sel = inv[grp[inv] == k]  # this group's queries in the cloud's own order
        c.pts = (tg[sel] - body[p]).astype(np.float32)  # the kernel's p: one float32 subtraction per component
        c.mask = oracle.reach(c.pts, c.leg, c.quat).astype(bool)
        d, _ = oracle.dist(c.pts, c.leg, c.quat)
        c.dn = np.linalg.norm(d.astype(np.float64), axis=1)
        c.solve(got_a[sel], got_s[sel])
        assert_contract_by_class(oracle, c)
        assert_gaps_are_real(c)
        gaps += int(c.gap.sum())
    assert gaps > 0
