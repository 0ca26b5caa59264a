"""lrm_footholds_dev (run with -m gpu on an MI355X): bit-identical to the host loop lrm_footholds_cpu, on both sides of
the 4096-target box threshold and at tile boundaries; count > 0 equals lrm_reach_any_dev's bit at config-3 size; the
answers do not depend on the order of the targets; every output is written on the caller's stream."""
import numpy as np
import pytest

from conftest import reference_terrain
from footholds_cases import QUATS, bits, legs_for, nominal_for, scene

pytestmark = pytest.mark.gpu

_CPU = {}  # host answers, shared by both modes


@pytest.fixture(autouse=True, params=["strict", "fast"])
def mode(request, lrm):
    """Every GPU test runs in both bit-exact modes; the answers must not depend on the mode."""
    lrm.set_mode(lrm.MODE_FAST if request.param == "fast" else lrm.MODE_STRICT)
    yield request.param
    lrm.set_mode(lrm.MODE_FAST)  # the library default


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def soa(torch, pts):
    t = torch.from_numpy(np.ascontiguousarray(pts.T)).cuda()
    return t[0], t[1], t[2]


def cpu(lrm, key, bodies, targets, legs, quat, nominal):
    if key not in _CPU:
        _CPU[key] = lrm.footholds_cpu(bodies, targets, legs, quat, nominal)[:3]
    return _CPU[key]


def run(lrm, torch, bodies, targets, legs, quat=None, nominal=None):
    bx, by, bz = soa(torch, bodies)
    tx, ty, tz = soa(torch, targets)
    c, b, d = lrm.device.footholds(bx, by, bz, tx, ty, tz, legs, quat, nominal)
    torch.cuda.synchronize()
    return c.cpu().numpy(), b.cpu().numpy(), d.cpu().numpy()


def assert_same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(bits(got[2]), bits(want[2]))


# nt: 4095 / 4096 are the two sides of the box threshold; 5119 / 5121 straddle the tile boundary 5 * 1024
@pytest.mark.parametrize("nlegs,nt,qname,with_nominal", [(1, 5003, "identity", True), (4, 4095, "tilted", True),
                                                        (6, 4096, "identity", False), (8, 5121, "tilted", True),
                                                        (6, 5119, "tilted", True), (4, 1025, "identity", False)])
def test_footholds_match_host_loop(lrm, torch_cuda, nlegs, nt, qname, with_nominal):
    quat = QUATS[qname]
    bodies, targets = scene(333, nt, seed=nlegs + nt, half=900.0)
    legs = legs_for(lrm, nlegs, quat)
    nominal = nominal_for(nlegs) if with_nominal else None
    want = cpu(lrm, ("scene", nlegs, nt, qname, with_nominal), bodies, targets, legs, quat, nominal)
    assert 0.02 < (want[0] > 0).mean() < 1.0
    assert_same(run(lrm, torch_cuda, bodies, targets, legs, quat, nominal), want)


def test_footholds_config3_against_reach_any(lrm, torch_cuda):
    """config 3 on the reference's terrain: count > 0 is reach_any's bit everywhere; 64 random bodies equal the host loop"""
    from lrm_amd import workloads
    t = reference_terrain()
    ground, bodies = t["ground"], t["bodies"]
    legs = workloads.hexapod(lrm.get_M2_leg, 6)
    nominal = nominal_for(6, seed=7)
    bx, by, bz = soa(torch_cuda, bodies)
    tx, ty, tz = soa(torch_cuda, ground)
    count, best, best_d2 = lrm.device.footholds(bx, by, bz, tx, ty, tz, legs, None, nominal)
    anyb, _ = lrm.device.reach_any(bx, by, bz, tx, ty, tz, legs)
    torch_cuda.cuda.synchronize()
    got = count.cpu().numpy(), best.cpu().numpy(), best_d2.cpu().numpy()
    assert np.array_equal((got[0] > 0).astype(np.uint8), anyb.cpu().numpy())
    pick = np.sort(np.random.default_rng(21).choice(len(bodies), 64, replace=False))
    want = cpu(lrm, ("config3", 64), bodies[pick], ground, legs, None, nominal)
    assert_same(tuple(a[:, pick] for a in got), want)


def test_footholds_independent_of_target_order(lrm, torch_cuda):
    from lrm_amd import workloads
    t = reference_terrain()
    ground = t["ground"]
    bodies = t["bodies"][np.random.default_rng(5).choice(len(t["bodies"]), 20000, replace=False)]
    legs = workloads.hexapod(lrm.get_M2_leg, 6)
    nominal = nominal_for(6, seed=9)
    order = lrm.morton_order(ground)
    c1, b1, d1 = run(lrm, torch_cuda, bodies, ground, legs, None, nominal)
    c2, b2, d2 = run(lrm, torch_cuda, bodies, ground[order], legs, None, nominal)
    assert (c1 > 0).mean() > 0.05
    assert np.array_equal(c1, c2) and np.array_equal(bits(d1), bits(d2))
    # the choice in original indexing has the same d2 (ties may pick another point of equal d2)
    has = c2 > 0
    chosen = np.where(has, order[np.maximum(b2, 0)], -1)
    assert np.array_equal(chosen >= 0, b1 >= 0)
    c = bodies[None, :, :] + nominal[:, None, :]
    p = ground[np.maximum(chosen, 0)]
    dd = p - c
    d2 = (dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]
    assert np.array_equal(bits(d2[has]), bits(d1[has]))


def test_footholds_on_the_callers_stream(lrm, torch_cuda):
    torch = torch_cuda
    bodies, targets = scene(300, 6000, seed=31, half=900.0)
    legs = legs_for(lrm, 6, QUATS["identity"])
    want = cpu(lrm, ("stream",), bodies, targets, legs, None, None)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        bx, by, bz = soa(torch, bodies)
        tx, ty, tz = soa(torch, targets)
        count = torch.full((6, 300), -7, dtype=torch.int32, device="cuda")
        best = torch.full((6, 300), -7, dtype=torch.int32, device="cuda")
        best_d2 = torch.full((6, 300), -7.0, dtype=torch.float32, device="cuda")
        lrm.device.footholds(bx, by, bz, tx, ty, tz, legs, count=count, best=best, best_d2=best_d2)
    s.synchronize()
    got = count.cpu().numpy(), best.cpu().numpy(), best_d2.cpu().numpy()
    assert (got[0] != -7).all() and (got[1] != -7).all() and (got[2] != -7.0).all()
    assert_same(got, want)
