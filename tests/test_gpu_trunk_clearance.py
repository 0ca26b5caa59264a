"""Trunk-leg clearance on the device (run with -m gpu on an MI355X): PoseSet.trunk_clearance / lrm_trunk_clearance_posed_dev
against the host loop lrm_trunk_clearance_posed_cpu bit for bit (links, worst, pen bits, free) over set counts around the
8-set wave, the 32-set block and the grid-stride boundaries, 1 to 8 legs, dead sets and invalid legs at the first, middle and
last lane of a set's group and of a wave, every scene and form of tests/test_trunk_clearance_cpu.py (which ties that host loop
to a numpy restatement of include/lrm.h), the NULL forms of the C ABI; lrm_dbg_trunk_link_dist_dev against _host; the chain
update -> footholds -> ik -> trunk_clearance -> self_clearance(live_in=free) on ONE PoseSet against the host chain, the edge
form, a graph replay; and the device straight against the float64 model of tests/trunk_model64.py with the bands measured on
the CPU.  Every output is prefilled with a sentinel, so an unwritten entry fails too."""
import os
import re

import numpy as np
import pytest

import leg_clearance_cases as lc
import pair_cases as pc
import posed_cases
import self_clearance_cases as sc
import trunk_clearance_cases as tc
import trunk_model64 as t64

pytestmark = pytest.mark.gpu

F = np.float32
SENT_B, SENT_F = 0xA5, -7.0
SETS_PER_WAVE, SETS_PER_BLOCK = 8, 32
GRID_SETS = 65536  # kMaxGrid workgroups of 32 sets


def test_the_constants_are_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged-robot-movability-cuda_amd", "csrc",
                            "lrm_trunk_clearance.hip")).read()
    assert int(re.search(r"constexpr unsigned kMaxGrid = (\d+);", src).group(1)) * SETS_PER_BLOCK == GRID_SETS
    assert int(re.search(r"constexpr int kBlock = (\d+);", src).group(1)) == 8 * SETS_PER_BLOCK == 64 * SETS_PER_BLOCK // SETS_PER_WAVE


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


def outputs(torch, nl, ns):
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    return (full((nl, ns), SENT_B, torch.uint8), full((nl, ns), SENT_B, torch.uint8), full((nl, ns), SENT_F, torch.float32),
            full((ns,), SENT_B, torch.uint8))


def run(lrm, torch, quats, legs, angles, trunk, radius=tc.RADIUS, margin=tc.MARGIN, tip_clear=tc.TIP_CLEAR, links=tc.LINKS, pose_idx=None,
        live_in=None, pen=True, free=True):
    """PoseSet.trunk_clearance into sentinel-filled outputs -> numpy (links, worst, pen or None, free or None)"""
    legs = np.asarray(legs, F).reshape(-1, 14)
    nl = len(legs)
    angles = np.asarray(angles, F).reshape(-1, 3)
    ns = len(angles) // nl
    ps = lrm.PoseSet(legs, len(quats), ik=True).update(dev(torch, np.asarray(quats, F)))
    a = dev(torch, angles.T)
    pi = dev(torch, None if pose_idx is None else np.asarray(pose_idx, np.int32))
    lv = dev(torch, None if live_in is None else np.asarray(live_in, np.uint8))
    out = outputs(torch, nl, ns)
    if pen and free:
        ps.trunk_clearance(a, radius, trunk[0], trunk[1], trunk[2], margin, tip_clear, links, pi, lv, *out)
    else:  # the NULL forms of the C ABI
        dp = lambda t: None if t is None else t.data_ptr()
        r = np.ascontiguousarray(radius, F)
        rc = lrm.load().lrm_trunk_clearance_posed_dev(dp(ps.workspace), dp(ps.ik_workspace), len(quats), nl, dp(pi), ns, dp(a[0]), dp(a[1]), dp(a[2]),
                                                      r.ctypes.data, float(margin), float(tip_clear), trunk[0], trunk[1], trunk[2], links, dp(lv),
                                                      dp(out[0]), dp(out[1]), dp(out[2] if pen else None), dp(out[3] if free else None),
                                                      torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    if not pen:
        assert (out[2] == SENT_F).all()
    if not free:
        assert (out[3] == SENT_B).all()
    got = [t.cpu().numpy() for t in out]
    return got[0], got[1], got[2] if pen else None, got[3] if free else None


def check(lrm, torch, quats, legs, angles, trunk, radius=tc.RADIUS, margin=tc.MARGIN, tip_clear=tc.TIP_CLEAR, links=tc.LINKS, pose_idx=None,
          live_in=None, mixed=True, **kw):
    """the device against the host loop, bit for bit -> the host's answer"""
    want = tc.host(lrm, quats, legs, angles, trunk, radius, margin, tip_clear, links, pose_idx, live_in)
    if mixed:  # sets with a hit and free sets
        assert (want["links"] != 0).any() and (want["free"] == 1).any()
    tc.assert_same(run(lrm, torch, quats, legs, angles, trunk, radius, margin, tip_clear, links, pose_idx, live_in, **kw), want)
    _, live = sc.set_poses(len(quats), want["links"].shape[1], pose_idx, live_in)
    tc.assert_consequences(want, margin, links, live)
    return want


def poses(n, seed):
    return posed_cases.random_unit_quats(n, np.random.default_rng(seed))


def trunk6(lrm):
    return tc.trunk_of(sc.legs_n(lrm, 6))


@pytest.mark.parametrize("ns", [1, 7, 8, 9, 31, 32, 33, 255, 256, 257])
def test_set_counts(lrm, torch_cuda, ns):
    """random angles, 24 poses repeated through pose_idx"""
    quats = poses(24, ns)
    pi = np.random.default_rng(ns).integers(0, 24, ns).astype(np.int32)
    check(lrm, torch_cuda, quats, sc.legs_n(lrm, 6), lc.random_angles(ns, 6, seed=ns), trunk6(lrm), pose_idx=pi, mixed=ns >= 31)


def test_set_count_past_the_grid_stride(lrm, torch_cuda):
    """kMaxGrid workgroups hold 65 536 sets; a workgroup and one more make the first workgroup and one lane group of the second
    take a second round"""
    ns = GRID_SETS + SETS_PER_BLOCK + 1
    quats = poses(24, 3)
    pi = np.random.default_rng(3).integers(0, 24, ns).astype(np.int32)
    legs = sc.legs_n(lrm, 6)
    trunk = trunk6(lrm)
    ang = lc.random_angles(ns, 6, seed=3).reshape(6, ns, 3)
    h = int(np.argmax(tc.host(lrm, quats, legs, ang[:, :64].reshape(-1, 3), trunk, pose_idx=pi[:64])["free"] == 0))  # a set with a hit
    ang[:, GRID_SETS::2], pi[GRID_SETS::2] = ang[:, h:h + 1], pi[h]
    want = check(lrm, torch_cuda, quats, legs, ang.reshape(-1, 3), trunk, pose_idx=pi)
    assert (want["links"][:, GRID_SETS:] != 0).any() and (want["free"][GRID_SETS::2] == 0).all() and (want["free"][GRID_SETS:] == 1).any()


@pytest.mark.parametrize("nlegs", range(1, 9))
def test_leg_counts(lrm, torch_cuda, nlegs):
    n = 130
    legs = sc.legs_n(lrm, nlegs)
    trunk = tc.trunk_of(legs)
    want = check(lrm, torch_cuda, poses(n, nlegs), legs, lc.random_angles(n, nlegs, seed=20 + nlegs), trunk, links=0b111, mixed=False)
    assert (want["links"] & 1 == 1).all() and (want["free"] == 0).all()  # every leg slot up to nlegs is answered
    check(lrm, torch_cuda, poses(n, nlegs), legs, lc.random_angles(n, nlegs, seed=40 + nlegs), trunk, mixed=False)


def test_dead_sets_and_invalid_legs_at_the_ends_of_a_group_and_a_wave(lrm, torch_cuda):
    ns = 96
    at = np.array([s for s in range(ns) if s % SETS_PER_WAVE in (0, 3, 7)])  # the first, a middle and the last set of every wave
    quats, legs, trunk = poses(ns, 5), sc.legs_n(lrm, 6), trunk6(lrm)
    ang = lc.random_angles(ns, 6, seed=31)
    live = np.ones(ns, np.uint8)
    live[at] = 0
    live[5], live[32:64] = 3, 0  # a whole block
    for lv in (np.ones(ns, np.uint8), np.zeros(ns, np.uint8), live):
        want = check(lrm, torch_cuda, quats, legs, ang, trunk, live_in=lv, mixed=lv.any())
        assert (want["free"][lv == 0] == 0).all()
    rng = np.random.default_rng(6)
    pi = rng.permutation(ns).astype(np.int32)
    pi[at[0::3]], pi[at[1::3]], pi[at[2::3]] = -1, ns, np.iinfo(np.int32).min
    want = check(lrm, torch_cuda, quats, legs, ang, trunk, pose_idx=pi)
    assert (want["free"][at] == 0).all() and (want["worst"][:, at] == 255).all()
    # one leg invalid -- the first, a middle and the last lane of the set's group -- at the spots, under the coxa bit: the
    # other legs of the set keep their hit, so free stays 0 through the masked ballot
    for leg, (k, bad) in zip((0, 3, 5, 2), enumerate((np.nan, 120.0, -1e30, np.inf))):
        a = ang.reshape(6, ns, 3).copy()
        a[leg, at, k % 3] = bad
        want = check(lrm, torch_cuda, quats, legs, a.reshape(-1, 3), trunk, links=0b111, mixed=False)
        assert (want["links"][leg, at] == 0).all() and (want["worst"][leg, at] == 255).all() and (want["free"] == 0).all()
        check(lrm, torch_cuda, quats, legs, a.reshape(-1, 3), trunk)
    # only ONE leg valid, at the first and the last lane: its hit alone decides free
    for leg in (0, 5):
        a = np.full((6, ns, 3), np.nan, F)
        a[leg] = ang.reshape(6, ns, 3)[leg]
        want = check(lrm, torch_cuda, quats, legs, a.reshape(-1, 3), trunk)
        assert np.array_equal(want["free"], (want["links"][leg] == 0).astype(np.uint8))
    a = ang.reshape(6, ns, 3).copy()
    a[:, at] = np.nan
    want = check(lrm, torch_cuda, quats, legs, a.reshape(-1, 3), trunk, links=0b111, mixed=False)
    assert (want["free"][at] == 1).all() and (want["worst"][:, at] == 255).all() and (np.delete(want["free"], at) == 0).all()


@pytest.fixture(scope="module")
def main(lrm):
    legs = sc.legs_n(lrm, 6)
    quats, body, targets = lc.main_scene(lrm)
    ang, st, best = lc.stance_angles(lrm, targets, quats, body, legs)
    return quats, body, targets, legs, ang, tc.trunk_of(legs)


@pytest.mark.parametrize("links", [0b110, 0b111, 0])
@pytest.mark.parametrize("margin", [0.0, 10.0])
@pytest.mark.parametrize("angles", ["stance", "random"])
def test_the_cpu_scenes(lrm, torch_cuda, main, angles, margin, links):
    quats, _, _, legs, ang, trunk = main
    if angles == "random":
        ang = lc.random_angles(len(quats), 6, seed=6)
    check(lrm, torch_cuda, quats, legs, ang, trunk, tc.RADIUS, margin, tc.TIP_CLEAR, links, mixed=links == 0b110)


def test_the_cpu_forms(lrm, torch_cuda, main):
    """radius 0 per link, the link mask, tip_clear beyond the tibia, a thin and a flat trunk, live_in and pose_idx forms, invalid
    legs, angles next to +-120, non-unit and nan quaternions, the NULL outputs: the scenes of tests/test_trunk_clearance_cpu.py"""
    torch = torch_cuda
    quats, body, targets, legs, ang, trunk = main
    n = len(quats)
    rnd = lc.random_angles(n, 6, seed=12)
    for r in ((0.0, 22.0, 16.0), (28.0, 0.0, 16.0), (28.0, 22.0, 0.0), (0.0, 0.0, 16.0)):
        check(lrm, torch, quats, legs, rnd, trunk, r, links=0b111, mixed=False)
    for links in (0b001, 0b010, 0b100, 0b011, 0b101):
        check(lrm, torch, quats, legs, rnd, trunk, links=links, mixed=False)
    check(lrm, torch, quats, legs, rnd, trunk, (0.0, 0.0, 0.0), links=0b111, mixed=False)
    check(lrm, torch, quats, legs, rnd, trunk, tip_clear=1e4, links=0b111, mixed=False)
    check(lrm, torch, quats, legs, ang, trunk, tip_clear=0.0)
    check(lrm, torch, quats, legs, rnd, (0.0, 40.0, -80.0), links=0b111, mixed=False)
    check(lrm, torch, quats, legs, rnd, (trunk[0], 0.001, 0.0), links=0b111, mixed=False)
    check(lrm, torch, quats, legs, rnd, (300.0, 200.0, -200.0), margin=0.0, mixed=False)
    for name, lv in lc.live_forms(lrm, targets, quats, body, legs).items():
        check(lrm, torch, quats, legs, ang, trunk, live_in=lv, mixed=name != "zeros")
    rng = np.random.default_rng(3)
    for pi in (np.arange(n), rng.permutation(n), rng.integers(0, n, n), np.full(n, 17)):
        check(lrm, torch, quats, legs, rnd, trunk, pose_idx=pi.astype(np.int32), mixed=False)
    check(lrm, torch, quats, legs, lc.random_angles(400, 6, seed=9), trunk, pose_idx=rng.integers(0, n, 400).astype(np.int32))
    a = rnd.reshape(6, n, 3).copy()
    a[0, ::3, 0], a[2, 1::4, 1], a[5, ::5, 2], a[3, 7], a[1, 9, 1], a[:, 11] = np.nan, 120.0, -500.0, np.inf, -120.0, np.nan
    check(lrm, torch, quats, legs, a.reshape(-1, 3), trunk, links=0b111, mixed=False)
    edge = lc.random_angles(n, 6, seed=11).reshape(6, n, 3)
    edge[1, ::2, 0], edge[2, ::3, 0], edge[4, ::5, 1] = 119.99, -119.99, 117.0
    check(lrm, torch, quats, legs, edge.reshape(-1, 3), trunk, links=0b111, mixed=False)
    q = (poses(90, 14) * rng.uniform(0.5, 2.0, (90, 1))).astype(F)
    q[5, 1], q[40], q[77, 3] = np.nan, np.nan, np.inf
    check(lrm, torch, q, legs, lc.random_angles(90, 6, seed=15), trunk)
    for kw in ({"pen": False}, {"free": False}, {"pen": False, "free": False}):
        check(lrm, torch, quats, legs, ang, trunk, **kw)


def test_link_distance_on_the_device(lrm, torch_cuda):
    """lrm_dbg_trunk_link_dist_dev against _host bit for bit: every hand-made kind and the random links, and cuts of their
    mixture around one and four waves"""
    torch = torch_cuda
    kinds = tc.hand_made_links()
    kinds["random"] = tc.random_links() + (None,)
    g = np.concatenate([np.concatenate([A, B], 1) for A, B, _ in kinds.values()])
    mix = g[np.random.default_rng(1).permutation(len(g))]
    for segs in (g, mix[:1], mix[:63], mix[:64], mix[:65], mix[:255], mix[:256], mix[:257]):
        out = torch.full((len(segs),), SENT_F, dtype=torch.float32, device="cuda")
        lrm.device.dbg_trunk_link_dist(dev(torch, segs), *tc.CYL, out)
        torch.cuda.synchronize()
        assert np.array_equal(pc.bits(out.cpu().numpy()), pc.bits(lrm.dbg_trunk_link_dist_host(segs, *tc.CYL)))
    assert lrm.device.dbg_trunk_link_dist(torch.empty((0, 6), dtype=torch.float32, device="cuda"), *tc.CYL).numel() == 0
    for bad in (dev(torch, g[:8]).double(), dev(torch, g[:8])[:, :5], dev(torch, g[:16])[::2], torch.from_numpy(g[:8])):
        with pytest.raises(ValueError):
            lrm.device.dbg_trunk_link_dist(bad, *tc.CYL)
    with pytest.raises(ValueError):
        lrm.device.dbg_trunk_link_dist(dev(torch, g[:8]), *tc.CYL, torch.empty(7, dtype=torch.float32, device="cuda"))
    L = lrm.load()
    assert L.lrm_dbg_trunk_link_dist_dev(None, 3, 1.0, 1.0, 0.0, None, None) == -1 and L.lrm_dbg_trunk_link_dist_dev(None, 0, 1.0, 1.0, 0.0, None, None) == 0


def test_refused_views_and_every_einval(lrm, torch_cuda, main):
    torch = torch_cuda
    quats, _, _, legs, ang, trunk = main
    n = len(quats)
    ps = lrm.PoseSet(legs, n, ik=True)
    a = dev(torch, ang.T)
    with pytest.raises(ValueError):
        ps.trunk_clearance(a, tc.RADIUS, *trunk)  # before update()
    ps.update(dev(torch, quats))
    ps.trunk_clearance(a, tc.RADIUS, *trunk)
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device="cuda")
    wide = dev(torch, np.repeat(ang.T, 2, 1))
    for kw in ({"angles": wide[:, ::2]}, {"angles": a.double()}, {"angles": a.cpu()}, {"angles": a[:2]}, {"angles": a[:, :-1]},
               {"angles": dev(torch, np.zeros((3, 6 * (n + 1)), F))}, {"radius": (1.0, 2.0)}, {"links": -1}, {"links": 256},
               {"pose_idx": torch.zeros(n, dtype=torch.int64, device="cuda")},
               {"pose_idx": torch.zeros(2 * n, dtype=torch.int32, device="cuda")[::2]}, {"pose_idx": torch.zeros(n - 1, dtype=torch.int32, device="cuda")},
               {"live_in": u8(2 * n)[::2]}, {"live_in": u8(n - 1)}, {"live_in": torch.empty(n, dtype=torch.uint8)},
               {"hit": torch.empty((6, n), dtype=torch.int32, device="cuda")}, {"hit": u8(6, n - 1)}, {"worst": u8(6, 2 * n)[:, ::2]},
               {"pen": torch.empty((6, n), dtype=torch.float64, device="cuda")}, {"free": u8(n - 1)}):
        with pytest.raises(ValueError):
            ps.trunk_clearance(kw.pop("angles", a), kw.pop("radius", tc.RADIUS), *trunk, **kw)
    for kw in ({"radius": (1.0, -1.0, 1.0)}, {"radius": (np.nan, 1.0, 1.0)}, {"radius": (1.0, 1.0, np.inf)}, {"margin": -1.0}, {"margin": np.nan},
               {"margin": np.inf}, {"tip_clear": -0.5}, {"tip_clear": np.nan}, {"tip_clear": np.inf}, {"links": 8}, {"links": 255}):
        with pytest.raises(lrm.LrmError):
            ps.trunk_clearance(a, kw.pop("radius", tc.RADIUS), *trunk, **kw)
    for bad in ((np.nan, 40.0, -80.0), (np.inf, 40.0, -80.0), (186.0, np.nan, -80.0), (186.0, 40.0, -np.inf), (-1.0, 40.0, -80.0),
                (186.0, -80.0, -80.0), (186.0, -80.0, 40.0)):
        with pytest.raises(lrm.LrmError):
            ps.trunk_clearance(a, tc.RADIUS, *bad)
    with pytest.raises(ValueError):
        lrm.PoseSet(legs, n).update(dev(torch, quats)).trunk_clearance(a, tc.RADIUS, *trunk)  # built without ik=True
    # the C ABI's own checks, in its order; nothing is launched
    L, dp = lrm.load(), lambda t: None if t is None else t.data_ptr()
    out = outputs(torch, 6, n)
    r = np.ascontiguousarray(tc.RADIUS, F)
    ok = dict(ws=ps.workspace, ik=ps.ik_workspace, nposes=n, nl=6, pose_idx=None, ns=n, coxa=a[0], radius=r.ctypes.data, R=186.0, pz=40.0, mz=-80.0,
              mask=6, links=out[0], worst=out[1])

    def rc(**kw):
        v = dict(ok, **kw)
        return L.lrm_trunk_clearance_posed_dev(dp(v["ws"]), dp(v["ik"]), v["nposes"], v["nl"], dp(v["pose_idx"]), v["ns"], dp(v["coxa"]), dp(a[1]),
                                               dp(a[2]), v["radius"], 0.0, 0.0, v["R"], v["pz"], v["mz"], v["mask"], None, dp(v["links"]),
                                               dp(v["worst"]), dp(out[2]), dp(out[3]), torch.cuda.current_stream().cuda_stream)

    assert rc() == 0
    big = 2 ** 31
    for kw in (dict(nl=0), dict(nl=9), dict(ns=big), dict(nposes=big), dict(ns=2 ** 30, nposes=2 ** 30, nl=8), dict(radius=None), dict(ns=n + 1),
               dict(R=float("nan")), dict(R=-0.5), dict(pz=-80.0), dict(mz=float("inf")), dict(mask=8),
               dict(ws=None), dict(ik=None), dict(coxa=None), dict(links=None), dict(worst=None)):
        assert rc(**kw) == -1, kw
    assert rc(ns=0, coxa=None, links=None) == 0  # nsets == 0 is a no-op
    assert rc(ns=0, mask=8) == -1
    torch.cuda.synchronize()


def test_chain_on_one_pose_set(lrm, torch_cuda):
    """update -> footholds -> ik(check=False) -> trunk_clearance -> self_clearance(live_in=free) on ONE PoseSet against the host
    chain"""
    torch = torch_cuda
    legs = sc.legs_n(lrm, 6)
    trunk = tc.trunk_of(legs)
    n = 192
    quats, body, targets = lc.main_scene(lrm, n, 3000, seed=51)
    ps = lrm.PoseSet(legs, n, ik=True, footholds=True).update(dev(torch, quats), dev(torch, body))
    tx, ty, tz = soa(torch, targets)
    best = ps.footholds(tx, ty, tz)[1]
    pi, li = lrm.device.footholds_layout(n, 6, "cuda")
    ang, st = ps.ik(tx, ty, tz, pi, li, target_idx=best.view(-1), check=False)
    got = ps.trunk_clearance(ang, tc.RADIUS, *trunk, tc.MARGIN, tc.TIP_CLEAR)
    slf = ps.self_clearance(ang, sc.RADIUS, sc.MARGIN, sc.TIP_CLEAR, live_in=got[3])
    torch.cuda.synchronize()
    h_ang, _, h_best = lc.stance_angles(lrm, targets, quats, body, legs)
    assert np.array_equal(best.cpu().numpy(), h_best) and np.array_equal(pc.bits(ang.cpu().numpy().T), pc.bits(h_ang))
    want = tc.host(lrm, quats, legs, h_ang, trunk)
    tc.assert_same(tuple(t.cpu().numpy() for t in got), want)
    assert 0 < want["free"].sum() < n
    h_slf = sc.host(lrm, quats, legs, h_ang, live_in=want["free"])
    sc.assert_same(tuple(t.cpu().numpy() for t in slf), h_slf)
    assert (h_slf["free"] <= want["free"]).all() and 0 < h_slf["free"].sum() < want["free"].sum()


def test_edge_form_against_the_host_chain(lrm, torch_cuda):
    """angles = ik() on foothold_edges()'s best under foothold_edges_layout, pose_idx = edge_a, then edge_b: do the legs stay
    out of the trunk in either pose on the common feet"""
    torch = torch_cuda
    legs = sc.legs_n(lrm, 6)
    trunk = tc.trunk_of(legs)
    n, ne = 150, 300
    quats, body, targets = lc.main_scene(lrm, n, 3000, seed=52)
    rng = np.random.default_rng(7)
    ea = rng.integers(0, n, ne).astype(np.int32)
    eb = np.clip(ea + rng.integers(-2, 3, ne), 0, n - 1).astype(np.int32)
    ps = lrm.PoseSet(legs, n, ik=True, footholds=True).update(dev(torch, quats), dev(torch, body))
    tx, ty, tz = soa(torch, targets)
    da, db = dev(torch, ea), dev(torch, eb)
    best = ps.foothold_edges(tx, ty, tz, da, db)[1]
    h_best = lrm.foothold_edges_posed_cpu(targets, quats, body, legs, ea, eb)[1]
    assert np.array_equal(best.cpu().numpy(), h_best)
    for which, edge, dedge in (("a", ea, da), ("b", eb, db)):
        pi, li = lrm.device.foothold_edges_layout(ne, 6, "cuda", da, db, which)
        ang = ps.ik(tx, ty, tz, pi, li, target_idx=best.view(-1), check=False)[0]
        got = ps.trunk_clearance(ang, tc.RADIUS, *trunk, tc.MARGIN, tc.TIP_CLEAR, pose_idx=dedge)
        torch.cuda.synchronize()
        h_ang = lrm.apply_ik_posed_cpu(targets, np.tile(edge, 6), np.repeat(np.arange(6, dtype=np.uint8), ne), quats, body, legs,
                                       target_idx=h_best.reshape(-1))[0]
        assert np.array_equal(pc.bits(ang.cpu().numpy().T), pc.bits(h_ang))
        want = tc.host(lrm, quats, legs, h_ang, trunk, pose_idx=edge)
        tc.assert_same(tuple(t.cpu().numpy() for t in got), want)
        assert (want["links"] != 0).any() and (want["free"] == 1).any()


def test_chain_replays_from_a_graph(lrm, torch_cuda):
    """update(), footholds(), ik(), trunk_clearance() and self_clearance() only launch once the box buffer holds the cloud's
    size: the linear chain captured on ONE side stream after a warm call, replayed once after new quaternions, bodies and
    targets were copied into the captured tensors"""
    torch = torch_cuda
    legs = sc.legs_n(lrm, 6)
    trunk = tc.trunk_of(legs)
    n = 128
    q0, b0, t0 = lc.main_scene(lrm, n, 4500, seed=41)
    q1, b1, t1 = lc.main_scene(lrm, n, 4500, seed=42)
    qt, bt, tt = dev(torch, q0), dev(torch, b0), dev(torch, t0.T.copy())
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device="cuda")
    cnt, bst, bd, al = i32(6, n), i32(6, n), torch.empty((6, n), dtype=torch.float32, device="cuda"), u8(n)
    ang, st = torch.empty((3, 6 * n), dtype=torch.float32, device="cuda"), u8(6 * n)
    out = outputs(torch, 6, n)
    sh, sw, sl, sx, sp, sf = i32(6, n), u8(6, n), u8(6, n), u8(6, n), torch.empty((6, n), dtype=torch.float32, device="cuda"), u8(n)
    pi, li = lrm.device.footholds_layout(n, 6, "cuda")
    ps = lrm.PoseSet(legs, n, ik=True, footholds=True)

    def work():
        ps.update(qt, bt)
        ps.footholds(tt[0], tt[1], tt[2], cnt, bst, bd, al)
        ps.ik(tt[0], tt[1], tt[2], pi, li, target_idx=bst.view(-1), out=ang, status=st, check=False)
        ps.trunk_clearance(ang, tc.RADIUS, trunk[0], trunk[1], trunk[2], tc.MARGIN, tc.TIP_CLEAR, tc.LINKS, None, None, *out)
        ps.self_clearance(ang, sc.RADIUS, sc.MARGIN, sc.TIP_CLEAR, None, out[3], sh, sw, sl, sx, sp, sf)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the warm call outside the capture: the box buffer grows here
        work()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            work()
        qt.copy_(dev(torch, q1))
        bt.copy_(dev(torch, b1))
        tt.copy_(dev(torch, t1.T.copy()))
        for t, v in zip(out, (SENT_B, SENT_B, SENT_F, SENT_B)):
            t.fill_(v)
        g.replay()
    torch.cuda.synchronize()
    h_ang = lc.stance_angles(lrm, t1, q1, b1, legs)[0]
    want = tc.host(lrm, q1, legs, h_ang, trunk)
    assert (want["links"] != 0).any() and (want["free"] == 1).any()
    tc.assert_same(tuple(t.cpu().numpy() for t in out), want)
    sc.assert_same(tuple(t.cpu().numpy() for t in (sh, sw, sl, sx, sp, sf)), sc.host(lrm, q1, legs, h_ang, live_in=want["free"]))
    del g


@pytest.mark.parametrize("ns", [1, 9, 257])
def test_the_device_against_the_float64_model(lrm, torch_cuda, main, ns):
    """the device's rows straight against tests/trunk_model64.py (joints from the leg's geometry, the true minimum distance to
    the cylinder) with the band measured on the CPU; unit quaternions, the chain's angles and random ones, margins 0 and 10"""
    quats, _, _, legs, ang, trunk = main
    n = len(quats)
    rng = np.random.default_rng(ns)
    pi = rng.integers(0, n, ns).astype(np.int32)
    stance = ang.reshape(6, n, 3)[:, pi].reshape(-1, 3)  # the chain's angles of the chosen poses
    rows = doubt = 0
    for angles in (stance, lc.random_angles(ns, 6, seed=ns)):
        J64 = t64.body_joints64(angles, legs, quats, tc.TIP_CLEAR, pose_of=pi)
        for margin in (0.0, 10.0):
            m = t64.trunk_clearance64(J64, tc.RADIUS, margin, trunk, 0b111)
            got = dict(zip(tc.KEYS, run(lrm, torch_cuda, quats, legs, angles, trunk, tc.RADIUS, margin, tc.TIP_CLEAR, 0b111, pose_idx=pi)))
            r, d = t64.check_trunk_rows(got, m, t64.BAND_TRUNK)
            rows, doubt = rows + r, doubt + d
    print(f"{ns} sets: {rows} rows compared, {doubt} in doubt")
    assert rows >= 4 * 6 * ns - doubt and doubt <= max(1, 0.02 * rows)
