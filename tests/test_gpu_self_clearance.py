"""Leg-leg self clearance on the device (run with -m gpu on an MI355X): PoseSet.self_clearance / lrm_self_clearance_posed_dev
against the host loop lrm_self_clearance_posed_cpu bit for bit (hits, with, links, worst, pen bits, free) over set counts
around the wave, block and grid-stride boundaries, 1 to 8 legs (the pair count crosses every 64-lane round), dead sets and
invalid legs at the first, second, middle and last positions of a 64-set group, every scene of
tests/test_self_clearance_cpu.py (which ties that host loop to a numpy restatement of include/lrm.h), the NULL forms of the
C ABI; lrm_dbg_link_pair_dist_dev against _host; the chain update -> footholds -> ik -> self_clearance ->
leg_clearance(live_in=free) on ONE PoseSet against the host chain, the edge form, a graph replay and two streams.  Every
output is prefilled with a sentinel, so an unwritten entry fails too."""
import os
import re

import numpy as np
import pytest

import leg_clearance_cases as lc
import pair_cases as pc
import posed_cases
import self_clearance_cases as sc

pytestmark = pytest.mark.gpu

F = np.float32
SENT_I, SENT_B, SENT_F = -77, 0xA5, -7.0
WAVES = 4
GRID_SETS = 65536  # kMaxGrid workgroups of four waves, one set per wave
SPOTS = (0, 1, 31, 32, 62, 63)


def test_the_constants_are_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged-robot-movability-cuda_amd", "csrc",
                            "lrm_self_clearance.hip")).read()
    assert int(re.search(r"constexpr unsigned kMaxGrid = (\d+);", src).group(1)) * WAVES == GRID_SETS
    assert int(re.search(r"constexpr int kBlock = (\d+);", src).group(1)) == 64 * WAVES
    assert int(re.search(r"constexpr int kRound = (\d+);", src).group(1)) == 64
    # the pair counts of 3 .. 8 legs cross every round of 64: 1, 1, 2, 3, 3, 4 rounds
    assert [-(-n * (n - 1) // 2 * 9 // 64) for n in range(3, 9)] == [1, 1, 2, 3, 3, 4]


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
    return (full((nl, ns), SENT_I, torch.int32), full((nl, ns), SENT_B, torch.uint8), full((nl, ns), SENT_B, torch.uint8),
            full((nl, ns), SENT_B, torch.uint8), full((nl, ns), SENT_F, torch.float32), full((ns,), SENT_B, torch.uint8))


def run(lrm, torch, quats, legs, angles, radius=sc.RADIUS, margin=sc.MARGIN, tip_clear=sc.TIP_CLEAR, pose_idx=None, live_in=None, pen=True,
        free=True):
    """PoseSet.self_clearance into sentinel-filled outputs -> numpy (hits, with, links, worst, pen or None, free or None)"""
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
        ps.self_clearance(a, radius, margin, tip_clear, pi, lv, *out)
    else:  # the NULL forms of the C ABI
        dp = lambda t: None if t is None else t.data_ptr()
        r = np.ascontiguousarray(radius, F)
        rc = lrm.load().lrm_self_clearance_posed_dev(dp(ps.workspace), dp(ps.ik_workspace), len(quats), nl, dp(pi), ns, dp(a[0]), dp(a[1]), dp(a[2]),
                                                     r.ctypes.data, float(margin), float(tip_clear), dp(lv), dp(out[0]), dp(out[1]), dp(out[2]),
                                                     dp(out[3]), dp(out[4] if pen else None), dp(out[5] if free else None),
                                                     torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    if not pen:
        assert (out[4] == SENT_F).all()
    if not free:
        assert (out[5] == SENT_B).all()
    got = [t.cpu().numpy() for t in out]
    return got[0], got[1], got[2], got[3], got[4] if pen else None, got[5] if free else None


def check(lrm, torch, quats, legs, angles, radius=sc.RADIUS, margin=sc.MARGIN, tip_clear=sc.TIP_CLEAR, pose_idx=None, live_in=None, mixed=True,
          **kw):
    """the device against the host loop, bit for bit -> the host's answer"""
    want = sc.host(lrm, quats, legs, angles, radius, margin, tip_clear, pose_idx, live_in)
    if mixed:  # sets with a hit and free sets
        assert (want["hits"] > 0).any() and (want["free"] == 1).any()
    sc.assert_same(run(lrm, torch, quats, legs, angles, radius, margin, tip_clear, pose_idx, live_in, **kw), want)
    _, live = sc.set_poses(len(quats), want["hits"].shape[1], pose_idx, live_in)
    sc.assert_consequences(want, margin, live)
    return want


def poses(n, seed):
    return posed_cases.random_unit_quats(n, np.random.default_rng(seed))


@pytest.mark.parametrize("ns", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257])
def test_set_counts(lrm, torch_cuda, ns):
    """random angles, 24 poses repeated through pose_idx"""
    quats = poses(24, ns)
    pi = np.random.default_rng(ns).integers(0, 24, ns).astype(np.int32)
    check(lrm, torch_cuda, quats, sc.legs_n(lrm, 6), lc.random_angles(ns, 6, seed=ns), pose_idx=pi, mixed=ns >= 63)


def test_set_count_past_the_grid_stride(lrm, torch_cuda):
    """kMaxGrid workgroups hold 65 536 sets; a workgroup and one more make the first five waves take a second set"""
    ns = GRID_SETS + WAVES + 1
    quats = poses(24, 3)
    pi = np.random.default_rng(3).integers(0, 24, ns).astype(np.int32)
    legs = sc.legs_n(lrm, 6)
    ang = lc.random_angles(ns, 6, seed=3).reshape(6, ns, 3)
    h = int(np.argmax(sc.host(lrm, quats, legs, ang[:, :64].reshape(-1, 3), pose_idx=pi[:64])["free"] == 0))  # a set with a hit
    ang[:, GRID_SETS::2], pi[GRID_SETS::2] = ang[:, h:h + 1], pi[h]
    want = check(lrm, torch_cuda, quats, legs, ang.reshape(-1, 3), pose_idx=pi)
    assert (want["hits"][:, GRID_SETS:] > 0).any() and (want["free"][GRID_SETS::2] == 0).all()


@pytest.mark.parametrize("nlegs", range(1, 9))
def test_leg_counts(lrm, torch_cuda, nlegs):
    n = 130
    want = check(lrm, torch_cuda, poses(n, nlegs), sc.legs_n(lrm, nlegs), lc.random_angles(n, nlegs, seed=20 + nlegs), mixed=False)
    assert (want["hits"] > 0).any() == (nlegs > 1)
    if nlegs > 2:  # every round of 64 pair codes (leg pair (i, j), i < j, holds codes 9 q .. 9 q + 8, q = j (j - 1) / 2 + i) has a hit
        rounds = set()
        for j in range(nlegs):
            for i in range(j):
                if ((want["with"][i] >> j) & 1).any():
                    q = j * (j - 1) // 2 + i
                    rounds |= {9 * q // 64, (9 * q + 8) // 64}
        assert rounds == set(range(-(-nlegs * (nlegs - 1) // 2 * 9 // 64))), rounds


def spots(ns):
    return np.array([g + s for g in range(0, ns, 64) for s in SPOTS if g + s < ns])


def test_dead_sets_and_invalid_legs_at_the_ends_of_a_group(lrm, torch_cuda):
    ns = 192
    at = spots(ns)
    quats, legs = poses(ns, 5), sc.legs_n(lrm, 6)
    ang = lc.random_angles(ns, 6, seed=31)
    live = np.ones(ns, np.uint8)
    live[at] = 0
    live[5], live[64:128] = 3, 0  # the four waves of sixteen whole blocks
    for lv in (np.ones(ns, np.uint8), np.zeros(ns, np.uint8), live):
        want = check(lrm, torch_cuda, quats, legs, ang, live_in=lv, mixed=lv.any())
        assert (want["free"][lv == 0] == 0).all()
    rng = np.random.default_rng(6)
    pi = rng.permutation(ns).astype(np.int32)
    pi[at[0::3]], pi[at[1::3]], pi[at[2::3]] = -1, ns, np.iinfo(np.int32).min
    want = check(lrm, torch_cuda, quats, legs, ang, pose_idx=pi)
    assert (want["free"][at] == 0).all() and (want["worst"][:, at] == 255).all()
    for k, bad in enumerate((np.nan, 120.0, -1e30, np.inf)):  # one leg invalid at the spots, then all of them
        a = ang.reshape(6, ns, 3).copy()
        a[k % 6, at, k % 3] = bad
        want = check(lrm, torch_cuda, quats, legs, a.reshape(-1, 3))
        assert (want["hits"][k % 6, at] == 0).all() and (((want["with"] >> (k % 6)) & 1)[:, at] == 0).all()
    a = ang.reshape(6, ns, 3).copy()
    a[:, at] = np.nan
    want = check(lrm, torch_cuda, quats, legs, a.reshape(-1, 3))
    assert (want["free"][at] == 1).all() and (want["worst"][:, at] == 255).all()


@pytest.fixture(scope="module")
def main(lrm):
    legs = sc.legs_n(lrm, 6)
    quats, body, targets = lc.main_scene(lrm)
    ang, st, best = lc.stance_angles(lrm, targets, quats, body, legs)
    return quats, body, targets, legs, ang


@pytest.mark.parametrize("tip_clear", [0.0, 30.0])
@pytest.mark.parametrize("margin", [0.0, 10.0])
@pytest.mark.parametrize("angles", ["stance", "random"])
def test_the_cpu_scenes(lrm, torch_cuda, main, angles, margin, tip_clear):
    quats, _, _, legs, ang = main
    if angles == "random":
        ang = lc.random_angles(len(quats), 6, seed=6)
    check(lrm, torch_cuda, quats, legs, ang, sc.RADIUS, margin, tip_clear)


def test_the_cpu_forms(lrm, torch_cuda, main):
    """thick coxa, radius 0 per link, tip_clear beyond the tibia, live_in and pose_idx forms, invalid legs, non-unit and nan
    quaternions, the NULL outputs: the scenes of tests/test_self_clearance_cpu.py"""
    torch = torch_cuda
    quats, body, targets, legs, ang = main
    n = len(quats)
    rnd = lc.random_angles(n, 6, seed=12)
    check(lrm, torch, quats, legs, ang, sc.RADIUS_COXA)
    for r in ((0.0, 22.0, 16.0), (90.0, 0.0, 16.0), (90.0, 22.0, 0.0), (0.0, 0.0, 16.0)):
        check(lrm, torch, quats, legs, rnd, r)
    check(lrm, torch, quats, legs, rnd, (0.0, 0.0, 0.0), mixed=False)
    check(lrm, torch, quats, legs, rnd, tip_clear=1e4)
    for name, lv in lc.live_forms(lrm, targets, quats, body, legs).items():
        check(lrm, torch, quats, legs, ang, live_in=lv, mixed=name != "zeros")
    rng = np.random.default_rng(3)
    for pi in (np.arange(n), rng.permutation(n), rng.integers(0, n, n), np.full(n, 17)):
        check(lrm, torch, quats, legs, rnd, pose_idx=pi.astype(np.int32))
    check(lrm, torch, quats, legs, lc.random_angles(400, 6, seed=9), pose_idx=rng.integers(0, n, 400).astype(np.int32))
    a = rnd.reshape(6, n, 3).copy()
    a[0, ::3, 0], a[2, 1::4, 1], a[5, ::5, 2], a[3, 7], a[:, 11] = np.nan, 120.0, -500.0, np.inf, np.nan
    check(lrm, torch, quats, legs, a.reshape(-1, 3))
    q = (poses(90, 14) * rng.uniform(0.5, 2.0, (90, 1))).astype(F)
    q[5, 1], q[40], q[77, 3] = np.nan, np.nan, np.inf
    check(lrm, torch, q, legs, lc.random_angles(90, 6, seed=15))
    for kw in ({"pen": False}, {"free": False}, {"pen": False, "free": False}):
        check(lrm, torch, quats, legs, ang, **kw)


def test_pair_distance_on_the_device(lrm, torch_cuda):
    """lrm_dbg_link_pair_dist_dev against _host bit for bit: every hand-made kind and the random pairs, and cuts of their
    mixture around one and four waves"""
    torch = torch_cuda
    g = sc.all_pairs()
    mix = g[np.random.default_rng(1).permutation(len(g))]
    for segs in (g, mix[:1], mix[:63], mix[:64], mix[:65], mix[:255], mix[:256], mix[:257]):
        out = torch.full((len(segs),), SENT_F, dtype=torch.float32, device="cuda")
        lrm.device.dbg_link_pair_dist(dev(torch, segs), out)
        torch.cuda.synchronize()
        assert np.array_equal(pc.bits(out.cpu().numpy()), pc.bits(lrm.dbg_link_pair_dist_host(segs)))
    assert lrm.device.dbg_link_pair_dist(torch.empty((0, 12), dtype=torch.float32, device="cuda")).numel() == 0
    for bad in (dev(torch, g[:8]).double(), dev(torch, g[:8])[:, :11], dev(torch, g[:16])[::2], torch.from_numpy(g[:8])):
        with pytest.raises(ValueError):
            lrm.device.dbg_link_pair_dist(bad)
    with pytest.raises(ValueError):
        lrm.device.dbg_link_pair_dist(dev(torch, g[:8]), torch.empty(7, dtype=torch.float32, device="cuda"))


def test_refused_views_and_every_einval(lrm, torch_cuda, main):
    torch = torch_cuda
    quats, _, _, legs, ang = main
    n = len(quats)
    ps = lrm.PoseSet(legs, n, ik=True)
    a = dev(torch, ang.T)
    with pytest.raises(ValueError):
        ps.self_clearance(a, sc.RADIUS)  # before update()
    ps.update(dev(torch, quats))
    ps.self_clearance(a, sc.RADIUS)
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device="cuda")
    wide = dev(torch, np.repeat(ang.T, 2, 1))
    for kw in ({"angles": wide[:, ::2]}, {"angles": a.double()}, {"angles": a.cpu()}, {"angles": a[:2]}, {"angles": a[:, :-1]},
               {"angles": dev(torch, np.zeros((3, 6 * (n + 1)), F))}, {"radius": (1.0, 2.0)}, {"pose_idx": torch.zeros(n, dtype=torch.int64, device="cuda")},
               {"pose_idx": torch.zeros(2 * n, dtype=torch.int32, device="cuda")[::2]}, {"pose_idx": torch.zeros(n - 1, dtype=torch.int32, device="cuda")},
               {"live_in": u8(2 * n)[::2]}, {"live_in": u8(n - 1)}, {"live_in": torch.empty(n, dtype=torch.uint8)},
               {"hits": torch.empty((6, n), dtype=torch.int64, device="cuda")}, {"with_": u8(6, n - 1)}, {"links": u8(6, 2 * n)[:, ::2]},
               {"worst": torch.empty((6, n), dtype=torch.int32, device="cuda")}, {"pen": torch.empty((6, n), dtype=torch.float64, device="cuda")},
               {"free": u8(n - 1)}):
        with pytest.raises(ValueError):
            ps.self_clearance(kw.pop("angles", a), kw.pop("radius", sc.RADIUS), **kw)
    for kw in ({"radius": (1.0, -1.0, 1.0)}, {"radius": (np.nan, 1.0, 1.0)}, {"radius": (1.0, 1.0, np.inf)}, {"margin": -1.0}, {"margin": np.nan},
               {"margin": np.inf}, {"tip_clear": -0.5}, {"tip_clear": np.nan}, {"tip_clear": np.inf}):
        with pytest.raises(lrm.LrmError):
            ps.self_clearance(a, kw.pop("radius", sc.RADIUS), **kw)
    with pytest.raises(ValueError):
        lrm.PoseSet(legs, n).update(dev(torch, quats)).self_clearance(a, sc.RADIUS)  # built without ik=True
    # the C ABI's own checks, in its order; nothing is launched
    L, dp = lrm.load(), lambda t: None if t is None else t.data_ptr()
    out = outputs(torch, 6, n)
    r = np.ascontiguousarray(sc.RADIUS, F)
    ok = dict(ws=ps.workspace, ik=ps.ik_workspace, nposes=n, nl=6, pose_idx=None, ns=n, coxa=a[0], radius=r.ctypes.data, hits=out[0], with_=out[1],
              links=out[2], worst=out[3])

    def rc(**kw):
        v = dict(ok, **kw)
        return L.lrm_self_clearance_posed_dev(dp(v["ws"]), dp(v["ik"]), v["nposes"], v["nl"], dp(v["pose_idx"]), v["ns"], dp(v["coxa"]), dp(a[1]),
                                              dp(a[2]), v["radius"], 0.0, 0.0, None, dp(v["hits"]), dp(v["with_"]), dp(v["links"]), dp(v["worst"]),
                                              dp(out[4]), dp(out[5]), torch.cuda.current_stream().cuda_stream)

    assert rc() == 0
    big = 2 ** 31
    for kw in (dict(nl=0), dict(nl=9), dict(ns=big), dict(nposes=big), dict(ns=2 ** 30, nposes=2 ** 30, nl=8), dict(radius=None), dict(ns=n + 1),
               dict(ws=None), dict(ik=None), dict(coxa=None), dict(hits=None), dict(with_=None), dict(links=None), dict(worst=None)):
        assert rc(**kw) == -1, kw
    assert rc(ns=0, coxa=None, hits=None) == 0  # nsets == 0 is a no-op
    assert L.lrm_dbg_link_pair_dist_dev(None, 3, None, None) == -1 and L.lrm_dbg_link_pair_dist_dev(None, 0, None, None) == 0
    torch.cuda.synchronize()


def test_chain_on_one_pose_set(lrm, torch_cuda):
    """update -> footholds -> ik(check=False) -> self_clearance -> leg_clearance(live_in=free) on ONE PoseSet against the host
    chain"""
    torch = torch_cuda
    legs = sc.legs_n(lrm, 6)
    n = 192
    quats, body, targets = lc.main_scene(lrm, n, 3000, seed=51)
    ps = lrm.PoseSet(legs, n, ik=True, footholds=True).update(dev(torch, quats), dev(torch, body))
    tx, ty, tz = soa(torch, targets)
    best = ps.footholds(tx, ty, tz)[1]
    pi, li = lrm.device.footholds_layout(n, 6, "cuda")
    ang, st = ps.ik(tx, ty, tz, pi, li, target_idx=best.view(-1), check=False)
    got = ps.self_clearance(ang, sc.RADIUS, sc.MARGIN, sc.TIP_CLEAR)
    leg = ps.leg_clearance(tx, ty, tz, ang, lc.RADIUS, lc.MARGIN, lc.TIP_CLEAR, live_in=got[5])
    torch.cuda.synchronize()
    h_ang, _, h_best = lc.stance_angles(lrm, targets, quats, body, legs)
    assert np.array_equal(best.cpu().numpy(), h_best) and np.array_equal(pc.bits(ang.cpu().numpy().T), pc.bits(h_ang))
    want = sc.host(lrm, quats, legs, h_ang)
    sc.assert_same(tuple(t.cpu().numpy() for t in got), want)
    assert 0 < want["free"].sum() < n
    h_leg = lc.host(lrm, targets, quats, body, legs, h_ang, live_in=want["free"])
    lc.assert_same(tuple(t.cpu().numpy() for t in leg), h_leg)
    assert (h_leg["free"] <= want["free"]).all() and 0 < h_leg["free"].sum() < want["free"].sum()


def test_edge_form_against_the_host_chain(lrm, torch_cuda):
    """angles = ik() on foothold_edges()'s best under foothold_edges_layout, pose_idx = edge_a, then edge_b: do the legs fit in
    either pose on the common feet"""
    torch = torch_cuda
    legs = sc.legs_n(lrm, 6)
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
        got = ps.self_clearance(ang, sc.RADIUS, sc.MARGIN, sc.TIP_CLEAR, pose_idx=dedge)
        torch.cuda.synchronize()
        h_ang = lrm.apply_ik_posed_cpu(targets, np.tile(edge, 6), np.repeat(np.arange(6, dtype=np.uint8), ne), quats, body, legs,
                                       target_idx=h_best.reshape(-1))[0]
        assert np.array_equal(pc.bits(ang.cpu().numpy().T), pc.bits(h_ang))
        want = sc.host(lrm, quats, legs, h_ang, pose_idx=edge)
        sc.assert_same(tuple(t.cpu().numpy() for t in got), want)
        assert (want["hits"] > 0).any() and (want["free"] == 1).any()


def test_chain_replays_from_a_graph(lrm, torch_cuda):
    """update(), footholds(), ik(), self_clearance() and leg_clearance() only launch once the box buffer holds the cloud's size:
    the linear chain captured on ONE side stream after a warm call, replayed once after new quaternions, bodies and targets were
    copied into the captured tensors"""
    torch = torch_cuda
    legs = sc.legs_n(lrm, 6)
    n = 128
    q0, b0, t0 = lc.main_scene(lrm, n, 4500, seed=41)
    q1, b1, t1 = lc.main_scene(lrm, n, 4500, seed=42)
    qt, bt, tt = dev(torch, q0), dev(torch, b0), dev(torch, t0.T.copy())
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
    cnt, bst, bd, al = i32(6, n), i32(6, n), torch.empty((6, n), dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    ang, st = torch.empty((3, 6 * n), dtype=torch.float32, device="cuda"), torch.empty(6 * n, dtype=torch.uint8, device="cuda")
    out = outputs(torch, 6, n)
    lh, ll, lw = i32(6, n), torch.empty((6, n), dtype=torch.uint8, device="cuda"), i32(6, n)
    lp, lf = torch.empty((6, n), dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    pi, li = lrm.device.footholds_layout(n, 6, "cuda")
    ps = lrm.PoseSet(legs, n, ik=True, footholds=True)

    def work():
        ps.update(qt, bt)
        ps.footholds(tt[0], tt[1], tt[2], cnt, bst, bd, al)
        ps.ik(tt[0], tt[1], tt[2], pi, li, target_idx=bst.view(-1), out=ang, status=st, check=False)
        ps.self_clearance(ang, sc.RADIUS, sc.MARGIN, sc.TIP_CLEAR, None, None, *out)
        ps.leg_clearance(tt[0], tt[1], tt[2], ang, lc.RADIUS, lc.MARGIN, lc.TIP_CLEAR, out[5], lh, ll, lw, lp, lf)

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
        for t, v in zip(out, (SENT_I, SENT_B, SENT_B, SENT_B, SENT_F, SENT_B)):
            t.fill_(v)
        g.replay()
    torch.cuda.synchronize()
    h_ang = lc.stance_angles(lrm, t1, q1, b1, legs)[0]
    want = sc.host(lrm, q1, legs, h_ang)
    assert (want["hits"] > 0).any() and (want["free"] == 1).any()
    sc.assert_same(tuple(t.cpu().numpy() for t in out), want)
    lc.assert_same((lh.cpu().numpy(), ll.cpu().numpy(), lw.cpu().numpy(), lp.cpu().numpy(), lf.cpu().numpy()),
                   lc.host(lrm, t1, q1, b1, legs, h_ang, live_in=want["free"]))
    del g


def test_two_streams_on_different_sets(lrm, torch_cuda, main):
    """self_clearance uses no shared buffer: two PoseSets answer different sets on two streams at once; both are the host's"""
    torch = torch_cuda
    quats, _, _, legs, ang = main
    n = len(quats)
    q2, a2 = poses(200, 8), lc.random_angles(200, 6, seed=8)
    ps1 = lrm.PoseSet(legs, n, ik=True).update(dev(torch, quats))
    ps2 = lrm.PoseSet(legs, 200, ik=True).update(dev(torch, q2))
    d1, d2 = dev(torch, ang.T), dev(torch, a2.T)
    o1, o2 = outputs(torch, 6, n), outputs(torch, 6, 200)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(s1):
            ps1.self_clearance(d1, sc.RADIUS, sc.MARGIN, sc.TIP_CLEAR, None, None, *o1)
        with torch.cuda.stream(s2):
            ps2.self_clearance(d2, sc.RADIUS_COXA, 0.0, 0.0, None, None, *o2)
    torch.cuda.synchronize()
    sc.assert_same(tuple(t.cpu().numpy() for t in o1), sc.host(lrm, quats, legs, ang))
    sc.assert_same(tuple(t.cpu().numpy() for t in o2), sc.host(lrm, q2, legs, a2, sc.RADIUS_COXA, 0.0, 0.0))
