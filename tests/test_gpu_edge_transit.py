"""Planted-foot reach along pose transitions on the device (run with -m gpu on an MI355X): device.edge_transit /
PoseSet.edge_transit / lrm_edge_transit_posed_dev against the host loop lrm_edge_transit_posed_cpu bit for bit on every output
(tests/test_edge_transit_cpu.py ties that host loop to lrm_reach_dist_posed_cpu on a numpy restatement of include/lrm.h):
edge counts around an edge slot, a wave and the grid cap; every S at which the number of edges per wave changes; 1 to 8 legs;
dead edges, unplanted legs and bad indices at the first, a middle and the last edge slot of a wave and of the grid; every CPU
scene; the NULL forms and refusals of the C ABI; the chain update -> footholds -> foothold_edges -> edge_transit ->
stance_stability(live_in = clear) on ONE PoseSet against the host chain; a graph replay; and the device's sampled path straight
against the float64 model of tests/transit_model64.py with the bands measured on the CPU.  Every output is prefilled with a
sentinel, so an unwritten entry fails too."""
import os
import re

import numpy as np
import pytest

import foothold_edges_cases as fe
import pair_cases as pc
import transit_cases as tr
import transit_model64 as t64
from test_edge_transit_cpu import BANDS
from test_pair_cpu import FAMILIES

pytestmark = pytest.mark.gpu

F = np.float32
SENT_B, SENT_I, SENT_F, SENT_M = 0xA5, -7, -7.0, 0x25A5A5A5A5A5A5A5
MAX_GRID = 2560  # kMaxGrid workgroups of one wave, 64 // S edges each
EDGE_S = (2, 3, 4, 7, 8, 9, 16, 21, 22, 31, 32, 33, 63, 64)  # 64 // S changes between neighbours


def test_the_constants_are_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged-robot-movability-cuda_amd", "csrc",
                            "lrm_edge_transit.hip")).read()
    assert int(re.search(r"constexpr unsigned kMaxGrid = (\d+);", src).group(1)) == MAX_GRID
    assert int(re.search(r"constexpr int kBlock = (\d+);", src).group(1)) == 64
    assert [64 // s for s in EDGE_S] == [32, 21, 16, 9, 8, 7, 4, 3, 2, 2, 2, 1, 1, 1]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def outputs(torch, nl, ne):
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    return {"mask": full((nl, ne), SENT_M, torch.int64), "reached": full((nl, ne), SENT_I, torch.int32),
            "first_miss": full((nl, ne), SENT_I, torch.int32), "worst": full((nl, ne), SENT_I, torch.int32),
            "worst_d2": full((nl, ne), SENT_F, torch.float32), "planted": full((ne,), SENT_B, torch.uint8),
            "clear": full((ne,), SENT_B, torch.uint8), "advance": full((ne,), SENT_I, torch.int32)}


SENTINELS = {"mask": SENT_M, "reached": SENT_I, "first_miss": SENT_I, "worst": SENT_I, "worst_d2": SENT_F, "planted": SENT_B,
             "clear": SENT_B, "advance": SENT_I}


def run(lrm, torch, targets, quats, body, legs, ea, eb, foot, S, live_in=None, drop=()):
    """device.edge_transit into sentinel-filled outputs -> dict of numpy arrays (None for a dropped output)"""
    legs = np.asarray(legs, F).reshape(-1, 14)
    nl, ne = len(legs), len(ea)
    t = dev(torch, np.asarray(targets, F).reshape(-1, 3).T)
    q, b = dev(torch, np.asarray(quats, F)), dev(torch, None if body is None else np.asarray(body, F))
    a, bb = dev(torch, np.asarray(ea, np.int32)), dev(torch, np.asarray(eb, np.int32))
    fo = dev(torch, np.asarray(foot, np.int32).reshape(nl, ne))
    lv = dev(torch, None if live_in is None else np.asarray(live_in, np.uint8))
    out = outputs(torch, nl, ne)
    if not drop:
        lrm.device.edge_transit(t[0], t[1], t[2], q, b, legs, a, bb, fo, S, lv, *(out[k] for k in tr.KEYS))
    else:  # the NULL forms of the C ABI
        dp = lambda x: None if x is None else x.data_ptr()
        rc = lrm.load().lrm_edge_transit_posed_dev(dp(t[0]), dp(t[1]), dp(t[2]), t.shape[1], dp(q), dp(b), len(quats), legs.ctypes.data, nl, dp(a),
                                                   dp(bb), ne, dp(fo), S, dp(lv), *(None if k in drop else dp(out[k]) for k in tr.KEYS),
                                                   torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    for k in drop:
        assert (out[k] == SENTINELS[k]).all(), k
    return {k: None if k in drop else out[k].cpu().numpy() for k in tr.KEYS}


def check(lrm, torch, targets, quats, body, legs, ea, eb, foot, S, live_in=None, mixed=True, drop=()):
    """the device against the host loop, bit for bit -> the host's answer"""
    want = tr.host(lrm, targets, quats, body, legs, ea, eb, foot, S, live_in)
    if mixed:  # entries that keep the foot and entries that lose it
        pl = want["reached"] >= 0
        assert (pl & (want["reached"] == S)).any() and (pl & (want["reached"] < S)).any()
    tr.assert_same(run(lrm, torch, targets, quats, body, legs, ea, eb, foot, S, live_in, drop), want)
    return want


@pytest.fixture(scope="module")
def main(lrm):
    quats, body, targets, ea, eb, legs, nominal = tr.main_scene(lrm)
    foot, _ = tr.foot_of(lrm, targets, quats, body, legs, nominal, ea, eb)
    return quats, body, targets, ea, eb, legs, foot


def many_edges(main, ne, nl=6, seed=0):
    """ne edges drawn from the main scene's 48 (with their feet), a tenth of the feet replaced by a random target"""
    quats, body, targets, ea, eb, legs, foot = main
    rng = np.random.default_rng(seed + ne)
    pick = rng.integers(0, len(ea), ne)
    pick[:min(ne, len(ea))] = np.arange(min(ne, len(ea)))
    f = foot[:nl, pick].copy()
    swap = rng.random(f.shape) < 0.1
    f[swap] = rng.integers(0, len(targets), int(swap.sum()))
    return ea[pick].copy(), eb[pick].copy(), np.ascontiguousarray(f)


@pytest.mark.parametrize("S", EDGE_S)
def test_edge_counts_around_an_edge_slot_and_a_wave(lrm, torch_cuda, main, S):
    """nedges 1, one wave's worth of edge slots - 1 .. + 1, and two waves' worth + 1"""
    quats, body, targets, _, _, legs, _ = main
    per = 64 // S
    for ne in sorted({1, max(1, per - 1), per, per + 1, 2 * per + 1}):
        ea, eb, foot = many_edges(main, ne)
        check(lrm, torch_cuda, targets, quats, body, legs, ea, eb, foot, S, mixed=ne >= 7)


@pytest.mark.parametrize("nl", range(1, 9))
def test_one_to_eight_legs(lrm, torch_cuda, main, nl):
    quats, body, targets, _, _, _, _ = main
    legs = np.stack([lrm.get_M2_leg(np.float32(2 * np.pi * k / nl)) for k in range(nl)]).astype(F)
    ea, eb = fe.edges_of(48, 13, extra=False)
    foot, _ = tr.foot_of(lrm, targets, quats, body, legs, pc.nominal_for(nl), ea, eb)
    check(lrm, torch_cuda, targets, quats, body, legs, ea, eb, foot, 9, mixed=nl >= 3)


def test_edge_count_past_the_grid_stride(lrm, torch_cuda, main):
    """S = 33: one edge per wave; kMaxGrid workgroups hold kMaxGrid edges, a workgroup and one more make the first two take a
    second round.  Dead edges, unplanted legs and bad indices sit at the first, a middle and the last slot of the grid."""
    quats, body, targets, _, _, legs, _ = main
    ne = MAX_GRID + 2
    ea, eb, foot = many_edges(main, ne, nl=1)
    spots = [0, 1, MAX_GRID // 2, MAX_GRID - 1, MAX_GRID, MAX_GRID + 1]
    live = np.ones(ne, np.uint8)
    live[spots[0]], live[spots[3]] = 0, 0
    foot[0, spots[1]], foot[0, spots[4]] = -1, len(targets)
    ea[spots[2]], eb[spots[5]] = len(quats), -1
    want = check(lrm, torch_cuda, targets, quats, body, legs[:1], ea, eb, foot, 33, live)
    assert (want["reached"][0, spots] == -1).all() and (want["clear"][[spots[1], spots[4]]] == 1).all()
    assert (want["clear"][[spots[0], spots[2], spots[3], spots[5]]] == 0).all()


@pytest.mark.parametrize("S", [9, 21, 64])
def test_dead_unplanted_and_bad_at_the_slots_of_a_wave(lrm, torch_cuda, main, S):
    """three waves' worth of edges; in turn a dead edge, an unplanted leg (every leg once), a bad end and a bad foot at the
    first, a middle and the last edge slot of the first and the last wave"""
    quats, body, targets, _, _, legs, _ = main
    per = 64 // S
    ne = 3 * per
    slots = sorted({0, per // 2, per - 1, 2 * per, 2 * per + per // 2, 3 * per - 1})
    for kind in ("dead", "air", "end", "foot"):
        ea, eb, foot = many_edges(main, ne, seed=S)
        live = None
        if kind == "dead":
            live = np.ones(ne, np.uint8)
            live[slots] = 0
        elif kind == "air":
            for k, e in enumerate(slots):
                foot[k % 6, e] = -1
        elif kind == "end":
            ea, eb = tr.hostile_edges(ea, eb, len(quats), slots)
        else:
            for k, e in enumerate(slots):
                foot[(k + 3) % 6, e] = [len(targets), np.iinfo(np.int32).min, np.iinfo(np.int32).max][k % 3]
        check(lrm, torch_cuda, targets, quats, body, legs, ea, eb, foot, S, live, mixed=False)


def test_a_single_planted_leg_decides_alone(lrm, torch_cuda, main):
    quats, body, targets, ea, eb, legs, foot = main
    for l in (0, 5):
        one = np.full_like(foot, -1)
        one[l] = np.where(foot[l] >= 0, foot[l], 0)
        want = check(lrm, torch_cuda, targets, quats, body, legs, ea, eb, one, 9)
        assert (want["planted"] == 1 << l).all() and np.array_equal(want["clear"], (want["reached"][l] == 9).astype(np.uint8))
        assert np.array_equal(want["advance"], np.where(want["first_miss"][l] >= 0, want["first_miss"][l], 9))
    none = check(lrm, torch_cuda, targets, quats, body, legs, ea, eb, np.full_like(foot, -1), 9, mixed=False)
    assert (none["clear"] == 1).all() and (none["advance"] == 9).all()


@pytest.mark.parametrize("S", [2, 3, 9, 33, 64])
def test_main_scene_and_pure_translation(lrm, torch_cuda, main, S):
    quats, body, targets, ea, eb, legs, foot = main
    check(lrm, torch_cuda, targets, quats, body, legs, ea, eb, foot, S, mixed=S > 2)
    q2, b2, t2, a2, e2, l2, nominal = tr.main_scene(lrm, rotate=False)
    f2, _ = tr.foot_of(lrm, t2, q2, b2, l2, nominal, a2, e2)
    check(lrm, torch_cuda, t2, q2, b2, l2, a2, e2, f2, S, mixed=S > 2)
    check(lrm, torch_cuda, targets, quats, None, legs, ea, eb, foot, S, mixed=False)  # body NULL = 0


@pytest.mark.parametrize("family", FAMILIES)
def test_every_leg_family_on_the_hostile_pose_pool(lrm, torch_cuda, family):
    legs, _ = pc.leg_families(lrm)[family]
    legs = np.ascontiguousarray(legs, F).reshape(-1, 14)
    quats, body, targets, ea, eb = fe.scene(lrm, 48, 4000, seed=len(family) + len(legs))
    foot, _ = tr.foot_of(lrm, targets, quats, body, legs, pc.nominal_for(len(legs)), ea, eb)
    check(lrm, torch_cuda, targets, quats, body, legs, ea, eb, foot, 9, mixed=False)
    own = np.tile(np.arange(len(ea), dtype=np.int32) % len(targets), (len(legs), 1))  # nan and non-unit ends are evaluated
    check(lrm, torch_cuda, targets, quats, body, legs, ea, eb, own, 9, mixed=False)


@pytest.mark.parametrize("kind", ["dense_cluster", "sparse_tiles"])
def test_every_scene(lrm, torch_cuda, kind):
    legs = tr.m2_legs(lrm)
    quats, body, targets, ea, eb = fe.scene(lrm, 40, 6000 if kind == "dense_cluster" else 9 * 1024, seed=2, kind=kind)
    foot, _ = tr.foot_of(lrm, targets, quats, body, legs, pc.nominal_for(6, seed=5), ea, eb)
    for S in (3, 9, 33):
        check(lrm, torch_cuda, targets, quats, body, legs, ea, eb, foot, S, mixed=False)


def test_degenerate_quaternions_and_nonfinite_bodies_and_targets(lrm, torch_cuda, main):
    _, body, targets, ea, eb, legs, foot = main
    rng = np.random.default_rng(5)
    quats = np.zeros((len(body), 4), F)
    quats[:, 0] = 1
    pool = np.array([[1, 0, 0, 0], [-1, 0, 0, 0], [0, 0, 0, 0], [np.nan, 0, 0, 0], [np.inf, 0, 0, 0], [3e38, 3e38, 0, 0],
                     [1e-30, 0, 1e-30, 0], [0, 1, 0, 0], [0, -1, 0, 0], [2, 0, 0, 0.5], [1e20, 0, 0, -1e20]], F)
    quats[ea] = pool[rng.integers(0, len(pool), len(ea))]
    quats[eb] = pool[rng.integers(0, len(pool), len(eb))]
    own = np.where(foot >= 0, foot, 0)
    body, targets = body.copy(), targets.copy()
    body[ea[0]], body[eb[1]] = np.nan, np.inf
    body[ea[2]] += F(4e6)
    targets[own[0, 3]], targets[own[1, 4]] = np.nan, -np.inf
    for S in (3, 9, 64):
        check(lrm, torch_cuda, targets, quats, body, legs, ea, eb, own, S, mixed=False)


def test_live_in_and_null_forms_through_the_c_abi(lrm, torch_cuda, main):
    quats, body, targets, ea, eb, legs, foot = main
    live = (np.arange(len(ea)) % 3 != 1).astype(np.uint8)
    check(lrm, torch_cuda, targets, quats, body, legs, ea, eb, foot, 9, live)
    optional = ("mask", "worst", "worst_d2", "planted", "clear", "advance")
    for drop in [(k,) for k in optional] + [optional]:
        check(lrm, torch_cuda, targets, quats, body, legs, ea, eb, tr.hostile_feet(foot, len(targets)), 9, live, drop=drop)
    # nt == 0 plants nothing
    got = run(lrm, torch_cuda, np.zeros((0, 3), F), quats, body, legs, ea, eb, foot, 9)
    assert (got["reached"] == -1).all() and (got["planted"] == 0).all() and (got["clear"] == 1).all() and (got["advance"] == 9).all()


def test_refusals_and_wrapper_checks(lrm, torch_cuda, main):
    torch = torch_cuda
    quats, body, targets, ea, eb, legs, foot = main
    L = lrm.load()
    d = torch.zeros(64, dtype=torch.int32, device="cuda").data_ptr()
    lg = legs.ctypes.data

    def raw(nt=4, nposes=1, nlegs=2, nedges=1, S=9, tg=d, qs=d, lgs=lg, a=d, b=d, ft=d, rc=d, fm=d):
        return L.lrm_edge_transit_posed_dev(tg, d, d, nt, qs, None, nposes, lgs, nlegs, a, b, nedges, ft, S, None, None, rc, fm, None, None,
                                            None, None, None, None)

    for kw in ({"nlegs": 0}, {"nlegs": 9}, {"S": 1}, {"S": 65}, {"nt": 2 ** 31}, {"nposes": 2 ** 31}, {"nedges": 2 ** 31, "nlegs": 2},
               {"qs": None}, {"lgs": None}, {"a": None}, {"b": None}, {"ft": None}, {"rc": None}, {"fm": None}, {"tg": None}):
        assert raw(**kw) == -1, kw
    assert raw(nedges=0, qs=None, a=None, rc=None) == 0
    t = dev(torch, targets.T.copy())
    q, b = dev(torch, quats), dev(torch, body)
    a, bb, fo = dev(torch, ea), dev(torch, eb), dev(torch, foot)
    call = lambda **kw: lrm.device.edge_transit(t[0], t[1], t[2], kw.pop("quats", q), kw.pop("body", b), kw.pop("legs", legs),
                                                kw.pop("ea", a), kw.pop("eb", bb), kw.pop("foot", fo), **kw)
    for kw in ({"quats": q[:, :3]}, {"quats": q.double()}, {"body": b[:-1]}, {"legs": np.zeros((9, 14), F)}, {"eb": bb[:-1]},
               {"ea": a.long()}, {"foot": fo[:5]}, {"foot": fo.T}, {"live_in": torch.zeros(3, dtype=torch.uint8, device="cuda")},
               {"reached": torch.zeros(5, dtype=torch.int32, device="cuda")}, {"mask": torch.zeros((6, 48), dtype=torch.int32, device="cuda")},
               {"clear": torch.zeros(48, dtype=torch.uint8)}):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(lrm.LrmError):
        call(nsamples=65)
    ps = lrm.PoseSet(legs, len(quats)).update(q, b)
    bad = a.clone()
    bad[3] = len(quats)
    with pytest.raises(ValueError):
        ps.edge_transit(t[0], t[1], t[2], q, b, bad, bb, fo)
    with pytest.raises(ValueError):
        ps.edge_transit(t[0], t[1], t[2], q[:-1], None, a, bb, fo)
    got = ps.edge_transit(t[0], t[1], t[2], q, b, bad, bb, fo, check=False)
    torch.cuda.synchronize()
    assert (got[1][:, 3] == -1).all() and got[6][3] == 0


def test_chain_on_one_pose_set_against_the_host_chain(lrm, torch_cuda, main):
    """update -> footholds -> foothold_edges(check=False) -> edge_transit -> stance_stability(live_in = clear)"""
    torch = torch_cuda
    quats, body, targets, ea, eb, legs, _ = main
    nominal = pc.nominal_for(6)
    t = dev(torch, targets.T.copy())
    q, b, a, bb = dev(torch, quats), dev(torch, body), dev(torch, ea), dev(torch, eb)
    ps = lrm.PoseSet(legs, len(quats), footholds=True, nominal=nominal).update(q, b)
    ps.footholds(t[0], t[1], t[2])
    _, best, _, all_legs = ps.foothold_edges(t[0], t[1], t[2], a, bb, check=False)
    out = ps.edge_transit(t[0], t[1], t[2], q, b, a, bb, best, 9, check=False)
    margin, edge, stable, feet = ps.stance_stability(t[0], t[1], t[2], best, q, b, pose_idx=bb, live_in=out[6])
    torch.cuda.synchronize()
    h_best, h_all = tr.foot_of(lrm, targets, quats, body, legs, nominal, ea, eb)
    assert np.array_equal(best.cpu().numpy(), h_best) and np.array_equal(all_legs.cpu().numpy(), h_all)
    want = tr.host(lrm, targets, quats, body, legs, ea, eb, h_best, 9)
    tr.assert_same(dict(zip(tr.KEYS, (x.cpu().numpy() for x in out))), want)
    feasible = h_all != 0
    assert (feasible & (want["clear"] == 0)).sum() >= 6 and (feasible & (want["clear"] == 1)).sum() >= 4
    hm, he, hs, hf, _ = lrm.stance_stability_cpu(targets, h_best, quats, body, pose_idx=eb, live_in=want["clear"])
    assert np.array_equal(pc.bits(margin.cpu().numpy()), pc.bits(hm)) and np.array_equal(edge.cpu().numpy(), he)
    assert np.array_equal(stable.cpu().numpy(), hs) and np.array_equal(feet.cpu().numpy(), hf)


def test_call_replays_from_a_graph(lrm, torch_cuda, main):
    """the call only launches: captured on a side stream after a warm call, replayed once after new poses, edges and feet were
    copied into the captured tensors"""
    torch = torch_cuda
    quats, body, targets, ea, eb, legs, foot = main
    q1, b1, t1, a1, e1, _, nominal = tr.main_scene(lrm, rotate=False)
    a1, e1 = e1.copy(), a1.copy()  # and the edges the other way round
    f1, _ = tr.foot_of(lrm, t1, q1, b1, legs, nominal, a1, e1)
    t = dev(torch, targets.T.copy())
    q, b, a, bb, fo = dev(torch, quats), dev(torch, body), dev(torch, ea), dev(torch, eb), dev(torch, foot)
    out = outputs(torch, 6, len(ea))
    work = lambda: lrm.device.edge_transit(t[0], t[1], t[2], q, b, legs, a, bb, fo, 9, None, *(out[k] for k in tr.KEYS))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            work()
        for dst, src in ((q, q1), (b, b1), (t, t1.T.copy()), (a, a1), (bb, e1), (fo, f1)):
            dst.copy_(dev(torch, src))
        for k in tr.KEYS:
            out[k].fill_(SENTINELS[k])
        g.replay()
    torch.cuda.synchronize()
    want = tr.host(lrm, t1, q1, b1, legs, a1, e1, f1, 9)
    assert ((want["reached"] >= 0) & (want["reached"] < 9)).any()
    tr.assert_same({k: out[k].cpu().numpy() for k in tr.KEYS}, want)
    del g


@pytest.mark.parametrize("n", [1, 9, 257])
def test_the_device_against_the_float64_model(lrm, torch_cuda, n):
    """the device's sampled path straight against tests/transit_model64.py with the bands measured on the CPU, and against the
    host's samples bit for bit"""
    torch = torch_cuda
    edges = t64.random_edges(n, seed=n)

    def device_samples(quats, body, ea, eb, S):
        got = lrm.device.dbg_edge_transit_samples(dev(torch, quats), dev(torch, body), dev(torch, ea), dev(torch, eb), S)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), lrm.dbg_edge_transit_samples_host(quats, body, ea, eb, S).view(np.uint32))
        return got

    for S in (3, 9, 64):
        got = t64.table(edges, device_samples, S)
        print(n, S, got)
        for k, band in BANDS.items():
            assert got[k] <= band, (n, S, k, got[k], band)
