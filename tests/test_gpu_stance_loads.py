"""Static foot loads and joint torques on the device (run with -m gpu on an MI355X): PoseSet.stance_loads /
lrm_stance_loads_posed_dev against the host loop lrm_stance_loads_posed_cpu bit for bit (status, holdable, peak bits, peak_at,
load bits, tau bits) over set counts around the wave, block and grid-stride boundaries, lift-set counts around the 64-lane
round and around the switch between the lane-per-set and the wave-per-set kernel (both kernels get the set counts), 3 to 8 legs, both planes, a zero and a non-zero centre of mass, tau_max with +inf, dead sets, bad pose indices and nan
angles on every leg lane, the NULL forms of the C ABI and views of longer buffers; the chain update -> footholds -> ik ->
stance_loads -> stance_stability(live_in = a holdable row) on ONE PoseSet against the host chain; one graph replay with new
angles; and the bands of tests/loads_model64.py on the device's own answers.  tests/test_stance_loads_cpu.py ties that host loop
to the float64 model.  Every output is prefilled with a sentinel, so an unwritten entry fails too."""
import os
import re

import numpy as np
import pytest

import leg_clearance_cases as lgc
import loads_cases as lc
import loads_model64 as m64
import pair_cases as pc
import self_clearance_cases as sc

pytestmark = pytest.mark.gpu

F = np.float32
SENT_B, SENT_F = 0xA5, -7.0
WAVES = 4
GRID_SETS = 65536  # kMaxGrid workgroups of four waves, one set per wave
LANE_MASKS = 8  # up to eight lift sets a lane owns a set (stance_loads_lane_kernel), from nine on a wave does
LANE_GRID_SETS = 262144  # kLaneMaxGrid workgroups of 256 lanes, one set per lane
WAVE_LIFT = [0, 1, 2, 3, 4, 5, 6, 7, 0]  # nine lift sets, good for three legs and more
MAPPINGS = {"lane": None, "wave": WAVE_LIFT}  # lift sets that take the one kernel and the other
KEYS = ("status", "holdable", "peak", "peak_at", "load", "tau")


def test_the_constants_are_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged-robot-movability-cuda_amd", "csrc",
                            "lrm_stance_loads.hip")).read()
    assert int(re.search(r"constexpr unsigned kMaxGrid = (\d+);", src).group(1)) * WAVES == GRID_SETS
    assert int(re.search(r"constexpr int kBlock = (\d+);", src).group(1)) == 64 * WAVES
    assert int(re.search(r"constexpr unsigned kLaneMaxGrid = (\d+);", src).group(1)) * 64 * WAVES == LANE_GRID_SETS
    assert int(re.search(r"#define LRM_LOADS_LANE_MAX_MASKS (\d+)", src).group(1)) == LANE_MASKS
    assert len(MAPPINGS["wave"]) == LANE_MASKS + 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def outputs(torch, nm, nl, ns, extra=0):
    full = lambda shape, v, dt: torch.full((int(np.prod(shape)) + extra,), v, dtype=dt, device="cuda")
    return {"status": full((nm, ns), SENT_B, torch.uint8), "holdable": full((nm, ns), SENT_B, torch.uint8),
            "peak": full((nm, ns), SENT_F, torch.float32), "peak_at": full((nm, ns), SENT_B, torch.uint8),
            "load": full((nm, nl, ns), SENT_F, torch.float32), "tau": full((nm, nl, 3, ns), SENT_F, torch.float32)}


def same(got, want):
    for k in KEYS:
        if want[k] is None:
            continue
        g, w = np.ascontiguousarray(got[k]).reshape(want[k].shape), want[k]
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (k, np.argwhere(g.view(w.dtype) != w)[:5])


def run(lrm, torch, quats, legs, angles, lift, tau_max=lc.TAU_MAX, pose_idx=None, com=None, plane=None, live_in=None, drop=(), extra=0):
    """PoseSet.stance_loads into sentinel-filled outputs (drop: the optional outputs passed as NULL; extra: every output is a
    view of a buffer that much longer, whose tail must stay untouched) -> dict of numpy arrays"""
    nl = len(legs)
    ns = len(angles) // nl
    nm = len(lrm.stance_lift(lift, nl))
    qt = dev(torch, np.asarray(quats, F))
    ps = lrm.PoseSet(legs, len(quats), ik=True).update(qt)
    out = outputs(torch, nm, nl, ns, extra)
    give = {k: (None if k in drop else v) for k, v in out.items()}
    ps.stance_loads(dev(torch, np.asarray(angles, F).T), qt, tau_max, dev(torch, pose_idx), com, plane, lift, dev(torch, live_in),
                    give["status"], give["holdable"], give["peak"], give["peak_at"], give["load"], give["tau"],
                    want_peak_at="peak_at" not in drop, want_load="load" not in drop, want_tau="tau" not in drop)
    torch.cuda.synchronize()
    got = {}
    for k, t in out.items():
        a = t.cpu().numpy()
        n = len(a) - extra
        sent = SENT_B if a.dtype == np.uint8 else F(SENT_F)
        assert (a[n:] == sent).all(), k
        if k in drop:
            assert (a == sent).all(), k
        got[k] = a[:n]
    return got


def check(lrm, torch, quats, legs, angles, lift, drop=(), **kw):
    want = lc.host(lrm, quats, legs, angles, lift=lift, **{k: v for k, v in kw.items() if k != "extra"})
    got = run(lrm, torch, quats, legs, angles, lift, drop=drop, **kw)
    for k in drop:
        want[k] = None
    same(got, want)
    return want


def pose_map(ns, nposes, seed):
    return np.random.default_rng(seed).integers(0, nposes, ns).astype(np.int32)


@pytest.mark.parametrize("mapping", ["lane", "wave"])
@pytest.mark.parametrize("ns", [1, 63, 64, 65, 255, 256, 257])
def test_set_counts(lrm, torch_cuda, ns, mapping):
    legs, quats, ang = lc.corpus(lrm, 30 + ns, ns, 6)
    want = check(lrm, torch_cuda, quats[:24] if ns > 24 else quats, legs, ang, MAPPINGS[mapping], pose_idx=pose_map(ns, min(ns, 24), ns),
                 com=lc.COMS[1])
    assert ns < 63 or len(np.unique(want["status"])) >= 2


@pytest.mark.parametrize("mapping", ["lane", "wave"])
def test_set_count_past_the_grid_stride(lrm, torch_cuda, mapping):
    """one set more than the grid keeps in flight: the first lane (262 144 sets), the first wave (65 536) takes a second set"""
    ns = (LANE_GRID_SETS if mapping == "lane" else GRID_SETS) + 1
    legs, quats, ang = lc.corpus(lrm, 7, 512, 6)
    pick = np.random.default_rng(7).integers(0, 512, ns)
    ang = ang.reshape(6, 512, 3)[:, pick].reshape(-1, 3)
    want = check(lrm, torch_cuda, quats, legs, ang, MAPPINGS[mapping], pose_idx=pick.astype(np.int32), com=lc.COMS[1])
    assert 1 <= want["status"][0, -1] <= 4 and set(np.unique(want["status"])) >= {1, 2}


@pytest.mark.parametrize("nm", [1, 2, 7, 8, 9, 63, 64, 65, 256])
def test_lift_set_counts(lrm, torch_cuda, nm):
    """every lane of the first round and the first, the 64th and the last of the later ones"""
    legs, quats, ang = lc.corpus(lrm, 50 + nm, 65, 8, 2)
    lift = np.random.default_rng(nm).permutation(256)[:nm].astype(np.uint8)
    lift[0] = 0
    want = check(lrm, torch_cuda, quats, legs, ang, lift, com=lc.COMS[2])
    assert set(np.unique(want["status"])) >= ({1, 2, 4} if nm > 6 else {1})
    if nm == 256:  # every lift set of eight legs: fewer than three planted feet is status 4
        few = np.array([bin(int(m) ^ 0xff).count("1") < 3 for m in lift])
        assert (want["status"][few] == lrm.LOADS_NONE).all() and (want["status"][~few] != lrm.LOADS_NONE).any()


@pytest.mark.parametrize("nlegs", [3, 4, 6, 8])
@pytest.mark.parametrize("plane", [None, "tilted"])
def test_leg_counts_planes_and_centres_of_mass(lrm, torch_cuda, nlegs, plane):
    plane = None if plane is None else lc.PLANE_TILTED
    legs, quats, ang = lc.corpus(lrm, 70 + nlegs, 130, nlegs, 2 if nlegs == 8 else 0)
    seen, held = set(), []
    for com, tau_max in ((None, lc.TAU_MAX), (lc.COMS[1], [np.inf, np.inf, np.inf]), (lc.COMS[2], [90.0, 40.0, 25.0])):
        want = check(lrm, torch_cuda, quats, legs, ang, "each", com=com, plane=plane, tau_max=tau_max)
        seen |= set(np.unique(want["status"]))
        solved = (want["status"] >= 1) & (want["status"] <= 3)
        if np.isinf(tau_max).all():  # nothing limits: every equilibrium is holdable, the peak is 0
            assert np.array_equal(want["holdable"].astype(bool), solved) and (want["peak"][solved] == 0).all()
        else:
            held += [want["holdable"][solved]]
    held = np.concatenate(held)
    assert seen >= {1, 4} and (nlegs < 6 or 2 in seen) and 0 < held.mean() < 1  # the finite limits hold some stances and not others


def test_the_tripod_stage_on_the_device(lrm, torch_cuda):
    """status 3 is rare: the corpus of tests/test_stance_loads_cpu.py that has one, and the twin legs that force it"""
    legs, quats, ang = lc.corpus(lrm, 108, 600, 8, 2)
    want = check(lrm, torch_cuda, quats, legs, ang, "each", com=lc.COMS[2])
    assert (want["status"] == lrm.LOADS_TRIPOD).any()
    rng = np.random.default_rng(4)
    legs = lc.legs_n(lrm, 4)
    legs[2] = legs[1]
    quat = np.array([[1, 0, 0, 0]], F)
    tripods = 0
    for _ in range(12):
        a = np.column_stack([rng.uniform(-0.7, 0.7, 4), rng.uniform(-0.6, 0.5, 4), rng.uniform(-2.2, -0.6, 4)]).astype(F)
        a[2] = a[1]
        tips = lrm.leg_joints_posed_cpu(a, quat, None, legs)[0][:, 0, 3]
        want = check(lrm, torch_cuda, quat, legs, a, [0, 8], com=((tips[0].astype(np.float64) + tips[1]) / 2).astype(F))
        tripods += int((want["status"] == lrm.LOADS_TRIPOD).sum())
    assert tripods > 0


@pytest.mark.parametrize("lift", [None, WAVE_LIFT])  # a lane per set, a wave per set
@pytest.mark.parametrize("nlegs", [3, 8])
def test_dead_sets_bad_poses_and_nan_angles_on_every_leg_lane(lrm, torch_cuda, nlegs, lift):
    ns = 130
    legs, quats, ang = lc.corpus(lrm, 90 + nlegs, ns, nlegs)
    ang = ang.reshape(nlegs, ns, 3).copy()
    for l in range(nlegs):  # leg l invalid in sets l, l + 8, ..: alone, and together with its neighbour
        ang[l, l::16] = np.nan
        ang[l, 8 + l::16, 1] = np.inf
        ang[(l + 1) % nlegs, 8 + l::16] = [200.0, 0.0, 0.0]
    live = (np.arange(ns) % 5 != 2).astype(np.uint8)
    live[[0, 63, 64, 129]] = [0, 0, 255, 0]
    pose = np.arange(ns, dtype=np.int32)
    pose[[1, 62, 65, 128]] = [-1, ns, np.iinfo(np.int32).min, np.iinfo(np.int32).max]
    want = check(lrm, torch_cuda, quats, legs, ang.reshape(-1, 3), lift, pose_idx=pose, live_in=live, com=lc.COMS[1])
    dead = (live == 0) | np.isin(np.arange(ns), [1, 62, 65, 128])
    assert (want["status"][:, dead] == 0).all() and (want["status"][:, ~dead] != 0).all()
    assert (want["load"][:, 0, 0::16] == 0).all()
    q2 = quats.copy()
    q2[3], q2[4], q2[5] = np.nan, 0, q2[5] * 1.5  # a centre of mass that is not finite is a dead set; a non-unit quaternion is not
    want = check(lrm, torch_cuda, q2, legs, ang.reshape(-1, 3), lift, com=lc.COMS[1])
    assert (want["status"][:, 3] == 0).all() and (want["status"][:, 5] != 0).all()


@pytest.mark.parametrize("lift", [None, WAVE_LIFT])
@pytest.mark.parametrize("drop", [("peak_at",), ("load",), ("tau",), ("peak_at", "load", "tau")])
def test_null_outputs(lrm, torch_cuda, drop, lift):
    legs, quats, ang = lc.corpus(lrm, 12, 70, 6)
    check(lrm, torch_cuda, quats, legs, ang, lift, drop=drop, com=lc.COMS[1])


def test_outputs_may_be_views_of_longer_buffers_and_bad_tensors_are_refused(lrm, torch_cuda):
    torch = torch_cuda
    legs, quats, ang = lc.corpus(lrm, 13, 70, 6)
    check(lrm, torch, quats, legs, ang, "each", extra=5, com=lc.COMS[1])
    check(lrm, torch, quats, legs, ang, WAVE_LIFT, extra=5, com=lc.COMS[1])
    qt, a = dev(torch, quats), dev(torch, ang.T)
    ps = lrm.PoseSet(legs, 70, ik=True).update(qt)
    with pytest.raises(ValueError):
        ps.stance_loads(a, qt, [1.0, 2.0])
    with pytest.raises(ValueError):
        ps.stance_loads(a, qt[:69], lc.TAU_MAX)
    with pytest.raises(ValueError):
        ps.stance_loads(a[:, :-1], qt, lc.TAU_MAX)
    with pytest.raises(ValueError):
        ps.stance_loads(a, qt, lc.TAU_MAX, status=torch.empty(69, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ps.stance_loads(a, qt, lc.TAU_MAX, load=torch.empty((1, 6, 70), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        ps.stance_loads(a, qt, lc.TAU_MAX, live_in=torch.ones(69, dtype=torch.uint8, device="cuda"))
    with pytest.raises(lrm.LrmError):
        ps.stance_loads(a, qt, [1.0, 0.0, 1.0])
    with pytest.raises(ValueError):
        lrm.PoseSet(legs, 70).update(qt).stance_loads(a, qt, lc.TAU_MAX)  # built without ik=True


def test_chain_on_one_pose_set(lrm, torch_cuda):
    """update -> footholds -> ik(check=False) -> stance_loads -> stance_stability(live_in = the holdable row of `nothing
    lifted`) on ONE PoseSet against the host chain"""
    torch = torch_cuda
    legs = sc.legs_n(lrm, 6)
    n = 192
    quats, body, targets = lgc.main_scene(lrm, n, 3000, seed=51)
    qt, bt = dev(torch, quats), dev(torch, body)
    ps = lrm.PoseSet(legs, n, ik=True, footholds=True).update(qt, bt)
    t = dev(torch, np.asarray(targets, F).T)
    best = ps.footholds(t[0], t[1], t[2])[1]
    pi, li = lrm.device.footholds_layout(n, 6, "cuda")
    ang = ps.ik(t[0], t[1], t[2], pi, li, target_idx=best.view(-1), check=False)[0]
    tau_max = [np.inf, 60.0, 30.0]
    got = ps.stance_loads(ang, qt, tau_max, com=lc.COMS[1], lift="each")
    stab = ps.stance_stability(t[0], t[1], t[2], best, qt, bt, com=lc.COMS[1], lift="each", live_in=got[1][0])
    torch.cuda.synchronize()
    h_ang, _, h_best = lgc.stance_angles(lrm, targets, quats, body, legs)
    assert np.array_equal(best.cpu().numpy(), h_best) and np.array_equal(pc.bits(ang.cpu().numpy().T), pc.bits(h_ang))
    want = lc.host(lrm, quats, legs, h_ang, tau_max, com=lc.COMS[1], lift="each")
    same(dict(zip(KEYS, (x.cpu().numpy() for x in got))), want)
    assert 0 < want["holdable"][0].sum() < n
    h_stab = lrm.stance_stability_cpu(targets, h_best, quats, body, com=lc.COMS[1], lift="each", live_in=want["holdable"][0])
    for g, w in zip(stab, h_stab[:4]):
        assert np.array_equal(g.cpu().numpy().view(np.uint8), w.view(np.uint8))
    assert np.isneginf(h_stab[0][:, want["holdable"][0] == 0]).all()


@pytest.mark.parametrize("lift", ["each", WAVE_LIFT])  # a lane per set, a wave per set
def test_replays_from_a_graph_with_new_angles(lrm, torch_cuda, lift):
    torch = torch_cuda
    legs, quats, a0 = lc.corpus(lrm, 21, 128, 6)
    a1 = lc.corpus(lrm, 22, 128, 6)[2]
    qt, ang = dev(torch, quats), dev(torch, a0.T)
    ps = lrm.PoseSet(legs, 128, ik=True).update(qt)
    out = outputs(torch, len(lrm.stance_lift(lift, 6)), 6, 128)
    work = lambda: ps.stance_loads(ang, qt, lc.TAU_MAX, None, lc.COMS[1], None, lift, None, *(out[k] for k in KEYS))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            work()
        ang.copy_(dev(torch, a1.T))
        for k in KEYS:
            out[k].fill_(SENT_B if out[k].dtype == torch.uint8 else SENT_F)
        g.replay()
    torch.cuda.synchronize()
    same({k: out[k].cpu().numpy() for k in KEYS}, lc.host(lrm, quats, legs, a1, com=lc.COMS[1], lift=lift))


def test_the_models_bands_hold_on_the_device(lrm, torch_cuda):
    """the device's own answers against the float64 model, inside the bands measured on the host loop"""
    worst = {}
    for nlegs, mb, plane in ((6, 0, None), (8, 2, lc.PLANE_TILTED)):
        legs, quats, ang = lc.corpus(lrm, 200 + nlegs, 300, nlegs, mb)
        lift = lrm.stance_lift("each", nlegs)
        got = run(lrm, torch_cuda, quats, legs, ang, lift, com=lc.COMS[1], plane=plane)
        got = {k: got[k].reshape(s) for k, s in (("status", (len(lift), 300)), ("load", (len(lift), nlegs, 300)), ("tau", (len(lift), nlegs, 3, 300)))}
        m64.measure(got, m64.statics64(ang, legs, quats, None, lc.COMS[1], plane), lift, worst)
    print({k: float(f"{v:.4g}") for k, v in worst.items()}, m64.BAND)
    assert worst["answers"] > 3000
    for k, band in m64.BAND.items():
        assert worst[k] <= band, (k, worst[k], band)
