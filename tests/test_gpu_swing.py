"""Swing-foot transit on the device (run with -m gpu on an MI355X): device.swing_transit / PoseSet.swing_transit /
lrm_swing_transit_posed_dev against the host loop lrm_swing_transit_posed_cpu bit for bit on EVERY output.  The host loop
consults no box (tests/test_swing_cpu.py ties it to lrm_reach_dist_posed_cpu, lrm_edge_transit_posed_cpu and an independent
float64 model), so equality also holds the terrain kernel's box cull to its promise never to drop a near target.  Edge counts
around a wave's and a workgroup's share; 1, 6 and 8 legs; every S x skip of the lists below; cloud sizes around the chunk, the
tile, the box threshold and one 64-tile round; a cloud 4e6 mm from the origin; targets within a few ulp of foot_radius + margin
from the path and at the cull distance from the path's box; margins of 0 and huge; non-finite inputs; bad indices; live_in; the
NULL forms; the foot_radius = 0 form; the chain on one PoseSet; a graph replay.  Every output is prefilled with a sentinel, so
an unwritten entry fails too."""
import numpy as np
import pytest

import swing_cases as sw
import transit_cases as tr

pytestmark = pytest.mark.gpu

F = np.float32
SENT_B, SENT_I, SENT_F, SENT_M = 0xA5, -7, -7.0, 0x25A5A5A5A5A5A5A5
SENTINELS = {"mask": SENT_M, "reached": SENT_I, "first_miss": SENT_I, "worst": SENT_I, "worst_d2": SENT_F, "hits": SENT_I,
             "hit_seg": SENT_I, "near": SENT_I, "pen": SENT_F, "swinging": SENT_B, "clear": SENT_B}
ALL_S = (2, 3, 5, 9, 33, 63, 64)
ALL_SKIP = (0, 1, 3, 31, 32, 63)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def outputs(torch, nl, ne):
    dt = {"mask": torch.int64, "worst_d2": torch.float32, "pen": torch.float32, "swinging": torch.uint8, "clear": torch.uint8}
    return {k: torch.full((ne,) if k in sw.EDGE_KEYS else (nl, ne), SENTINELS[k], dtype=dt.get(k, torch.int32), device="cuda") for k in sw.KEYS}


def scalars(kw):
    return (kw.get("lift", 0.0), kw.get("up"), kw.get("foot_radius", 0.0), kw.get("margin", 0.0), kw.get("skip", 0))


def run(lrm, torch, scene, S, live_in=None, drop=(), **kw):
    """device.swing_transit into sentinel-filled outputs -> dict of numpy arrays (None for a dropped output)"""
    quats, body, targets, ea, eb, legs, ffrom, fto = scene
    legs = np.asarray(legs, F).reshape(-1, 14)
    nl, ne = len(legs), len(ea)
    t = dev(torch, np.asarray(targets, F).reshape(-1, 3).T)
    q, b = dev(torch, np.asarray(quats, F)), dev(torch, None if body is None else np.asarray(body, F))
    a, bb = dev(torch, np.asarray(ea, np.int32)), dev(torch, np.asarray(eb, np.int32))
    ff, ft = dev(torch, np.asarray(ffrom, np.int32).reshape(nl, ne)), dev(torch, np.asarray(fto, np.int32).reshape(nl, ne))
    lv = dev(torch, None if live_in is None else np.asarray(live_in, np.uint8))
    out = outputs(torch, nl, ne)
    lift, up, fr, margin, skip = scalars(kw)
    if not drop:
        lrm.device.swing_transit(t[0], t[1], t[2], q, b, legs, a, bb, ff, ft, S, lift, up, fr, margin, skip, lv, *(out[k] for k in sw.KEYS))
    else:  # the NULL forms of the C ABI
        dp = lambda x: None if x is None else x.data_ptr()
        upv = None if up is None else np.asarray(up, F)
        rc = lrm.load().lrm_swing_transit_posed_dev(dp(t[0]), dp(t[1]), dp(t[2]), t.shape[1], dp(q), dp(b), len(quats), legs.ctypes.data, nl,
                                                    dp(a), dp(bb), ne, dp(ff), dp(ft), S, lift, None if upv is None else upv.ctypes.data, fr,
                                                    margin, skip, dp(lv), *(None if k in drop else dp(out[k]) for k in sw.KEYS),
                                                    torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    for k in drop:
        assert (out[k] == SENTINELS[k]).all(), k
    return {k: None if k in drop else out[k].cpu().numpy() for k in sw.KEYS}


def check(lrm, torch, scene, S, live_in=None, drop=(), mixed=False, **kw):
    """the device against the host loop, bit for bit -> the host's answer"""
    quats, body, targets, ea, eb, legs, ffrom, fto = scene
    lift, up, fr, margin, skip = scalars(kw)
    want = sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, S, live_in, lift, up, fr, margin, skip)
    if mixed:  # entries that keep the foot and entries that lose it, entries that hit and entries that do not
        swg = want["reached"] >= 0
        assert (swg & (want["reached"] == S)).any() and (swg & (want["reached"] < S)).any()
        assert (swg & (want["hits"] > 0)).any() and (swg & (want["hits"] == 0)).any() and (want["pen"][want["near"] >= 0] < 0).any()
    sw.assert_same(run(lrm, torch, scene, S, live_in, drop, **kw), want)
    return want


@pytest.fixture(scope="module")
def main(lrm):
    return sw.main_scene(lrm)


@pytest.fixture(scope="module")
def big(lrm):
    """past the box threshold: the cull is on"""
    return sw.grid_scene(lrm, 9 * 1024 + 37, 48, 6)


def many_edges(scene, ne, seed=0):
    """ne edges drawn from the scene's, with their feet"""
    quats, body, targets, ea, eb, legs, ffrom, fto = scene
    rng = np.random.default_rng(seed + ne)
    pick = rng.integers(0, len(ea), ne)
    pick[:min(ne, len(ea))] = np.arange(min(ne, len(ea)))
    return quats, body, targets, ea[pick].copy(), eb[pick].copy(), legs, np.ascontiguousarray(ffrom[:, pick]), np.ascontiguousarray(fto[:, pick])


@pytest.mark.parametrize("ne", [1, 3, 4, 5, 63, 64, 65, 257])
def test_edge_counts_around_a_wave_and_a_workgroup(lrm, torch_cuda, main, big, ne):
    """the terrain kernel gives a wave an edge and a workgroup four; the reach kernel packs 64 // S edges into a wave"""
    check(lrm, torch_cuda, many_edges(main, ne), 9, mixed=ne >= 63, **sw.MAIN)
    quats, body, targets, ea, eb, legs, ffrom, fto = many_edges(big, ne)
    check(lrm, torch_cuda, (quats, body, targets, ea, eb, legs) + sw.lift_some(ffrom, fto, 2, seed=ne), 5, **sw.MAIN)


@pytest.mark.parametrize("nl", [1, 6, 8])
def test_leg_counts_every_leg_swinging(lrm, torch_cuda, nl):
    for nt in (3000, 5000):
        check(lrm, torch_cuda, sw.grid_scene(lrm, nt, 21, nl, seed=nl), 9, **sw.MAIN)


@pytest.mark.parametrize("S", ALL_S)
def test_every_sample_count_and_skip(lrm, torch_cuda, main, big, S):
    for skip in ALL_SKIP:
        kw = {**sw.MAIN, "skip": skip}
        want = check(lrm, torch_cuda, main, S, mixed=(S >= 5 and skip == 1), **kw)
        if 2 * skip >= S - 1:
            assert (want["near"] == -1).all()
        elif S >= 5:
            assert (want["near"] >= 0).any()
    quats, body, targets, ea, eb, legs, ffrom, fto = big
    scene = (quats, body, targets, ea, eb, legs) + sw.lift_some(ffrom, fto, 1, seed=S)
    for skip in ALL_SKIP:
        if skip == 0 or 2 * skip < S - 1:
            check(lrm, torch_cuda, scene, S, **{**sw.MAIN, "skip": skip})


@pytest.mark.parametrize("nt", [0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 65600])
def test_cloud_sizes_around_chunk_tile_threshold_and_round(lrm, torch_cuda, nt):
    quats, body, targets, ea, eb, legs, ffrom, fto = sw.grid_scene(lrm, nt, 24, 4, seed=3)
    scene = (quats, body, targets, ea, eb, legs) + sw.lift_some(ffrom, fto, 2, seed=nt)
    want = check(lrm, torch_cuda, scene, 9, **sw.MAIN)
    assert (want["swinging"] != 0).all() == (nt > 0)
    if nt >= 63:
        assert (want["hits"] > 0).any() and (want["near"] >= 0).any()
    if nt >= 1023:  # the last target of the cloud, alone in its chunk past a boundary, is found
        f, t = scene[6].copy(), scene[7].copy()
        l = np.argmax(f[:, 0] >= 0)
        targets = targets.copy()
        A, B = targets[f[l, 0]].astype(np.float64), targets[t[l, 0]].astype(np.float64)
        targets[nt - 1] = (A + 0.5 * (B - A) + [0, 0, 20.0 - 3.0]).astype(F)  # 3 mm under the top of the bump
        if nt - 1 not in (f[l, 0], t[l, 0]):
            want = check(lrm, torch_cuda, (quats, body, targets, ea, eb, legs, f, t), 9, **sw.MAIN)
            assert want["hits"][l, 0] >= 1 and want["pen"][l, 0] > 8.0


def test_a_cloud_far_from_the_origin(lrm, torch_cuda, main):
    quats, body, targets, ea, eb, legs, ffrom, fto = main
    shift = np.array([4e6, -3e6, 1e6], F)
    check(lrm, torch_cuda, (quats, (body + shift).astype(F), (targets + shift).astype(F), ea, eb, legs, ffrom, fto), 9, mixed=True, **sw.MAIN)
    check(lrm, torch_cuda, sw.grid_scene(lrm, 6000, 30, 6, shift=[4e6, 4e6, -4e6]), 9, **sw.MAIN)


def shell_scene(lrm, reach, at_box, seed=0):
    """a 200 mm step along x with a 30 mm bump and 8192 targets in 64-target chunks whose boxes the cull must decide exactly:
    every chunk of the first 48 lies at a distance d from the path (at_box False: beside it in a plane y = const or above it along
    the segments' normals, so d is the computed distance up to rounding) or from the path's BOX (at_box True), with d
    within a few ulp of `reach` (foot_radius + margin), of R = reach * 1.0001 + 1e-5 L and of the values between; x runs
    along the path.  The rest of the cloud is far away.  A is no round number, so t - A rounds."""
    rng = np.random.default_rng(seed)
    A = np.array([0.53, -0.27, 0.11], F)  # small, so that t = A + offset keeps the offset's last bits
    B = (A + np.array([200.0, 0.0, 0.0], F)).astype(F)
    S, lift = 9, 30.0
    P, _ = sw.path_np(A[None], B[None], S, lift)
    P = P[0].astype(np.float64)
    lo, hi = P.min(0), P.max(0)
    L = float((hi - lo).sum())
    R = reach * 1.0001 + 1e-5 * L
    ds = []
    for base in (reach, R, 0.5 * (reach + R)):
        ds += [float(np.nextafter(F(base), F(s), dtype=F)) if k else float(F(base)) for s, k in ((0, 1), (0, 0), (np.inf, 1))]
        ds += [float(F(base) * F(1 - 3e-7)), float(F(base) * F(1 + 3e-7))]
    nt = 8192
    targets = np.empty((nt, 3), np.float64)
    targets[:] = A.astype(np.float64) + [5000.0, 5000.0, 0.0] + rng.uniform(-300, 300, (nt, 3))
    chunk = 0
    for d in ds[:12]:
        for axis, sign in ((1, 1), (1, -1), (2, 1), (2, -1)):
            x = rng.uniform(lo[0], hi[0], 64)
            rows = np.zeros((64, 3))
            rows[:, 0] = x
            if at_box or axis == 1:  # the path lies in the plane y = 0: the distance from it IS the y offset
                rows[:, axis] = (hi[axis] + d) if sign > 0 else (lo[axis] - d)
            elif sign < 0:  # under the bump a neighbouring segment can be nearer: these chunks go sideways too
                rows[:, 1] = -d
            else:  # above the polyline (its convex side): d along the normal of the segment under x, whose foot is then the nearest point
                k = np.clip(np.searchsorted(P[:, 0], x) - 1, 0, S - 2)
                seg = P[k + 1] - P[k]
                normal = np.column_stack([-seg[:, 2], np.zeros(64), seg[:, 0]]) / np.linalg.norm(seg, axis=1)[:, None]
                rows[:, 0], rows[:, 2] = x, np.interp(x, P[:, 0], P[:, 2])
                rows += d * normal
            targets[chunk * 64:(chunk + 1) * 64] = A.astype(np.float64) + rows
            chunk += 1
    targets = np.ascontiguousarray(targets, F)
    targets[nt - 2], targets[nt - 1] = A, B
    quats = np.array([[1, 0, 0, 0], [1, 0, 0, 0]], F)
    body = np.array([A + F([100, 250, 190]), A + F([130, 250, 190])], F)
    legs = lrm.get_M2_leg(F(-np.pi / 2)).astype(F).reshape(1, 14)
    one = lambda v: np.array([[v]], np.int32)
    return (quats, body, targets, np.array([0], np.int32), np.array([1], np.int32), legs, one(nt - 2), one(nt - 1)), S, lift


@pytest.mark.parametrize("at_box", [False, True])
def test_cull_stress_targets_at_the_reach_and_at_the_cull_distance(lrm, torch_cuda, at_box):
    for fr, margin in ((12.0, 15.0), (27.0, 0.0), (0.5, 26.5)):
        scene, S, lift = shell_scene(lrm, fr + margin, at_box, seed=int(fr))
        want = check(lrm, torch_cuda, scene, S, lift=lift, foot_radius=fr, margin=margin, skip=0)
        if at_box:  # these chunks are as far from the path's box as said, and further from the path under its bump
            continue
        # the deepest near target sits a few ulp inside the reach: the shells straddle it, and nothing else is anywhere near
        d = float(F(fr) - want["pen"][0, 0])
        assert want["near"][0, 0] >= 0 and (want["hits"][0, 0] > 0) == (margin == 0) and (fr + margin) * (1 - 2e-6) <= d < fr + margin, d


def test_margins_of_zero_and_huge(lrm, torch_cuda, main, big):
    for margin in (0.0, 1e4, 3e38):  # 3e38: the sum and the cull distance overflow to +inf and nothing is culled
        check(lrm, torch_cuda, main, 9, **{**sw.MAIN, "margin": margin})
        check(lrm, torch_cuda, many_edges(big, 6), 9, **{**sw.MAIN, "margin": margin})
    check(lrm, torch_cuda, many_edges(big, 6), 9, lift=-30.0, up=[0.3, -0.2, 0.8], foot_radius=3e38, margin=0.0, skip=2)
    check(lrm, torch_cuda, main, 9, lift=1e30, foot_radius=12.0, margin=5.0, skip=0)  # a bump that overflows the distances, not the path


def test_nonfinite_targets_quaternions_and_bodies(lrm, torch_cuda, main, big):
    for scene in (main, big):
        hostile, bad = sw.nonfinite_scene(scene)
        for S in (3, 9, 64):
            want = check(lrm, torch_cuda, hostile, S, **sw.MAIN)
            for l, e in bad:
                assert want["reached"][l, e] >= 0 and want["hits"][l, e] == 0 and want["near"][l, e] == -1


def test_bad_indices_at_several_places_in_a_wave(lrm, torch_cuda, big):
    """every leg (a lane of the terrain kernel), and the first, a middle and the last edge slot of the reach kernel's waves"""
    quats, body, targets, ea, eb, legs, ffrom, fto = many_edges(big, 3 * 7)  # S = 9: seven edges per wave
    nt = len(targets)
    bad = [-1, nt, sw.I32.min, sw.I32.max, nt + 1, -2]
    slots = [0, 3, 6, 14, 17, 20]
    for which in (0, 1, 2):
        f, t = ffrom.copy(), fto.copy()
        for k, e in enumerate(slots):
            for l in range(6):
                if which in (0, 2):
                    f[(l + k) % 6, e] = bad[(l + k) % 6] if l % 2 == 0 else f[(l + k) % 6, e]
                if which in (1, 2):
                    t[(l + k) % 6, e] = bad[(l + 2 * k) % 6] if l % 3 != 1 else t[(l + k) % 6, e]
        want = check(lrm, torch_cuda, (quats, body, targets, ea, eb, legs, f, t), 9, **sw.MAIN)
        assert (want["reached"][:, slots] == -1).any() and (want["reached"][:, slots] >= 0).any()
    a, b = tr.hostile_edges(ea, eb, len(quats), slots)
    want = check(lrm, torch_cuda, (quats, body, targets, a, b, legs, ffrom, fto), 9, **sw.MAIN)
    assert (want["swinging"][slots] == 0).all() and (want["clear"][slots] == 0).all()
    f, t = sw.hostile_feet(ffrom, fto, nt)
    check(lrm, torch_cuda, (quats, body, targets, a, b, legs, f, t), 64, **sw.MAIN)


def test_live_in_null_forms_views_and_the_radius_zero_form(lrm, torch_cuda, main, big):
    torch = torch_cuda
    for scene in (main, many_edges(big, 13)):
        ne = len(scene[3])
        live = (np.arange(ne) % 3 != 1).astype(np.uint8)
        want = check(lrm, torch, scene, 9, live, **sw.MAIN)
        assert (want["clear"][live == 0] == 0).all() and (want["reached"][:, live == 0] == -1).all()
        for drop in [(k,) for k in sw.OPTIONAL] + [sw.OPTIONAL]:
            check(lrm, torch, scene, 9, live, drop=drop, **sw.MAIN)
            check(lrm, torch, scene, 9, live, drop=drop, lift=20.0)  # the one-kernel form writes the same rows
        check(lrm, torch, scene[:1] + (None,) + scene[2:], 9, **sw.MAIN)  # body NULL = 0
        zero = check(lrm, torch, scene, 9, lift=20.0, foot_radius=0.0, margin=1e6)  # no terrain test at all
        assert (zero["hits"] == 0).all() and (zero["near"] == -1).all() and (zero["pen"] == -np.inf).all()
    # nt == 0 lets nothing swing
    quats, body, targets, ea, eb, legs, ffrom, fto = main
    got = run(lrm, torch, (quats, body, np.zeros((0, 3), F), ea, eb, legs, ffrom, fto), 9, **sw.MAIN)
    assert (got["reached"] == -1).all() and (got["swinging"] == 0).all() and (got["clear"] == 1).all() and (got["hits"] == 0).all()
    # views: every tensor a slice of a larger buffer at an odd offset
    nl, ne = ffrom.shape
    t = dev(torch, np.concatenate([np.zeros((3, 5), F), targets.T], axis=1))[:, 5:]
    pad = lambda a, dt: torch.cat([torch.zeros(3, dtype=dt, device="cuda"), dev(torch, a).reshape(-1)])[3:].reshape(a.shape)
    q, b = pad(quats, torch.float32), pad(body, torch.float32)
    a, bb, ff, ft = (pad(x, torch.int32) for x in (ea, eb, ffrom, fto))
    store = {k: torch.full((v.numel() + 3,), SENTINELS[k], dtype=v.dtype, device="cuda") for k, v in outputs(torch, nl, ne).items()}
    out = {k: v[3:].reshape((ne,) if k in sw.EDGE_KEYS else (nl, ne)) for k, v in store.items()}
    lrm.device.swing_transit(t[0].contiguous(), t[1].contiguous(), t[2].contiguous(), q, b, legs, a, bb, ff, ft, 9, sw.MAIN["lift"], None,
                             sw.MAIN["foot_radius"], sw.MAIN["margin"], sw.MAIN["skip"], None, *(out[k] for k in sw.KEYS))
    torch.cuda.synchronize()
    sw.assert_same({k: out[k].cpu().numpy() for k in sw.KEYS}, sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, 9, **sw.MAIN))
    for k, v in store.items():
        assert (v[:3] == SENTINELS[k]).all(), k


def test_refusals_and_wrapper_checks(lrm, torch_cuda, main):
    torch = torch_cuda
    quats, body, targets, ea, eb, legs, ffrom, fto = main
    L = lrm.load()
    d = torch.zeros(64, dtype=torch.int32, device="cuda").data_ptr()
    lg = legs.ctypes.data
    nan, inf = float("nan"), float("inf")
    bad_up = np.array([0, nan, 1], F)

    def raw(nt=4, nposes=1, nlegs=2, nedges=1, S=9, lift=10.0, up=None, fr=5.0, margin=1.0, skip=0, tg=d, qs=d, lgs=lg, a=d, b=d, ff=d, ft=d,
            rc=d, fm=d, hi=d, hs=d, nr=d):
        return L.lrm_swing_transit_posed_dev(tg, d, d, nt, qs, None, nposes, lgs, nlegs, a, b, nedges, ff, ft, S, lift, up, fr, margin, skip,
                                             None, None, rc, fm, None, None, hi, hs, nr, None, None, None, None)

    for kw in ({"nlegs": 0}, {"nlegs": 9}, {"S": 1}, {"S": 65}, {"nt": 2 ** 31}, {"nposes": 2 ** 31}, {"nedges": 2 ** 31, "nlegs": 2},
               {"lift": nan}, {"lift": inf}, {"fr": nan}, {"fr": inf}, {"fr": -1.0}, {"margin": nan}, {"margin": inf}, {"margin": -1.0},
               {"skip": 64}, {"up": bad_up.ctypes.data}, {"qs": None}, {"lgs": None}, {"a": None}, {"b": None}, {"ff": None}, {"ft": None},
               {"rc": None}, {"fm": None}, {"hi": None}, {"hs": None}, {"nr": None}, {"tg": None}):
        assert raw(**kw) == -1, kw
    assert raw(nedges=0, skip=64) == -1 and raw(nedges=0, fr=-1.0) == -1  # the scalars are checked before the no-op
    assert raw(nedges=0, qs=None, a=None, rc=None, hi=None) == 0
    t = dev(torch, targets.T.copy())
    q, b = dev(torch, quats), dev(torch, body)
    a, bb, ff, ft = dev(torch, ea), dev(torch, eb), dev(torch, ffrom), dev(torch, fto)
    call = lambda **kw: lrm.device.swing_transit(t[0], t[1], t[2], kw.pop("quats", q), kw.pop("body", b), kw.pop("legs", legs),
                                                 kw.pop("ea", a), kw.pop("eb", bb), kw.pop("ff", ff), kw.pop("ft", ft), **kw)
    for kw in ({"quats": q[:, :3]}, {"quats": q.double()}, {"body": b[:-1]}, {"legs": np.zeros((9, 14), F)}, {"eb": bb[:-1]},
               {"ea": a.long()}, {"ff": ff[:5]}, {"ft": ft.T}, {"ft": ft.long()}, {"live_in": torch.zeros(3, dtype=torch.uint8, device="cuda")},
               {"hits": torch.zeros(5, dtype=torch.int32, device="cuda")}, {"pen": torch.zeros((6, 48), dtype=torch.int32, device="cuda")},
               {"clear": torch.zeros(48, dtype=torch.uint8)}, {"up": [0, 1]}, {"skip": 64}, {"skip": -1}):
        with pytest.raises(ValueError):
            call(**kw)
    for kw in ({"nsamples": 65}, {"foot_radius": -1.0}, {"margin": nan}, {"lift": inf}, {"up": [0, inf, 1]}):
        with pytest.raises(lrm.LrmError):
            call(**kw)
    ps = lrm.PoseSet(legs, len(quats)).update(q, b)
    bad = a.clone()
    bad[3] = len(quats)
    with pytest.raises(ValueError):
        ps.swing_transit(t[0], t[1], t[2], q, b, bad, bb, ff, ft)
    with pytest.raises(ValueError):
        ps.swing_transit(t[0], t[1], t[2], q[:-1], None, a, bb, ff, ft)
    got = ps.swing_transit(t[0], t[1], t[2], q, b, bad, bb, ff, ft, check=False, **sw.MAIN)
    torch.cuda.synchronize()
    assert (got[1][:, 3] == -1).all() and got[10][3] == 0 and got[9][3] == 0


def test_chain_on_one_pose_set_against_the_host_chain(lrm, torch_cuda, main):
    """update -> footholds -> foothold_edges -> edge_transit -> swing_layout -> swing_transit(live_in = clear) on one PoseSet"""
    torch = torch_cuda
    quats, body, targets, ea, eb, legs, ffrom, fto = main
    nominal = sw.pc.nominal_for(6)
    t = dev(torch, targets.T.copy())
    q, b, a, bb = dev(torch, quats), dev(torch, body), dev(torch, ea), dev(torch, eb)
    ps = lrm.PoseSet(legs, len(quats), footholds=True, nominal=nominal).update(q, b)
    _, best, _, _ = ps.footholds(t[0], t[1], t[2])
    _, common, _, _ = ps.foothold_edges(t[0], t[1], t[2], a, bb, check=False)
    lift_mask = dev(torch, (1 << (np.arange(len(ea)) % 6)).astype(np.uint8))
    ff, ft = lrm.swing_layout(best, a, bb, lift_mask)
    assert np.array_equal(ff.cpu().numpy(), ffrom) and np.array_equal(ft.cpu().numpy(), fto)
    planted = torch.where(ff >= 0, torch.full_like(common, -1), common)  # the other five legs stay on their common foothold
    transit = ps.edge_transit(t[0], t[1], t[2], q, b, a, bb, planted, 9, check=False)
    out = ps.swing_transit(t[0], t[1], t[2], q, b, a, bb, ff, ft, 9, live_in=transit[6], check=False, **sw.MAIN)
    torch.cuda.synchronize()
    h_common, _ = tr.foot_of(lrm, targets, quats, body, legs, nominal, ea, eb)
    h_transit = tr.host(lrm, targets, quats, body, legs, ea, eb, np.where(ffrom >= 0, -1, h_common), 9)
    want = sw.host(lrm, targets, quats, body, legs, ea, eb, ffrom, fto, 9, h_transit["clear"], **sw.MAIN)
    sw.assert_same(dict(zip(sw.KEYS, (x.cpu().numpy() for x in out))), want)
    assert (h_transit["clear"] == 1).sum() >= 4 and ((h_transit["clear"] == 1) & (want["clear"] == 0)).any()


def test_call_replays_from_a_graph(lrm, torch_cuda, big):
    """after a warm call on the largest cloud the box buffer has its size and the call only launches: captured on a side stream
    through PoseSet.swing_transit(check=False), replayed once after new foot_from / foot_to were copied into the captured
    tensors; the answers are the host's for the new feet"""
    torch = torch_cuda
    quats, body, targets, ea, eb, legs, ffrom, fto = big
    f0, t0 = sw.lift_some(ffrom, fto, 2, seed=1)
    f1, t1 = sw.lift_some(np.roll(fto, 5, axis=1), np.roll(ffrom, 3, axis=1), 3, seed=2)
    t = dev(torch, targets.T.copy())
    q, b, a, bb, ff, ft = dev(torch, quats), dev(torch, body), dev(torch, ea), dev(torch, eb), dev(torch, f0), dev(torch, t0)
    ps = lrm.PoseSet(legs, len(quats)).update(q, b)
    out = outputs(torch, 6, len(ea))
    work = lambda: ps.swing_transit(t[0], t[1], t[2], q, b, a, bb, ff, ft, 9, sw.MAIN["lift"], None, sw.MAIN["foot_radius"], sw.MAIN["margin"],
                                    sw.MAIN["skip"], None, *(out[k] for k in sw.KEYS), check=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()
    torch.cuda.synchronize()
    sw.assert_same({k: out[k].cpu().numpy() for k in sw.KEYS}, sw.host(lrm, targets, quats, body, legs, ea, eb, f0, t0, 9, **sw.MAIN))
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            work()
        ff.copy_(dev(torch, f1))
        ft.copy_(dev(torch, t1))
        for k in sw.KEYS:
            out[k].fill_(SENTINELS[k])
        g.replay()
    torch.cuda.synchronize()
    want = sw.host(lrm, targets, quats, body, legs, ea, eb, f1, t1, 9, **sw.MAIN)
    assert (want["hits"] > 0).any() and (want["reached"] >= 0).sum() > 100
    sw.assert_same({k: out[k].cpu().numpy() for k in sw.KEYS}, want)
    del g
