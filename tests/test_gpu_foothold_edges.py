"""Common-foothold counts and choice per pose transition on the device (run with -m gpu on an MI355X):
PoseSet.foothold_edges / lrm_foothold_edges_posed_dev against the host loop lrm_foothold_edges_posed_cpu bit for bit
(count, best, best_d2 bits, all_legs) over cloud sizes, edge counts, leg counts, quaternion kinds, edge shapes, bad
indices, NULL outputs and the scenes that make each cull reject and accept (tests/test_foothold_edges_cpu.py ties that
host loop to a brute force over the oracle); one scale case against the oracle directly; the chain update -> footholds
-> foothold_edges -> ik on ONE PoseSet; and a graph capture of update() + foothold_edges().  Every output is prefilled
with a sentinel, so an unwritten entry fails too."""
import numpy as np
import pytest

import foothold_edges_cases as fe
import footholds_posed_cases as fc
import pair_cases as pc
import posed_cases
from conftest import reference_terrain

pytestmark = pytest.mark.gpu

SENTINEL = -7
TILE, GROUP, GRID_EDGES = 1024, 64, 16384 * 4  # targets per tile, tiles per outer iteration, edges per grid stride


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def test_constants_match_the_kernel():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged-robot-movability-cuda_amd",
                            "csrc", "lrm_footholds_posed.hip")).read()
    assert int(re.search(r"constexpr int kTargetTile = (\d+);", src).group(1)) == TILE
    assert int(re.search(r"tg0 < ntiles; tg0 \+= (\d+)\)", src).group(1)) == GROUP  # the edge kernel's own loop
    assert int(re.search(r"constexpr unsigned kMaxGrid = (\d+);", src).group(1)) * 4 == GRID_EDGES


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def soa(torch, pts):
    t = dev(torch, np.asarray(pts, np.float32).reshape(-1, 3).T)
    return t[0], t[1], t[2]


def run(lrm, torch, targets, quats, body, legs, nominal, ea, eb, d2=True, all_legs=True, ps=None, check=True):
    """PoseSet.foothold_edges into sentinel-filled outputs -> numpy (count, best, best_d2 or None, all_legs or None)"""
    npz, nl, ne = len(quats), len(legs), len(ea)
    if ps is None:
        ps = lrm.PoseSet(legs, npz, footholds=True, nominal=nominal)
    ps.update(dev(torch, quats), dev(torch, body))
    count = torch.full((nl, ne), SENTINEL, dtype=torch.int32, device="cuda")
    best = torch.full((nl, ne), SENTINEL, dtype=torch.int32, device="cuda")
    bd2 = torch.full((nl, ne), float(SENTINEL), dtype=torch.float32, device="cuda")
    al = torch.full((ne,), 9, dtype=torch.uint8, device="cuda")
    tx, ty, tz = soa(torch, targets)
    ta, tb = dev(torch, np.asarray(ea, np.int32)), dev(torch, np.asarray(eb, np.int32))
    if d2 and all_legs:
        ps.foothold_edges(tx, ty, tz, ta, tb, count, best, bd2, al, check=check)
    else:  # the NULL forms of the C ABI
        L, dp = lrm.load(), lambda t: None if t is None else t.data_ptr()
        rc = L.lrm_foothold_edges_posed_dev(dp(tx), dp(ty), dp(tz), len(targets), dp(ps.workspace), dp(ps.fh_workspace), npz, nl,
                                            dp(ta), dp(tb), ne, dp(count), dp(best), dp(bd2 if d2 else None),
                                            dp(al if all_legs else None), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    if not d2:
        assert (bd2 == float(SENTINEL)).all()
    if not all_legs:
        assert (al == 9).all()
    return count.cpu().numpy(), best.cpu().numpy(), bd2.cpu().numpy() if d2 else None, al.cpu().numpy() if all_legs else None


def check(lrm, torch, targets, quats, body, legs, nominal, ea, eb, both=True, **kw):
    want = fe.host(lrm, targets, quats, body, legs, nominal, ea, eb)
    if both:
        pc.assert_both_outcomes(want)
    fe.assert_same(run(lrm, torch, targets, quats, body, legs, nominal, ea, eb, **kw), want)
    return want


@pytest.mark.parametrize("nt", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 4095, 4096, 4097, (GROUP + 1) * TILE + 1])
def test_every_cloud_size(lrm, torch_cuda, nt):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets, ea, eb = fe.scene(lrm, 32 if nt > 20000 else 64, nt, seed=nt % 97)
    check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(6), ea, eb, both=nt >= TILE - 1)


@pytest.mark.parametrize("nedges", [1, 2, 3, 5, 255, 257])
@pytest.mark.parametrize("nt", [3000, 5000])
def test_every_edge_count(lrm, torch_cuda, nedges, nt):
    legs, _ = pc.leg_families(lrm)["mixed_5_tilted"]
    quats, body, targets, ea, eb = fe.scene(lrm, 200, nt, seed=nedges + nt)
    assert len(ea) >= 257
    check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(5), ea[:nedges], eb[:nedges], both=nedges > 100)


def test_edges_past_the_grid_stride(lrm, torch_cuda):
    """more edges than one pass of the grid holds: a wave walks on to edge + GRID_EDGES"""
    legs, _ = pc.leg_families(lrm)["m2_1_identity"]
    n = GRID_EDGES + 777
    quats, body, targets, _, _ = fe.scene(lrm, 300, 200, seed=3, extra=False)
    targets = targets * np.float32(0.25)  # 200 targets within 230 mm of the origin
    body[:, :2] = body[:, :2] * np.float32(0.1)
    rng = np.random.default_rng(8)
    ea = rng.integers(0, 600, n).astype(np.int32)
    eb = np.where(rng.random(n) < 0.7, (ea + 300) % 600, rng.integers(0, 600, n)).astype(np.int32)
    want = check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(1), ea, eb)
    tail = want["count"][:, GRID_EDGES:]
    assert (tail > 0).sum() > 20 and (tail == 0).sum() > 20


@pytest.mark.parametrize("family", ["m2_1_identity", "m2_6_tilted", "m2_8_identity", "random_7_tilted"])
def test_leg_counts(lrm, torch_cuda, family):
    legs, _ = pc.leg_families(lrm)[family]
    quats, body, targets, ea, eb = fe.scene(lrm, 96, 6000, seed=len(family) + len(legs))
    for nominal in (None, pc.nominal_for(len(legs))):
        want = check(lrm, torch_cuda, targets, quats, body, legs, nominal, ea, eb)
    # the device agrees with the host, whose two directions agree bit for bit: so do the device's
    fe.assert_same(run(lrm, torch_cuda, targets, quats, body, legs, nominal, eb, ea), want)


def test_non_unit_quaternion_at_one_end_and_at_both(lrm, torch_cuda):
    """a +inf sphere excludes nothing on ITS side only: edges (unit, non-unit), (non-unit, unit) and (non-unit, non-unit)
    among unit ones, on a cloud with boxes"""
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6)
    quats, body, targets, _, _ = fe.scene(lrm, 60, 6000, seed=14, extra=False)
    quats[:] = posed_cases.random_unit_quats(len(quats), np.random.default_rng(2))
    quats[::2] = np.array([1, 0, 0, 0], np.float32)
    # scaled identities (qtInvRotate of (s, 0, 0, 0) is still the identity map, so these poses reach what their unit
    # twins reach) and two scaled random ones: a only, b only, both ends
    off = [2, 60 + 8, 20, 60 + 20, 30, 60 + 30, 40, 60 + 40, 13, 60 + 27]
    quats[off] = (quats[off].astype(np.float64) * np.array([0.6, 1.4, 0.8, 1.9, 1.2, 0.7, 1.05, 0.95, 1.3, 0.75])[:, None]).astype(np.float32)
    ea = np.arange(60, dtype=np.int32)
    eb = ea + 60
    r2 = lrm.dbg_pose_footholds_compile_host(quats, legs, nominal)[:, 0, 3]
    inf_a, inf_b = np.isposinf(r2[ea]), np.isposinf(r2[eb])
    assert (inf_a & ~inf_b).sum() >= 1 and (~inf_a & inf_b).sum() >= 1 and (inf_a & inf_b).sum() >= 3 and (~inf_a & ~inf_b).sum() > 40
    want = check(lrm, torch_cuda, targets, quats, body, legs, nominal, ea, eb)
    check(lrm, torch_cuda, targets, quats, body, legs, nominal, eb, ea)
    assert (want["count"][:, inf_a ^ inf_b] > 0).any() and (want["count"][:, inf_a & inf_b] > 0).any()


def test_edge_shapes(lrm, torch_cuda):
    """a == b equals footholds() of that pose with best_d2 doubled; duplicated edges get equal answers; one pose named
    1000 times"""
    torch = torch_cuda
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6)
    quats, body, targets, ea, eb = fe.scene(lrm, 70, 5000, seed=31)
    npz = len(quats)
    same = np.arange(npz, dtype=np.int32)
    got = run(lrm, torch, targets, quats, body, legs, nominal, same, same)
    fe.assert_same(got, fe.host(lrm, targets, quats, body, legs, nominal, same, same))
    ps = lrm.PoseSet(legs, npz, footholds=True, nominal=nominal).update(dev(torch, quats), dev(torch, body))
    count, best, bd2, al = (t.cpu().numpy() for t in ps.footholds(*soa(torch, targets)))
    assert np.array_equal(got[0], count) and np.array_equal(got[1], best) and np.array_equal(got[3], al)
    assert np.array_equal(pc.bits(got[2]), pc.bits(bd2 + bd2)) and (count > 0).any() and (count == 0).any()
    # every edge three times, shuffled
    perm = np.random.default_rng(3).permutation(3 * len(ea))
    ea3, eb3 = np.tile(ea, 3)[perm], np.tile(eb, 3)[perm]
    want = check(lrm, torch, targets, quats, body, legs, nominal, ea3, eb3)
    first = {}
    for k, key in enumerate(zip(ea3, eb3)):
        j = first.setdefault(key, k)
        assert np.array_equal(want["count"][:, k], want["count"][:, j]) and np.array_equal(want["best"][:, k], want["best"][:, j])
    # pose 6 at one end of 1000 edges: 500 times as a, 500 times as b, its neighbour 70 + 6 among the other ends
    other = np.random.default_rng(4).integers(0, npz, 1000).astype(np.int32)
    other[::9] = 76
    six = np.full(1000, 6, np.int32)
    want = check(lrm, torch, targets, quats, body, legs, nominal, np.where(np.arange(1000) < 500, six, other),
                 np.where(np.arange(1000) < 500, other, six))
    assert (want["count"][:, ::9] > 0).any()


def test_bad_indices(lrm, torch_cuda):
    """check=False leaves every index to the kernel: edges with an end outside [0, nposes) get 0, -1, +inf, 0 and their
    neighbours in the list are answered; check=True refuses them on the host"""
    torch = torch_cuda
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6)
    quats, body, targets, ea, eb = fe.scene(lrm, 64, 5000, seed=37)
    npz = len(quats)
    ea, eb = ea.copy(), eb.copy()
    i32 = np.iinfo(np.int32)
    ea[0], ea[3], eb[5], eb[7], ea[63], eb[64] = -1, npz, npz + 1000, i32.min, i32.max, -2 ** 20
    ea[9], eb[9] = i32.max, -7
    bad = [0, 3, 5, 7, 9, 63, 64]
    want = check(lrm, torch, targets, quats, body, legs, nominal, ea, eb, check=False)
    assert (want["count"][:, bad] == 0).all() and (want["best"][:, bad] == -1).all()
    assert np.isposinf(want["best_d2"][:, bad]).all() and (want["all_legs"][bad] == 0).all()
    ps = lrm.PoseSet(legs, npz, footholds=True, nominal=nominal).update(dev(torch, quats), dev(torch, body))
    for k in (0, 3, 5, 7):
        with pytest.raises(ValueError):
            ps.foothold_edges(*soa(torch, targets), dev(torch, ea[k:k + 1]), dev(torch, eb[k:k + 1]))
    # a table compiled for fewer poses than the set holds room for: nposes is update()'s, not nposes_max
    ps = lrm.PoseSet(legs, npz + 50, footholds=True, nominal=nominal)
    fe.assert_same(run(lrm, torch, targets, quats, body, legs, nominal, ea, eb, ps=ps, check=False), want)


def test_null_outputs(lrm, torch_cuda):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets, ea, eb = fe.scene(lrm, 45, 5000, seed=12)
    check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(6), ea, eb, d2=False)
    check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(6), ea, eb, all_legs=False)
    lrm.set_mode(lrm.MODE_STRICT)  # the answers do not depend on the mode
    try:
        check(lrm, torch_cuda, targets, quats, body, legs, None, ea, eb, d2=False, all_legs=False)
    finally:
        lrm.set_mode(lrm.MODE_FAST)  # the library default


@pytest.mark.parametrize("kind", ["dense_cluster_boxes", "dense_cluster_plain", "sparse_tiles"])
def test_scenes_against_each_cull(lrm, torch_cuda, kind):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    if kind == "sparse_tiles":
        quats, body, targets, ea, eb = fe.scene(lrm, 80, 9 * 1024, seed=2, kind="sparse_tiles")
    else:
        quats, body, targets, ea, eb = fe.scene(lrm, 80, 6000 if kind.endswith("boxes") else 3500, seed=1, kind="dense_cluster")
    check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(6, seed=5), ea, eb)


def test_bad_and_extreme_input(lrm, torch_cuda):
    legs, _ = pc.leg_families(lrm)["m2_5_identity"]
    quats, body, targets, ea, eb = fe.scene(lrm, 80, 6000, seed=8)
    bad_t = targets.copy()
    bad_t[::7] = np.nan
    bad_t[3::11, 1] = np.inf
    bad_t[5::13] = -np.inf
    bad_t[1024:1088] = np.nan
    check(lrm, torch_cuda, bad_t, quats, body, legs, pc.nominal_for(5), ea, eb)
    bad_b = body.copy()
    bad_b[1] = np.nan
    bad_b[2, 0] = np.inf
    bad_b[85] = -np.inf
    check(lrm, torch_cuda, targets, quats, bad_b, legs, pc.nominal_for(5), ea, eb)
    want = check(lrm, torch_cuda, targets, quats, body, legs, np.full((5, 3), 1e30, np.float32), ea, eb)
    assert np.isposinf(want["best_d2"]).all()


def test_far_from_the_origin(lrm, torch_cuda):
    """a cloud 4e6 mm from the origin: the float32 grid there is 0.25-0.5 mm, and both sides round alike"""
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets, ea, eb = fe.scene(lrm, 96, 6000, seed=9)
    body, targets = pc.translated(body, targets, 4e6)
    check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(6), ea, eb)


def test_two_clouds_share_the_box_buffer(lrm, torch_cuda):
    """a large cloud, then a smaller one, then one below the box threshold, on one PoseSet: no box of an earlier cloud
    leaks into a later answer"""
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6)
    ps = lrm.PoseSet(legs, 128, footholds=True, nominal=nominal)
    for k, nt in enumerate((30_000, 6_000, 3_000)):
        quats, body, targets, ea, eb = fe.scene(lrm, 64, nt, seed=20 + k)
        want = fe.host(lrm, targets, quats, body, legs, nominal, ea, eb)
        pc.assert_both_outcomes(want)
        fe.assert_same(run(lrm, torch_cuda, targets, quats, body, legs, nominal, ea, eb, ps=ps), want)


def lattice_edges(body, k):
    """every pose to its k nearest other poses (both directions arise), and to itself"""
    d = np.linalg.norm(body[:, None, :].astype(np.float64) - body[None, :, :], axis=-1)
    np.fill_diagonal(d, np.inf)
    nb = np.argsort(d, axis=1, kind="stable")[:, :k]
    a = np.concatenate([np.repeat(np.arange(len(body)), k), np.arange(len(body))])
    b = np.concatenate([nb.reshape(-1), np.arange(len(body))])
    return a.astype(np.int32), b.astype(np.int32)


def test_scale_against_the_oracle(lrm, oracle, torch_cuda):
    """the reference terrain (65 536 targets), the 96 lattice poses nearest its middle (50 mm apart) with a sweep orientation
    each, 6 M2 legs, every pose to its 24 nearest neighbours and to itself (2400 edges), against the oracle brute force
    (96 x 6 x 65 536 = 3.8e7 evaluations, within MAX_TRIPLES)"""
    from lrm_amd import workloads
    t = reference_terrain()
    ground = np.ascontiguousarray(t["ground"], np.float32)
    assert len(ground) == 65536
    bodies = np.ascontiguousarray(t["bodies"], np.float32)
    mid = np.median(bodies[:, :2], axis=0)
    body = np.ascontiguousarray(bodies[np.argsort(np.linalg.norm(bodies[:, :2] - mid, axis=1), kind="stable")[:96]])
    quats = fc.sweep_pose_quats(lrm, 96)
    legs = workloads.hexapod(lrm.get_M2_leg, 6)
    nominal = pc.nominal_for(6, seed=7)
    ea, eb = lattice_edges(body, 24)
    assert len(ea) == 2400 and 6 * 96 * len(ground) <= fe.MAX_TRIPLES
    got = run(lrm, torch_cuda, ground, quats, body, legs, nominal, ea, eb)
    want = fe.brute(oracle, ground, quats, body, legs, fc.nominal_w_of(lrm, quats, legs, nominal), ea, eb)
    pc.assert_both_outcomes(want)
    fe.assert_same(got, want)
    one = want["count"][:, 2304:]  # the a == b edges: the poses' own counts
    fe.assert_not_vacuous(want["count"][:, :2304], one[:, ea[:2304]], one[:, eb[:2304]], want["all_legs"], share=0.1)


def test_chain_on_one_pose_set(lrm, torch_cuda):
    """update -> footholds -> foothold_edges -> ik on the SAME PoseSet: every chosen common foothold solved under BOTH
    poses of its edge has status 1 or 3 exactly where count > 0, and status 0 where best is -1"""
    from lrm_amd import workloads
    torch = torch_cuda
    t = reference_terrain()
    ground = np.ascontiguousarray(t["ground"], np.float32)
    bodies = np.ascontiguousarray(t["bodies"], np.float32)
    n, nl = 4096, 6
    body = np.ascontiguousarray(bodies[40_000:40_000 + n])  # lattice order: index neighbours are 50 mm apart, mostly
    quats = fc.sweep_pose_quats(lrm, n, seed=8)
    legs = workloads.hexapod(lrm.get_M2_leg, nl)
    nominal = np.stack([lrm.apply_fk_cpu(np.array([[0.0, 0.3, -1.2]], np.float32), leg, (1, 0, 0, 0))[0][0] for leg in legs])
    rng = np.random.default_rng(9)
    ea = rng.integers(0, n, 12_000).astype(np.int32)
    eb = np.where(rng.random(len(ea)) < 0.8, np.clip(ea + rng.integers(-2, 3, len(ea)), 0, n - 1), rng.integers(0, n, len(ea))).astype(np.int32)
    ps = lrm.PoseSet(legs, n, ik=True, footholds=True, nominal=nominal).update(dev(torch, quats), dev(torch, body))
    tx, ty, tz = soa(torch, ground)
    single = ps.footholds(tx, ty, tz)[0]
    ta, tb = dev(torch, ea), dev(torch, eb)
    count, best, best_d2, all_legs = ps.foothold_edges(tx, ty, tz, ta, tb)
    torch.cuda.synchronize()
    c, ti = count.cpu().numpy(), best.cpu().numpy().reshape(-1)
    s1 = single.cpu().numpy()
    assert (c <= np.minimum(s1[:, ea], s1[:, eb])).all()
    assert (ti == -1).any() and (ti >= 0).sum() > 5_000 and np.array_equal(ti >= 0, c.reshape(-1) > 0)
    for which in ("a", "b"):
        pi, li = lrm.device.foothold_edges_layout(len(ea), nl, "cuda", ta, tb, which)
        ang, st = ps.ik(tx, ty, tz, pi, li, target_idx=best.view(-1))
        torch.cuda.synchronize()
        s = st.cpu().numpy()
        assert np.array_equal(np.isin(s, (1, 3)), ti >= 0) and np.array_equal(s == 0, ti == -1), which
        assert (s == 1).sum() > 5_000


def test_update_and_foothold_edges_replay_from_a_graph(lrm, torch_cuda):
    """update() and foothold_edges(check=False) only launch once the box buffer holds the cloud's size: captured on ONE
    side stream after a warm-up call, replayed after new quaternions, bodies, targets and edges were copied into the
    captured tensors"""
    torch = torch_cuda
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6)
    q0, b0, t0, a0, e0 = fe.scene(lrm, 128, 9000, seed=41)
    q1, b1, t1, a1, e1 = fe.scene(lrm, 128, 9000, seed=42)
    a1, e1 = e1[::-1].copy(), a1[::-1].copy()
    assert len(a0) == len(a1)
    ne = len(a0)
    qt, bt, tt = dev(torch, q0), dev(torch, b0), dev(torch, t0.T.copy())
    at, et = dev(torch, a0), dev(torch, e0)
    count = torch.empty((6, ne), dtype=torch.int32, device="cuda")
    best = torch.empty((6, ne), dtype=torch.int32, device="cuda")
    bd2 = torch.empty((6, ne), dtype=torch.float32, device="cuda")
    al = torch.empty(ne, dtype=torch.uint8, device="cuda")
    ps = lrm.PoseSet(legs, 256, footholds=True, nominal=nominal)

    def work():
        ps.update(qt, bt)
        ps.foothold_edges(tt[0], tt[1], tt[2], at, et, count, best, bd2, al, check=False)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture: the box buffer grows here
        work()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            work()
        qt.copy_(dev(torch, q1))
        bt.copy_(dev(torch, b1))
        tt.copy_(dev(torch, t1.T.copy()))
        at.copy_(dev(torch, a1))
        et.copy_(dev(torch, e1))
        count.fill_(SENTINEL)
        best.fill_(SENTINEL)
        bd2.fill_(SENTINEL)
        al.fill_(9)
        g.replay()
    torch.cuda.synchronize()
    want = fe.host(lrm, t1, q1, b1, legs, nominal, a1, e1)
    pc.assert_both_outcomes(want)
    fe.assert_same((count.cpu().numpy(), best.cpu().numpy(), bd2.cpu().numpy(), al.cpu().numpy()), want)
    del g
