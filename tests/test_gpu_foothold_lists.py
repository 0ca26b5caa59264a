"""Reachable-foothold lists per (pose, leg) on the device (run with -m gpu on an MI355X): lrm_foothold_offsets_dev against
np.cumsum in int64, and lrm_foothold_lists_posed_dev against the host loop lrm_foothold_lists_posed_cpu bit for bit -- idx,
the bits of d2, written and the untouched sentinels -- around every boundary of the traversal, for every kind of offsets
array, and through PoseSet (the chain into ik(), a graph replay).  tests/test_foothold_lists_cpu.py ties that host loop to
the oracle.  Conditions on a scene (a list longer than 128, ...) are asserted on the host result, never on the device's."""
import functools

import numpy as np
import pytest

import foothold_lists_cases as flc
import footholds_posed_cases as fpc
import pair_cases as pc

pytestmark = pytest.mark.gpu

SCAN_SLICE = 8192  # counts per slice of foothold_offsets_kernel
NT_CASES = [1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097, 65 * 1024 + 3]


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
    block = int(re.search(r"constexpr int kScanBlock = (\d+);", src).group(1))
    items = int(re.search(r"constexpr int kScanItems = (\d+);", src).group(1))
    assert block * items == SCAN_SLICE


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def soa(torch, pts):
    t = dev(torch, np.asarray(pts, np.float32).reshape(-1, 3).T)
    return t[0], t[1], t[2]


def run(lrm, torch, targets, quats, body, legs, nominal, offsets, capacity, d2=True, written=True, ps=None):
    """lrm_foothold_lists_posed_dev into sentinel-filled buffers with a guard behind capacity -> (idx, d2, written)"""
    npz, nl = len(quats), len(legs)
    if ps is None:
        ps = lrm.PoseSet(legs, npz, footholds=True, nominal=nominal)
    ps.update(dev(torch, quats), None if body is None else dev(torch, body))
    hi, hd = flc.buffers(capacity)
    idx, dd = dev(torch, hi), dev(torch, hd)
    wr = torch.full((nl, npz), int(flc.SENT_I), dtype=torch.int32, device="cuda")
    off = dev(torch, np.asarray(offsets, np.int64))
    tx, ty, tz = soa(torch, targets)
    dp = lambda t: None if t is None else t.data_ptr()
    rc = lrm.load().lrm_foothold_lists_posed_dev(dp(tx), dp(ty), dp(tz), len(targets), dp(ps.workspace), dp(ps.fh_workspace), npz, nl,
                                                 dp(off), int(capacity), dp(idx), dp(dd if d2 else None), dp(wr if written else None),
                                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    if not d2:
        assert (dd == float(flc.SENT_F)).all()
    if not written:
        assert (wr == int(flc.SENT_I)).all()
    return idx.cpu().numpy(), dd.cpu().numpy(), wr.cpu().numpy().reshape(-1)


def check(lrm, torch, targets, quats, body, legs, nominal, offsets=None, capacity=None, **kw):
    """device == host loop for `offsets` (default: the whole lists) -> the host's count per o"""
    count = lrm.footholds_posed_cpu(targets, quats, body, legs, nominal)[0].reshape(-1).astype(np.int64)
    if offsets is None:
        offsets = flc.csr_offsets(count)
        capacity = int(offsets[-1])
    assert flc.disjoint(offsets, capacity, count)
    want = flc.host_lists(lrm, targets, quats, body, legs, nominal, offsets, capacity)
    got = run(lrm, torch, targets, quats, body, legs, nominal, offsets, capacity, **kw)
    flc.assert_same(got, want, d2=kw.get("d2", True), written=kw.get("written", True))
    return count


# ---- the scan ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, SCAN_SLICE - 1, SCAN_SLICE, SCAN_SLICE + 1, 2 * SCAN_SLICE + 1, 600_011])
def test_offsets_against_cumsum(lrm, torch_cuda, n):
    torch = torch_cuda
    rng = np.random.default_rng(n)
    count = rng.integers(-50, 400, n).astype(np.int32)
    count[rng.random(n) < 0.3] = 0
    for k, c in enumerate((count, np.full(n, np.iinfo(np.int32).max, np.int32))):
        if k and n:
            c[::5] = -3
            assert n < 3 or int(np.maximum(c.astype(np.int64), 0).sum()) > 2 ** 32
        out = torch.full((n + 1 + 8,), -5, dtype=torch.int64, device="cuda")
        got = lrm.device.foothold_offsets(dev(torch, c) if n else torch.empty(0, dtype=torch.int32, device="cuda"), out)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert np.array_equal(got[:n + 1], flc.csr_offsets(c)) and (got[n + 1:] == -5).all()
    fresh = lrm.foothold_offsets(dev(torch, count)) if n else None
    assert fresh is None or (fresh.dtype == torch.int64 and np.array_equal(fresh.cpu().numpy(), flc.csr_offsets(count)))


# ---- the traversal's boundaries ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rough_case(nt):
    import lrm_amd as lrm
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fpc.scene(lrm, 5, nt, seed=nt % 97)
    if nt < 1000:  # a small cloud on a small patch, so that some leg reaches some of it
        half = np.float32(250.0 / 900.0)
        targets = (targets * half).astype(np.float32)
        body[:, :2] = body[:, :2] * half
    return legs, quats, body, targets, pc.nominal_for(6)


@pytest.mark.parametrize("nt", NT_CASES)
def test_every_cloud_size(lrm, torch_cuda, nt):
    """the 64-target chunk and the 128-entry queue, the 1024 tile, the 4096 box threshold, the 64-tile group"""
    legs, quats, body, targets, nominal = rough_case(nt)
    check(lrm, torch_cuda, targets, quats, body, legs, nominal)
    check(lrm, torch_cuda, targets, quats, body, legs, nominal, np.arange(31, dtype=np.int64) * 3, 90)


def test_rough_cases_are_populated(lrm):
    """on the host alone: over the cloud sizes above, at least a quarter of the (pose, leg) pairs with a unit quaternion
    have a non-empty list"""
    some = pairs = 0
    for nt in NT_CASES:
        legs, quats, body, targets, nominal = rough_case(nt)
        unit = np.abs(np.linalg.norm(quats.astype(np.float64), axis=1) - 1) < 1e-6
        count = lrm.footholds_posed_cpu(targets, quats, body, legs, nominal)[0]
        some += int((count[:, unit] > 0).sum())
        pairs += int(unit.sum()) * len(legs)
    assert pairs >= 3 * 6 * len(NT_CASES) // 2 and 4 * some >= pairs, (some, pairs)


@pytest.mark.parametrize("nposes", [1, 2, 3, 4, 5, 255, 257])
def test_every_pose_count(lrm, torch_cuda, nposes):
    legs, _ = pc.leg_families(lrm)["mixed_5_tilted"]
    quats, body, targets = fpc.scene(lrm, nposes, 5000, seed=nposes)
    count = check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(5))
    assert nposes < 100 or ((count > 2).any() and (count == 0).any())


def test_poses_past_the_grid_stride(lrm, torch_cuda):
    """65 536 + 3 poses: a wave walks on to pose + 65 536 and must take that pose's segment"""
    legs, _ = pc.leg_families(lrm)["m2_2_tilted"]
    n = 65536 + 3
    quats, body, targets = fpc.scene(lrm, n, 64, seed=6)  # a seed with non-empty lists in the last three poses
    targets = targets * np.float32(0.05)  # 64 targets within 50 mm of the origin
    body[:, :2] = body[:, :2] * np.float32(0.02)
    count = check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(2)).reshape(2, n)
    assert (count[:, 65536:] > 0).any() and (count[:, :65536] > 0).sum() > 1000 and (count == 0).sum() > 1000


def test_dense_cluster_carries_the_rank_across_batches(lrm, torch_cuda):
    """the queue stays above 64, so batches carry over: a list longer than 128 takes its ranks from at least three batches"""
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6, seed=5)
    for nt in (3500, 6000):  # without and with boxes
        quats, body, targets = fpc.scene(lrm, 40, nt, seed=1, kind="dense_cluster")
        count = check(lrm, torch_cuda, targets, quats, body, legs, nominal).reshape(6, 40)
        assert count.max() > 128
        _, off, idx, _, _ = flc.host_whole(lrm, targets, quats, body, legs, nominal)
        lists = [[idx[off[l * 40 + p]:off[l * 40 + p + 1]].tolist() for l in range(6)] for p in range(40)]
        assert any(a and b and a != b for ls in lists for a in ls for b in ls)  # two legs of one pose, different lists


def test_sparse_tiles(lrm, torch_cuda):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fpc.scene(lrm, 40, 9 * 1024, seed=2, kind="sparse_tiles")
    count = check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(6, seed=5))
    assert (count > 2).any() and (count == 0).any()


# ---- the segment rule -------------------------------------------------------------------------------------------------
def test_segment_rule_for_every_kind_of_offsets(lrm, torch_cuda):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fpc.scene(lrm, 20, 3000, seed=33)
    nominal = pc.nominal_for(6)
    count = lrm.footholds_posed_cpu(targets, quats, body, legs, nominal)[0].reshape(-1).astype(np.int64)
    assert (count > 66).any() and (count == 0).any()
    cases = flc.offset_cases(count)
    assert {"stride_1", "stride_64", "stride_65", "capacity_cuts_a_list", "decreasing", "negative_and_decreasing", "gaps"} <= set(cases)
    ps = lrm.PoseSet(legs, 20, footholds=True, nominal=nominal)
    for name, (off, cap) in cases.items():
        check(lrm, torch_cuda, targets, quats, body, legs, nominal, off, cap, ps=ps)
    off, cap = cases["negative_and_decreasing"]
    check(lrm, torch_cuda, targets, quats, body, legs, nominal, off, cap, ps=ps, d2=False)
    check(lrm, torch_cuda, targets, quats, body, legs, nominal, off, cap, ps=ps, written=False)
    check(lrm, torch_cuda, targets, quats, body, legs, nominal, *cases["whole"], ps=ps, d2=False, written=False)


@pytest.mark.parametrize("family", ["m2_1_identity", "m2_6_tilted", "m2_8_identity", "random_8_identity", "mixed_5_tilted"])
def test_leg_counts_and_quaternions(lrm, torch_cuda, family):
    """1, 6 and 8 legs; among the first five poses a non-unit quaternion (the sphere that excludes nothing) and a nan one
    (an empty list); body = None"""
    legs, _ = pc.leg_families(lrm)[family]
    quats, body, targets = fpc.scene(lrm, 48, 5000, seed=len(family))
    n = np.linalg.norm(quats[:5].astype(np.float64), axis=1)
    assert abs(n[3] - 1) > 0.05 and np.isnan(n[4])
    count = check(lrm, torch_cuda, targets, quats, body, legs, pc.nominal_for(len(legs))).reshape(len(legs), 48)
    assert (count[:, 4] == 0).all() and (count > 2).any()
    check(lrm, torch_cuda, targets - body[0], quats, None, legs, None)
    lrm.set_mode(lrm.MODE_STRICT)  # the answers do not depend on the mode
    try:
        check(lrm, torch_cuda, targets, quats, body, legs, None)
    finally:
        lrm.set_mode(lrm.MODE_FAST)  # the library default


def test_bad_targets(lrm, torch_cuda):
    legs, _ = pc.leg_families(lrm)["m2_5_identity"]
    quats, body, targets = fpc.scene(lrm, 40, 5000, seed=8)
    bad_t = targets.copy()
    bad_t[::7] = np.nan
    bad_t[3::11, 1] = np.inf
    bad_t[5::13] = -np.inf
    bad_t[1024:1088] = np.nan
    assert (check(lrm, torch_cuda, bad_t, quats, body, legs, pc.nominal_for(5)) > 2).any()
    check(lrm, torch_cuda, targets, quats, body, legs, np.full((5, 3), 1e30, np.float32))


def test_no_targets_and_no_capacity(lrm, torch_cuda):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fpc.scene(lrm, 9, 500, seed=5)
    off = np.arange(55, dtype=np.int64) * 4
    for t, cap in ((np.zeros((0, 3), np.float32), 216), (targets, 0)):
        idx, d2, written = run(lrm, torch_cuda, t, quats, body, legs, None, off, cap)
        assert (idx == flc.SENT_I).all() and (d2 == flc.SENT_F).all() and (written == 0).all()
        run(lrm, torch_cuda, t, quats, body, legs, None, off, cap, written=False)


def test_two_clouds_share_the_box_buffer(lrm, torch_cuda):
    """one above and one below the 4096-target threshold in one process on one PoseSet, the smaller after the larger"""
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6)
    ps = lrm.PoseSet(legs, 48, footholds=True, nominal=nominal)
    for k, nt in enumerate((20_000, 3_000, 6_000)):
        quats, body, targets = fpc.scene(lrm, 48, nt, seed=20 + k)
        count = check(lrm, torch_cuda, targets, quats, body, legs, nominal, ps=ps)
        assert (count > 2).any() and (count == 0).any()


# ---- through PoseSet --------------------------------------------------------------------------------------------------
def test_chain_into_ik_with_the_second_entry(lrm, torch_cuda):
    """update -> footholds -> foothold_lists -> ik on ONE PoseSet, target_idx = the second entry of each list that has
    one (-1 elsewhere): the status bytes equal lrm_ik_posed_cpu's for those queries"""
    torch = torch_cuda
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    npz, nl = 64, 6
    quats, body, targets = fpc.scene(lrm, npz, 6000, seed=14)
    nominal = pc.nominal_for(6)
    ps = lrm.PoseSet(legs, npz, ik=True, footholds=True, nominal=nominal).update(dev(torch, quats), dev(torch, body))
    tx, ty, tz = soa(torch, targets)
    count, best, _, _ = ps.footholds(tx, ty, tz)
    offsets, idx, d2, written = ps.foothold_lists(tx, ty, tz, count=count)  # reads offsets[-1] back
    assert idx.numel() == int(count.sum()) and d2.numel() == idx.numel() and torch.equal(written, count)
    has2 = count.view(-1) >= 2
    second = torch.full((nl * npz,), -1, dtype=torch.int32, device="cuda")
    second[has2] = idx[(offsets[:-1][has2] + 1)]
    pi, li = lrm.device.footholds_layout(npz, nl, "cuda")
    ang, st = ps.ik(tx, ty, tz, pi, li, target_idx=second)
    torch.cuda.synchronize()
    # the host loop gives the same lists, so the same second entries
    _, off, hidx, _, _ = flc.host_whole(lrm, targets, quats, body, legs, nominal)
    assert np.array_equal(offsets.cpu().numpy(), off) and np.array_equal(idx.cpu().numpy(), hidx[:off[-1]])
    sec = second.cpu().numpy()
    assert (sec >= 0).sum() > 50 and (sec == -1).sum() > 50
    assert (sec[sec >= 0] != best.cpu().numpy().reshape(-1)[sec >= 0]).any()
    _, want_st, _ = lrm.apply_ik_posed_cpu(targets, pi.cpu().numpy(), li.cpu().numpy(), quats, body, legs, target_idx=sec)
    assert np.array_equal(st.cpu().numpy(), want_st) and (want_st[sec >= 0] != 0).all() and (want_st[sec == -1] == 0).all()
    # want_d2=False, and everything chained from nothing but the targets
    o2, i2, none, w2 = ps.foothold_lists(tx, ty, tz, want_d2=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(o2, offsets) and torch.equal(i2, idx) and torch.equal(w2, written)


def test_the_chain_replays_from_a_graph(lrm, torch_cuda):
    """update + footholds + foothold_offsets + foothold_lists with a fixed capacity only launch once the box buffer holds
    the cloud: captured on ONE side stream after a warm call, replayed after new quaternions, bodies and targets were
    copied into the captured tensors"""
    torch = torch_cuda
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    nominal = pc.nominal_for(6)
    npz, n = 128, 6 * 128
    q0, b0, t0 = fpc.scene(lrm, npz, 9000, seed=41)
    q1, b1, t1 = fpc.scene(lrm, npz, 9000, seed=42)
    q1 = q1[::-1].copy()
    count1, off1, idx1, d21, written1 = flc.host_whole(lrm, t1, q1, b1, legs, nominal)
    cap = int(off1[-1]) - 7  # fixed beforehand, and short of the last list: it is cut, nothing is written behind it
    assert cap > 0 and count1[count1 > 0][-1] > 7  # the cut falls inside the last non-empty list
    want = flc.host_lists(lrm, t1, q1, b1, legs, nominal, off1, cap)
    qt, bt, tt = dev(torch, q0), dev(torch, b0), dev(torch, t0.T.copy())
    count = torch.empty((6, npz), dtype=torch.int32, device="cuda")
    best, bd2 = torch.empty_like(count), torch.empty((6, npz), dtype=torch.float32, device="cuda")
    al = torch.empty(npz, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    hi, hd = flc.buffers(cap)
    idx, d2 = dev(torch, hi), dev(torch, hd)
    written = torch.empty((6, npz), dtype=torch.int32, device="cuda")
    ps = lrm.PoseSet(legs, npz, footholds=True, nominal=nominal)

    def work():
        ps.update(qt, bt)
        ps.footholds(tt[0], tt[1], tt[2], count, best, bd2, al)
        lrm.device.foothold_offsets(count, offsets)
        ps.foothold_lists(tt[0], tt[1], tt[2], offsets=offsets, capacity=cap, idx=idx, d2=d2, written=written)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm call outside the capture: the box buffer grows here
        work()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            work()
        qt.copy_(dev(torch, q1))
        bt.copy_(dev(torch, b1))
        tt.copy_(dev(torch, t1.T.copy()))
        idx.copy_(dev(torch, hi))
        d2.copy_(dev(torch, hd))
        written.fill_(int(flc.SENT_I))
        offsets.fill_(-5)
        g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(offsets.cpu().numpy(), off1)
    flc.assert_same((idx.cpu().numpy(), d2.cpu().numpy(), written.cpu().numpy()), want)
    del g
