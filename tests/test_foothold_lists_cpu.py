"""Reachable-foothold lists per (pose, leg) on the host (lrm_foothold_lists_posed_cpu, include/lrm.h): the host loop
against lists built from the oracle's reachability_global alone, its consistency with lrm_footholds_posed_cpu, the
segment rule for every kind of offsets array, and the argument checks.  Everything is exact: indices equal, d2 equal bit
for bit, sentinels untouched outside the written ranges."""
import ctypes as C

import numpy as np
import pytest

import foothold_lists_cases as flc
import footholds_posed_cases as fpc
import pair_cases as pc
from test_pair_cpu import FAMILIES

LRM_EINVAL = -1


def check_host_equals_oracle(lrm, oracle, targets, quats, body, legs, nominal):
    nw = fpc.nominal_w_of(lrm, quats, legs, nominal)
    lists, d2s = flc.oracle_lists(oracle, targets, quats, body, legs, nw)
    off = flc.csr_offsets(flc.counts_of(lists))
    want = flc.expected(lists, d2s, off, int(off[-1]))
    got = flc.host_lists(lrm, targets, quats, body, legs, nominal, off, int(off[-1]))
    flc.assert_same(got, want)
    return lists, d2s


@pytest.mark.parametrize("family", FAMILIES)
def test_host_loop_matches_the_oracle_for_every_leg_family(lrm, oracle, family):
    legs, _ = pc.leg_families(lrm)[family]
    quats, body, targets = fpc.scene(lrm, 40, 3000, seed=len(family) + len(legs))
    n = np.linalg.norm(quats[:5].astype(np.float64), axis=1)
    assert np.array_equal(quats[0], [1, 0, 0, 0]) and abs(n[3] - 1) > 0.05 and np.isnan(n[4])
    lists, _ = check_host_equals_oracle(lrm, oracle, targets, quats, body, legs, pc.nominal_for(len(legs)))
    count = flc.counts_of(lists)
    assert (count > 2).any() and (count == 0).any()
    assert (count.reshape(len(legs), -1)[:, np.isnan(quats).any(1)] == 0).all()


@pytest.mark.parametrize("kind", ["dense_cluster", "sparse_tiles"])
def test_host_loop_matches_the_oracle_on_every_scene(lrm, oracle, kind):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fpc.scene(lrm, 24, 4000 if kind == "dense_cluster" else 5 * 1024, seed=2, kind=kind)
    lists, _ = check_host_equals_oracle(lrm, oracle, targets, quats, body, legs, pc.nominal_for(6, seed=5))
    assert flc.counts_of(lists).max() > (128 if kind == "dense_cluster" else 2)


def test_host_loop_on_bad_and_extreme_input(lrm, oracle):
    legs, _ = pc.leg_families(lrm)["m2_5_identity"]
    quats, body, targets = fpc.scene(lrm, 30, 3000, seed=8)
    bad_t = targets.copy()
    bad_t[::7] = np.nan
    bad_t[3::11, 1] = np.inf
    bad_t[5::13] = -np.inf
    bad_t[1024:1088] = np.nan
    lists, _ = check_host_equals_oracle(lrm, oracle, bad_t, quats, body, legs, pc.nominal_for(5))
    assert flc.counts_of(lists).max() > 2
    # a nominal point 1e30 mm away: every d2 is +inf, the lists are the same
    lists2, d2s = check_host_equals_oracle(lrm, oracle, targets, quats, body, legs, np.full((5, 3), 1e30, np.float32))
    assert flc.counts_of(lists2).max() > 2 and all(np.isposinf(d).all() for d in d2s)
    check_host_equals_oracle(lrm, oracle, targets, quats, None, legs, None)  # body NULL, nominal NULL


def test_lists_agree_with_the_count_and_choice_call(lrm):
    """with room for everything: written == count of lrm_footholds_posed_cpu, every list strictly ascending, best the
    first index at the list's minimum d2, best_d2 that minimum bit for bit, empty lists exactly where best == -1"""
    legs, _ = pc.leg_families(lrm)["mixed_5_tilted"]
    for kind, nt in (("rough", 5000), ("dense_cluster", 3000)):
        quats, body, targets = fpc.scene(lrm, 60, nt, seed=17, kind=kind)
        nominal = pc.nominal_for(5, seed=2)
        count, best, best_d2, _, _ = lrm.footholds_posed_cpu(targets, quats, body, legs, nominal)
        cnt, off, idx, d2, written = flc.host_whole(lrm, targets, quats, body, legs, nominal)
        assert np.array_equal(written, count.reshape(-1)) and (cnt > 0).any() and (cnt == 0).any()
        for o in range(len(cnt)):
            seg, sd2 = idx[off[o]:off[o + 1]], d2[off[o]:off[o + 1]]
            assert (np.diff(seg) > 0).all() and (len(seg) == 0 or (seg[0] >= 0 and seg[-1] < nt))
            assert (len(seg) == 0) == (best.reshape(-1)[o] == -1)
            if len(seg):
                k = int(np.argmin(sd2))  # the first occurrence of the minimum
                assert seg[k] == best.reshape(-1)[o]
                assert pc.bits(sd2[k:k + 1])[0] == pc.bits(best_d2.reshape(-1)[o:o + 1])[0]
        assert (idx[off[-1]:] == flc.SENT_I).all() and (d2[off[-1]:] == flc.SENT_F).all()


def test_segment_rule_for_every_kind_of_offsets(lrm, oracle):
    legs, _ = pc.leg_families(lrm)["m2_6_tilted"]
    quats, body, targets = fpc.scene(lrm, 20, 3000, seed=33)
    nominal = pc.nominal_for(6)
    lists, d2s = flc.oracle_lists(oracle, targets, quats, body, legs, fpc.nominal_w_of(lrm, quats, legs, nominal))
    count = flc.counts_of(lists)
    assert (count > 66).any() and (count == 0).any()
    cases = flc.offset_cases(count)
    full, total = cases["whole"]
    assert cases["capacity_cuts_a_list"][1] < total and not (full == cases["capacity_cuts_a_list"][1]).any()
    for name, (off, cap) in cases.items():
        assert flc.disjoint(off, cap, count), name
        want = flc.expected(lists, d2s, off, cap)
        flc.assert_same(flc.host_lists(lrm, targets, quats, body, legs, nominal, off, cap), want), name
        if name in ("whole", "stride_64", "negative_and_decreasing"):  # the NULL forms
            flc.assert_same(flc.host_lists(lrm, targets, quats, body, legs, nominal, off, cap, want_d2=False), want, d2=False)
            flc.assert_same(flc.host_lists(lrm, targets, quats, body, legs, nominal, off, cap, want_written=False), want, written=False)
    assert (flc.expected(lists, d2s, *cases["decreasing"])[2] == 0).all()
    assert np.array_equal(flc.expected(lists, d2s, *cases["stride_65"])[2], np.minimum(count, 65))
    assert np.array_equal(flc.expected(lists, d2s, *cases["room_count_plus_1"])[2], count)


def test_argument_checks_and_conventions(lrm):
    L = lrm.load()
    p = lrm._capi._ptr
    legs = np.stack([lrm.get_M2_leg(0.3 * k) for k in range(9)]).astype(np.float32)
    f = np.zeros(64, np.float32)
    i = np.zeros(64, np.int32)
    off = np.zeros(64, np.int64)
    d = C.c_void_p(16)  # never dereferenced: every call below returns before its launch
    q = np.array([[1, 0, 0, 0]], np.float32)
    for nt, nlegs in ((2 ** 31, 6), (4, 0), (4, 9)):
        assert L.lrm_foothold_lists_posed_cpu(p(f), nt, p(q), None, 0, p(legs), nlegs, None, p(off), 8, p(i), p(f), p(i), None) == LRM_EINVAL
        assert L.lrm_foothold_lists_posed_dev(d, d, d, nt, d, d, 0, nlegs, d, 8, d, d, d, None) == LRM_EINVAL
    assert L.lrm_foothold_lists_posed_dev(d, d, d, 4, d, d, 2 ** 31, 2, d, 8, d, d, d, None) == LRM_EINVAL
    assert L.lrm_foothold_lists_posed_dev(d, d, d, 4, d, d, 2 ** 30, 8, d, 8, d, d, d, None) == LRM_EINVAL
    # NULL offsets or idx_out: LRM_EINVAL even with nposes == 0; otherwise nposes == 0 is a no-op
    assert L.lrm_foothold_lists_posed_dev(d, d, d, 4, d, d, 0, 2, None, 8, d, d, d, None) == LRM_EINVAL
    assert L.lrm_foothold_lists_posed_dev(d, d, d, 4, d, d, 0, 2, d, 8, None, d, d, None) == LRM_EINVAL
    assert L.lrm_foothold_lists_posed_cpu(p(f), 4, p(q), None, 0, p(legs), 2, None, None, 8, p(i), p(f), p(i), None) == LRM_EINVAL
    assert L.lrm_foothold_lists_posed_cpu(p(f), 4, p(q), None, 0, p(legs), 2, None, p(off), 8, None, p(f), p(i), None) == LRM_EINVAL
    assert L.lrm_foothold_lists_posed_dev(None, None, None, 2 ** 31 - 1, None, None, 0, 8, d, 8, d, None, None, None) == 0
    assert L.lrm_foothold_lists_posed_cpu(None, 2 ** 31 - 1, None, None, 0, p(legs), 8, None, p(off), 8, p(i), None, None, None) == 0
    # null or misaligned tables, null clouds
    assert L.lrm_foothold_lists_posed_dev(d, d, d, 4, None, d, 1, 2, d, 8, d, d, d, None) == LRM_EINVAL
    assert L.lrm_foothold_lists_posed_dev(d, d, d, 4, d, None, 1, 2, d, 8, d, d, d, None) == LRM_EINVAL
    assert L.lrm_foothold_lists_posed_dev(d, d, d, 4, d, C.c_void_p(24), 1, 2, d, 8, d, d, d, None) == LRM_EINVAL
    assert L.lrm_foothold_lists_posed_dev(None, d, d, 4, d, d, 1, 2, d, 8, d, d, d, None) == LRM_EINVAL
    # lrm_foothold_offsets_dev: NULL pointers and more than 2^32 - 1 counts
    assert L.lrm_foothold_offsets_dev(None, 4, d, None) == LRM_EINVAL
    assert L.lrm_foothold_offsets_dev(d, 4, None, None) == LRM_EINVAL
    assert L.lrm_foothold_offsets_dev(d, 2 ** 32, d, None) == LRM_EINVAL
    # nt == 0 or capacity == 0: written = 0 everywhere and nothing else
    quats = fpc.pose_quats(lrm, 7)
    body = np.zeros((7, 3), np.float32)
    tip = lrm.apply_fk_cpu(np.array([[0.0, 0.2, 0.3]], np.float32), legs[0], (1, 0, 0, 0))[0]
    for targets, cap in ((np.zeros((0, 3), np.float32), 5), (tip, 0)):
        idx, d2, written = flc.host_lists(lrm, targets, quats, body, legs[:3], None, np.arange(22, dtype=np.int64), cap)
        assert (idx == flc.SENT_I).all() and (d2 == flc.SENT_F).all() and (written == 0).all()
    # one target every leg of pose 0 reaches and pose 1 does not
    q2 = np.array([[1, 0, 0, 0], [1, 0, 0, 0]], np.float32)
    b2 = np.array([[0, 0, 0], [5000, 0, 0]], np.float32)
    idx, d2, written, _ = lrm.foothold_lists_posed_cpu(tip, q2, b2, np.stack([legs[0], legs[0]]), [0, 1, 2, 3, 4])
    assert written.tolist() == [[1, 0], [1, 0]] and idx[0] == 0 and idx[2] == 0 and np.isfinite(d2[[0, 2]]).all()


def test_symbols_are_declared_and_exported(lrm):
    names = {"lrm_foothold_offsets_dev", "lrm_foothold_lists_posed_dev", "lrm_foothold_lists_posed_cpu"}
    assert names <= set(lrm.declared_symbols())
    assert names <= set(lrm.exported_symbols())
    assert callable(lrm.device.foothold_offsets) and callable(lrm.PoseSet.foothold_lists) and callable(lrm.foothold_offsets)
