"""Shared cases of the foothold-list tests (tests/test_foothold_lists_cpu.py, tests/test_gpu_foothold_lists.py): the
reachable targets per (pose, leg) from the oracle alone, the segment rule of include/lrm.h restated in Python, and the
offset arrays (whole lists, fixed stride, gaps, decreasing, negative) both files feed to the host loop and the device.
Every output buffer is prefilled with a sentinel and carries GUARD extra entries behind `capacity`, so a write outside a
segment fails a comparison instead of going unnoticed."""
import numpy as np

import footholds_posed_cases as fpc
import pair_cases as pc

SENT_I = np.int32(-77)
SENT_F = np.float32(-7.5)
GUARD = 64


def oracle_lists(oracle, targets, quats, body, legs, nominal_w):
    """-> ([idx int32 per o = l*P + p], [d2 float32 per o]) from the oracle's reachability_global on targets - body[p]
    (footholds_posed_cases.brute's mask) and d2 in numpy float32 written as (dx*dx + dy*dy) + dz*dz"""
    targets = np.ascontiguousarray(targets, np.float32).reshape(-1, 3)
    legs = np.ascontiguousarray(legs, np.float32).reshape(-1, 14)
    nl, npz, nt = len(legs), len(quats), len(targets)
    assert nl * npz * nt <= fpc.MAX_TRIPLES, "brute force too large"
    idx, d2s = [None] * (nl * npz), [None] * (nl * npz)
    with np.errstate(over="ignore", invalid="ignore"):
        for p in range(npz):
            b = np.zeros(3, np.float32) if body is None else body[p]
            rel = (targets - b).astype(np.float32)
            for l in range(nl):
                r = oracle.reach(rel, legs[l], quats[p]).astype(bool) if nt else np.zeros(0, bool)
                hit = np.flatnonzero(r).astype(np.int32)
                c = (b + nominal_w[p, l]).astype(np.float32)
                d = (targets[hit] - c).astype(np.float32)
                idx[l * npz + p] = hit
                d2s[l * npz + p] = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)
    return idx, d2s


def counts_of(lists):
    return np.array([len(a) for a in lists], np.int64)


def csr_offsets(count):
    """what lrm_foothold_offsets_dev computes, in numpy int64"""
    return np.concatenate([[0], np.cumsum(np.maximum(np.asarray(count, np.int64).reshape(-1), 0))]).astype(np.int64)


def buffers(capacity):
    n = max(int(capacity), 0) + GUARD
    return np.full(n, SENT_I, np.int32), np.full(n, SENT_F, np.float32)


def expected(lists, d2s, offsets, capacity):
    """the segment rule: base = offsets[o], room = min(offsets[o+1], capacity) - base, 0 if negative or base < 0; the
    first min(count, room) entries at base + k; everything else keeps the sentinel -> (idx, d2, written[o])"""
    idx, d2 = buffers(capacity)
    written = np.zeros(len(lists), np.int32)
    for o, (a, d) in enumerate(zip(lists, d2s)):
        base, end = int(offsets[o]), min(int(offsets[o + 1]), int(capacity))
        room = end - base if base >= 0 and end > base else 0
        k = min(len(a), room)
        idx[base:base + k] = a[:k]
        d2[base:base + k] = d[:k]
        written[o] = k
    return idx, d2, written


def disjoint(offsets, capacity, count):
    """no two written ranges overlap: the result does not depend on the order the segments are filled in"""
    spans = []
    for o in range(len(count)):
        base, end = int(offsets[o]), min(int(offsets[o + 1]), int(capacity))
        k = min(int(count[o]), end - base if base >= 0 and end > base else 0)
        if k:
            spans.append((base, base + k))
    spans.sort()
    return all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def offset_cases(count, seed=0):
    """name -> (offsets int64[n + 1], capacity) around the lists `count` describes"""
    count = np.asarray(count, np.int64).reshape(-1)
    n = len(count)
    full = csr_offsets(count)
    total = int(full[-1])
    rng = np.random.default_rng(seed)
    cases = {"whole": (full, total), "whole_spare_capacity": (full, total + 9)}
    for name, room in (("room_0", 0 * count), ("room_1", 0 * count + 1), ("room_count_minus_1", np.maximum(count - 1, 0)),
                       ("room_count_plus_1", count + 1)):
        off = csr_offsets(room)
        cases[name] = (off, int(off[-1]))
    for k in (1, 64, 65):
        cases[f"stride_{k}"] = (np.arange(n + 1, dtype=np.int64) * k, n * k)
    # capacity below offsets[-1], cutting inside the first list that crosses the middle of the buffer
    inside = np.flatnonzero((full[:-1] < total // 2) & (full[1:] > total // 2 + 1))
    cut = int(full[inside[0]] + 1) if len(inside) else total // 2
    cases["capacity_cuts_a_list"] = (full, cut)
    gaps = csr_offsets(count + rng.integers(0, 5, n))
    cases["gaps"] = (gaps, int(gaps[-1]))
    dec = (np.arange(n + 1, dtype=np.int64)[::-1] * 3).copy()
    cases["decreasing"] = (dec, int(dec[0]) + 1)
    zig = gaps.copy()  # o % 3 == 1 negative: segments o % 3 == 0 end below their base, o % 3 == 1 start below 0
    zig[1::3] = -1 - np.arange(len(zig[1::3]), dtype=np.int64) * 1000003
    cases["negative_and_decreasing"] = (zig, int(gaps[-1]))
    huge = full.copy()
    huge[-1] = np.iinfo(np.int64).max  # the last segment is cut by capacity alone
    cases["int64_max_end"] = (huge, total)
    return cases


def host_lists(lrm, targets, quats, body, legs, nominal, offsets, capacity, want_d2=True, want_written=True):
    """lrm_foothold_lists_posed_cpu into sentinel-filled buffers -> (idx, d2, written[o] or None)"""
    idx, d2 = buffers(capacity)
    written = np.full((len(legs), len(quats)), SENT_I, np.int32)
    lrm.foothold_lists_posed_cpu(targets, quats, body, legs, offsets, capacity, nominal, idx, d2, written, want_d2, want_written)
    if not want_d2:
        assert (d2 == SENT_F).all()
    if not want_written:
        assert (written == SENT_I).all()
    return idx, d2, written.reshape(-1) if want_written else None


def assert_same(got, want, d2=True, written=True):
    assert np.array_equal(got[0], want[0])
    if d2:
        assert np.array_equal(pc.bits(got[1]), pc.bits(want[1]))
    if written:
        assert np.array_equal(np.asarray(got[2]).reshape(-1), np.asarray(want[2]).reshape(-1))


def host_whole(lrm, targets, quats, body, legs, nominal):
    """the whole lists from the two host loops: count from lrm_footholds_posed_cpu, then the lists
    -> (count int64[n], offsets, idx, d2, written)"""
    count = lrm.footholds_posed_cpu(targets, quats, body, legs, nominal)[0].reshape(-1).astype(np.int64)
    off = csr_offsets(count)
    idx, d2, written = host_lists(lrm, targets, quats, body, legs, nominal, off, int(off[-1]))
    return count, off, idx, d2, written
