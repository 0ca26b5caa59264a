// lrm_self_clearance.h -- the arithmetic of lrm_self_clearance_posed_dev / _cpu (include/lrm.h): how close do the links of
// two DIFFERENT legs of one body come to each other under given joint angles.  One source for the kernel
// (lrm_self_clearance.hip) and the host loop (lrm_capi.cpp): float32 only, no contraction, only + - * /, comparisons and
// lrm_sqrtf, so that both give the same bits.  The joints are lrm_leg_clearance.h's (lrm_leg_joints, with tip_clear), which
// this header includes and leaves alone; everything that decides an output is here, the kernel only spreads it over lanes.
#pragma once
#include <stdint.h>
#include "lrm_leg_clearance.h"

// ---- pair codes ----
// A PAIR is two links of two different legs: legs i < j, link ka of leg i, link kb of leg j.  Its code is
// q * 9 + ka * 3 + kb with q = j (j - 1) / 2 + i the index of the leg pair: the codes of `nlegs` legs are exactly
// 0 .. lrm_self_npairs(nlegs) - 1, whatever nlegs is.  (The order decides no output: every pair's d is computed once.)
#define LRM_SELF_MAX_PAIRS 252 // eight legs: 28 leg pairs of nine link pairs
LRM_HD uint32_t lrm_self_npairs(uint32_t nlegs) { return nlegs * (nlegs - 1u) / 2u * 9u; }
// what a lane or a loop iteration reads of its pair, packed: bits 0..2 i, 3..5 j, 6..7 ka, 8..9 kb
LRM_HD uint32_t lrm_self_pair_pack(uint32_t i, uint32_t j, uint32_t ka, uint32_t kb) { return i | (j << 3) | (ka << 6) | (kb << 8); }
LRM_HD uint32_t lrm_self_pair_i(uint32_t pk) { return pk & 7u; }
LRM_HD uint32_t lrm_self_pair_j(uint32_t pk) { return (pk >> 3) & 7u; }
LRM_HD uint32_t lrm_self_pair_ka(uint32_t pk) { return (pk >> 6) & 3u; }
LRM_HD uint32_t lrm_self_pair_kb(uint32_t pk) { return (pk >> 8) & 3u; }
// code (< LRM_SELF_MAX_PAIRS) -> packed pair
LRM_HD uint32_t lrm_self_pair_of(uint32_t code) {
    uint32_t q = code / 9u;
    const uint32_t k = code - q * 9u;
    uint32_t j = 1u;
    while (q >= j) { // at most six steps
        q -= j;
        j++;
    }
    return lrm_self_pair_pack(q, j, k / 3u, k - (k / 3u) * 3u);
}

// ---- the distance of two links ----
LRM_HD float lrm_self_dot(LrmVec3 u, LrmVec3 v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
LRM_HD float lrm_self_clamp01(float x) { return !(x > 0.f) ? 0.f : (x > 1.f ? 1.f : x); }
// Segment 1 from A1 to B1 (the link of the leg with the smaller index), segment 2 from A2 to B2: the clamped closest-point
// step, then the four endpoint distances folded in (A1, B1 against segment 2; A2, B2 against segment 1).  Every candidate is
// a distance between two points of the segments, so d never under-reports; the fold bounds what the clamped step
// over-reports on nearly parallel links.
LRM_HD float lrm_self_pair_dist(LrmVec3 A1, LrmVec3 B1, LrmVec3 A2, LrmVec3 B2) {
    const LrmVec3 d1{B1.x - A1.x, B1.y - A1.y, B1.z - A1.z};
    const LrmVec3 d2{B2.x - A2.x, B2.y - A2.y, B2.z - A2.z};
    const LrmVec3 r{A1.x - A2.x, A1.y - A2.y, A1.z - A2.z};
    const float a = lrm_self_dot(d1, d1), e = lrm_self_dot(d2, d2), f = lrm_self_dot(d2, r), c = lrm_self_dot(d1, r),
                b = lrm_self_dot(d1, d2);
    float s, t;
    if (!(a > 0.f) && !(e > 0.f)) {
        s = 0.f;
        t = 0.f;
    } else if (!(a > 0.f)) {
        s = 0.f;
        t = lrm_self_clamp01(f / e);
    } else if (!(e > 0.f)) {
        t = 0.f;
        s = lrm_self_clamp01(-c / a);
    } else {
        const float den = a * e - b * b;
        s = den > 0.f ? lrm_self_clamp01((b * f - c * e) / den) : 0.f;
        const float tn = b * s + f;
        if (!(tn > 0.f)) {
            t = 0.f;
            s = lrm_self_clamp01(-c / a);
        } else if (tn > e) {
            t = 1.f;
            s = lrm_self_clamp01((b - c) / a);
        } else {
            t = tn / e;
        }
    }
    const float wx = (r.x + s * d1.x) - t * d2.x, wy = (r.y + s * d1.y) - t * d2.y, wz = (r.z + s * d1.z) - t * d2.z;
    float d = lrm_sqrtf((wx * wx + wy * wy) + wz * wz);
    float dk = lrm_leg_link_dist(A2, d2, e, A1);
    d = dk < d ? dk : d;
    dk = lrm_leg_link_dist(A2, d2, e, B1);
    d = dk < d ? dk : d;
    dk = lrm_leg_link_dist(A1, d1, a, A2);
    d = dk < d ? dk : d;
    dk = lrm_leg_link_dist(A1, d1, a, B2);
    d = dk < d ? dk : d;
    return d;
}

// ---- the test of a pair ----
// The nine sums of two radii and the nine reaches, formed once per call: entry ka * 3 + kb.
struct LrmSelfRadii {
    float rr[9], reach[9];
    uint32_t tested; // bit ka * 3 + kb: both radii are non-zero
};
LRM_HD LrmSelfRadii lrm_self_radii(const float radius[3], float margin) {
    LrmSelfRadii R;
    R.tested = 0u;
    for (int ka = 0; ka < 3; ka++)
        for (int kb = 0; kb < 3; kb++) {
            const int k = ka * 3 + kb;
            R.rr[k] = radius[ka] + radius[kb];
            R.reach[k] = R.rr[k] + margin;
            if (radius[ka] != 0.f && radius[kb] != 0.f) R.tested |= 1u << k;
        }
    return R;
}
#define LRM_SELF_NEAR 1u // bits of lrm_self_clearance_test
#define LRM_SELF_HIT 2u
// hit = d < rr, near = d < rr + margin, *pen = (rr - d) + 0 (-0 turned into +0; written when near).  A nan d is neither.
// hit implies near (margin >= 0, rounding is monotone).
LRM_HD unsigned lrm_self_clearance_test(float d, float rr, float reach, float* pen) {
    if (!(d < reach)) return 0u;
    *pen = (rr - d) + 0.f;
    return LRM_SELF_NEAR | (d < rr ? LRM_SELF_HIT : 0u);
}

// ---- what a leg keeps of its pairs ----
// the worst code of leg l for a pair with leg `other`: other * 9 + own_link * 3 + other_link (at most 71)
LRM_HD uint32_t lrm_self_worst_code(uint32_t other, uint32_t own_link, uint32_t other_link) { return other * 9u + own_link * 3u + other_link; }
// The key of a near pair is lrm_leg_clearance_key(pen, code): the smallest key is the largest pen, ties the smaller code.
struct LrmSelfLeg {
    int32_t hits;
    uint32_t with, links;
    uint64_t key;
};
LRM_HD LrmSelfLeg lrm_self_leg_empty() { return LrmSelfLeg{0, 0u, 0u, kLrmLegClearanceNone}; }
// leg `l` takes a near pair in (bits != 0); nothing changes unless l is one of the pair's two legs
LRM_HD void lrm_self_leg_take(LrmSelfLeg* L, uint32_t l, uint32_t pk, unsigned bits, float pen) {
    const uint32_t i = lrm_self_pair_i(pk), j = lrm_self_pair_j(pk), ka = lrm_self_pair_ka(pk), kb = lrm_self_pair_kb(pk);
    if (l != i && l != j) return;
    const uint32_t other = l == i ? j : i, own = l == i ? ka : kb, oth = l == i ? kb : ka;
    if (bits & LRM_SELF_HIT) {
        L->hits++;
        L->with |= 1u << other;
        L->links |= 1u << own;
    }
    const uint64_t key = lrm_leg_clearance_key(pen, lrm_self_worst_code(other, own, oth));
    L->key = key < L->key ? key : L->key;
}
// worst_out and pen_out of a key: 255 and -inf for kLrmLegClearanceNone
struct LrmSelfWorst {
    uint8_t code;
    float pen;
};
LRM_HD LrmSelfWorst lrm_self_key_decode(uint64_t key) {
    const LrmLegClearanceWorst w = lrm_leg_clearance_key_decode(key);
    return LrmSelfWorst{(uint8_t)(w.index < 0 ? 255 : w.index), w.pen};
}

#if defined(__HIPCC__)
// launch functions (lrm_self_clearance.hip); only launch.  records / ik_records: the pose and IK tables (entry of (pose, leg)
// at pose * nlegs + leg); angles and per-(set, leg) outputs at [l * nsets + s]; everything is checked by the C ABI:
// nsets >= 1, nlegs in 1..8, nlegs * nsets < 2^32.  pose_idx, live_in, pen_out, free_out may be null.
hipError_t lrm_launch_self_clearance_posed(const void* records, const void* ik_records, size_t nposes, size_t nlegs,
                                           const int32_t* pose_idx, size_t nsets, const float* coxa, const float* femur,
                                           const float* tibia, const float radius[3], float margin, float tip_clear,
                                           const uint8_t* live_in, int32_t* hits_out, uint8_t* with_out, uint8_t* links_out,
                                           uint8_t* worst_out, float* pen_out, uint8_t* free_out, hipStream_t st);
// out[i] = lrm_self_pair_dist of segs[12 i ..]: A1, B1, A2, B2; one pair per lane
hipError_t lrm_launch_link_pair_dist(const float* segs, size_t n, float* out, hipStream_t st);
#endif
