// lrm_leg_clearance.h -- the per-(pose, leg) joints and the per-(link, target) arithmetic of lrm_leg_clearance_posed_dev /
// _cpu and lrm_leg_joints_posed_dev / _cpu (include/lrm.h): where do the leg's links stand under given joint angles, and how
// deep does a terrain target stand inside one of them.  One source for the kernels (lrm_leg_clearance.hip) and the host
// loops (lrm_capi.cpp): float32 only, no contraction, only + - * /, comparisons, lrm_sqrtf and lrm_sincosf, so that both
// give the same bits.  These functions decide outputs; the kernel's box cull (see there) may only skip what they reject.
#pragma once
#include <stdint.h>
#include "lrm_ik.h"

// The four joints of (pose, leg) under angles (c, f, t), in the caller's frame RELATIVE TO body[p] (no body added):
// J[0] the coxa joint, J[1] the femur joint, J[2] the knee, J[3] the tibia's end, tip_clear short of the foot.  The chain
// is lrm_fk_point's: with tip_clear == 0 and T > 0, J[3] has the bits of its tip (the same grouping of h and z).
LRM_HD void lrm_leg_joints(const LrmLegHead& L, const LrmIkLeg& K, float c, float f, float t, float tip_clear, LrmVec3 J[4]) {
    float sc, cc, sf, cf, sa, ca;
    lrm_sincosf(c, &sc, &cc);
    lrm_sincosf(f, &sf, &cf);
    lrm_sincosf(f + t, &sa, &ca);
    float T = K.T - tip_clear;
    T = !(T > 0.f) ? 0.f : T;
    const float h2 = K.C + K.F * cf;
    const float h3 = K.C + (K.F * cf + T * ca);
    J[0] = lrm_ik_from_coxa(L, K, LrmVec3{0.f, 0.f, 0.f});
    J[1] = lrm_ik_from_coxa(L, K, LrmVec3{cc * K.C, sc * K.C, 0.f});
    J[2] = lrm_ik_from_coxa(L, K, LrmVec3{cc * h2, sc * h2, K.F * sf});
    J[3] = lrm_ik_from_coxa(L, K, LrmVec3{cc * h3, sc * h3, K.F * sf + T * sa});
}

// A leg is tested iff all twelve coordinates are finite: nan angles (IK status 0) and angles outside lrm_sincosf's range
// (|x| < 120, lrm_exact_math.h) give nan joints.
LRM_HD bool lrm_leg_joints_finite(const LrmVec3 J[4]) {
    bool ok = true;
    for (int k = 0; k < 4; k++) ok = ok && lrm_ik_finite(J[k].x) && lrm_ik_finite(J[k].y) && lrm_ik_finite(J[k].z);
    return ok;
}

// One coordinate of lrm_leg_joints_posed_dev / _cpu's output: the joint plus the body position (one addition); a nan is
// stored as the canonical quiet nan (0x7fc00000), because sign and payload of a propagated nan are not the same on host and
// device (operand order, negation folded into an operand modifier).
LRM_HD float lrm_leg_joint_out(float j, float body) {
    const float s = j + body;
    return s != s ? lrm_u2f(0x7fc00000u) : s;
}

// The three links of a leg as the per-target test reads them: link k runs from a[k] = J[k] along ab[k] = J[k+1] - J[k],
// den[k] = |ab[k]|^2.  Formed once per (pose, leg).
struct LrmLegLinks {
    LrmVec3 a[3], ab[3];
    float den[3];
};
LRM_HD void lrm_leg_links(const LrmVec3 J[4], LrmLegLinks* S) {
    for (int k = 0; k < 3; k++) {
        S->a[k] = J[k];
        S->ab[k] = LrmVec3{J[k + 1].x - J[k].x, J[k + 1].y - J[k].y, J[k + 1].z - J[k].z};
        S->den[k] = (S->ab[k].x * S->ab[k].x + S->ab[k].y * S->ab[k].y) + S->ab[k].z * S->ab[k].z;
    }
}

// distance of q = t - body[p] to the segment a + s ab, s in [0, 1]; a nan s (0 / 0 is excluded by den > 0, inf / inf is
// not) counts as 0
LRM_HD float lrm_leg_link_dist(LrmVec3 a, LrmVec3 ab, float den, LrmVec3 q) {
    const float apx = q.x - a.x, apy = q.y - a.y, apz = q.z - a.z;
    const float num = (apx * ab.x + apy * ab.y) + apz * ab.z;
    float s = den > 0.f ? num / den : 0.f;
    s = !(s > 0.f) ? 0.f : (s > 1.f ? 1.f : s);
    const float ex = apx - s * ab.x, ey = apy - s * ab.y, ez = apz - s * ab.z;
    return lrm_sqrtf((ex * ex + ey * ey) + ez * ez);
}

#define LRM_LEG_NEAR 8u // bit 3 of lrm_leg_clearance_test: some link is near; bits 0..2: link k is hit

// Target q against the links with radius[k] != 0 (radius >= 0, checked by the C ABI): hit_k = d < radius[k],
// near_k = d < reach[k] with reach[k] = radius[k] + margin formed once per call, pen_k = radius[k] - d (-0 turned into +0).
// *pen = the largest pen_k of the near links, by comparisons (a near link's pen is never nan); untouched when none is near.
// A nan d is neither near nor hit.  hit_k implies near_k (margin >= 0, rounding is monotone).
LRM_HD unsigned lrm_leg_clearance_test(const LrmLegLinks& S, const float radius[3], const float reach[3], LrmVec3 q, float* pen) {
    unsigned bits = 0u;
    float best = 0.f;
    for (int k = 0; k < 3; k++) {
        if (radius[k] == 0.f) continue;
        const float d = lrm_leg_link_dist(S.a[k], S.ab[k], S.den[k], q);
        if (d < reach[k]) {
            const float pk = (radius[k] - d) + 0.f;
            best = (!(bits & LRM_LEG_NEAR) || pk > best) ? pk : best;
            bits |= LRM_LEG_NEAR | (d < radius[k] ? 1u << k : 0u);
        }
    }
    if (bits) *pen = best;
    return bits;
}

// 64-bit key of a near target: the smallest key is the largest pen, ties the smallest index (the idea of
// lrm_body_clearance.h's key; pen takes both signs like its height, so the sign handling is the same).  The high word is
// 0x7fffffff - bits for a pen >= +0 and the bits themselves (sign set) for a negative one: it falls as pen rises.  The pen
// of a near target is finite, so no key equals kLrmLegClearanceNone.
constexpr uint64_t kLrmLegClearanceNone = ~0ull;
LRM_HD uint64_t lrm_leg_clearance_key(float pen, uint32_t index) {
    const uint32_t u = lrm_f2u(pen);
    return ((uint64_t)((u >> 31) ? u : 0x7fffffffu - u) << 32) | index;
}
// What a key holds: the near target's index (< nt) and pen, or -1 and -inf for kLrmLegClearanceNone.
struct LrmLegClearanceWorst {
    int32_t index;
    float pen;
};
LRM_HD LrmLegClearanceWorst lrm_leg_clearance_key_decode(uint64_t key) {
    const uint32_t h = (uint32_t)(key >> 32);
    const bool have = key != kLrmLegClearanceNone;
    return LrmLegClearanceWorst{have ? (int32_t)(uint32_t)key : -1, have ? lrm_u2f((h >> 31) ? h : 0x7fffffffu - h) : -__builtin_inff()};
}

#if defined(__HIPCC__)
// launch functions (lrm_leg_clearance.hip); only launch.  records / ik_records: the pose and IK tables (entry of (pose, leg)
// at pose * nlegs + leg); angles and per-(pose, leg) outputs at [l * nposes + p]; tile_boxes as lrm_launch_body_clearance_posed
// (lrm_launch.h); the scalars are checked by the C ABI.
hipError_t lrm_launch_leg_clearance_posed(const float* tx, const float* ty, const float* tz, size_t nt, const void* records,
                                          const void* ik_records, size_t nposes, size_t nlegs, float* tile_boxes, const float* coxa,
                                          const float* femur, const float* tibia, const float radius[3], float margin,
                                          float tip_clear, const uint8_t* live_in, int32_t* hits_out, uint8_t* links_out,
                                          int32_t* worst_out, float* pen_out, uint8_t* free_out, hipStream_t st);
hipError_t lrm_launch_leg_joints_posed(const float* coxa, const float* femur, const float* tibia, size_t nposes, size_t nlegs,
                                       const void* records, const void* ik_records, float tip_clear, float* joints_out, hipStream_t st);
#endif
