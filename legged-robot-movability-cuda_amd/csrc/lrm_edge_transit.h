// lrm_edge_transit.h -- the arithmetic of lrm_edge_transit_posed_dev / _cpu (include/lrm.h): does a planted foot stay
// reachable while the body moves from pose a to pose b.  One source for the gfx950 kernel (lrm_edge_transit.hip) and the
// host loop (lrm_capi.cpp); float32 without contraction, only + - * /, comparisons and lrm_sqrtf on top of the head
// compiler (lrm_compile_head.h) and the strict evaluation (lrm_point.h), so device and host give the same bits.
//
// The path: sample s of S is u = s / (S - 1) of the way.  The quaternion is the normalised linear blend of qa and +-qb
// (the sign that makes the blend the short way round).  That blend lies in the plane of qa and qb, so after the
// normalisation it traces the same great arc as slerp; only the speed along the arc differs (slower near the ends, faster
// in the middle).  The body position is the linear blend.  The two end samples are the poses themselves, untouched.
#pragma once
#include <math.h>
#include <stdint.h>
#include "lrm_compile_head.h"
#include "lrm_point.h"

#define LRM_TRANSIT_MAX_SAMPLES 64

struct LrmTransitSample {
    float q[4];
    LrmVec3 body;
};

// sample s of an edge whose ends are (qa, ba) and (qb, bb); 2 <= S <= LRM_TRANSIT_MAX_SAMPLES, s < S
LRM_HD LrmTransitSample lrm_transit_sample(const float qa[4], const float qb[4], LrmVec3 ba, LrmVec3 bb, uint32_t s, uint32_t S) {
    LrmTransitSample r;
    if (s == 0u || s == S - 1u) { // the table's own quaternion and body, bit for bit and not normalised
        const float* q = s == 0u ? qa : qb;
        for (int i = 0; i < 4; i++) r.q[i] = q[i];
        r.body = s == 0u ? ba : bb;
        return r;
    }
    const float u = (float)s / (float)(S - 1u);
    const float w = 1.f - u;
    const float dot = ((qa[0] * qb[0] + qa[1] * qb[1]) + qa[2] * qb[2]) + qa[3] * qb[3];
    const float sg = dot < 0.f ? -1.f : 1.f; // a nan dot gives +1
    float m[4];
    for (int i = 0; i < 4; i++) m[i] = w * qa[i] + u * (sg * qb[i]);
    const float n2 = ((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]) + m[3] * m[3];
    const float n = lrm_sqrtf(n2);
    for (int i = 0; i < 4; i++) r.q[i] = m[i] / n; // n2 = 0, nan or inf: evaluated as it comes out
    r.body.x = ba.x + u * (bb.x - ba.x);
    r.body.y = ba.y + u * (bb.y - ba.y);
    r.body.z = ba.z + u * (bb.z - ba.z);
    return r;
}

// (e, l) of a live edge with both ends in range is planted iff its foot names a target of the cloud
LRM_HD bool lrm_transit_foot_in_cloud(int32_t ft, uint32_t nt) { return ft >= 0 && (uint32_t)ft < nt; }

// The strict evaluation of p = target - body_s on the head of lrm_compile_head(leg, q_s, 1), compiled into *H (the caller's
// storage: an LDS slot or private memory on the device, a local on the host).
// Returns r_s; where r_s is false *d2 receives the squared norm of distance_global's vector (its validity byte is not
// consulted), a nan as +inf.  Where r_s is true *d2 is left alone.
LRM_HD bool lrm_transit_eval(const LrmLegDimensions& leg, const float q[4], LrmVec3 p, LrmLegHead* H, float* d2) {
    lrm_compile_head(leg, q, 1, H, (LrmLegDimensions*)nullptr);
    const LrmCircle* lists = &H->lists[0][0];
    if (lrm_reach_global(*H, lists, p)) return true;
    lrm_dist_global(*H, lists, p);
    const float d = (p.x * p.x + p.y * p.y) + p.z * p.z;
    *d2 = d != d ? INFINITY : d;
    return false;
}

// worst: the unreachable sample with the largest d2, ties to the smaller s.  d2 >= +0 or +inf, so its bits order as the
// floats do and the largest key (d2 bits << 32) | (63 - s) is that sample.
LRM_HD uint64_t lrm_transit_key(float d2, uint32_t s) { return ((uint64_t)lrm_f2u(d2) << 32) | (uint64_t)(63u - s); }
LRM_HD int32_t lrm_transit_key_sample(uint64_t key) { return (int32_t)(63u - (uint32_t)(key & 63u)); }
LRM_HD float lrm_transit_key_d2(uint64_t key) { return lrm_u2f((uint32_t)(key >> 32)); }

// the S low bits
LRM_HD uint64_t lrm_transit_full(uint32_t S) { return S >= 64u ? ~0ull : (1ull << S) - 1ull; }

// The answer of one (edge, leg) from its reach bits and its largest key among the misses.
struct LrmTransitLeg {
    uint64_t mask;
    int32_t reached, first_miss, worst;
    float worst_d2;
};
LRM_HD LrmTransitLeg lrm_transit_leg_unplanted() { return LrmTransitLeg{0ull, -1, -1, -1, 0.f}; }
LRM_HD int lrm_transit_ctz64(uint64_t v) { // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll((unsigned long long)v) - 1;
#else
    return __builtin_ctzll(v);
#endif
}
LRM_HD int lrm_transit_popc64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll((unsigned long long)v);
#else
    return __builtin_popcountll(v);
#endif
}
LRM_HD LrmTransitLeg lrm_transit_leg(uint64_t mask, uint64_t worst_key, uint32_t S) {
    const uint64_t miss = ~mask & lrm_transit_full(S);
    LrmTransitLeg A;
    A.mask = mask;
    A.reached = lrm_transit_popc64(mask);
    A.first_miss = miss ? lrm_transit_ctz64(miss) : -1;
    A.worst = miss ? lrm_transit_key_sample(worst_key) : -1;
    A.worst_d2 = miss ? lrm_transit_key_d2(worst_key) : 0.f;
    return A;
}

#if defined(__HIPCC__)
// launch function (lrm_edge_transit.hip); only launches.  Everything is checked by the C ABI: nedges >= 1, nlegs in 1..8,
// nsamples in 2..64, nt and nposes <= INT32_MAX, nlegs * nedges < 2^32.  body, live_in and every output but reached_out and
// first_miss_out may be null.
hipError_t lrm_launch_edge_transit_posed(const float* tx, const float* ty, const float* tz, size_t nt, const float* quats,
                                         const float* body, size_t nposes, const LrmLegDimensions* legs, size_t nlegs,
                                         const int32_t* edge_a, const int32_t* edge_b, size_t nedges, const int32_t* foot,
                                         size_t nsamples, const uint8_t* live_in, uint64_t* mask_out, int32_t* reached_out,
                                         int32_t* first_miss_out, int32_t* worst_out, float* worst_d2_out, uint8_t* planted_out,
                                         uint8_t* clear_out, int32_t* advance_out, hipStream_t st);
// out[(e * nsamples + s) * 7 ..] = lrm_transit_sample of (edge e, sample s): q[4], body[3]; one sample per lane
hipError_t lrm_launch_edge_transit_samples(const float* quats, const float* body, size_t nposes, const int32_t* edge_a,
                                           const int32_t* edge_b, size_t nedges, size_t nsamples, float* out, hipStream_t st);
#endif
