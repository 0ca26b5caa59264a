// lrm_swing.h -- the arithmetic of lrm_swing_transit_posed_dev / _cpu (include/lrm.h): can a LIFTED foot get from its foothold
// under pose a to its foothold under pose b -- does it stay inside the leg's workspace on the way, and does it pass through the
// terrain.  One source for the gfx950 kernels (lrm_swing.hip) and the host loop (lrm_capi.cpp); float32 without contraction,
// only + - * /, comparisons and lrm_sqrtf on top of lrm_edge_transit.h (the sampled pose path, the strict evaluation, the
// per-leg reach answer) and lrm_leg_clearance.h (the point-segment distance and the 64-bit key), so device and host give the
// same bits.  These functions decide outputs; the kernel's box cull (lrm_swing.hip) may only skip what they reject.
//
// The foot path lives in the frame ABOUT A = t[from]: P_0 = 0, P_{S-1} = D = B - A, an interior P_s = u D + h up with
// h = lift * 4 u (1 - u): a straight line from A to B with a parabolic bump of height `lift` along `up` at the middle.  The
// terrain test forms q = t - A about the same point, so the coordinates it works on are the step's own size however far the
// cloud lies from the origin.
#pragma once
#include <stdint.h>
#include "lrm_edge_transit.h"
#include "lrm_leg_clearance.h"

#define LRM_SWING_MAX_SKIP 63u

// path point of sample s relative to A; 2 <= S <= LRM_TRANSIT_MAX_SAMPLES, s < S
LRM_HD LrmVec3 lrm_swing_path_point(LrmVec3 D, float lift, LrmVec3 up, uint32_t s, uint32_t S) {
    if (s == 0u) return LrmVec3{0.f, 0.f, 0.f};
    if (s == S - 1u) return D;
    const float u = (float)s / (float)(S - 1u);
    const float w = 1.f - u;
    const float h = lift * ((4.f * u) * w);
    return LrmVec3{u * D.x + h * up.x, u * D.y + h * up.y, u * D.z + h * up.z};
}

// the foot of sample s in the caller's frame: the two footholds themselves at the ends, A + P_s in between
LRM_HD LrmVec3 lrm_swing_foot(LrmVec3 A, LrmVec3 B, LrmVec3 P, uint32_t s, uint32_t S) {
    if (s == 0u) return A;
    if (s == S - 1u) return B;
    return LrmVec3{A.x + P.x, A.y + P.y, A.z + P.z};
}

// the tested segments k of a path of S samples: skip <= k < S - 1 - skip; an empty range when 2 * skip >= S - 1
struct LrmSwingRange {
    uint32_t k0, k1; // k0 <= k < k1; the tested path points are P_k0 .. P_k1
};
LRM_HD LrmSwingRange lrm_swing_range(uint32_t S, uint32_t skip) {
    const uint32_t nseg = S - 1u;
    return 2u * skip >= nseg ? LrmSwingRange{0u, 0u} : LrmSwingRange{skip, nseg - skip};
}

LRM_HD bool lrm_swing_point_finite(LrmVec3 P) { return lrm_ik_finite(P.x) && lrm_ik_finite(P.y) && lrm_ik_finite(P.z); }

// segment k as the per-target test reads it: from a = P_k along ab = P_{k+1} - P_k, den = |ab|^2 (lrm_leg_links' form)
struct LrmSwingSeg {
    LrmVec3 a, ab;
    float den;
};
LRM_HD LrmSwingSeg lrm_swing_seg(LrmVec3 P0, LrmVec3 P1) {
    LrmSwingSeg g;
    g.a = P0;
    g.ab = LrmVec3{P1.x - P0.x, P1.y - P0.y, P1.z - P0.z};
    g.den = (g.ab.x * g.ab.x + g.ab.y * g.ab.y) + g.ab.z * g.ab.z;
    return g;
}

#define LRM_SWING_HIT 1u
#define LRM_SWING_NEAR 2u

// Target q = t - A against the tested segments segs[k0 .. k1): hit = d_k < radius, near = d_k < reach with reach = radius +
// margin formed once per call, pen_k = radius - d_k (-0 turned into +0).  *pen = the largest pen_k of the near segments, by
// comparisons; *first_hit = the smallest k with a hit; both untouched when there is none.  A nan d is neither near nor hit;
// a hit is near (margin >= 0, rounding is monotone).
LRM_HD unsigned lrm_swing_test(const LrmSwingSeg* segs, LrmSwingRange r, float radius, float reach, LrmVec3 q, float* pen,
                               uint32_t* first_hit) {
    unsigned bits = 0u;
    float best = 0.f;
    for (uint32_t k = r.k0; k < r.k1; k++) {
        const LrmSwingSeg g = segs[k];
        const float d = lrm_leg_link_dist(g.a, g.ab, g.den, q);
        if (d < reach) {
            const float pk = (radius - d) + 0.f;
            best = (!bits || pk > best) ? pk : best;
            if (d < radius && !(bits & LRM_SWING_HIT)) {
                *first_hit = k;
                bits |= LRM_SWING_HIT;
            }
            bits |= LRM_SWING_NEAR;
        }
    }
    if (bits) *pen = best;
    return bits;
}

// The terrain answer of one (edge, leg): what a leg that is not swinging, or whose test is skipped, gets is the empty one.
struct LrmSwingTerrain {
    int32_t hits, hit_seg, near;
    float pen;
};
LRM_HD LrmSwingTerrain lrm_swing_terrain_empty() { return LrmSwingTerrain{0, -1, -1, -__builtin_inff()}; }
constexpr uint32_t kLrmSwingNoSeg = 0xffffffffu;
LRM_HD LrmSwingTerrain lrm_swing_terrain(uint32_t hits, uint32_t first_hit, uint64_t key) {
    const LrmLegClearanceWorst w = lrm_leg_clearance_key_decode(key);
    return LrmSwingTerrain{(int32_t)hits, first_hit == kLrmSwingNoSeg ? -1 : (int32_t)first_hit, w.index, w.pen};
}

#if defined(__HIPCC__)
// launch function (lrm_swing.hip); only launches.  Everything is checked by the C ABI as for lrm_launch_edge_transit_posed,
// and lift, up, foot_radius >= 0, margin >= 0 finite, skip <= 63.  tile_boxes: the cloud's box workspace
// (lrm_launch_tile_boxes), filled first; null = no cull (clouds below the C ABI's threshold); never touched when
// foot_radius == 0.  body, live_in, mask_out, worst_out, worst_d2_out, pen_out, swinging_out and clear_out may be null.
hipError_t lrm_launch_swing_transit_posed(const float* tx, const float* ty, const float* tz, size_t nt, const float* quats,
                                          const float* body, size_t nposes, const LrmLegDimensions* legs, size_t nlegs,
                                          const int32_t* edge_a, const int32_t* edge_b, size_t nedges, const int32_t* foot_from,
                                          const int32_t* foot_to, size_t nsamples, float lift, const float up[3], float foot_radius,
                                          float margin, uint32_t skip, float* tile_boxes, const uint8_t* live_in, uint64_t* mask_out,
                                          int32_t* reached_out, int32_t* first_miss_out, int32_t* worst_out, float* worst_d2_out,
                                          int32_t* hits_out, int32_t* hit_seg_out, int32_t* near_out, float* pen_out,
                                          uint8_t* swinging_out, uint8_t* clear_out, hipStream_t st);
#endif
