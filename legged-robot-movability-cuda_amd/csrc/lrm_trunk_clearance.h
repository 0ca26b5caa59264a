// lrm_trunk_clearance.h -- the arithmetic of lrm_trunk_clearance_posed_dev / _cpu (include/lrm.h): how close do the links of
// a leg come to the robot's own trunk, the body cylinder of lrm_body_clearance_posed_dev, under given joint angles.  One source
// for the kernel (lrm_trunk_clearance.hip) and the host loop (lrm_capi.cpp): float32 only, no contraction, only + - * /,
// comparisons and lrm_sqrtf, so that both give the same bits.  The joints are lrm_leg_clearance.h's (lrm_leg_joints, with
// tip_clear), which this header includes and leaves alone; everything that decides an output is here, the kernel only spreads
// it over lanes.
#pragma once
#include <stdint.h>
#include "lrm_leg_clearance.h"

#define LRM_TRUNK_ROUNDS 32 // N: rounds of the ternary search along a link; [lo, hi] shrinks to (2/3)^32 = 2.3e-6 of the link

// The body cylinder in the BODY frame: axis z, centred on the body origin, radius R, minus_z <= z <= plus_z.
struct LrmTrunk {
    float R, plus_z, minus_z;
};

// h(P): the squared distance of the body-frame point P to the solid cylinder; 0 inside.  Convex in P.
LRM_HD float lrm_trunk_h(const LrmTrunk C, float x, float y, float z) {
    const float rho = lrm_sqrtf(x * x + y * y);
    const float dr = rho > C.R ? rho - C.R : 0.f;
    const float dz = z > C.plus_z ? z - C.plus_z : (z < C.minus_z ? C.minus_z - z : 0.f);
    return dr * dr + dz * dz;
}
// A joint (caller's frame, relative to the body) in the body frame, as lrm_body_clearance.h takes a target
LRM_HD LrmVec3 lrm_trunk_to_body(const float* inv_rot, LrmVec3 J) { return lrm_qrot(inv_rot, J); }

// The distance of the link from A to B (body frame) to the cylinder: h is convex along the link, so a ternary search of
// LRM_TRUNK_ROUNDS rounds on the parameter u of P(u) = A + u (B - A) closes in on its minimum; d is the square root of the
// least h evaluated, h(A) and h(B) included (best = h(A), then every further value by h < best ? h : best, h(B) first and
// then m1 and m2 of each round).  Every candidate is the distance of a point of the link, so d never under-reports; what the
// search over-reports is measured.
LRM_HD float lrm_trunk_link_dist(const LrmTrunk C, LrmVec3 A, LrmVec3 B) {
    const float ex = B.x - A.x, ey = B.y - A.y, ez = B.z - A.z;
    float best = lrm_trunk_h(C, A.x, A.y, A.z);
    float hk = lrm_trunk_h(C, B.x, B.y, B.z);
    best = hk < best ? hk : best;
    float lo = 0.f, hi = 1.f;
    for (int i = 0; i < LRM_TRUNK_ROUNDS; i++) {
        const float w = (hi - lo) / 3.f;
        const float m1 = lo + w, m2 = hi - w;
        const float h1 = lrm_trunk_h(C, A.x + m1 * ex, A.y + m1 * ey, A.z + m1 * ez);
        const float h2 = lrm_trunk_h(C, A.x + m2 * ex, A.y + m2 * ey, A.z + m2 * ez);
        best = h1 < best ? h1 : best;
        best = h2 < best ? h2 : best;
        if (h1 <= h2)
            hi = m2;
        else
            lo = m1;
    }
    return lrm_sqrtf(best);
}

// The three sums radius[k] + margin, formed once per call, and the links that are tested: bit k of `links` set and
// radius[k] != 0.
struct LrmTrunkRadii {
    float radius[3], reach[3];
    uint32_t tested;
};
LRM_HD LrmTrunkRadii lrm_trunk_radii(const float radius[3], float margin, uint32_t links) {
    LrmTrunkRadii R;
    R.tested = 0u;
    for (int k = 0; k < 3; k++) {
        R.radius[k] = radius[k];
        R.reach[k] = radius[k] + margin;
        if (((links >> k) & 1u) && radius[k] != 0.f) R.tested |= 1u << k;
    }
    return R;
}

// What a leg keeps: the hit bits, the near link with the largest pen (ties to the smaller k; 255: none) and that pen (-inf).
struct LrmTrunkLeg {
    uint32_t links, worst;
    float pen;
};
LRM_HD LrmTrunkLeg lrm_trunk_leg_empty() { return LrmTrunkLeg{0u, 255u, -__builtin_inff()}; }

// One valid leg: J[0..3] relative to the body in the caller's frame, inv_rot the pose record's.  hit_k = d_k < radius[k],
// near_k = d_k < reach[k], pen_k = (radius[k] - d_k) + 0 (-0 turned into +0); a nan d is neither.  hit implies near
// (margin >= 0, rounding is monotone).
LRM_HD LrmTrunkLeg lrm_trunk_leg(const LrmTrunk C, const LrmTrunkRadii& R, const float* inv_rot, const LrmVec3 J[4]) {
    LrmTrunkLeg A = lrm_trunk_leg_empty();
    if (R.tested == 0u) return A;
    LrmVec3 v[4];
    for (int k = 0; k < 4; k++) v[k] = lrm_trunk_to_body(inv_rot, J[k]);
    for (int k = 0; k < 3; k++) {
        if (!((R.tested >> k) & 1u)) continue;
        const float d = lrm_trunk_link_dist(C, v[k], v[k + 1]);
        if (!(d < R.reach[k])) continue;
        const float pen = (R.radius[k] - d) + 0.f;
        if (d < R.radius[k]) A.links |= 1u << k;
        if (A.worst == 255u || pen > A.pen) {
            A.worst = (uint32_t)k;
            A.pen = pen;
        }
    }
    return A;
}

#if defined(__HIPCC__)
// launch functions (lrm_trunk_clearance.hip); only launch.  records / ik_records: the pose and IK tables (entry of
// (pose, leg) at pose * nlegs + leg); angles and per-(set, leg) outputs at [l * nsets + s]; everything is checked by the C
// ABI: nsets >= 1, nlegs in 1..8, nlegs * nsets < 2^32.  pose_idx, live_in, pen_out, free_out may be null.
hipError_t lrm_launch_trunk_clearance_posed(const void* records, const void* ik_records, size_t nposes, size_t nlegs,
                                            const int32_t* pose_idx, size_t nsets, const float* coxa, const float* femur,
                                            const float* tibia, const float radius[3], float margin, float tip_clear,
                                            float trunk_radius, float plus_z, float minus_z, uint32_t links, const uint8_t* live_in,
                                            uint8_t* links_out, uint8_t* worst_out, float* pen_out, uint8_t* free_out, hipStream_t st);
// out[i] = lrm_trunk_link_dist of segs[6 i ..]: A, B in the body frame; one link per lane
hipError_t lrm_launch_trunk_link_dist(const float* segs, size_t n, float trunk_radius, float plus_z, float minus_z, float* out,
                                      hipStream_t st);
#endif
