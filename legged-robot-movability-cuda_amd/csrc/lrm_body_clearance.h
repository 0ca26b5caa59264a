// lrm_body_clearance.h -- the per-(pose, target) arithmetic of lrm_body_clearance_posed_dev / _cpu (include/lrm.h): is the
// target inside the body volume of the pose, and how high does it stand over the belly plane.  One source for the kernel
// (lrm_body_clearance.hip) and the host loop (lrm_capi.cpp): float32 only, no contraction, so that both give the same
// bits.  These functions decide outputs; the kernel's box culls (see there) are only allowed to skip what they reject.
#pragma once
#include <stdint.h>
#include "lrm_point.h"

#define LRM_CLEARANCE_COLUMN 1u // in_cylinder(radius, plus_z, floor_z, 0, v)
#define LRM_CLEARANCE_HIT 2u    // in_cylinder(radius, plus_z, minus_z, 0, v); implies COLUMN (floor_z <= minus_z)

// q = t - body[p], already subtracted (one float32 subtraction per component); inv_rot: the pose record's.
// v = qtInvRotate(quats[p], q) as reachability_global forms it; in_cylinder is collision.cu.h:12-23 about the origin
// (t - 0 is t), norm3df restated as sqrtf of the sum in its order, as oracle/oracle.c does.  *height = v.z - minus_z with
// -0 turned into +0 (x + 0 is x for every other x).  A nan or infinite q gives a nan in v.x, v.y or v.z, or an
// infinite one: no bit is set.
LRM_HD unsigned lrm_clearance_test(const float* inv_rot, LrmVec3 q, float radius, float plus_z, float minus_z, float floor_z,
                                   float* height) {
    const LrmVec3 v = lrm_qrot(inv_rot, q);
    const bool in = (lrm_sqrtf(v.x * v.x + v.y * v.y + 0.f) < radius) && (v.z < plus_z);
    *height = (v.z - minus_z) + 0.f;
    return (in && v.z > floor_z ? LRM_CLEARANCE_COLUMN : 0u) | (in && v.z > minus_z ? LRM_CLEARANCE_HIT : 0u);
}

// 64-bit key of a column target: the smallest key is the largest height, ties the smallest index.  The high word is
// 0x7fffffff - bits for a height >= +0 and the bits themselves (sign set) for a negative one: it falls as the height
// rises.  The height of a column target is never nan, so no key equals kLrmClearanceNone.
constexpr uint64_t kLrmClearanceNone = ~0ull;
LRM_HD uint64_t lrm_clearance_key(float height, uint32_t index) {
    const uint32_t u = lrm_f2u(height);
    return ((uint64_t)((u >> 31) ? u : 0x7fffffffu - u) << 32) | index;
}
// What a key holds: the column target's index (< nt) and height, or -1 and -inf for kLrmClearanceNone.
struct LrmClearanceTop {
    int32_t index;
    float height;
};
LRM_HD LrmClearanceTop lrm_clearance_key_decode(uint64_t key) {
    const uint32_t h = (uint32_t)(key >> 32);
    const bool have = key != kLrmClearanceNone;
    return LrmClearanceTop{have ? (int32_t)(uint32_t)key : -1, have ? lrm_u2f((h >> 31) ? h : 0x7fffffffu - h) : -__builtin_inff()};
}
