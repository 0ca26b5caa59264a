// lrm_pose_edges.h -- the arithmetic of lrm_pose_edge_counts_dev / lrm_pose_edges_dev / lrm_pose_edges_cpu (include/lrm.h):
// which pose can step to which.  One source for the kernels (lrm_pose_edges.hip) and the host loop (lrm_capi.cpp): which pose
// is valid, the squared distance, the turn test, the box gap of the cull, the segment rule and the launch arithmetic.
// float32, compiled with -ffp-contract=off, every sum in the order written here, so device and host agree bit for bit.
//
// THE RELATION IS SYMMETRIC BIT FOR BIT.  dx = x_q - x_p is the exact negative of x_p - x_q (IEEE subtraction rounds to
// nearest, ties to even: symmetric about zero), so dx*dx is the same float either way and the three squares are summed in
// the same order; c and n_p*n_q are sums and products of commuting factors in an order that does not name p or q first.
// Hence neighbours(p, q) == neighbours(q, p), and d2 and cos2 of (p, q) are the bits of (q, p): form 1 is the exact
// symmetrisation of form 0.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "lrm_types.h"

#define LRM_EDGES_CHUNK 64  // poses per chunk: the lanes of a wave, one box per chunk
#define LRM_EDGES_ROUND 64  // boxes a wave tests per walk round, one per lane; also the chunks under one second-level box
#define LRM_EDGES_BLOCK 256 // threads per workgroup: LRM_EDGES_BLOCK / LRM_EDGES_CHUNK waves, a chunk each
#define LRM_EDGES_BOX_FLOATS 8 // a chunk box in the workspace: lo.xyz, the number of valid poses, hi.xyz, 0

// finite: every comparison with a NaN is false
LRM_HD bool lrm_edges_finite(float v) { return (v < 0.f ? -v : v) <= 3.40282347e38f; }

// The pose as the pair test reads it: v[0..2] the body (0 with body == NULL), v[3] = n_p, v[4..7] the quaternion in storage
// order.  Returns VALID: live, three finite body coordinates, n_p finite and > 0.
LRM_HD bool lrm_edges_pose(const float* quats, const float* body, const uint8_t* pose_live, size_t p, float v[8]) {
    const float q0 = quats[4 * p], q1 = quats[4 * p + 1], q2 = quats[4 * p + 2], q3 = quats[4 * p + 3];
    v[0] = body ? body[3 * p] : 0.f;
    v[1] = body ? body[3 * p + 1] : 0.f;
    v[2] = body ? body[3 * p + 2] : 0.f;
    v[3] = ((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3;
    v[4] = q0, v[5] = q1, v[6] = q2, v[7] = q3;
    const bool live = !(pose_live && pose_live[p] == 0);
    return live && lrm_edges_finite(v[0]) && lrm_edges_finite(v[1]) && lrm_edges_finite(v[2]) && lrm_edges_finite(v[3]) && v[3] > 0.f;
}

// d2 of the pair: (dx*dx + dy*dy) + dz*dz with dx = x_q - x_p
LRM_HD float lrm_edges_d2(float px, float py, float pz, float qx, float qy, float qz) {
    const float dx = qx - px, dy = qy - py, dz = qz - pz;
    return (dx * dx + dy * dy) + dz * dz;
}

// c of the pair: ((p0*q0 + p1*q1) + p2*q2) + p3*q3
LRM_HD float lrm_edges_dot(const float* p, const float* q) { return ((p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]) + p[3] * q[3]; }

// the turn test: c*c >= dot2 * (n_p * n_q); false when a side is NaN (0 * inf: dot2 == 0 with an overflowing n_p * n_q)
LRM_HD bool lrm_edges_turn(float c, float np, float nq, float dot2) { return c * c >= dot2 * (np * nq); }

// cos2 of the pair: (c*c) / (n_p*n_q), one IEEE division
LRM_HD float lrm_edges_cos2(float c, float np, float nq) { return (c * c) / (np * nq); }

// The gap between two boxes along one axis, max(lo_b - hi_a, lo_a - hi_b, 0): a lower bound of |x_q - x_p| AS COMPUTED for
// every x_p in [lo_a, hi_a] and x_q in [lo_b, hi_b], since float32 subtraction is monotone in both operands.
LRM_HD float lrm_edges_gap(float lo_a, float hi_a, float lo_b, float hi_b) {
    const float u = lo_b - hi_a, w = lo_a - hi_b;
    const float m = u > w ? u : w;
    return m > 0.f ? m : 0.f;
}

// The gap of two boxes (LRM_EDGES_BOX_FLOATS each) squared and summed in d2's order: a lower bound of every pair's computed
// d2 (multiplication of non-negative floats and addition are monotone too), so culling on `> step2` loses no pair.
LRM_HD float lrm_edges_box_gap2(const float* a, const float* b) {
    const float gx = lrm_edges_gap(a[0], a[4], b[0], b[4]), gy = lrm_edges_gap(a[1], a[5], b[1], b[5]), gz = lrm_edges_gap(a[2], a[6], b[2], b[6]);
    return (gx * gx + gy * gy) + gz * gz;
}

// The segment of row p: lrm_foothold_lists_posed_dev's rule.  *base = offsets[p]; returns the room,
// min(offsets[p + 1], capacity) - base, and 0 if that is negative or base < 0: [base, base + room) lies inside [0, capacity).
LRM_HD int64_t lrm_edges_room(const int64_t* offsets, size_t p, int64_t capacity, int64_t* base) {
    const int64_t b = offsets[p], e = offsets[p + 1] < capacity ? offsets[p + 1] : capacity;
    *base = b;
    return (b >= 0 && e > b) ? e - b : 0;
}

inline uint64_t lrm_edges_chunks(size_t nposes) { return ((uint64_t)nposes + LRM_EDGES_CHUNK - 1) / LRM_EDGES_CHUNK; }
// second-level boxes: one per LRM_EDGES_ROUND consecutive chunks (the poses one walk round over chunk boxes covers)
inline uint64_t lrm_edges_supers(size_t nposes) { return (lrm_edges_chunks(nposes) + LRM_EDGES_ROUND - 1) / LRM_EDGES_ROUND; }

// The launch arithmetic of the count and fill kernels on nposes poses: out = {poses per chunk, boxes per walk round,
// workgroups, block}.  A wave owns a chunk, so a workgroup covers LRM_EDGES_BLOCK poses.
inline void lrm_edges_plan(size_t nposes, uint64_t out[4]) {
    out[0] = LRM_EDGES_CHUNK;
    out[1] = LRM_EDGES_ROUND;
    out[2] = ((uint64_t)nposes + LRM_EDGES_BLOCK - 1) / LRM_EDGES_BLOCK;
    out[3] = LRM_EDGES_BLOCK;
}

// the workspace: one box per chunk, then one box per LRM_EDGES_ROUND chunks (never 0 bytes, so that an allocation of it has
// an address)
inline size_t lrm_edges_workspace_bytes(size_t nposes) {
    const uint64_t c = lrm_edges_chunks(nposes) + lrm_edges_supers(nposes);
    return (size_t)(c ? c : 1) * LRM_EDGES_BOX_FLOATS * sizeof(float);
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// what the launches take; everything is checked by the C ABI (1 <= nposes <= INT32_MAX, form 0 or 1, step2 and dot2 not NaN)
struct LrmEdgesArgs {
    const float *quats, *body;
    const uint8_t* pose_live;
    uint32_t nposes;
    float step2, dot2;
    int form;
};
// launch functions (lrm_pose_edges.hip); each launches the two box kernels, then its own; only launches
hipError_t lrm_launch_pose_edge_counts(const LrmEdgesArgs& A, float* boxes, int32_t* count_out, hipStream_t st);
hipError_t lrm_launch_pose_edges(const LrmEdgesArgs& A, float* boxes, const int64_t* offsets, int64_t capacity, int32_t* edge_a_out,
                                 int32_t* edge_b_out, float* d2_out, float* cos2_out, int32_t* written_out, hipStream_t st);
#endif
