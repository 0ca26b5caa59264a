// lrm_trunk_clearance.hip -- gfx950 kernels of lrm_trunk_clearance_posed_dev and lrm_dbg_trunk_link_dist_dev: per set (a pose
// and three joint angles per leg), how close do the links of every leg come to the robot's own trunk, the body cylinder of
// lrm_body_clearance_posed_dev: per (set, leg) the links that hit, the deepest link within `margin` and its pen; per set
// whether no leg hits.
// The joints are lrm_leg_clearance.h's; the cylinder distance, the test and the per-leg answer lrm_trunk_clearance.h's, shared
// with the host loop; this file only spreads them over lanes.
//
// trunk_clearance_posed_kernel: lane = (set, leg slot).  A wave holds 8 sets of LRM_MAX_LEGS = 8 leg slots, so the legs of a
// set are 8 adjacent lanes and a workgroup holds kSetsPerBlock = 32 sets; the grid is capped and strides over the rest, a wave
// at a time, so every lane of a wave takes the same number of rounds and the ballot below is always whole.
//   Each lane with slot < nlegs of a live set reads its own two table entries and three angles, runs lrm_leg_joints and
//   lrm_trunk_leg (three links of LRM_TRUNK_ROUNDS ternary rounds in registers) and stores its own row.
//   free: one ballot of "valid and some link hits", shifted to the set's 8 lanes; slot 0 stores it.
// A leg's answer depends on nothing but its own record and angles, so the mapping decides no output.  No LDS, no atomics,
// no global scratch, no __syncthreads.  A dead set (live_in 0, pose out of range) is answered before any table or angle is
// read; slots at or above nlegs read and write nothing.
//
// Compiled with -ffp-contract=off (see lrm_point.h).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "lrm_types.h"
#include "lrm_compile_head.h"
#include "lrm_point.h"
#include "lrm_ik.h"
#include "lrm_trunk_clearance.h"

namespace {

constexpr int kBlock = 256;
constexpr int kSetsPerBlock = kBlock / LRM_MAX_LEGS;
constexpr unsigned kMaxGrid = 2048; // 65 536 sets in flight (eight workgroups per CU); a wave strides over the rest
static_assert(LRM_MAX_LEGS == 8, "a set's legs are 8 adjacent lanes");

__global__ __launch_bounds__(kBlock) void trunk_clearance_posed_kernel(
    const LrmPoseRecord* __restrict__ recs, const LrmIkLeg* __restrict__ iks, uint32_t nposes, uint32_t nlegs,
    const int32_t* __restrict__ pose_idx /* may be null */, uint32_t nsets, const float* __restrict__ coxa,
    const float* __restrict__ femur, const float* __restrict__ tibia, const LrmTrunkRadii R, const LrmTrunk C, float tip_clear,
    const uint8_t* __restrict__ live_in /* may be null */, uint8_t* __restrict__ links_out, uint8_t* __restrict__ worst_out,
    float* __restrict__ pen_out /* may be null */, uint8_t* __restrict__ free_out /* may be null */) {
    const uint32_t slot = threadIdx.x & (LRM_MAX_LEGS - 1);   // the leg
    const uint32_t in_block = threadIdx.x / LRM_MAX_LEGS;     // the set within the workgroup
    const uint32_t wave_first = (threadIdx.x & ~63u) / LRM_MAX_LEGS; // the first set of this lane's wave within the workgroup
    const unsigned group = (threadIdx.x & 63u) & ~(LRM_MAX_LEGS - 1u); // the first lane of the set's 8 within the wave
    // wave-uniform loop: base is the first set of the WAVE, so all 64 lanes leave together
    for (uint64_t base = (uint64_t)blockIdx.x * kSetsPerBlock; base + wave_first < nsets; base += (uint64_t)gridDim.x * kSetsPerBlock) {
        const uint64_t s64 = base + in_block;
        const bool have = s64 < nsets && slot < nlegs;
        const uint32_t s = (uint32_t)s64;
        bool live = false;
        int32_t p = 0;
        if (have) {
            p = pose_idx ? pose_idx[s] : (int32_t)s;
            live = !(live_in && live_in[s] == 0) && p >= 0 && (uint32_t)p < nposes;
        }
        LrmTrunkLeg A = lrm_trunk_leg_empty();
        if (live) {
            const size_t rec = (size_t)p * nlegs + slot;
            const size_t o = (size_t)slot * nsets + s;
            LrmVec3 J[4];
            lrm_leg_joints(recs[rec].head, iks[rec], coxa[o], femur[o], tibia[o], tip_clear, J);
            if (lrm_leg_joints_finite(J)) A = lrm_trunk_leg(C, R, recs[rec].head.inv_rot, J);
        }
        if (have) {
            const size_t o = (size_t)slot * nsets + s; // < 2^32 (checked by the C ABI)
            links_out[o] = (uint8_t)A.links;
            worst_out[o] = (uint8_t)A.worst;
            if (pen_out) pen_out[o] = A.pen;
        }
        const unsigned long long hit = __ballot(A.links != 0u); // slots at or above nlegs and dead sets keep the empty answer
        if (free_out && have && slot == 0) free_out[s] = live && ((hit >> group) & 0xffull) == 0ull;
    }
}

__global__ __launch_bounds__(kBlock) void trunk_link_dist_kernel(const float* __restrict__ segs, size_t n, const LrmTrunk C,
                                                                 float* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const float* g = segs + i * 6;
        out[i] = lrm_trunk_link_dist(C, LrmVec3{g[0], g[1], g[2]}, LrmVec3{g[3], g[4], g[5]});
    }
}

} // namespace

hipError_t lrm_launch_trunk_clearance_posed(const void* records, const void* ik_records, size_t nposes, size_t nlegs,
                                            const int32_t* pose_idx, size_t nsets, const float* coxa, const float* femur,
                                            const float* tibia, const float radius[3], float margin, float tip_clear,
                                            float trunk_radius, float plus_z, float minus_z, uint32_t links, const uint8_t* live_in,
                                            uint8_t* links_out, uint8_t* worst_out, float* pen_out, uint8_t* free_out, hipStream_t st) {
    size_t g = (nsets + kSetsPerBlock - 1) / kSetsPerBlock;
    if (g > kMaxGrid) g = kMaxGrid;
    hipLaunchKernelGGL(trunk_clearance_posed_kernel, dim3((unsigned)g), dim3(kBlock), 0, st, (const LrmPoseRecord*)records,
                       (const LrmIkLeg*)ik_records, (uint32_t)nposes, (uint32_t)nlegs, pose_idx, (uint32_t)nsets, coxa, femur, tibia,
                       lrm_trunk_radii(radius, margin, links), LrmTrunk{trunk_radius, plus_z, minus_z}, tip_clear, live_in, links_out,
                       worst_out, pen_out, free_out);
    return hipGetLastError();
}

hipError_t lrm_launch_trunk_link_dist(const float* segs, size_t n, float trunk_radius, float plus_z, float minus_z, float* out,
                                      hipStream_t st) {
    size_t g = (n + kBlock - 1) / kBlock;
    if (g > kMaxGrid) g = kMaxGrid;
    hipLaunchKernelGGL(trunk_link_dist_kernel, dim3((unsigned)(g < 1 ? 1 : g)), dim3(kBlock), 0, st, segs, n,
                       LrmTrunk{trunk_radius, plus_z, minus_z}, out);
    return hipGetLastError();
}
