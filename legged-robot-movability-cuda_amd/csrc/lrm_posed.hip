// lrm_posed.hip -- batched multi-pose reach / distance queries (lrm_pose_compile_dev, lrm_reach_dist_posed_dev).
//
// Query i = (target i, pose pose_idx[i], leg leg_idx[i]); p = target - body[pose] in f32; the outputs are
// reachability_global / distance_global of p for (legs[leg], quats[pose]) in the reference's operation order
// (lrm_point.h, LRM_MODE_STRICT), bit-identical to the single-pose calls.
//
// Two kernels:
//  * pose_compile_kernel: one thread per (pose, leg) record.  The record (LrmPoseRecord, 512 B) is the strict
//    head of lrm_compile_leg(leg, quat, 1) -- lrm_compile_head.h, the host compiler's own arithmetic -- plus the
//    pose's body position.  Reads the quaternions and body positions where the caller keeps them (device), the
//    legs from the kernarg segment: no allocation, no host round trip, graph-capturable.
//  * posed_kernel: one query per lane.  Each wave checks with one ballot whether all its active lanes share one
//    record (the pair-major layout [pose, leg, target]):
//      - yes: the record address is wave-uniform (readfirstlane): its scalar constants come through s_load (the
//        scalar cache), its 4 x 4 circle table (256 B, per-lane indexed by the region) is copied to the wave's
//        LDS slot -- one float per lane -- whenever the wave's record changes;
//      - no (interleaved or shuffled queries): every lane reads its own record with vector loads.  The table is
//        nposes x nlegs x 512 B (12.6 MB for 4096 x 6): it stays in L2 / the Infinity Cache.
//    Out-of-range indices are clamped before any load (the kernel never reads outside the records) and the
//    query's outputs are then overwritten with mask 0, valid 0, nan field.
//
// Compiled with -ffp-contract=off (see lrm_point.h).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "lrm_compile_head.h"
#include "lrm_launch.h"
#include "lrm_point.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

struct PosedLegs { // the legs of a compile, by value in the kernarg segment (8 x 56 B)
    LrmLegDimensions l[LRM_MAX_LEGS];
};

__global__ __launch_bounds__(kBlock) void pose_compile_kernel(const float* __restrict__ quats, const float* __restrict__ body,
                                                              uint32_t nposes, uint32_t nlegs, const PosedLegs legs,
                                                              LrmPoseRecord* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (size_t)nposes * nlegs) return;
    const uint32_t pose = (uint32_t)(t / nlegs), leg = (uint32_t)(t % nlegs);
    const float q[4] = {quats[4 * (size_t)pose], quats[4 * (size_t)pose + 1], quats[4 * (size_t)pose + 2], quats[4 * (size_t)pose + 3]};
    LrmPoseRecord* r = out + t;
    lrm_compile_head(legs.l[leg], q, 1, &r->head, (LrmLegDimensions*)nullptr);
    r->body_pos[0] = body ? body[3 * (size_t)pose] : 0.f;
    r->body_pos[1] = body ? body[3 * (size_t)pose + 1] : 0.f;
    r->body_pos[2] = body ? body[3 * (size_t)pose + 2] : 0.f;
    for (int k = 0; k < 5; k++) r->pad_[k] = 0.f;
}

__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The strict evaluation of one query against a record's head.
// p: the body-relative target in, the distance vector out (kDist)
template <bool kReach, bool kDist>
__device__ __forceinline__ void eval_query(const LrmLegHead& L, const LrmCircle* lists, LrmVec3& p, bool& reach, bool& valid) {
    if (kReach) reach = lrm_reach_global(L, lists, p);
    if (kDist) valid = lrm_dist_global(L, lists, p);
    else (void)valid;
}

#ifndef LRM_POSED_MIN_WAVES
#define LRM_POSED_MIN_WAVES 4
#endif

// kReach: mask; kDist: validity byte + field.  Any output pointer may be null.
template <bool kReach, bool kDist>
__global__ __launch_bounds__(kBlock, LRM_POSED_MIN_WAVES) void posed_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, size_t n,
    const int32_t* __restrict__ pose_idx, const uint8_t* __restrict__ leg_idx, const LrmPoseRecord* __restrict__ recs,
    uint32_t nposes, uint32_t nlegs, uint8_t* __restrict__ mask, uint8_t* __restrict__ valid_out, float* __restrict__ dx,
    float* __restrict__ dy, float* __restrict__ dz) {
    __shared__ LrmCircle s_lists[kWaves][4 * LRM_N_CIRCLES];
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned lane = threadIdx.x & 63;
    LrmCircle* my_lists = s_lists[wave];
    uint32_t staged = 0xffffffffu; // record whose circle table the wave's LDS slot holds
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i0 = (size_t)blockIdx.x * kBlock + (size_t)wave * 64; i0 < n; i0 += stride) { // wave-uniform trip count
        const size_t i = i0 + lane;
        const bool act = i < n;
        const int32_t pi = (act && pose_idx) ? pose_idx[i] : 0;
        const uint32_t li = (act && leg_idx) ? leg_idx[i] : 0u;
        const bool in_range = (uint32_t)pi < nposes && li < nlegs;
        // clamp before any load of a record
        const uint32_t r = (in_range ? (uint32_t)pi : 0u) * nlegs + (in_range ? li : 0u);
        const uint32_t r0 = __builtin_amdgcn_readfirstlane(r); // lane 0 is active whenever the wave iterates
        const bool uniform = __ballot(act && r != r0) == 0;
        LrmVec3 p{0.f, 0.f, 0.f};
        if (act) p = LrmVec3{x[i], y[i], z[i]};
        bool reach = false, v = false;
        if (uniform) {
            const LrmPoseRecord& R = lrm_fresh(recs[r0]);
            if (r0 != staged) {
                wave_lds_fence(); // every lane is done with the previous table
                reinterpret_cast<float*>(my_lists)[lane] = reinterpret_cast<const float*>(&recs[r0].head.lists[0][0])[lane];
                wave_lds_fence();
                staged = r0;
            }
            p.x -= R.body_pos[0];
            p.y -= R.body_pos[1];
            p.z -= R.body_pos[2];
            eval_query<kReach, kDist>(R.head, my_lists, p, reach, v);
        } else {
            const LrmPoseRecord& R = recs[r];
            p.x -= R.body_pos[0];
            p.y -= R.body_pos[1];
            p.z -= R.body_pos[2];
            eval_query<kReach, kDist>(R.head, &R.head.lists[0][0], p, reach, v);
        }
        if (act) {
            if (!in_range) {
                reach = v = false;
                p.x = p.y = p.z = __builtin_nanf("");
            }
            if (kReach && mask) mask[i] = reach;
            if (kDist) {
                if (valid_out) valid_out[i] = v;
                if (dx) {
                    dx[i] = p.x;
                    dy[i] = p.y;
                    dz[i] = p.z;
                }
            }
        }
    }
}

int grid_for_posed(size_t n) {
    // compute-bound with a data-dependent iteration time: several workgroups per resident one (256 CUs) even out the tail
    size_t g = (n + kBlock - 1) / kBlock;
    const size_t cap = 256 * 8 * 8;
    if (g > cap) g = cap;
    return (int)(g < 1 ? 1 : g);
}

} // namespace

hipError_t lrm_launch_pose_compile(const float* quats, const float* body, size_t nposes, const LrmLegDimensions* legs,
                                   size_t nlegs, void* records, hipStream_t st) {
    PosedLegs L{};
    for (size_t k = 0; k < nlegs; k++) L.l[k] = legs[k];
    const size_t total = nposes * nlegs;
    const int grid = (int)((total + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(pose_compile_kernel, dim3(grid), dim3(kBlock), 0, st, quats, body, (uint32_t)nposes, (uint32_t)nlegs, L,
                       (LrmPoseRecord*)records);
    return hipGetLastError();
}

hipError_t lrm_launch_posed(const float* x, const float* y, const float* z, size_t n, const int32_t* pose_idx,
                            const uint8_t* leg_idx, const void* records, size_t nposes, size_t nlegs, uint8_t* mask,
                            uint8_t* valid, float* dx, float* dy, float* dz, hipStream_t st) {
    const LrmPoseRecord* R = (const LrmPoseRecord*)records;
    const bool want_dist = valid || dx;
    const dim3 grid(grid_for_posed(n));
    if (mask && want_dist)
        hipLaunchKernelGGL((posed_kernel<true, true>), grid, dim3(kBlock), 0, st, x, y, z, n, pose_idx, leg_idx, R, (uint32_t)nposes,
                           (uint32_t)nlegs, mask, valid, dx, dy, dz);
    else if (want_dist)
        hipLaunchKernelGGL((posed_kernel<false, true>), grid, dim3(kBlock), 0, st, x, y, z, n, pose_idx, leg_idx, R, (uint32_t)nposes,
                           (uint32_t)nlegs, mask, valid, dx, dy, dz);
    else
        hipLaunchKernelGGL((posed_kernel<true, false>), grid, dim3(kBlock), 0, st, x, y, z, n, pose_idx, leg_idx, R, (uint32_t)nposes,
                           (uint32_t)nlegs, mask, valid, dx, dy, dz);
    return hipGetLastError();
}
