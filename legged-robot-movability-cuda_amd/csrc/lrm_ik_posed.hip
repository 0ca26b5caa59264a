// lrm_ik_posed.hip -- joint-angle queries per (target, pose, leg): lrm_pose_ik_compile_dev, lrm_ik_posed_dev, lrm_fk_posed_dev.
//
// Query i = (target target_idx[i] (or i), pose pose_idx[i], leg leg_idx[i]); p = target - body[pose] in f32; the angles
// and the status are lrm_ik_point's (lrm_ik.h) for (legs[leg], quats[pose]), bit-identical to the single-pose calls.
//
// Two tables, both one entry per (pose, leg) at pose * nlegs + leg: the pose records of lrm_posed.hip (LrmPoseRecord,
// 512 B: the strict head + the body position) and the IK constants (LrmIkLeg, 128 B), which have no room in the record.
//  * pose_ik_compile_kernel: one thread per (pose, leg): lrm_ik_compile_pose (lrm_ik.h), the host's own arithmetic.
//  * ik_posed_kernel / fk_posed_kernel: one query per lane, posed_kernel's shape (lrm_posed.hip).  One ballot per wave
//    tells whether all its active lanes share a (pose, leg): then both addresses are wave-uniform (readfirstlane), the
//    head and the IK constants come through s_load, and the circle table sits in the wave's LDS slot, copied when the
//    wave's record changes.  Otherwise (the [l*nb + b] order of lrm_footholds_dev: a pose per lane) every lane reads its
//    own two entries with vector loads.
//    Pose, leg and target indices are clamped before any load (the kernels never read outside their tables); a query
//    with one out of range gets status LRM_IK_NONE and nan angles (a nan position from the FK).
//
// Compiled with -ffp-contract=off (see lrm_point.h).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "lrm_compile_head.h"
#include "lrm_ik.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

struct PosedLegs { // the legs of a compile, by value in the kernarg segment (8 x 56 B)
    LrmLegDimensions l[LRM_MAX_LEGS];
};

__global__ __launch_bounds__(kBlock) void pose_ik_compile_kernel(const float* __restrict__ quats, uint32_t nposes, uint32_t nlegs,
                                                                 const PosedLegs legs, LrmIkLeg* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (size_t)nposes * nlegs) return;
    const uint32_t pose = (uint32_t)(t / nlegs), leg = (uint32_t)(t % nlegs);
    const float q[4] = {quats[4 * (size_t)pose], quats[4 * (size_t)pose + 1], quats[4 * (size_t)pose + 2], quats[4 * (size_t)pose + 3]};
    LrmIkLeg K;
    lrm_ik_compile_pose(legs.l[leg], q, &K);
    out[t] = K;
}

__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The (pose, leg) entry of a lane, clamped into the tables; ok: both indices were in range.
__device__ __forceinline__ uint32_t entry_of(bool act, size_t i, const int32_t* pose_idx, const uint8_t* leg_idx, uint32_t nposes,
                                             uint32_t nlegs, bool& ok) {
    const int32_t pi = (act && pose_idx) ? pose_idx[i] : 0;
    const uint32_t li = (act && leg_idx) ? leg_idx[i] : 0u;
    ok = (uint32_t)pi < nposes && li < nlegs;
    return (ok ? (uint32_t)pi : 0u) * nlegs + (ok ? li : 0u);
}

#ifndef LRM_IK_POSED_MIN_WAVES
#define LRM_IK_POSED_MIN_WAVES 4
#endif

__global__ __launch_bounds__(kBlock, LRM_IK_POSED_MIN_WAVES) void ik_posed_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, uint32_t nt,
    const int32_t* __restrict__ target_idx, size_t n, const int32_t* __restrict__ pose_idx, const uint8_t* __restrict__ leg_idx,
    const LrmPoseRecord* __restrict__ recs, const LrmIkLeg* __restrict__ iks, uint32_t nposes, uint32_t nlegs,
    const float* __restrict__ seed_c, const float* __restrict__ seed_f, const float* __restrict__ seed_t, float* __restrict__ coxa,
    float* __restrict__ femur, float* __restrict__ tibia, uint8_t* __restrict__ status) {
    __shared__ LrmCircle s_lists[kWaves][4 * LRM_N_CIRCLES];
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned lane = threadIdx.x & 63;
    LrmCircle* my_lists = s_lists[wave];
    uint32_t staged = 0xffffffffu; // record whose circle table the wave's LDS slot holds
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i0 = (size_t)blockIdx.x * kBlock + (size_t)wave * 64; i0 < n; i0 += stride) { // wave-uniform trip count
        const size_t i = i0 + lane;
        const bool act = i < n;
        bool in_range;
        const uint32_t r = entry_of(act, i, pose_idx, leg_idx, nposes, nlegs, in_range); // clamped before any table load
        // the target: index i without target_idx (n <= nt then); a negative or too large index loads nothing
        const uint32_t ti = target_idx ? (act ? (uint32_t)target_idx[i] : 0u) : (uint32_t)i;
        const bool t_ok = act && ti < nt;
        in_range = in_range && t_ok;
        LrmVec3 p{0.f, 0.f, 0.f};
        if (t_ok) p = LrmVec3{x[ti], y[ti], z[ti]};
        LrmVec3 seed{0.f, 0.f, 0.f};
        if (seed_c && act) seed = LrmVec3{seed_c[i], seed_f[i], seed_t[i]};
        const uint32_t r0 = __builtin_amdgcn_readfirstlane(r); // lane 0 is active whenever the wave iterates
        const bool uniform = __ballot(act && r != r0) == 0;
        LrmVec3 ang;
        uint8_t st;
        if (uniform) {
            const LrmPoseRecord& R = lrm_fresh(recs[r0]);
            const LrmIkLeg& K = lrm_fresh(iks[r0]);
            if (r0 != staged) {
                wave_lds_fence(); // every lane is done with the previous table
                reinterpret_cast<float*>(my_lists)[lane] = reinterpret_cast<const float*>(&recs[r0].head.lists[0][0])[lane];
                wave_lds_fence();
                staged = r0;
            }
            p.x -= R.body_pos[0];
            p.y -= R.body_pos[1];
            p.z -= R.body_pos[2];
            if (!seed_c) seed = LrmVec3{K.seed[0], K.seed[1], K.seed[2]};
            st = lrm_ik_point(R.head, my_lists, K, p, seed, ang);
        } else {
            const LrmPoseRecord& R = recs[r];
            const LrmIkLeg& K = iks[r];
            p.x -= R.body_pos[0];
            p.y -= R.body_pos[1];
            p.z -= R.body_pos[2];
            if (!seed_c) seed = LrmVec3{K.seed[0], K.seed[1], K.seed[2]};
            st = lrm_ik_point(R.head, &R.head.lists[0][0], K, p, seed, ang);
        }
        if (act) {
            if (!in_range) {
                st = LRM_IK_NONE;
                ang.x = ang.y = ang.z = __builtin_nanf("");
            }
            coxa[i] = ang.x;
            femur[i] = ang.y;
            tibia[i] = ang.z;
            status[i] = st;
        }
    }
}

__global__ __launch_bounds__(kBlock) void fk_posed_kernel(const float* __restrict__ coxa, const float* __restrict__ femur,
                                                          const float* __restrict__ tibia, size_t n,
                                                          const int32_t* __restrict__ pose_idx, const uint8_t* __restrict__ leg_idx,
                                                          const LrmPoseRecord* __restrict__ recs, const LrmIkLeg* __restrict__ iks,
                                                          uint32_t nposes, uint32_t nlegs, float* __restrict__ x,
                                                          float* __restrict__ y, float* __restrict__ z) {
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned lane = threadIdx.x & 63;
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i0 = (size_t)blockIdx.x * kBlock + (size_t)wave * 64; i0 < n; i0 += stride) { // wave-uniform trip count
        const size_t i = i0 + lane;
        const bool act = i < n;
        bool in_range;
        const uint32_t r = entry_of(act, i, pose_idx, leg_idx, nposes, nlegs, in_range);
        const uint32_t r0 = __builtin_amdgcn_readfirstlane(r);
        const bool uniform = __ballot(act && r != r0) == 0;
        float c = 0.f, f = 0.f, t = 0.f;
        if (act) {
            c = coxa[i];
            f = femur[i];
            t = tibia[i];
        }
        LrmVec3 p;
        if (uniform) {
            const LrmPoseRecord& R = lrm_fresh(recs[r0]);
            const LrmIkLeg& K = lrm_fresh(iks[r0]);
            p = lrm_fk_point(R.head, K, c, f, t);
            p.x += R.body_pos[0];
            p.y += R.body_pos[1];
            p.z += R.body_pos[2];
        } else {
            const LrmPoseRecord& R = recs[r];
            p = lrm_fk_point(R.head, iks[r], c, f, t);
            p.x += R.body_pos[0];
            p.y += R.body_pos[1];
            p.z += R.body_pos[2];
        }
        if (act) {
            if (!in_range) p.x = p.y = p.z = __builtin_nanf("");
            x[i] = p.x;
            y[i] = p.y;
            z[i] = p.z;
        }
    }
}

int grid_for(size_t n, size_t cap) {
    // compute-bound with a data-dependent iteration time: several workgroups per resident one (256 CUs) even out the tail
    size_t g = (n + kBlock - 1) / kBlock;
    if (g > cap) g = cap;
    return (int)(g < 1 ? 1 : g);
}

} // namespace

hipError_t lrm_launch_pose_ik_compile(const float* quats, size_t nposes, const LrmLegDimensions* legs, size_t nlegs, void* ik_records,
                                      hipStream_t st) {
    PosedLegs L{};
    for (size_t k = 0; k < nlegs; k++) L.l[k] = legs[k];
    const size_t total = nposes * nlegs;
    const int grid = (int)((total + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(pose_ik_compile_kernel, dim3(grid), dim3(kBlock), 0, st, quats, (uint32_t)nposes, (uint32_t)nlegs, L,
                       (LrmIkLeg*)ik_records);
    return hipGetLastError();
}

hipError_t lrm_launch_ik_posed(const float* x, const float* y, const float* z, size_t nt, const int32_t* target_idx, size_t n,
                               const int32_t* pose_idx, const uint8_t* leg_idx, const void* records, const void* ik_records,
                               size_t nposes, size_t nlegs, const float* seed_c, const float* seed_f, const float* seed_t,
                               float* coxa, float* femur, float* tibia, uint8_t* status, hipStream_t st) {
    hipLaunchKernelGGL(ik_posed_kernel, dim3(grid_for(n, 256 * LRM_IK_POSED_MIN_WAVES * 8)), dim3(kBlock), 0, st, x, y, z,
                       (uint32_t)nt, target_idx, n, pose_idx, leg_idx, (const LrmPoseRecord*)records, (const LrmIkLeg*)ik_records,
                       (uint32_t)nposes, (uint32_t)nlegs, seed_c, seed_f, seed_t, coxa, femur, tibia, status);
    return hipGetLastError();
}

hipError_t lrm_launch_fk_posed(const float* coxa, const float* femur, const float* tibia, size_t n, const int32_t* pose_idx,
                               const uint8_t* leg_idx, const void* records, const void* ik_records, size_t nposes, size_t nlegs,
                               float* x, float* y, float* z, hipStream_t st) {
    hipLaunchKernelGGL(fk_posed_kernel, dim3(grid_for(n, 256 * 32)), dim3(kBlock), 0, st, coxa, femur, tibia, n, pose_idx, leg_idx,
                       (const LrmPoseRecord*)records, (const LrmIkLeg*)ik_records, (uint32_t)nposes, (uint32_t)nlegs, x, y, z);
    return hipGetLastError();
}
