// lrm_ik.hip -- gfx950 kernels of the joint-angle queries (lrm_ik_dev, lrm_fk_dev): one point per lane, SoA in and out.
//
// The per-(leg, orientation) constants are two kernel arguments by value: the strict head of the compiled leg (LrmLegHead,
// 480 B) and LrmIkLeg (128 B).  No allocation, no host synchronisation: graph-capturable.  Both
// are read through the kernarg pointer (lrm_kernarg, as lrm_kernels.hip does) so that their loads stay s_loads at the
// point of use; the head's 4 x 4 circle table is staged in LDS (per-lane indexed by the region).
//
// ik_kernel: every lane runs the strict reach test; only the unreachable lanes (96 % of a config-2 cloud) then run the
// strict distance evaluation for their goal p - d; the candidate solve after it is the same code for both kinds of
// lane (lrm_ik.h: lrm_ik_point).
//
// Compiled with -ffp-contract=off (see lrm_point.h).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "lrm_compile_head.h"
#include "lrm_ik.h"

namespace {

constexpr int kBlock = 256;

struct KernargIk { // the leading parameters of both kernels, in order
    const float *a, *b, *c;
    size_t n;
    LrmLegHead H;
    LrmIkLeg K;
};
constexpr unsigned kHeadArg = (unsigned)offsetof(KernargIk, H), kIkArg = (unsigned)offsetof(KernargIk, K);
static_assert(kHeadArg == 32 && kIkArg == 512, "kernarg layout");

#ifndef LRM_IK_MIN_WAVES
#define LRM_IK_MIN_WAVES 4
#endif

__global__ __launch_bounds__(kBlock, LRM_IK_MIN_WAVES) void ik_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, size_t n, const LrmLegHead H_kernarg,
    const LrmIkLeg K_kernarg, const float* __restrict__ seed_c, const float* __restrict__ seed_f, const float* __restrict__ seed_t,
    float* __restrict__ coxa, float* __restrict__ femur, float* __restrict__ tibia, uint8_t* __restrict__ status) {
    __shared__ LrmCircle s_lists[4 * LRM_N_CIRCLES];
    const LrmLegHead& L = lrm_kernarg<LrmLegHead>(kHeadArg);
    const LrmIkLeg& K = lrm_kernarg<LrmIkLeg>(kIkArg);
    if (threadIdx.x < 64) reinterpret_cast<float*>(s_lists)[threadIdx.x] = reinterpret_cast<const float*>(&L.lists[0][0])[threadIdx.x];
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const LrmVec3 seed = seed_c ? LrmVec3{seed_c[i], seed_f[i], seed_t[i]} : LrmVec3{K.seed[0], K.seed[1], K.seed[2]};
        LrmVec3 ang;
        const uint8_t s = lrm_ik_point(L, s_lists, K, LrmVec3{x[i], y[i], z[i]}, seed, ang);
        coxa[i] = ang.x;
        femur[i] = ang.y;
        tibia[i] = ang.z;
        status[i] = s;
    }
}

__global__ __launch_bounds__(kBlock) void fk_kernel(const float* __restrict__ coxa, const float* __restrict__ femur,
                                                    const float* __restrict__ tibia, size_t n, const LrmLegHead H_kernarg,
                                                    const LrmIkLeg K_kernarg, float* __restrict__ x, float* __restrict__ y,
                                                    float* __restrict__ z) {
    const LrmLegHead& L = lrm_kernarg<LrmLegHead>(kHeadArg);
    const LrmIkLeg& K = lrm_kernarg<LrmIkLeg>(kIkArg);
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const LrmVec3 p = lrm_fk_point(L, K, coxa[i], femur[i], tibia[i]);
        x[i] = p.x;
        y[i] = p.y;
        z[i] = p.z;
    }
}

int grid_for(size_t n, size_t cap) {
    // compute-bound with a data-dependent iteration time: several workgroups per resident one (256 CUs) even out the tail
    size_t g = (n + kBlock - 1) / kBlock;
    if (g > cap) g = cap;
    return (int)(g < 1 ? 1 : g);
}

} // namespace

hipError_t lrm_launch_ik(const float* x, const float* y, const float* z, size_t n, const LrmCompiledLeg& L, const LrmIkLeg& K,
                         const float* seed_c, const float* seed_f, const float* seed_t, float* coxa, float* femur, float* tibia,
                         uint8_t* status, hipStream_t st) {
    hipLaunchKernelGGL(ik_kernel, dim3(grid_for(n, 256 * LRM_IK_MIN_WAVES * 8)), dim3(kBlock), 0, st, x, y, z, n, LrmLegHead(L), K,
                       seed_c, seed_f, seed_t, coxa, femur, tibia, status);
    return hipGetLastError();
}

hipError_t lrm_launch_fk(const float* coxa, const float* femur, const float* tibia, size_t n, const LrmCompiledLeg& L,
                         const LrmIkLeg& K, float* x, float* y, float* z, hipStream_t st) {
    hipLaunchKernelGGL(fk_kernel, dim3(grid_for(n, 256 * 32)), dim3(kBlock), 0, st, coxa, femur, tibia, n, LrmLegHead(L), K, x, y, z);
    return hipGetLastError();
}
