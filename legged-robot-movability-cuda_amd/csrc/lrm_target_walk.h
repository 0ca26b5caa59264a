// lrm_target_walk.h -- the small device helpers of the kernels that walk a target cloud with one wave per body, pose or edge
// (lrm_footholds.hip, lrm_footholds_posed.hip, lrm_foothold_misses.hip, lrm_body_clearance.hip, lrm_leg_clearance.hip;
// lrm_foothold_support.hip takes the fence and the minimum).  The walk itself, the survivor queue and the per-leg key fold
// stay written out in those kernels: DESIGN.md 3.18 has the figures of the attempt to share them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// orders a wave's LDS writes before its later LDS reads: the wave is the only user of its LDS slice, no __syncthreads
__device__ __forceinline__ void lrm_wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// squared distance of (x, y, z) from the box bb = (lo, hi) of tile_aabb_kernel (lrm_kernels.hip): a lower bound of the
// distance to every target inside it
__device__ __forceinline__ float lrm_box_dist2(const float* bb, float x, float y, float z) {
    const float ex = fmaxf(fmaxf(bb[0] - x, x - bb[3]), 0.f);
    const float ey = fmaxf(fmaxf(bb[1] - y, y - bb[4]), 0.f);
    const float ez = fmaxf(fmaxf(bb[2] - z, z - bb[5]), 0.f);
    return ex * ex + ey * ey + ez * ez;
}
__device__ __forceinline__ uint64_t lrm_min_u64(uint64_t a, uint64_t b) { return b < a ? b : a; }
// the wave's smallest key, in every lane: six xor steps
__device__ __forceinline__ uint64_t lrm_wave_min_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, off), hi = __shfl_xor((uint32_t)(v >> 32), off);
        v = lrm_min_u64(v, ((uint64_t)hi << 32) | lo);
    }
    return v;
}
