// lrm_dbg_math.hip -- the device side of lrm_dbg_exact_math_sums_dev: the checksums of lrm_dbg_math.h, one workgroup per
// block of 65536 bit patterns.  A diagnostic in a translation unit of its own, so that the device code of the product's
// kernels does not depend on it.  Compiled with the library's flags (-ffp-contract=off): what it sums is what the product's
// kernels compute.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "lrm_dbg_math.h"
#include "lrm_launch.h"

namespace {

constexpr int kBlock = 256; // four waves
constexpr int kWaves = kBlock / 64;

// Every lane accumulates its own j (j = lane, lane + 256, ...: 256 patterns), the wave adds its 64 lanes by shuffles, lane 0
// of wave 0 adds the four waves from LDS and stores the sum.  No atomics: a sum has one writer.
template <int kFn>
__global__ __launch_bounds__(kBlock) void exact_math_sums_kernel(uint32_t first_block, uint64_t* __restrict__ sums) {
    __shared__ uint64_t s_wave[kWaves];
    const uint32_t base = (first_block + blockIdx.x) * LRM_DBG_MATH_BLOCK; // first_block + blockIdx.x < 65536: no overflow
    uint64_t acc = 0;
    for (uint32_t j = threadIdx.x; j < LRM_DBG_MATH_BLOCK; j += kBlock) acc += lrm_dbg_math_term<kFn>(base + j, j);
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t total = 0;
        for (int w = 0; w < kWaves; w++) total += s_wave[w];
        sums[blockIdx.x] = total;
    }
}

} // namespace

// fn in [0, 3), nblocks >= 1 and first_block + nblocks <= 65536 are the C ABI's to check; sums_dev: [nblocks], device.
hipError_t lrm_launch_exact_math_sums(int fn, uint32_t first_block, uint32_t nblocks, uint64_t* sums_dev, hipStream_t st) {
    const dim3 grid(nblocks), block(kBlock);
    switch (fn) {
    case 0: hipLaunchKernelGGL(exact_math_sums_kernel<0>, grid, block, 0, st, first_block, sums_dev); break;
    case 1: hipLaunchKernelGGL(exact_math_sums_kernel<1>, grid, block, 0, st, first_block, sums_dev); break;
    case 2: hipLaunchKernelGGL(exact_math_sums_kernel<2>, grid, block, 0, st, first_block, sums_dev); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
