// lrm_dbg_math.h -- block checksums of lrm_exact_math.h's one-argument functions over float bit patterns
// (lrm_dbg_exact_math_sums_host / _dev).  One source for the host loop (lrm_capi.cpp) and the kernel (lrm_dbg_math.hip).
//
// The domain is all 2^32 patterns u; block b holds the 65536 patterns u = b * 65536 + j.  Function 0 is lrm_atanf(x),
// 1 the sine and 2 the cosine of lrm_sincosf(x).  r(u) = the result's bits, every nan replaced by 0x7fc00000 (hosts and
// devices may differ in nan payloads and nothing downstream reads them); sum[b] = sum_j r(u) * (2 j + 1) mod 2^64.  The
// weights are odd, so one wrong result in a block always changes its sum, and integer addition makes the sum independent
// of the order of evaluation.
#pragma once
#include "lrm_exact_math.h"

#define LRM_DBG_MATH_FNS 3
#define LRM_DBG_MATH_BLOCK 65536u  // patterns per block
#define LRM_DBG_MATH_BLOCKS 65536u // blocks in the domain

template <int kFn>
LRM_HD uint64_t lrm_dbg_math_term(uint32_t u, uint32_t j) {
    const float x = lrm_u2f(u);
    float v;
    if (kFn == 0) v = lrm_atanf(x);
    else {
        float s, c;
        lrm_sincosf(x, &s, &c);
        v = kFn == 1 ? s : c;
    }
    uint32_t r = lrm_f2u(v);
    r = (r & 0x7fffffffu) > 0x7f800000u ? 0x7fc00000u : r;
    return (uint64_t)r * (uint64_t)(2u * j + 1u);
}

// the plain loop of the host side: the checksum of one block
template <int kFn>
inline uint64_t lrm_dbg_math_block_sum(uint32_t block) {
    const uint32_t base = block * LRM_DBG_MATH_BLOCK;
    uint64_t acc = 0;
    for (uint32_t j = 0; j < LRM_DBG_MATH_BLOCK; j++) acc += lrm_dbg_math_term<kFn>(base + j, j);
    return acc;
}
