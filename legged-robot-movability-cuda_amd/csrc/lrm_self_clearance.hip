// lrm_self_clearance.hip -- gfx950 kernels of lrm_self_clearance_posed_dev and lrm_dbg_link_pair_dist_dev: per set (a pose
// and three joint angles per leg), how close do the links of two DIFFERENT legs come to each other: per (set, leg) the
// number of link pairs that hit, the legs and the own links they involve, and the deepest pair within `margin`.
// The joints are lrm_leg_clearance.h's, the pair distance, the test, the per-leg fold and the key lrm_self_clearance.h's,
// shared with the host loop; this file only spreads them over a wave.
//
// self_clearance_posed_kernel: a wave owns one set and strides over the rest under a capped grid.  It never sees the cloud
// or the body position: both legs of a pair are relative to the same body.
//   prologue, once per wave: lane -> its pair (i, j, ka, kb), the pair's two sums rr and rr + margin and whether both radii
//     are non-zero, for each of the up to four rounds of kRound pair codes (27 .. 252 pairs for 3 .. 8 legs).  The codes do
//     not depend on the set, so none of this is repeated in the set loop.
//   phase 1, lane = leg: lanes 0 .. nlegs - 1 read their own two table entries and three angles, compute J0..J3 ONCE per
//     (set, leg) and write the twelve coordinates into the wave's LDS slab (8 x 12 floats); a ballot gives the valid legs.
//   phase 2, lane = pair code, in rounds of kRound: the lane reads its two links -- six consecutive floats each, the slab
//     is laid out [leg][joint][xyz] -- and computes d, hit, near and pen.
//   phase 3, lane = leg again: a ballot of the near lanes; for every set bit (a scalar loop) the pair's packed code and its
//     pen come from that lane into scalars (v_readlane), and the two lanes whose leg takes part fold it into their count,
//     masks and 64-bit key.  A round without a near pair costs the ballot and one scalar branch.
//   Lanes 0 .. nlegs - 1 then store their leg's row; lane 0 stores free.
// Why the slab and not __shfl: a pair lane needs 12 of its two legs' 24 coordinates, chosen by ka and kb.  By __shfl that is
// 24 ds_bpermute and 18 selects per round; from the slab it is 12 floats in 6 ds_read2_b32, the link folded into the address.
// Why the scalar loop and not ballots and __shfl_xor per leg: a leg's answer is a count, two masks and a key over up to 63 pairs
// spread over four rounds; a xor fold costs six steps of four registers per leg and round whether or not anything is near,
// while feasible sets -- the common case behind ik() -- have few near pairs or none.  DESIGN.md 3.20 has the resource table.
// No atomics, no global scratch, no __syncthreads: the slab belongs to one wave, ordered by lrm_wave_lds_fence.  The fold
// order is the lane order of the ballot, and a minimum of keys does not depend on the order: bit-deterministic.
// A dead set (live_in 0, pose out of range) is answered before any table or angle is read.
//
// Compiled with -ffp-contract=off (see lrm_point.h).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "lrm_types.h"
#include "lrm_compile_head.h"
#include "lrm_point.h"
#include "lrm_ik.h"
#include "lrm_self_clearance.h"
#include "lrm_target_walk.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr unsigned kMaxGrid = 16384; // 65 536 sets in flight; a wave strides over the rest
constexpr int kRound = 64;           // pair codes per round: one per lane
constexpr int kRounds = (LRM_SELF_MAX_PAIRS + kRound - 1) / kRound;
constexpr uint32_t kPairOn = 1u << 10; // above lrm_self_pair_pack's bits: the lane's code is a pair and both radii are non-zero

__global__ __launch_bounds__(kBlock) void self_clearance_posed_kernel(
    const LrmPoseRecord* __restrict__ recs, const LrmIkLeg* __restrict__ iks, uint32_t nposes, uint32_t nlegs,
    const int32_t* __restrict__ pose_idx /* may be null */, uint32_t nsets, const float* __restrict__ coxa,
    const float* __restrict__ femur, const float* __restrict__ tibia, const LrmSelfRadii R, float tip_clear,
    const uint8_t* __restrict__ live_in /* may be null */, int32_t* __restrict__ hits_out, uint8_t* __restrict__ with_out,
    uint8_t* __restrict__ links_out, uint8_t* __restrict__ worst_out, float* __restrict__ pen_out /* may be null */,
    uint8_t* __restrict__ free_out /* may be null */) {
    __shared__ float slab[kWaves][LRM_MAX_LEGS * 12];
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    float* const J = slab[wave];
    const uint32_t npairs = lrm_self_npairs(nlegs);

    // ---- prologue: this lane's pair of every round ----
    uint32_t pk[kRounds];
    float rr[kRounds], reach[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; r++) {
        const uint32_t code = (uint32_t)(r * kRound) + lane;
        const bool in = code < npairs;
        pk[r] = lrm_self_pair_of(in ? code : 0u);
        const uint32_t k = lrm_self_pair_ka(pk[r]) * 3u + lrm_self_pair_kb(pk[r]);
        rr[r] = R.rr[k];
        reach[r] = R.reach[k];
        if (in && ((R.tested >> k) & 1u)) pk[r] |= kPairOn;
    }

    for (uint32_t s = blockIdx.x * kWaves + wave; s < nsets; s += gridDim.x * kWaves) { // wave-uniform
        const int32_t p = pose_idx ? pose_idx[s] : (int32_t)s;
        const bool live = !(live_in && live_in[s] == 0) && p >= 0 && (uint32_t)p < nposes;
        LrmSelfLeg A = lrm_self_leg_empty(); // lane = leg
        if (live) {
            // ---- phase 1: the joints, once per (set, leg) ----
            bool valid = false;
            if (lane < nlegs) {
                const size_t rec = (size_t)p * nlegs + lane;
                const size_t o = (size_t)lane * nsets + s;
                LrmVec3 Jl[4];
                lrm_leg_joints(recs[rec].head, iks[rec], coxa[o], femur[o], tibia[o], tip_clear, Jl);
                valid = lrm_leg_joints_finite(Jl);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    J[lane * 12 + 3 * k] = Jl[k].x;
                    J[lane * 12 + 3 * k + 1] = Jl[k].y;
                    J[lane * 12 + 3 * k + 2] = Jl[k].z;
                }
            }
            lrm_wave_lds_fence();
            const uint32_t legs_ok = (uint32_t)__ballot(valid) & 0xffu; // wave-uniform

#pragma unroll
            for (int r = 0; r < kRounds; r++) {
                if ((uint32_t)(r * kRound) >= npairs) break; // wave-uniform
                // ---- phase 2: lane = pair code ----
                const uint32_t i = lrm_self_pair_i(pk[r]), j = lrm_self_pair_j(pk[r]);
                const float* const P1 = J + i * 12u + lrm_self_pair_ka(pk[r]) * 3u; // A1, B1: six consecutive floats
                const float* const P2 = J + j * 12u + lrm_self_pair_kb(pk[r]) * 3u;
                const float d = lrm_self_pair_dist(LrmVec3{P1[0], P1[1], P1[2]}, LrmVec3{P1[3], P1[4], P1[5]}, LrmVec3{P2[0], P2[1], P2[2]},
                                                   LrmVec3{P2[3], P2[4], P2[5]});
                float pen = 0.f;
                unsigned bits = lrm_self_clearance_test(d, rr[r], reach[r], &pen);
                if (!((pk[r] & kPairOn) && ((legs_ok >> i) & 1u) && ((legs_ok >> j) & 1u))) bits = 0u;
                // ---- phase 3: lane = leg; a scalar loop over the near pairs ----
                unsigned long long near = __ballot(bits != 0u);
                const unsigned long long hit = __ballot((bits & LRM_SELF_HIT) != 0u);
                while (near != 0ull) {
                    const int b = __builtin_ctzll(near);
                    near &= near - 1ull;
                    const uint32_t pkb = (uint32_t)__builtin_amdgcn_readlane((int)pk[r], b);
                    const float penb = lrm_u2f((uint32_t)__builtin_amdgcn_readlane((int)lrm_f2u(pen), b));
                    lrm_self_leg_take(&A, lane, pkb, LRM_SELF_NEAR | (((hit >> b) & 1ull) ? LRM_SELF_HIT : 0u), penb);
                }
            }
            lrm_wave_lds_fence(); // the reads above before the next set's writes
        }
        if (lane < nlegs) {
            const size_t o = (size_t)lane * nsets + s; // < 2^32 (checked by the C ABI)
            const LrmSelfWorst W = lrm_self_key_decode(A.key);
            hits_out[o] = A.hits;
            with_out[o] = (uint8_t)A.with;
            links_out[o] = (uint8_t)A.links;
            worst_out[o] = W.code;
            if (pen_out) pen_out[o] = W.pen;
        }
        const bool any = __ballot(A.hits != 0) != 0ull; // lanes at or above nlegs keep the empty answer
        if (free_out && lane == 0) free_out[s] = live && !any;
    }
}

__global__ __launch_bounds__(kBlock) void link_pair_dist_kernel(const float* __restrict__ segs, size_t n, float* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const float* g = segs + i * 12;
        out[i] = lrm_self_pair_dist(LrmVec3{g[0], g[1], g[2]}, LrmVec3{g[3], g[4], g[5]}, LrmVec3{g[6], g[7], g[8]}, LrmVec3{g[9], g[10], g[11]});
    }
}

} // namespace

hipError_t lrm_launch_self_clearance_posed(const void* records, const void* ik_records, size_t nposes, size_t nlegs,
                                           const int32_t* pose_idx, size_t nsets, const float* coxa, const float* femur,
                                           const float* tibia, const float radius[3], float margin, float tip_clear,
                                           const uint8_t* live_in, int32_t* hits_out, uint8_t* with_out, uint8_t* links_out,
                                           uint8_t* worst_out, float* pen_out, uint8_t* free_out, hipStream_t st) {
    size_t g = (nsets + kWaves - 1) / kWaves;
    if (g > kMaxGrid) g = kMaxGrid;
    hipLaunchKernelGGL(self_clearance_posed_kernel, dim3((unsigned)g), dim3(kBlock), 0, st, (const LrmPoseRecord*)records,
                       (const LrmIkLeg*)ik_records, (uint32_t)nposes, (uint32_t)nlegs, pose_idx, (uint32_t)nsets, coxa, femur, tibia,
                       lrm_self_radii(radius, margin), tip_clear, live_in, hits_out, with_out, links_out, worst_out, pen_out, free_out);
    return hipGetLastError();
}

hipError_t lrm_launch_link_pair_dist(const float* segs, size_t n, float* out, hipStream_t st) {
    size_t g = (n + kBlock - 1) / kBlock;
    if (g > 256 * 32) g = 256 * 32;
    hipLaunchKernelGGL(link_pair_dist_kernel, dim3((unsigned)(g < 1 ? 1 : g)), dim3(kBlock), 0, st, segs, n, out);
    return hipGetLastError();
}
