// lrm_leg_clearance.hip -- gfx950 kernels of lrm_leg_clearance_posed_dev and lrm_leg_joints_posed_dev: per (pose, leg) of a
// pose table and given joint angles, how many terrain targets stand inside one of the leg's three links (capsules about
// coxa, femur and tibia), which links are hit, and which target within `margin` of a link stands deepest.
//
// The joints J0..J3 (relative to body[p]), the distance of q = t - body[p] to a link, hit / near / pen and the 64-bit key are
// lrm_leg_clearance.h's, shared with the host loop.
//
// leg_clearance_posed_kernel follows body_clearance_posed_kernel (lrm_body_clearance.hip, which this file leaves alone): a
// wave owns one pose and strides over the rest; a pose with live_in[p] == 0 is answered before any table is read.  Within a
// live pose the wave loops over the legs.  Per leg every lane computes the joints from the same three angles (three sincos
// and four small matrix products: cheaper than a broadcast from one lane per leg would be to organise), and
// v_readfirstlane makes the twelve coordinates, the three ab vectors, the three den values and the leg's box wave-uniform
// (SGPRs).  Then lane = tile walks the 1024-target tile boxes, lane = chunk the sixteen 64-target chunk boxes of a near
// tile, and every lane of a near chunk tests the target it loaded against the up-to-three links, with the next near chunk's
// loads in flight.  popcount(__ballot(any hit)) adds to the leg's count, every lane ORs its link bits and folds one 64-bit
// key, six __shfl_xor steps reduce the keys, three ballots the link bits, lane 0 stores.  free is wave-local: the wave owns
// the pose.  No atomics, no __syncthreads, no LDS.
//
// THE CULL BOX NEVER DROPS A NEAR TARGET.  The box is the axis-aligned box [lo, hi] of the four COMPUTED joints (relative to
// body[p]), and a target box is skipped iff on some axis it lies further than R from it.
//   - near means a computed d < fl(radius[k] + margin) for a tested link k, so d < (rmax + margin)(1 + eps), eps = 2^-24,
//     rmax the largest radius;
//   - d is the rounded length of e, e_c = fl(fl(q_c - A_c) - fl(s fl(B_c - A_c))) with SOME s in [0, 1] (whatever num / den
//     gave, the clamp leaves s there; a nan s is 0).  With P = A + s (B - A), a point of the segment and so of [lo, hi],
//     e_c = (q_c - P_c) + err, |err| <= eps |q_c - A_c| + 2 eps |B_c - A_c| + O(eps^2), and |q_c - A_c| <= |q_c - P_c| + |B_c - A_c|:
//     |q_c - P_c| <= |e_c| (1 + 2 eps) + 4 eps |B_c - A_c|.  The gap g_c of q_c to [lo_c, hi_c] is at most |q_c - P_c|, so per
//     axis g_c <= d (1 + 4 eps) + 4 eps L with L = (hi.x - lo.x) + (hi.y - lo.y) + (hi.z - lo.z), the roundings of the sum of
//     squares and of the square root included;
//   - the target box is compared as fl(fl(bb_lo - body) - hi) and fl(lo - fl(bb_hi - body)): q is formed as t - body about
//     the same point, rounding is monotone, so for a target inside the box fl(bb_lo_c - body_c) <= q_c <= fl(bb_hi_c - body_c)
//     EXACTLY (the argument of lrm_body_clearance.hip) and the compared gap is at most g_c (1 + eps): no absolute slack
//     for coordinates far from the origin is needed, and none is carried;
//   - R = (rmax + margin) * 1.0001 + 1e-5 L: a relative slack of 1e-4 where 6 eps = 3.6e-7 is needed, and 1e-5 L where
//     4.5e-7 L is.  Overflow anywhere gives R = +inf or a d that is nan or inf (never near).
//   Because the test is defined on the computed joints, a non-unit quaternion needs no special case.  The comparisons are
//   written negated, !(gap > R): a nan (a nan body) keeps the box.  An infinite margin gives R = +inf: nothing is culled.
//   Empty chunks carry an inverted box: infinitely far, unless R is +inf, and then no lane of them has a target (i < nt).
//
// boxes == null (clouds below the 4096-target threshold of the C ABI): every tile and every chunk counts as near.
//
// leg_joints_posed_kernel: one (pose, leg) per lane in the [l * nposes + p] order, every lane reads its own two table
// entries; indices are clamped before any load as in fk_posed_kernel (lrm_ik_posed.hip).
//
// Compiled with -ffp-contract=off (see lrm_point.h).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "lrm_types.h"
#include "lrm_compile_head.h"
#include "lrm_point.h"
#include "lrm_ik.h"
#include "lrm_launch.h"
#include "lrm_leg_clearance.h"
#include "lrm_target_walk.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTargetTile = 1024; // the tiles of tile_aabb_kernel (lrm_kernels.hip)
constexpr unsigned kMaxGrid = 16384; // 65 536 poses in flight; a wave strides over the rest (body_clearance_posed_kernel's cap)

__device__ __forceinline__ float uni(float v) { // a value every lane computed alike, moved to an SGPR
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ LrmVec3 uni(LrmVec3 v) { return LrmVec3{uni(v.x), uni(v.y), uni(v.z)}; }

// is the box bb (a tile's or a chunk's, in the caller's frame) within R of the leg's box [lo, hi] about `body` on every axis
__device__ __forceinline__ bool box_near(const float* bb, LrmVec3 body, LrmVec3 lo, LrmVec3 hi, float R) {
    const float b0 = bb[0], b1 = bb[1], b2 = bb[2], b3 = bb[3], b4 = bb[4], b5 = bb[5]; // six loads in flight, no branch between them
    const bool far = ((b0 - body.x) - hi.x > R) | (lo.x - (b3 - body.x) > R) | ((b1 - body.y) - hi.y > R) | (lo.y - (b4 - body.y) > R) |
                     ((b2 - body.z) - hi.z > R) | (lo.z - (b5 - body.z) > R);
    return !far; // every comparison false on a nan: the box is kept
}

// Minimum waves per SIMD asked of the compiler; chosen from build/lrm_leg_clearance.resource.txt.
#ifndef LRM_LEG_CLEARANCE_MIN_WAVES
#define LRM_LEG_CLEARANCE_MIN_WAVES 4
#endif
__global__ __launch_bounds__(kBlock, LRM_LEG_CLEARANCE_MIN_WAVES) void leg_clearance_posed_kernel(
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz, size_t nt,
    const LrmPoseRecord* __restrict__ recs, const LrmIkLeg* __restrict__ iks, uint32_t nposes, uint32_t nlegs,
    const float* __restrict__ boxes /* null = every tile near */, const float* __restrict__ coxa, const float* __restrict__ femur,
    const float* __restrict__ tibia, float r0, float r1, float r2, float margin, float tip_clear,
    const uint8_t* __restrict__ live_in /* may be null */, int32_t* __restrict__ hits_out, uint8_t* __restrict__ links_out,
    int32_t* __restrict__ worst_out, float* __restrict__ pen_out /* may be null */, uint8_t* __restrict__ free_out /* may be null */) {
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const size_t ntiles = (nt + kTargetTile - 1) / kTargetTile;
    const float inf = __builtin_inff();
    const float radius[3] = {r0, r1, r2};
    const float reach[3] = {r0 + margin, r1 + margin, r2 + margin}; // the sums formed once
    float rmax = r0 > r1 ? r0 : r1;
    rmax = r2 > rmax ? r2 : rmax;
    const bool any_link = rmax > 0.f; // radius 0 everywhere: no link is tested at all

    for (uint32_t p = blockIdx.x * kWaves + wave; p < nposes; p += gridDim.x * kWaves) { // wave-uniform
        if (live_in && live_in[p] == 0) { // a skipped pose: the empty answer, before any table is read (lane = leg)
            if ((uint32_t)lane < nlegs) {
                const size_t o = (size_t)lane * nposes + p;
                hits_out[o] = 0;
                links_out[o] = 0;
                worst_out[o] = -1;
                if (pen_out) pen_out[o] = -inf;
            }
            if (lane == 0 && free_out) free_out[p] = 0;
            continue;
        }
        const uint32_t rp = p * nlegs; // nposes * nlegs < 2^32 (checked by the C ABI)
        const LrmPoseRecord& R0 = lrm_fresh(recs[rp]);
        const LrmVec3 body{R0.body_pos[0], R0.body_pos[1], R0.body_pos[2]}; // the same in every record of the pose
        bool pose_free = true;

        for (uint32_t l = 0; l < nlegs; l++) { // wave-uniform
            const size_t o = (size_t)l * nposes + p;
            uint32_t hits = 0u;                     // wave-uniform
            unsigned mybits = 0u;                   // this lane's hit links
            uint64_t key = kLrmLegClearanceNone;    // this lane's deepest near target
            LrmVec3 J[4];
            {
                const LrmPoseRecord& R = lrm_fresh(recs[rp + l]);
                const LrmIkLeg& K = lrm_fresh(iks[rp + l]);
                lrm_leg_joints(R.head, K, coxa[o], femur[o], tibia[o], tip_clear, J);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) J[k] = uni(J[k]);
            if (any_link && ntiles && lrm_leg_joints_finite(J)) { // wave-uniform; a leg with a non-finite joint is skipped
                LrmLegLinks S;
                lrm_leg_links(J, &S);
                LrmVec3 lo = J[0], hi = J[0];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    S.ab[k] = uni(S.ab[k]);
                    S.den[k] = uni(S.den[k]);
                    lo = LrmVec3{J[k + 1].x < lo.x ? J[k + 1].x : lo.x, J[k + 1].y < lo.y ? J[k + 1].y : lo.y, J[k + 1].z < lo.z ? J[k + 1].z : lo.z};
                    hi = LrmVec3{J[k + 1].x > hi.x ? J[k + 1].x : hi.x, J[k + 1].y > hi.y ? J[k + 1].y : hi.y, J[k + 1].z > hi.z ? J[k + 1].z : hi.z};
                }
                lo = uni(lo);
                hi = uni(hi);
                const float span = (hi.x - lo.x) + (hi.y - lo.y) + (hi.z - lo.z);
                const float R = uni((rmax + margin) * 1.0001f + 1.0e-5f * span); // header comment; +inf culls nothing

                for (size_t tw0 = 0; tw0 < ntiles; tw0 += 64) {
                    const size_t tl = tw0 + lane; // lane = tile
                    unsigned long long near = __ballot(tl < ntiles && (!boxes || box_near(boxes + tl * 6, body, lo, hi, R)));
                    while (near != 0ull) {
                        const int tb = __builtin_ctzll(near);
                        near &= near - 1ull;
                        const size_t tile = tw0 + tb;
                        const size_t t0 = tile * kTargetTile;
                        uint32_t cnear; // lane = chunk of this tile
                        if (boxes) {
                            cnear = (uint32_t)__ballot(lane < 16 && box_near(boxes + (ntiles + tile * 16 + (lane & 15)) * 6, body, lo, hi, R)) & 0xffffu;
                        } else {
                            const size_t left = nt - t0; // > 0: tile < ntiles
                            const int chunks = left >= (size_t)kTargetTile ? 16 : (int)((left + 63) / 64);
                            cnear = chunks == 16 ? 0xffffu : (1u << chunks) - 1u;
                        }
                        if (!cnear) continue; // the tile box touches the leg's box, no chunk box does
                        // software pipeline: the next near chunk's loads are issued before this one is tested
                        LrmVec3 nxt{0.f, 0.f, 0.f};
                        uint32_t nxt_i = 0u;
                        bool nxt_ok = false;
                        auto fetch = [&](int chunk) {
                            const size_t i = t0 + (size_t)chunk * 64 + lane;
                            nxt_ok = i < nt;
                            nxt_i = (uint32_t)i; // nt <= INT32_MAX (checked by the C ABI)
                            if (nxt_ok) nxt = LrmVec3{tx[i], ty[i], tz[i]};
                        };
                        fetch(__builtin_ctz(cnear));
                        cnear &= cnear - 1u;
                        bool more = true;
                        while (more) {
                            const LrmVec3 t = nxt;
                            const uint32_t ti = nxt_i;
                            const bool ok = nxt_ok;
                            more = cnear != 0u;
                            if (more) {
                                fetch(__builtin_ctz(cnear));
                                cnear &= cnear - 1u;
                            }
                            float pen = 0.f;
                            unsigned in = lrm_leg_clearance_test(S, radius, reach, LrmVec3{t.x - body.x, t.y - body.y, t.z - body.z}, &pen);
                            if (!ok) in = 0u;
                            hits += (uint32_t)__builtin_popcountll(__ballot((in & 7u) != 0u));
                            mybits |= in & 7u;
                            if (in & LRM_LEG_NEAR) key = lrm_min_u64(key, lrm_leg_clearance_key(pen, ti));
                        }
                    }
                }
            }

            key = lrm_wave_min_u64(key);
            const unsigned links = (__ballot(mybits & 1u) != 0ull ? 1u : 0u) | (__ballot(mybits & 2u) != 0ull ? 2u : 0u) |
                                   (__ballot(mybits & 4u) != 0ull ? 4u : 0u);
            if (lane == 0) {
                const LrmLegClearanceWorst worst = lrm_leg_clearance_key_decode(key);
                hits_out[o] = (int32_t)hits;
                links_out[o] = (uint8_t)links;
                worst_out[o] = worst.index;
                if (pen_out) pen_out[o] = worst.pen;
            }
            pose_free = pose_free && hits == 0u;
        }
        if (lane == 0 && free_out) free_out[p] = pose_free;
    }
}

__global__ __launch_bounds__(kBlock) void leg_joints_posed_kernel(const float* __restrict__ coxa, const float* __restrict__ femur,
                                                                  const float* __restrict__ tibia, uint32_t nposes, uint32_t nlegs,
                                                                  const LrmPoseRecord* __restrict__ recs, const LrmIkLeg* __restrict__ iks,
                                                                  float tip_clear, float* __restrict__ joints_out) {
    const size_t n = (size_t)nposes * nlegs;
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        // entry i = l * nposes + p; clamped into the tables before any load (i < n keeps both in range already)
        uint32_t l = (uint32_t)(i / nposes), p = (uint32_t)(i % nposes);
        l = l < nlegs ? l : 0u;
        p = p < nposes ? p : 0u;
        const uint32_t r = p * nlegs + l;
        const LrmPoseRecord& R = recs[r];
        LrmVec3 J[4];
        lrm_leg_joints(R.head, iks[r], coxa[i], femur[i], tibia[i], tip_clear, J);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            joints_out[i * 12 + 3 * k] = lrm_leg_joint_out(J[k].x, R.body_pos[0]);
            joints_out[i * 12 + 3 * k + 1] = lrm_leg_joint_out(J[k].y, R.body_pos[1]);
            joints_out[i * 12 + 3 * k + 2] = lrm_leg_joint_out(J[k].z, R.body_pos[2]);
        }
    }
}

} // namespace

hipError_t lrm_launch_leg_clearance_posed(const float* tx, const float* ty, const float* tz, size_t nt, const void* records,
                                          const void* ik_records, size_t nposes, size_t nlegs, float* tile_boxes, const float* coxa,
                                          const float* femur, const float* tibia, const float radius[3], float margin,
                                          float tip_clear, const uint8_t* live_in, int32_t* hits_out, uint8_t* links_out,
                                          int32_t* worst_out, float* pen_out, uint8_t* free_out, hipStream_t st) {
    const LrmWalkLaunch w = lrm_walk_launch(tx, ty, tz, nt, tile_boxes, nposes, kWaves, kMaxGrid, st);
    if (w.err != hipSuccess) return w.err;
    hipLaunchKernelGGL(leg_clearance_posed_kernel, w.grid, dim3(kBlock), 0, st, tx, ty, tz, nt, (const LrmPoseRecord*)records,
                       (const LrmIkLeg*)ik_records, (uint32_t)nposes, (uint32_t)nlegs, w.boxes, coxa, femur, tibia, radius[0], radius[1],
                       radius[2], margin, tip_clear, live_in, hits_out, links_out, worst_out, pen_out, free_out);
    return hipGetLastError();
}

hipError_t lrm_launch_leg_joints_posed(const float* coxa, const float* femur, const float* tibia, size_t nposes, size_t nlegs,
                                       const void* records, const void* ik_records, float tip_clear, float* joints_out, hipStream_t st) {
    size_t g = (nposes * nlegs + kBlock - 1) / kBlock;
    if (g > 256 * 32) g = 256 * 32; // fk_posed_kernel's cap
    hipLaunchKernelGGL(leg_joints_posed_kernel, dim3((unsigned)(g < 1 ? 1 : g)), dim3(kBlock), 0, st, coxa, femur, tibia, (uint32_t)nposes,
                       (uint32_t)nlegs, (const LrmPoseRecord*)records, (const LrmIkLeg*)ik_records, tip_clear, joints_out);
    return hipGetLastError();
}
