// lrm_swing.hip -- gfx950 kernels of lrm_swing_transit_posed_dev: per pose transition (edge) and LIFTED leg, does the swinging
// foot stay reachable at S sampled poses while it travels from its foothold under pose a to its foothold under pose b, and
// does the polyline it travels along pass through the terrain cloud.  The path, the evaluation, the per-target test and the
// per-leg answers are lrm_swing.h's (on top of lrm_edge_transit.h and lrm_leg_clearance.h), shared with the host loop; this
// file only spreads them over lanes.  Two kernels, the second only when something is tested (foot_radius > 0, a cloud, a
// segment left by `skip`):
//
// swing_reach_kernel: edge_transit_kernel's scheme (lrm_edge_transit.hip).  lane = (edge slot, sample), a wave holds 64 / S
//   edge slots, a workgroup is one wave, the grid is capped and strides.  A busy lane of a live edge forms its sample pose
//   once; per swinging leg it forms its own path point and foot, compiles the head of (leg, q_s) into its own 496-byte LDS
//   slot and evaluates the foot.  One ballot gives the mask, a segmented shuffle maximum the worst miss, the edge's first
//   lane stores the leg's row and the edge's swinging byte.  When no terrain kernel follows it also stores the empty terrain
//   answer and the clear byte.
//
// swing_terrain_kernel: leg_clearance_posed_kernel's scheme (lrm_leg_clearance.hip).  A wave owns an edge and strides over
//   the rest.  lane = leg reads the edge's foot indices once; the wave then loops over the swinging legs.  Per leg lane =
//   sample computes P_s into the wave's own LDS slice (64 x 7 floats: P_k, ab_k, den_k), lane = segment completes ab_k and
//   den_k from its neighbour's point; lrm_wave_lds_fence orders the three steps, there is no __syncthreads, and the slice is
//   later read at wave-uniform addresses only.  Then lane = tile walks the 1024-target tile boxes, lane = chunk the sixteen
//   chunk boxes of a near tile, and every lane of a near chunk tests the target it loaded against the tested segments.
//   popcount(__ballot(hit)) adds to the leg's count, every lane folds its smallest hit segment and one 64-bit key
//   (lrm_leg_clearance_key), two wave minima reduce them, lane 0 stores the row.  The clear byte reads reached_out, which
//   swing_reach_kernel wrote earlier on the same stream.  No atomics, no global scratch; every output has one writer.
//
// THE CULL BOX NEVER DROPS A NEAR TARGET.  The frame is ABOUT A = t[from], not about a body: the box [lo, hi] is the
// axis-aligned box of the tested COMPUTED path points P_k0 .. P_k1 (relative to A), and a target box is skipped iff on some
// axis it lies further than R from it.
//   - near means a computed d < fl(foot_radius + margin) for a tested segment, so d < (foot_radius + margin)(1 + eps),
//     eps = 2^-24;
//   - d is the rounded length of e, e_c = fl(fl(q_c - P_k,c) - fl(s fl(P_k+1,c - P_k,c))) with SOME s in [0, 1] (whatever
//     num / den gave, the clamp leaves s there; a nan s is 0).  With X = P_k + s (P_k+1 - P_k), a point of the segment and so
//     of [lo, hi], e_c = (q_c - X_c) + err, |err| <= eps |q_c - P_k,c| + 2 eps |ab_c| + O(eps^2) and
//     |q_c - P_k,c| <= |q_c - X_c| + |ab_c|: |q_c - X_c| <= |e_c| (1 + 2 eps) + 4 eps |ab_c|.  The gap g_c of q_c to
//     [lo_c, hi_c] is at most |q_c - X_c| and |ab_c| <= L = (hi.x - lo.x) + (hi.y - lo.y) + (hi.z - lo.z), so per axis
//     g_c <= d (1 + 4 eps) + 4 eps L, the roundings of the sum of squares and of the square root included;
//   - the target box is compared as fl(fl(bb_lo - A) - hi) and fl(lo - fl(bb_hi - A)): q is formed as t - A about the same
//     point and rounding is monotone, so for a target inside the box fl(bb_lo_c - A_c) <= q_c <= fl(bb_hi_c - A_c) EXACTLY
//     and the compared gap is at most g_c (1 + eps): no absolute slack for a cloud far from the origin is needed;
//   - R = (foot_radius + margin) * 1.0001 + 1e-5 L: a relative slack of 1e-4 where 6 eps = 3.6e-7 is needed, and 1e-5 L where
//     4.5e-7 L is.  Overflow anywhere gives R = +inf or a d that is nan or inf (never near).
//   A leg with a non-finite tested path point is not tested at all (lrm_swing.h), so lo, hi and L are finite.  The comparisons
//   are written negated, !(gap > R): a nan (a nan A cannot occur here, a nan box can) keeps the box.  Empty chunks carry an
//   inverted box: infinitely far, unless R is +inf, and then no lane of them has a target (i < nt).
//
// boxes == null (clouds below the 4096-target threshold of the C ABI): every tile and every chunk counts as near.
// A dead edge, a leg that is not swinging, a foot or an end out of range are answered before any address is formed from them.
//
// Compiled with -ffp-contract=off (see lrm_point.h).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "lrm_launch.h"
#include "lrm_swing.h"
#include "lrm_target_walk.h"

namespace {

// ---- reach part ----
constexpr int kReachBlock = 64;
constexpr unsigned kReachMaxGrid = 2560; // edge_transit_kernel's cap
constexpr int kSlotBytes = 496;          // edge_transit_kernel's LDS slot of a head
static_assert(kSlotBytes >= (int)sizeof(LrmLegHead) && kSlotBytes % 16 == 0 && (kSlotBytes / 16) % 2 == 1, "LDS slot of a head");

struct SwingLegs { // the legs, by value in the kernarg segment (8 x 56 B)
    LrmLegDimensions l[LRM_MAX_LEGS];
};

__device__ __forceinline__ bool edge_live(const int32_t* __restrict__ edge_a, const int32_t* __restrict__ edge_b,
                                          const uint8_t* __restrict__ live_in, uint32_t e, uint32_t nposes, int32_t* a, int32_t* b) {
    *a = edge_a[e];
    *b = edge_b[e];
    return !(live_in && live_in[e] == 0) && *a >= 0 && *b >= 0 && (uint32_t)*a < nposes && (uint32_t)*b < nposes;
}

__global__ __launch_bounds__(kReachBlock) void swing_reach_kernel(
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz, uint32_t nt,
    const float* __restrict__ quats, const float* __restrict__ body /* may be null */, uint32_t nposes, const SwingLegs legs,
    uint32_t nlegs, const int32_t* __restrict__ edge_a, const int32_t* __restrict__ edge_b, const int32_t* __restrict__ foot_from,
    const int32_t* __restrict__ foot_to, uint32_t nedges, uint32_t S, float lift, LrmVec3 up, bool terrain_follows,
    const uint8_t* __restrict__ live_in /* may be null */, uint64_t* __restrict__ mask_out /* may be null */,
    int32_t* __restrict__ reached_out, int32_t* __restrict__ first_miss_out, int32_t* __restrict__ worst_out /* may be null */,
    float* __restrict__ worst_d2_out /* may be null */, int32_t* __restrict__ hits_out, int32_t* __restrict__ hit_seg_out,
    int32_t* __restrict__ near_out, float* __restrict__ pen_out /* may be null */, uint8_t* __restrict__ swinging_out /* may be null */,
    uint8_t* __restrict__ clear_out /* may be null */) {
    __shared__ __attribute__((aligned(16))) unsigned char s_heads[kReachBlock * kSlotBytes];
    LrmLegHead* const H = reinterpret_cast<LrmLegHead*>(s_heads + threadIdx.x * kSlotBytes);
    const uint32_t lane = threadIdx.x;
    const uint32_t per_wave = 64u / S;  // edge slots of a wave
    const uint32_t slot = lane / S;     // this lane's edge slot
    const uint32_t s = lane - slot * S; // and sample
    const uint32_t first = slot * S;    // the first lane of the slot
    const bool busy = slot < per_wave;
    const uint64_t full = lrm_transit_full(S);

    for (uint64_t base = (uint64_t)blockIdx.x * per_wave; base < nedges; base += (uint64_t)gridDim.x * per_wave) { // wave-uniform
        const uint64_t e64 = base + slot;
        const bool have = busy && e64 < nedges;
        const uint32_t e = (uint32_t)e64;
        // ---- the edge and this lane's sample pose ----
        bool live = false;
        LrmTransitSample smp{};
        if (have) {
            int32_t a, b;
            live = edge_live(edge_a, edge_b, live_in, e, nposes, &a, &b);
            if (live) {
                const float* pa = quats + (size_t)a * 4;
                const float* pb = quats + (size_t)b * 4;
                const float qa[4] = {pa[0], pa[1], pa[2], pa[3]}, qb[4] = {pb[0], pb[1], pb[2], pb[3]};
                LrmVec3 ba{0.f, 0.f, 0.f}, bb{0.f, 0.f, 0.f};
                if (body) {
                    ba = LrmVec3{body[(size_t)a * 3], body[(size_t)a * 3 + 1], body[(size_t)a * 3 + 2]};
                    bb = LrmVec3{body[(size_t)b * 3], body[(size_t)b * 3 + 1], body[(size_t)b * 3 + 2]};
                }
                smp = lrm_transit_sample(qa, qb, ba, bb, s, S);
            }
        }
        uint32_t swing_bits = 0u;
        bool all_reach = true;
        for (uint32_t l = 0; l < nlegs; l++) { // wave-uniform
            const size_t o = (size_t)l * nedges + e; // < 2^32 (checked by the C ABI)
            int32_t from = -1, to = -1;
            if (live) {
                from = foot_from[o];
                to = foot_to[o];
            }
            const bool swinging = live && lrm_transit_foot_in_cloud(from, nt) && lrm_transit_foot_in_cloud(to, nt);
            bool reach = false;
            uint64_t key = 0ull;
            if (swinging) {
                const LrmVec3 A{tx[from], ty[from], tz[from]}, B{tx[to], ty[to], tz[to]};
                const LrmVec3 D{B.x - A.x, B.y - A.y, B.z - A.z};
                const LrmVec3 F = lrm_swing_foot(A, B, lrm_swing_path_point(D, lift, up, s, S), s, S);
                const LrmVec3 p{F.x - smp.body.x, F.y - smp.body.y, F.z - smp.body.z};
                float d2 = 0.f;
                reach = lrm_transit_eval(legs.l[l], smp.q, p, H, &d2);
                if (!reach) key = lrm_transit_key(d2, s);
            }
            const uint64_t mask = ((uint64_t)__ballot(reach) >> first) & full;
            // segmented maximum: after the step with offset k, lane s holds the maximum over samples [s, s + 2k) of its edge
            for (uint32_t off = 1u; off < S; off <<= 1) { // wave-uniform
                const uint64_t other = __shfl(key, (int)((lane + off) & 63u));
                if (s + off < S && other > key) key = other;
            }
            if (have && s == 0u) {
                const LrmTransitLeg T = swinging ? lrm_transit_leg(mask, key, S) : lrm_transit_leg_unplanted();
                if (mask_out) mask_out[o] = T.mask;
                reached_out[o] = T.reached;
                first_miss_out[o] = T.first_miss;
                if (worst_out) worst_out[o] = T.worst;
                if (worst_d2_out) worst_d2_out[o] = T.worst_d2;
                if (!terrain_follows) {
                    const LrmSwingTerrain N = lrm_swing_terrain_empty();
                    hits_out[o] = N.hits;
                    hit_seg_out[o] = N.hit_seg;
                    near_out[o] = N.near;
                    if (pen_out) pen_out[o] = N.pen;
                }
                if (swinging) {
                    swing_bits |= 1u << l;
                    all_reach = all_reach && T.first_miss < 0;
                }
            }
        }
        if (have && s == 0u) {
            if (swinging_out) swinging_out[e] = (uint8_t)swing_bits;
            if (clear_out && !terrain_follows) clear_out[e] = live && all_reach;
        }
    }
}

// ---- terrain part ----
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTargetTile = 1024;    // the tiles of tile_aabb_kernel (lrm_kernels.hip)
constexpr unsigned kMaxGrid = 16384; // 65 536 edges in flight; a wave strides over the rest (leg_clearance_posed_kernel's cap)
static_assert(sizeof(LrmSwingSeg) == 7 * sizeof(float), "a segment is seven floats");

__device__ __forceinline__ float uni(float v) { // a value every lane holds alike, moved to an SGPR
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ LrmVec3 uni(LrmVec3 v) { return LrmVec3{uni(v.x), uni(v.y), uni(v.z)}; }
__device__ __forceinline__ float wave_min_f(float v) { // finite or +-inf values only
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}

// is the box bb (a tile's or a chunk's, in the caller's frame) within R of the path's box [lo, hi] about A on every axis
__device__ __forceinline__ bool box_near(const float* bb, LrmVec3 A, LrmVec3 lo, LrmVec3 hi, float R) {
    const float b0 = bb[0], b1 = bb[1], b2 = bb[2], b3 = bb[3], b4 = bb[4], b5 = bb[5]; // six loads in flight, no branch between them
    const bool far = ((b0 - A.x) - hi.x > R) | (lo.x - (b3 - A.x) > R) | ((b1 - A.y) - hi.y > R) | (lo.y - (b4 - A.y) > R) |
                     ((b2 - A.z) - hi.z > R) | (lo.z - (b5 - A.z) > R);
    return !far; // every comparison false on a nan: the box is kept
}

__global__ __launch_bounds__(kBlock) void swing_terrain_kernel(
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz, size_t nt, uint32_t nposes, uint32_t nlegs,
    const int32_t* __restrict__ edge_a, const int32_t* __restrict__ edge_b, const int32_t* __restrict__ foot_from,
    const int32_t* __restrict__ foot_to, uint32_t nedges, uint32_t S, float lift, LrmVec3 up, float foot_radius, float margin,
    uint32_t skip, const float* __restrict__ boxes /* null = every tile near */, const uint8_t* __restrict__ live_in /* may be null */,
    const int32_t* __restrict__ reached /* swing_reach_kernel's reached_out */, int32_t* __restrict__ hits_out,
    int32_t* __restrict__ hit_seg_out, int32_t* __restrict__ near_out, float* __restrict__ pen_out /* may be null */,
    uint8_t* __restrict__ clear_out /* may be null */) {
    __shared__ LrmSwingSeg s_seg[kWaves][LRM_TRANSIT_MAX_SAMPLES];
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    LrmSwingSeg* const seg = s_seg[wave];
    const size_t ntiles = (nt + kTargetTile - 1) / kTargetTile;
    const float inf = __builtin_inff();
    const float reach = foot_radius + margin; // the sum formed once
    const LrmSwingRange range = lrm_swing_range(S, skip); // not empty: the launcher does not start this kernel otherwise
    const bool tested_point = lane >= range.k0 && lane <= range.k1;

    for (uint32_t e = blockIdx.x * kWaves + wave; e < nedges; e += gridDim.x * kWaves) { // wave-uniform
        int32_t a, b;
        const bool live = edge_live(edge_a, edge_b, live_in, e, nposes, &a, &b); // wave-uniform
        // lane = leg: the edge's foot indices, the rows of the legs that do not swing
        int32_t from = -1, to = -1;
        int32_t my_reached = -1;
        const size_t ol = (size_t)lane * nedges + e; // used by lanes < nlegs only; < 2^32 (checked by the C ABI)
        if (live && lane < nlegs) {
            from = foot_from[ol];
            to = foot_to[ol];
            my_reached = reached[ol];
        }
        const bool my_swing = lrm_transit_foot_in_cloud(from, (uint32_t)nt) && lrm_transit_foot_in_cloud(to, (uint32_t)nt);
        if (lane < nlegs && !my_swing) {
            const LrmSwingTerrain N = lrm_swing_terrain_empty();
            hits_out[ol] = N.hits;
            hit_seg_out[ol] = N.hit_seg;
            near_out[ol] = N.near;
            if (pen_out) pen_out[ol] = N.pen;
        }
        uint32_t swing = (uint32_t)__ballot(my_swing);
        bool clear = live && __ballot(my_swing && my_reached != (int32_t)S) == 0ull; // wave-uniform

        while (swing != 0u) { // wave-uniform
            const int l = __builtin_ctz(swing);
            swing &= swing - 1u;
            const size_t o = (size_t)l * nedges + e;
            const uint32_t ifrom = (uint32_t)__shfl(from, l), ito = (uint32_t)__shfl(to, l); // both < nt
            const LrmVec3 A = uni(LrmVec3{tx[ifrom], ty[ifrom], tz[ifrom]});
            const LrmVec3 B = uni(LrmVec3{tx[ito], ty[ito], tz[ito]});
            const LrmVec3 D{B.x - A.x, B.y - A.y, B.z - A.z};
            // lane = sample: the path point; lane = segment: its direction and squared length
            const LrmVec3 P = lane < S ? lrm_swing_path_point(D, lift, up, lane, S) : LrmVec3{0.f, 0.f, 0.f};
            lrm_wave_lds_fence(); // the previous leg's reads are done
            seg[lane].a = P;
            lrm_wave_lds_fence();
            if (lane + 1u < S) {
                const LrmSwingSeg g = lrm_swing_seg(P, seg[lane + 1u].a);
                seg[lane].ab = g.ab;
                seg[lane].den = g.den;
            }
            lrm_wave_lds_fence();

            uint32_t hits = 0u;                   // wave-uniform
            uint32_t first_hit = kLrmSwingNoSeg;  // this lane's smallest hit segment
            uint64_t key = kLrmLegClearanceNone;  // this lane's deepest near target
            if (__ballot(tested_point && !lrm_swing_point_finite(P)) == 0ull) { // wave-uniform; else the empty answer
                const LrmVec3 lo = uni(LrmVec3{wave_min_f(tested_point ? P.x : inf), wave_min_f(tested_point ? P.y : inf),
                                               wave_min_f(tested_point ? P.z : inf)});
                const LrmVec3 hi = uni(LrmVec3{-wave_min_f(tested_point ? -P.x : inf), -wave_min_f(tested_point ? -P.y : inf),
                                               -wave_min_f(tested_point ? -P.z : inf)});
                const float span = (hi.x - lo.x) + (hi.y - lo.y) + (hi.z - lo.z);
                const float R = uni(reach * 1.0001f + 1.0e-5f * span); // header comment; +inf culls nothing

                for (size_t tw0 = 0; tw0 < ntiles; tw0 += 64) {
                    const size_t tl = tw0 + lane; // lane = tile
                    unsigned long long near = __ballot(tl < ntiles && (!boxes || box_near(boxes + tl * 6, A, lo, hi, R)));
                    while (near != 0ull) {
                        const int tb = __builtin_ctzll(near);
                        near &= near - 1ull;
                        const size_t tile = tw0 + tb;
                        const size_t t0 = tile * kTargetTile;
                        uint32_t cnear; // lane = chunk of this tile
                        if (boxes) {
                            cnear = (uint32_t)__ballot(lane < 16 && box_near(boxes + (ntiles + tile * 16 + (lane & 15)) * 6, A, lo, hi, R)) & 0xffffu;
                        } else {
                            const size_t left = nt - t0; // > 0: tile < ntiles
                            const int chunks = left >= (size_t)kTargetTile ? 16 : (int)((left + 63) / 64);
                            cnear = chunks == 16 ? 0xffffu : (1u << chunks) - 1u;
                        }
                        while (cnear != 0u) {
                            const int chunk = __builtin_ctz(cnear);
                            cnear &= cnear - 1u;
                            const size_t i = t0 + (size_t)chunk * 64 + lane;
                            const uint32_t ti = (uint32_t)i; // nt <= INT32_MAX (checked by the C ABI)
                            unsigned in = 0u;
                            float pen = 0.f;
                            uint32_t fh = kLrmSwingNoSeg;
                            if (i < nt && ti != ifrom && ti != ito) // the two footholds themselves are never tested
                                in = lrm_swing_test(seg, range, foot_radius, reach, LrmVec3{tx[i] - A.x, ty[i] - A.y, tz[i] - A.z}, &pen, &fh);
                            hits += (uint32_t)__builtin_popcountll(__ballot((in & LRM_SWING_HIT) != 0u));
                            first_hit = fh < first_hit ? fh : first_hit;
                            if (in & LRM_SWING_NEAR) key = lrm_min_u64(key, lrm_leg_clearance_key(pen, ti));
                        }
                    }
                }
            }
            key = lrm_wave_min_u64(key);
            first_hit = wave_min_u32(first_hit);
            if (lane == 0) {
                const LrmSwingTerrain T = lrm_swing_terrain(hits, first_hit, key);
                hits_out[o] = T.hits;
                hit_seg_out[o] = T.hit_seg;
                near_out[o] = T.near;
                if (pen_out) pen_out[o] = T.pen;
            }
            clear = clear && hits == 0u;
        }
        if (lane == 0 && clear_out) clear_out[e] = clear;
    }
}

} // namespace

hipError_t lrm_launch_swing_transit_posed(const float* tx, const float* ty, const float* tz, size_t nt, const float* quats,
                                          const float* body, size_t nposes, const LrmLegDimensions* legs, size_t nlegs,
                                          const int32_t* edge_a, const int32_t* edge_b, size_t nedges, const int32_t* foot_from,
                                          const int32_t* foot_to, size_t nsamples, float lift, const float up[3], float foot_radius,
                                          float margin, uint32_t skip, float* tile_boxes, const uint8_t* live_in, uint64_t* mask_out,
                                          int32_t* reached_out, int32_t* first_miss_out, int32_t* worst_out, float* worst_d2_out,
                                          int32_t* hits_out, int32_t* hit_seg_out, int32_t* near_out, float* pen_out,
                                          uint8_t* swinging_out, uint8_t* clear_out, hipStream_t st) {
    SwingLegs L{};
    for (size_t k = 0; k < nlegs; k++) L.l[k] = legs[k];
    const LrmVec3 upv{up[0], up[1], up[2]};
    const LrmSwingRange range = lrm_swing_range((uint32_t)nsamples, skip);
    const bool terrain = foot_radius > 0.f && nt != 0 && range.k0 < range.k1;
    const size_t per_wave = 64 / nsamples;
    size_t g = (nedges + per_wave - 1) / per_wave;
    if (g > kReachMaxGrid) g = kReachMaxGrid;
    hipLaunchKernelGGL(swing_reach_kernel, dim3((unsigned)g), dim3(kReachBlock), 0, st, tx, ty, tz, (uint32_t)nt, quats, body,
                       (uint32_t)nposes, L, (uint32_t)nlegs, edge_a, edge_b, foot_from, foot_to, (uint32_t)nedges, (uint32_t)nsamples, lift,
                       upv, terrain, live_in, mask_out, reached_out, first_miss_out, worst_out, worst_d2_out, hits_out, hit_seg_out,
                       near_out, pen_out, swinging_out, clear_out);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess || !terrain) return err;
    const LrmWalkLaunch w = lrm_walk_launch(tx, ty, tz, nt, tile_boxes, nedges, kWaves, kMaxGrid, st);
    if (w.err != hipSuccess) return w.err;
    hipLaunchKernelGGL(swing_terrain_kernel, w.grid, dim3(kBlock), 0, st, tx, ty, tz, nt, (uint32_t)nposes, (uint32_t)nlegs, edge_a, edge_b,
                       foot_from, foot_to, (uint32_t)nedges, (uint32_t)nsamples, lift, upv, foot_radius, margin, skip, w.boxes, live_in,
                       reached_out, hits_out, hit_seg_out, near_out, pen_out, clear_out);
    return hipGetLastError();
}
