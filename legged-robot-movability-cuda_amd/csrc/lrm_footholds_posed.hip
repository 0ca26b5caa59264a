// lrm_footholds_posed.hip -- gfx950 kernels of lrm_pose_footholds_compile_dev and lrm_footholds_posed_dev: per
// (pose, leg) of a pose table, how many targets the leg can reach under that pose and which reachable target lies
// nearest the leg's nominal point.
//
// A pair (pose p, leg l, target t) is reachable iff reachability_global(t - body[p], legs[l], quats[p]): the strict
// evaluation of lrm_point.h on the pose record (LrmPoseRecord, lrm_compile_head.h) that the posed queries read.
//
//  * pose_footholds_compile_kernel: one thread per (pose, leg) writes the 32-byte entry of lrm_footholds_posed.h
//    (bounding sphere and nominal point in the caller's frame), the host's own arithmetic.
//  * footholds_posed_kernel is footholds_wave_kernel (lrm_footholds.hip) with the leg constants per pose.  A wave owns
//    one pose, walks the tile boxes (lane = tile) and, inside a near tile, the chunk boxes (lane = chunk), reads only
//    the 64-target chunks whose box touches some leg's sphere, with the next chunk's loads in flight while the current
//    one is tested, and queues the targets inside the pose's reach sphere in LDS with their index.  A full batch of 64
//    is tested against every leg whose own sphere it touches; popcount(__ballot(hit)) adds to lane l's count, every
//    hit lane folds the key (d2 bits << 32 | index, lrm_footholds.h) into its own per-leg minimum, and six __shfl_xor
//    steps per leg reduce the keys at the end.  No atomics, no __syncthreads: every wave stages its own tables.
//    What differs from footholds_wave_kernel:
//      - the nlegs records and entries of the wave's pose sit at wave-uniform addresses (readfirstlane): their
//        scalars come through s_load at the point of use (lrm_fresh), as in posed_kernel's uniform path;
//      - the 4 x 4 circle tables, per-lane indexed by the region, are copied to the wave's LDS slot when the wave's
//        pose changes -- all nlegs of them at once (8 x 256 B per wave), one float per lane and leg, between two
//        wave fences -- and so are the nlegs spheres the chunk cull indexes per lane;
//      - the tile cull and the queue use the largest reach_r2_max of the pose's records about the body position, or
//        +inf when some leg's sphere is the one that excludes nothing (non-unit quaternion);
//      - the point test is lrm_reach_global on t - body: strict, whatever lrm_set_mode says.
//
//  * foothold_lists_posed_kernel (lrm_foothold_lists_posed_dev) is the same traversal (footholds_posed_traverse<true>)
//    without the keys: survivors reach process() in ascending target index, so a hit's rank in the list of (pose, leg)
//    is the leg's running count plus the hits in lower lanes, and it is stored at that rank in the caller's segment.
//  * foothold_offsets_kernel (lrm_foothold_offsets_dev): the exclusive scan between the two, one workgroup with a carry.
//  * foothold_edges_posed_kernel (lrm_foothold_edges_posed_dev): a wave per pose TRANSITION (a, b); counts and chooses
//    among the targets a leg reaches under both poses, with every cull the intersection of the two poses' (see there).
//
// boxes == null (clouds below the 4096-target threshold of the C ABI): every tile and every chunk counts as near.
//
// Compiled with -ffp-contract=off (see lrm_point.h and lrm_footholds.h).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "lrm_launch.h"
#include "lrm_types.h"
#include "lrm_compile_head.h"
#include "lrm_point.h"
#include "lrm_footholds.h"
#include "lrm_footholds_posed.h"
#include "lrm_target_walk.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTargetTile = 1024; // the tiles of tile_aabb_kernel (lrm_kernels.hip)
constexpr int kQueue = 128;
constexpr unsigned kMaxGrid = 16384; // 65 536 poses in flight; a wave strides over the rest

struct PosedLegs { // the legs of a compile, by value in the kernarg segment (8 x 56 B)
    LrmLegDimensions l[LRM_MAX_LEGS];
};

__global__ __launch_bounds__(kBlock) void pose_footholds_compile_kernel(const float* __restrict__ quats, uint32_t nposes, uint32_t nlegs,
                                                                        const PosedLegs legs, const LrmFootNominal nominal,
                                                                        LrmPoseFootEntry* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (size_t)nposes * nlegs) return;
    const uint32_t pose = (uint32_t)(t / nlegs), leg = (uint32_t)(t % nlegs);
    const float q[4] = {quats[4 * (size_t)pose], quats[4 * (size_t)pose + 1], quats[4 * (size_t)pose + 2], quats[4 * (size_t)pose + 3]};
    const float nom[3] = {nominal.v[leg][0], nominal.v[leg][1], nominal.v[leg][2]};
    LrmPoseFootEntry E;
    lrm_pose_foothold_entry(legs.l[leg], q, nom, &E);
    out[t] = E;
}


#ifndef LRM_FOOTHOLDS_POSED_MIN_WAVES
#define LRM_FOOTHOLDS_POSED_MIN_WAVES 8 // footholds_wave_kernel's setting
#endif
// The traversal of both kernels.  kLists = false: footholds_posed_kernel (counts and choice).  kLists = true:
// foothold_lists_posed_kernel -- no keys; every hit is stored at its rank in the (pose, leg) segment instead.
template <bool kLists>
__device__ __forceinline__ void footholds_posed_traverse(
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz, size_t nt,
    const LrmPoseRecord* __restrict__ recs, const LrmPoseFootEntry* __restrict__ fh, uint32_t nposes, uint32_t nlegs,
    const float* __restrict__ boxes /* null = every tile near */, int32_t* __restrict__ count_out, int32_t* __restrict__ best_out,
    float* __restrict__ best_d2_out, uint8_t* __restrict__ all_legs_out, const int64_t* __restrict__ offsets, int64_t capacity,
    int32_t* __restrict__ idx_out, float* __restrict__ d2_out, int32_t* __restrict__ written_out) {
    __shared__ float s_qx[kWaves][kQueue], s_qy[kWaves][kQueue], s_qz[kWaves][kQueue];
    __shared__ uint32_t s_qi[kWaves][kQueue];
    __shared__ LrmCircle s_lists[kWaves][LRM_MAX_LEGS][4 * LRM_N_CIRCLES]; // the circle tables of the wave's pose
    __shared__ float s_sphere[kWaves][LRM_MAX_LEGS][4];                    // its legs' spheres: centre (relative to the body), r^2
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    float* qx = s_qx[wave];
    float* qy = s_qy[wave];
    float* qz = s_qz[wave];
    uint32_t* qi = s_qi[wave];
    LrmCircle(*my_lists)[4 * LRM_N_CIRCLES] = s_lists[wave];
    float(*my_sphere)[4] = s_sphere[wave];
    const size_t ntiles = (nt + kTargetTile - 1) / kTargetTile;

    for (uint32_t p = blockIdx.x * kWaves + wave; p < nposes; p += gridDim.x * kWaves) { // wave-uniform
        const uint32_t r0 = p * nlegs; // nposes * nlegs < 2^32 (checked by the C ABI)
        // stage the pose's tables: every lane is done with the previous pose's
        lrm_wave_lds_fence();
        for (uint32_t l = 0; l < nlegs; l++)
            reinterpret_cast<float*>(my_lists[l])[lane] = reinterpret_cast<const float*>(&recs[r0 + l].head.lists[0][0])[lane];
        if ((uint32_t)lane < nlegs * 4) my_sphere[lane >> 2][lane & 3] = reinterpret_cast<const float*>(&fh[r0 + (lane >> 2)])[lane & 3];
        lrm_wave_lds_fence();
        const LrmPoseRecord& R0 = lrm_fresh(recs[r0]);
        const LrmVec3 body{R0.body_pos[0], R0.body_pos[1], R0.body_pos[2]}; // the same in every record of the pose
        float r2max = 0.f;
        for (uint32_t l = 0; l < nlegs; l++)
            r2max = fmaxf(r2max, lrm_fresh(fh[r0 + l]).cull_r2 < __builtin_inff() ? lrm_fresh(recs[r0 + l]).head.reach_r2_max : __builtin_inff());

        int count = 0;        // survivors waiting in this wave's queue
        uint32_t legs_n = 0;  // lane l: leg l's reachable targets
        [[maybe_unused]] uint64_t key[LRM_MAX_LEGS]; // kLists = false: this lane's best candidate per leg (constant indices only: registers)
        if constexpr (!kLists) {
#pragma unroll
            for (int k = 0; k < LRM_MAX_LEGS; k++) key[k] = kLrmFootholdNone;
        }
        // kLists, lane l: leg l's segment [seg_base, seg_base + seg_room) of idx_out, clamped here, before any store:
        // 0 <= seg_base and seg_base + seg_room <= capacity, or seg_room == 0
        int64_t seg_base = 0;
        uint32_t seg_room = 0u;
        if constexpr (kLists) {
            if ((uint32_t)lane < nlegs) {
                const size_t o = (size_t)lane * nposes + p;
                const int64_t b = offsets[o], e = offsets[o + 1] < capacity ? offsets[o + 1] : capacity; // e <= capacity
                if (b >= 0 && e > b) { // both non-negative: e - b does not overflow
                    seg_base = b;
                    seg_room = e - b > (int64_t)INT32_MAX ? (uint32_t)INT32_MAX : (uint32_t)(e - b); // a list has at most nt <= INT32_MAX entries
                }
            }
        }

        auto process = [&](int m) {
            LrmVec3 t{0.f, 0.f, 0.f};
            uint32_t ti = 0u;
            if (lane < m) {
                t = LrmVec3{qx[lane], qy[lane], qz[lane]};
                ti = qi[lane];
            }
            const LrmVec3 rel{t.x - body.x, t.y - body.y, t.z - body.z};
            for (uint32_t l = 0; l < nlegs; l++) {
                const LrmPoseFootEntry& E = lrm_fresh(fh[r0 + l]);
                const float ex = rel.x - E.cull_center[0], ey = rel.y - E.cull_center[1], ez = rel.z - E.cull_center[2];
                const bool inside = (lane < m) && __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex)) <= E.cull_r2;
                if (__ballot(inside) == 0ull) continue;
                bool hit = false;
                if (inside) {
                    const LrmPoseRecord& R = lrm_fresh(recs[r0 + l]);
                    hit = lrm_reach_global(R.head, my_lists[l], rel);
                }
                const unsigned long long hm = __ballot(hit);
                if (hm == 0ull) continue; // wave-uniform
                if constexpr (kLists) {
                    // the queue is first-in first-out over ascending targets: a hit's rank in the list is the leg's
                    // running count plus the hits in lower lanes; one ballot's stores are consecutive addresses
                    const uint32_t rank = __builtin_amdgcn_readlane(legs_n, l) +
                                          __builtin_amdgcn_mbcnt_hi((uint32_t)(hm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hm, 0u));
                    const uint32_t room = __builtin_amdgcn_readlane(seg_room, l);
                    const int64_t base = (int64_t)(((uint64_t)__builtin_amdgcn_readlane((uint32_t)((uint64_t)seg_base >> 32), l) << 32) |
                                                   __builtin_amdgcn_readlane((uint32_t)seg_base, l));
                    if (hit && rank < room) {
                        idx_out[base + rank] = (int32_t)ti;
                        if (d2_out) d2_out[base + rank] = lrm_foothold_d2(t, body, E.nominal_w);
                    }
                    if ((uint32_t)lane == l) legs_n += (uint32_t)__builtin_popcountll(hm);
                } else {
                    if ((uint32_t)lane == l) legs_n += (uint32_t)__builtin_popcountll(hm);
                    const uint64_t kk = hit ? lrm_foothold_key(lrm_foothold_d2(t, body, E.nominal_w), ti) : kLrmFootholdNone;
#pragma unroll
                    for (int k = 0; k < LRM_MAX_LEGS; k++)
                        if ((uint32_t)k == l) key[k] = lrm_min_u64(key[k], kk); // l is wave-uniform: one branch taken
                }
            }
        };

        for (size_t tw0 = 0; tw0 < ntiles; tw0 += 64) {
            // lane = tile: box distance is a lower bound of every member's distance; 1e-3 relative slack for the
            // rounding of the bound itself
            const size_t tl = tw0 + lane;
            unsigned long long near =
                __ballot(tl < ntiles && (!boxes || lrm_box_dist2(boxes + tl * 6, body.x, body.y, body.z) * 0.999f <= r2max));
            while (near != 0ull) {
                const int tb = __builtin_ctzll(near);
                near &= near - 1ull;
                const size_t tile = tw0 + tb;
                const size_t t0 = tile * kTargetTile;
                // lane = (chunk of this tile, one of four legs): a chunk is read when its box touches the bounding
                // sphere of some leg (empty chunks carry an inverted box)
                uint32_t cnear = 0u;
                if (boxes) {
                    const float* cb = boxes + (ntiles + tile * 16 + (lane & 15)) * 6;
                    for (uint32_t l0 = 0; l0 < nlegs; l0 += 4) { // wave-uniform
                        const uint32_t l = l0 + (lane >> 4);
                        bool touch = false;
                        if (l < nlegs)
                            touch = lrm_box_dist2(cb, body.x + my_sphere[l][0], body.y + my_sphere[l][1], body.z + my_sphere[l][2]) * 0.999f <=
                                    my_sphere[l][3];
                        const unsigned long long mm = __ballot(touch);
                        cnear |= (uint32_t)((mm | (mm >> 16) | (mm >> 32) | (mm >> 48)) & 0xffffull);
                    }
                } else {
                    const size_t left = nt - t0; // > 0: tile < ntiles
                    const int chunks = left >= (size_t)kTargetTile ? 16 : (int)((left + 63) / 64);
                    cnear = chunks == 16 ? 0xffffu : (1u << chunks) - 1u;
                }
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
                if (cnear) {
                    fetch(__builtin_ctz(cnear));
                    cnear &= cnear - 1u;
                }
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
                    const float ddx = t.x - body.x, ddy = t.y - body.y, ddz = t.z - body.z;
                    const bool keep = ok && __builtin_fmaf(ddz, ddz, __builtin_fmaf(ddy, ddy, ddx * ddx)) <= r2max;
                    const unsigned long long m = __ballot(keep);
                    if (m == 0ull) continue;
                    if (keep) {
                        const int pos = count + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                        qx[pos] = t.x;
                        qy[pos] = t.y;
                        qz[pos] = t.z;
                        qi[pos] = ti;
                    }
                    count += __builtin_popcountll(m);
                    lrm_wave_lds_fence();
                    if (count >= 64) {
                        process(64);
                        count -= 64;
                        // the (< 64) entries behind the processed batch move to the front
                        float mx = 0.f, my = 0.f, mz = 0.f;
                        uint32_t mi = 0u;
                        if (lane < count) { mx = qx[64 + lane]; my = qy[64 + lane]; mz = qz[64 + lane]; mi = qi[64 + lane]; }
                        lrm_wave_lds_fence();
                        if (lane < count) { qx[lane] = mx; qy[lane] = my; qz[lane] = mz; qi[lane] = mi; }
                        lrm_wave_lds_fence();
                    }
                }
            }
        }
        if (count > 0) process(count);

        if constexpr (kLists) {
            if (written_out && (uint32_t)lane < nlegs) written_out[(size_t)lane * nposes + p] = (int32_t)(legs_n < seg_room ? legs_n : seg_room);
        } else {
            // per leg: the wave's smallest key; lane l keeps leg l's
            uint64_t best = kLrmFootholdNone;
#pragma unroll
            for (int k = 0; k < LRM_MAX_LEGS; k++) {
                if ((uint32_t)k >= nlegs) break; // wave-uniform
                const uint64_t v = lrm_wave_min_u64(key[k]);
                if (lane == k) best = v;
            }
            const bool mine = (uint32_t)lane < nlegs;
            if (mine) {
                const size_t o = (size_t)lane * nposes + p;
                const LrmFootholdChoice c = lrm_foothold_key_decode(best, legs_n != 0u);
                count_out[o] = (int32_t)legs_n;
                best_out[o] = c.index;
                if (best_d2_out) best_d2_out[o] = c.d2;
            }
            if (all_legs_out) { // wave-uniform
                const unsigned long long have = __ballot(mine && legs_n != 0u);
                if (lane == 0) all_legs_out[p] = have == ((1ull << nlegs) - 1ull);
            }
        }
    }
}

__global__ __launch_bounds__(kBlock, LRM_FOOTHOLDS_POSED_MIN_WAVES) void footholds_posed_kernel(
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz, size_t nt,
    const LrmPoseRecord* __restrict__ recs, const LrmPoseFootEntry* __restrict__ fh, uint32_t nposes, uint32_t nlegs,
    const float* __restrict__ boxes /* null = every tile near */, int32_t* __restrict__ count_out, int32_t* __restrict__ best_out,
    float* __restrict__ best_d2_out, uint8_t* __restrict__ all_legs_out) {
    footholds_posed_traverse<false>(tx, ty, tz, nt, recs, fh, nposes, nlegs, boxes, count_out, best_out, best_d2_out, all_legs_out,
                                    nullptr, 0, nullptr, nullptr, nullptr);
}

// lrm_foothold_lists_posed_dev: the same traversal; the reachable targets of (pose p, leg l) in ascending index go to
// idx_out[base + k] (their d2 to d2_out), base = offsets[l*nposes + p], as far as the segment has room (include/lrm.h).
// The launch bound is footholds_posed_kernel's, carried over, not compared.
__global__ __launch_bounds__(kBlock, LRM_FOOTHOLDS_POSED_MIN_WAVES) void foothold_lists_posed_kernel(
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz, size_t nt,
    const LrmPoseRecord* __restrict__ recs, const LrmPoseFootEntry* __restrict__ fh, uint32_t nposes, uint32_t nlegs,
    const float* __restrict__ boxes /* null = every tile near */, const int64_t* __restrict__ offsets, int64_t capacity,
    int32_t* __restrict__ idx_out, float* __restrict__ d2_out /* may be null */, int32_t* __restrict__ written_out /* may be null */) {
    footholds_posed_traverse<true>(tx, ty, tz, nt, recs, fh, nposes, nlegs, boxes, nullptr, nullptr, nullptr, nullptr, offsets,
                                   capacity, idx_out, d2_out, written_out);
}

// lrm_foothold_offsets_dev: out[0] = 0, out[k + 1] = out[k] + max(count[k], 0).  ONE workgroup strides over n in slices
// of kScanSlice with a running carry: no second workgroup to wait for, no scratch.  A thread sums kScanItems
// consecutive counts, the waves scan those sums (__shfl_up, then the 16 wave totals through LDS), and the next slice's
// counts are loaded before the current slice is scanned.
constexpr int kScanBlock = 1024;
constexpr int kScanItems = 8;
constexpr int kScanSlice = kScanBlock * kScanItems;

__global__ __launch_bounds__(kScanBlock) void foothold_offsets_kernel(const int32_t* __restrict__ count, size_t n, int64_t* __restrict__ out) {
    __shared__ int64_t s_wave[kScanBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) out[0] = 0;
    int64_t carry = 0; // the same in every thread
    int32_t c[kScanItems], nx[kScanItems];
    auto load = [&](size_t s0, int32_t* v) {
#pragma unroll
        for (int k = 0; k < kScanItems; k++) {
            const size_t i = s0 + (size_t)tid * kScanItems + k;
            const int32_t x = i < n ? count[i] : 0;
            v[k] = x > 0 ? x : 0;
        }
    };
    load(0, nx);
    for (size_t s0 = 0; s0 < n; s0 += kScanSlice) {
#pragma unroll
        for (int k = 0; k < kScanItems; k++) c[k] = nx[k];
        if (s0 + kScanSlice < n) load(s0 + kScanSlice, nx);
        int64_t mine = 0;
#pragma unroll
        for (int k = 0; k < kScanItems; k++) mine += c[k];
        int64_t incl = mine; // inclusive scan over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int64_t up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int64_t before = carry, total = 0;
#pragma unroll
        for (int w = 0; w < kScanBlock / 64; w++) {
            const int64_t v = s_wave[w];
            if (w < wave) before += v;
            total += v;
        }
        __syncthreads(); // s_wave is rewritten in the next slice
        int64_t run = before + incl - mine;
#pragma unroll
        for (int k = 0; k < kScanItems; k++) {
            const size_t i = s0 + (size_t)tid * kScanItems + k;
            run += c[k];
            if (i < n) out[i + 1] = run;
        }
        carry += total;
    }
}

// lrm_foothold_edges_posed_dev: per (edge e = (pose a, pose b), leg l) the targets leg l reaches under BOTH poses -- the
// footholds a stance foot can keep while the body moves from a to b -- counted, and the one with the smallest
// d2(a) + d2(b) chosen.  A sibling of footholds_posed_traverse (that template is left alone: its two kernels keep their
// code): a wave per edge, the same walk over tile boxes and chunk boxes, the same pipelined loads, LDS queue, ballots and
// key minima.  Every cull is the intersection of the two poses':
//   - a tile is near when its box is within r2max of both bodies;
//   - a chunk is read when, for some leg, its box touches that leg's sphere under a AND under b;
//   - a target is queued when it is within r2max of both bodies;
//   - process() tests a target against leg l when it lies in both of l's spheres, runs the strict test of pose b only in
//     the lanes where pose a's hit, and skips b for the wave when none did.
// A +inf sphere or r2max excludes nothing on its side only.  Each wave stages the circle tables and spheres of both poses
// (2 x 8 x 256 B + 2 x 128 B): 25 600 B of LDS per workgroup, which admits 6 workgroups on a CU's 160 KiB, i.e. 6 waves
// per SIMD -- so the launch bound asks for 6, not 8, and the compiler gets 80 VGPRs instead of 64.
// edge_a / edge_b are checked against nposes before any record is touched; a bad edge gets count 0, best -1, d2 +inf.
#ifndef LRM_FOOTHOLD_EDGES_MIN_WAVES
#define LRM_FOOTHOLD_EDGES_MIN_WAVES 6
#endif
__global__ __launch_bounds__(kBlock, LRM_FOOTHOLD_EDGES_MIN_WAVES) void foothold_edges_posed_kernel(
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz, size_t nt,
    const LrmPoseRecord* __restrict__ recs, const LrmPoseFootEntry* __restrict__ fh, uint32_t nposes, uint32_t nlegs,
    const float* __restrict__ boxes /* null = every tile near */, const int32_t* __restrict__ edge_a,
    const int32_t* __restrict__ edge_b, uint32_t nedges, int32_t* __restrict__ count_out, int32_t* __restrict__ best_out,
    float* __restrict__ best_d2_out, uint8_t* __restrict__ all_legs_out) {
    __shared__ float s_qx[kWaves][kQueue], s_qy[kWaves][kQueue], s_qz[kWaves][kQueue];
    __shared__ uint32_t s_qi[kWaves][kQueue];
    __shared__ LrmCircle s_lists[kWaves][2][LRM_MAX_LEGS][4 * LRM_N_CIRCLES]; // [0]: pose a's circle tables, [1]: pose b's
    __shared__ float s_sphere[kWaves][2][LRM_MAX_LEGS][4];                    // the legs' spheres: centre (relative to the body), r^2
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    float* qx = s_qx[wave];
    float* qy = s_qy[wave];
    float* qz = s_qz[wave];
    uint32_t* qi = s_qi[wave];
    LrmCircle(*lists_a)[4 * LRM_N_CIRCLES] = s_lists[wave][0];
    LrmCircle(*lists_b)[4 * LRM_N_CIRCLES] = s_lists[wave][1];
    float(*sph_a)[4] = s_sphere[wave][0];
    float(*sph_b)[4] = s_sphere[wave][1];
    const size_t ntiles = (nt + kTargetTile - 1) / kTargetTile;
    const bool mine = (uint32_t)lane < nlegs;

    for (uint64_t e = blockIdx.x * kWaves + wave; e < nedges; e += (uint64_t)gridDim.x * kWaves) { // wave-uniform
        const uint32_t pa = (uint32_t)__builtin_amdgcn_readfirstlane(edge_a[e]);
        const uint32_t pb = (uint32_t)__builtin_amdgcn_readfirstlane(edge_b[e]);
        if (pa >= nposes || pb >= nposes) { // negative indices included; before any record is read
            if (mine) {
                const size_t o = (size_t)lane * nedges + e;
                count_out[o] = 0;
                best_out[o] = -1;
                if (best_d2_out) best_d2_out[o] = __builtin_inff();
            }
            if (all_legs_out && lane == 0) all_legs_out[e] = 0;
            continue;
        }
        const uint32_t ra0 = pa * nlegs, rb0 = pb * nlegs; // nposes * nlegs < 2^32 (checked by the C ABI)
        // stage both poses' tables: every lane is done with the previous edge's
        lrm_wave_lds_fence();
        for (uint32_t l = 0; l < nlegs; l++) {
            reinterpret_cast<float*>(lists_a[l])[lane] = reinterpret_cast<const float*>(&recs[ra0 + l].head.lists[0][0])[lane];
            reinterpret_cast<float*>(lists_b[l])[lane] = reinterpret_cast<const float*>(&recs[rb0 + l].head.lists[0][0])[lane];
        }
        { // lanes 0-31: pose a's spheres, lanes 32-63: pose b's
            const uint32_t k = (uint32_t)lane & 31u;
            if (k < nlegs * 4) s_sphere[wave][lane >> 5][k >> 2][k & 3] = reinterpret_cast<const float*>(&fh[(lane < 32 ? ra0 : rb0) + (k >> 2)])[k & 3];
        }
        lrm_wave_lds_fence();
        const LrmPoseRecord& RA = lrm_fresh(recs[ra0]);
        const LrmPoseRecord& RB = lrm_fresh(recs[rb0]);
        const LrmVec3 body_a{RA.body_pos[0], RA.body_pos[1], RA.body_pos[2]}; // the same in every record of the pose
        const LrmVec3 body_b{RB.body_pos[0], RB.body_pos[1], RB.body_pos[2]};
        float r2a = 0.f, r2b = 0.f;
        for (uint32_t l = 0; l < nlegs; l++) {
            r2a = fmaxf(r2a, lrm_fresh(fh[ra0 + l]).cull_r2 < __builtin_inff() ? lrm_fresh(recs[ra0 + l]).head.reach_r2_max : __builtin_inff());
            r2b = fmaxf(r2b, lrm_fresh(fh[rb0 + l]).cull_r2 < __builtin_inff() ? lrm_fresh(recs[rb0 + l]).head.reach_r2_max : __builtin_inff());
        }

        int count = 0;        // survivors waiting in this wave's queue
        uint32_t legs_n = 0;  // lane l: leg l's common targets
        uint64_t key[LRM_MAX_LEGS]; // this lane's best candidate per leg (constant indices only: registers)
#pragma unroll
        for (int k = 0; k < LRM_MAX_LEGS; k++) key[k] = kLrmFootholdNone;

        auto process = [&](int m) {
            LrmVec3 t{0.f, 0.f, 0.f};
            uint32_t ti = 0u;
            if (lane < m) {
                t = LrmVec3{qx[lane], qy[lane], qz[lane]};
                ti = qi[lane];
            }
            const LrmVec3 rel_a{t.x - body_a.x, t.y - body_a.y, t.z - body_a.z};
            const LrmVec3 rel_b{t.x - body_b.x, t.y - body_b.y, t.z - body_b.z};
            for (uint32_t l = 0; l < nlegs; l++) {
                const LrmPoseFootEntry& EA = lrm_fresh(fh[ra0 + l]);
                const LrmPoseFootEntry& EB = lrm_fresh(fh[rb0 + l]);
                const float ax = rel_a.x - EA.cull_center[0], ay = rel_a.y - EA.cull_center[1], az = rel_a.z - EA.cull_center[2];
                const float bx = rel_b.x - EB.cull_center[0], by = rel_b.y - EB.cull_center[1], bz = rel_b.z - EB.cull_center[2];
                const bool inside = (lane < m) && __builtin_fmaf(az, az, __builtin_fmaf(ay, ay, ax * ax)) <= EA.cull_r2 &&
                                    __builtin_fmaf(bz, bz, __builtin_fmaf(by, by, bx * bx)) <= EB.cull_r2;
                if (__ballot(inside) == 0ull) continue;
                bool hit = false;
                if (inside) {
                    const LrmPoseRecord& R = lrm_fresh(recs[ra0 + l]);
                    hit = lrm_reach_global(R.head, lists_a[l], rel_a);
                }
                if (__ballot(hit) == 0ull) continue; // nobody reaches it under a: b is not asked
                if (hit) {
                    const LrmPoseRecord& R = lrm_fresh(recs[rb0 + l]);
                    hit = lrm_reach_global(R.head, lists_b[l], rel_b);
                }
                const unsigned long long hm = __ballot(hit);
                if (hm == 0ull) continue; // wave-uniform
                if ((uint32_t)lane == l) legs_n += (uint32_t)__builtin_popcountll(hm);
                // one f32 add of the two poses' d2 (no contraction: -ffp-contract=off); it commutes
                const uint64_t kk = hit ? lrm_foothold_key(lrm_foothold_d2(t, body_a, EA.nominal_w) + lrm_foothold_d2(t, body_b, EB.nominal_w), ti)
                                        : kLrmFootholdNone;
#pragma unroll
                for (int k = 0; k < LRM_MAX_LEGS; k++)
                    if ((uint32_t)k == l) key[k] = lrm_min_u64(key[k], kk); // l is wave-uniform: one branch taken
            }
        };

        for (size_t tg0 = 0; tg0 < ntiles; tg0 += 64) {
            // lane = tile: near only when the box is within reach of BOTH bodies (0.999: the rounding of the bound itself)
            const size_t tl = tg0 + lane;
            unsigned long long near = __ballot(tl < ntiles && (!boxes || (lrm_box_dist2(boxes + tl * 6, body_a.x, body_a.y, body_a.z) * 0.999f <= r2a &&
                                                                          lrm_box_dist2(boxes + tl * 6, body_b.x, body_b.y, body_b.z) * 0.999f <= r2b)));
            while (near != 0ull) {
                const int tb = __builtin_ctzll(near);
                near &= near - 1ull;
                const size_t tile = tg0 + tb;
                const size_t t0 = tile * kTargetTile;
                // lane = (chunk of this tile, one of four legs): a chunk is read when, for some leg, its box touches
                // that leg's sphere under a and under b (empty chunks carry an inverted box)
                uint32_t cnear = 0u;
                if (boxes) {
                    const float* cb = boxes + (ntiles + tile * 16 + (lane & 15)) * 6;
                    for (uint32_t l0 = 0; l0 < nlegs; l0 += 4) { // wave-uniform
                        const uint32_t l = l0 + (lane >> 4);
                        bool touch = false;
                        if (l < nlegs)
                            touch = lrm_box_dist2(cb, body_a.x + sph_a[l][0], body_a.y + sph_a[l][1], body_a.z + sph_a[l][2]) * 0.999f <= sph_a[l][3] &&
                                    lrm_box_dist2(cb, body_b.x + sph_b[l][0], body_b.y + sph_b[l][1], body_b.z + sph_b[l][2]) * 0.999f <= sph_b[l][3];
                        const unsigned long long mm = __ballot(touch);
                        cnear |= (uint32_t)((mm | (mm >> 16) | (mm >> 32) | (mm >> 48)) & 0xffffull);
                    }
                } else {
                    const size_t left = nt - t0; // > 0: tile < ntiles
                    const int chunks = left >= (size_t)kTargetTile ? 16 : (int)((left + 63) / 64);
                    cnear = chunks == 16 ? 0xffffu : (1u << chunks) - 1u;
                }
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
                if (cnear) {
                    fetch(__builtin_ctz(cnear));
                    cnear &= cnear - 1u;
                }
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
                    const float ax = t.x - body_a.x, ay = t.y - body_a.y, az = t.z - body_a.z;
                    const float bx = t.x - body_b.x, by = t.y - body_b.y, bz = t.z - body_b.z;
                    const bool keep = ok && __builtin_fmaf(az, az, __builtin_fmaf(ay, ay, ax * ax)) <= r2a &&
                                      __builtin_fmaf(bz, bz, __builtin_fmaf(by, by, bx * bx)) <= r2b;
                    const unsigned long long m = __ballot(keep);
                    if (m == 0ull) continue;
                    if (keep) {
                        const int pos = count + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                        qx[pos] = t.x;
                        qy[pos] = t.y;
                        qz[pos] = t.z;
                        qi[pos] = ti;
                    }
                    count += __builtin_popcountll(m);
                    lrm_wave_lds_fence();
                    if (count >= 64) {
                        process(64);
                        count -= 64;
                        // the (< 64) entries behind the processed batch move to the front
                        float mx = 0.f, my = 0.f, mz = 0.f;
                        uint32_t mi = 0u;
                        if (lane < count) { mx = qx[64 + lane]; my = qy[64 + lane]; mz = qz[64 + lane]; mi = qi[64 + lane]; }
                        lrm_wave_lds_fence();
                        if (lane < count) { qx[lane] = mx; qy[lane] = my; qz[lane] = mz; qi[lane] = mi; }
                        lrm_wave_lds_fence();
                    }
                }
            }
        }
        if (count > 0) process(count);

        // per leg: the wave's smallest key; lane l keeps leg l's
        uint64_t best = kLrmFootholdNone;
#pragma unroll
        for (int k = 0; k < LRM_MAX_LEGS; k++) {
            if ((uint32_t)k >= nlegs) break; // wave-uniform
            const uint64_t v = lrm_wave_min_u64(key[k]);
            if (lane == k) best = v;
        }
        if (mine) {
            const size_t o = (size_t)lane * nedges + e;
            const LrmFootholdChoice c = lrm_foothold_key_decode(best, legs_n != 0u);
            count_out[o] = (int32_t)legs_n;
            best_out[o] = c.index;
            if (best_d2_out) best_d2_out[o] = c.d2;
        }
        if (all_legs_out) { // wave-uniform
            const unsigned long long have = __ballot(mine && legs_n != 0u);
            if (lane == 0) all_legs_out[e] = have == ((1ull << nlegs) - 1ull);
        }
    }
}

} // namespace

hipError_t lrm_launch_pose_footholds_compile(const float* quats, size_t nposes, const LrmLegDimensions* legs, size_t nlegs,
                                             const LrmFootNominal& nominal, void* fh_records, hipStream_t st) {
    PosedLegs L{};
    for (size_t k = 0; k < nlegs; k++) L.l[k] = legs[k];
    const size_t total = nposes * nlegs;
    const int grid = (int)((total + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(pose_footholds_compile_kernel, dim3(grid), dim3(kBlock), 0, st, quats, (uint32_t)nposes, (uint32_t)nlegs, L,
                       nominal, (LrmPoseFootEntry*)fh_records);
    return hipGetLastError();
}

hipError_t lrm_launch_footholds_posed(const float* tx, const float* ty, const float* tz, size_t nt, const void* records,
                                      const void* fh_records, size_t nposes, size_t nlegs, float* tile_boxes, int32_t* count_out,
                                      int32_t* best_out, float* best_d2_out, uint8_t* all_legs_out, hipStream_t st) {
    const LrmWalkLaunch w = lrm_walk_launch(tx, ty, tz, nt, tile_boxes, nposes, kWaves, kMaxGrid, st);
    if (w.err != hipSuccess) return w.err;
    hipLaunchKernelGGL(footholds_posed_kernel, w.grid, dim3(kBlock), 0, st, tx, ty, tz, nt, (const LrmPoseRecord*)records,
                       (const LrmPoseFootEntry*)fh_records, (uint32_t)nposes, (uint32_t)nlegs, w.boxes, count_out, best_out, best_d2_out,
                       all_legs_out);
    return hipGetLastError();
}

hipError_t lrm_launch_foothold_lists_posed(const float* tx, const float* ty, const float* tz, size_t nt, const void* records,
                                           const void* fh_records, size_t nposes, size_t nlegs, float* tile_boxes,
                                           const int64_t* offsets, size_t capacity, int32_t* idx_out, float* d2_out,
                                           int32_t* written_out, hipStream_t st) {
    const LrmWalkLaunch w = lrm_walk_launch(tx, ty, tz, nt, tile_boxes, nposes, kWaves, kMaxGrid, st);
    if (w.err != hipSuccess) return w.err;
    const int64_t cap = capacity > (size_t)INT64_MAX ? INT64_MAX : (int64_t)capacity;
    hipLaunchKernelGGL(foothold_lists_posed_kernel, w.grid, dim3(kBlock), 0, st, tx, ty, tz, nt, (const LrmPoseRecord*)records,
                       (const LrmPoseFootEntry*)fh_records, (uint32_t)nposes, (uint32_t)nlegs, w.boxes, offsets, cap, idx_out, d2_out,
                       written_out);
    return hipGetLastError();
}

hipError_t lrm_launch_foothold_edges_posed(const float* tx, const float* ty, const float* tz, size_t nt, const void* records,
                                           const void* fh_records, size_t nposes, size_t nlegs, float* tile_boxes,
                                           const int32_t* edge_a, const int32_t* edge_b, size_t nedges, int32_t* count_out,
                                           int32_t* best_out, float* best_d2_out, uint8_t* all_legs_out, hipStream_t st) {
    const LrmWalkLaunch w = lrm_walk_launch(tx, ty, tz, nt, tile_boxes, nedges, kWaves, kMaxGrid, st);
    if (w.err != hipSuccess) return w.err;
    hipLaunchKernelGGL(foothold_edges_posed_kernel, w.grid, dim3(kBlock), 0, st, tx, ty, tz, nt, (const LrmPoseRecord*)records,
                       (const LrmPoseFootEntry*)fh_records, (uint32_t)nposes, (uint32_t)nlegs, w.boxes, edge_a, edge_b, (uint32_t)nedges,
                       count_out, best_out, best_d2_out, all_legs_out);
    return hipGetLastError();
}

hipError_t lrm_launch_foothold_offsets(const int32_t* count, size_t n, int64_t* offsets_out, hipStream_t st) {
    hipLaunchKernelGGL(foothold_offsets_kernel, dim3(1), dim3(kScanBlock), 0, st, count, n, offsets_out);
    return hipGetLastError();
}
