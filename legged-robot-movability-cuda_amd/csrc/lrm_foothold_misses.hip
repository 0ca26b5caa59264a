// lrm_foothold_misses.hip -- gfx950 kernel of lrm_foothold_misses_posed_dev: per (pose, leg) of a pose table, the target
// that is closest to being reachable and the body translation that would put it on the workspace boundary.
//
// With q = t - body[p] and E the foothold entry of (p, l) (lrm_footholds_posed.h):
//   candidate  lrm_foothold_miss_candidate(q, E.cull_center, rm2), rm2 = lrm_foothold_miss_rm2(E.cull_r2, margin);
//   miss       a candidate with reachability_global(q, legs[l], quats[p]) == 0; its vector d = distance_global(q, ...),
//              m2 = lrm_foothold_miss_m2(d); eligible iff m2 < +inf;
//   answer     the eligible miss with the smallest lrm_foothold_key(m2, t), its m2 and d, and the number of misses.
// Strict arithmetic (lrm_point.h on the pose record), whatever lrm_set_mode says.
//
// foothold_misses_posed_kernel is a sibling of footholds_posed_traverse and foothold_edges_posed_kernel
// (lrm_footholds_posed.hip, which this file leaves alone): a wave per pose, the same walk over tile boxes (lane = tile)
// and chunk boxes (lane = chunk x one of four legs), the same pipelined chunk loads, per-wave LDS queue with indices,
// ballots and per-lane per-leg 64-bit key minima reduced by six __shfl_xor steps per leg.  No atomics, no
// __syncthreads, no cross-wave communication.  What differs:
//   - lane l reads count_in[l*nposes + p] first; a leg with count_in > 0 is skipped, and a wave whose legs are all
//     skipped writes the empty answers and leaves before it stages anything;
//   - the spheres are the entries' widened by `margin` (rm2), per non-skipped leg; there is no pose-wide reach sphere:
//     tiles, chunks and queue entries are kept when SOME non-skipped leg wants them;
//   - the queue keeps a target iff it is a candidate of some non-skipped leg -- the exact shared test, not a cull;
//   - process() runs the shared candidate test per leg, then lrm_reach_global, then lrm_dist_global only in the lanes
//     whose mask is 0 (skipped for the wave when that ballot is empty);
//   - after the key reduction lane l holds leg l's winner and evaluates its distance vector once more, from its own
//     record (vector loads, the non-uniform path of posed_kernel): the same strict operations on the same inputs, so
//     the same bits as the evaluation that produced the key.  No d is kept in registers during the traversal.
//
// THE BOX CULLS NEVER DROP A CANDIDATE.  The candidate test is formed as (t - body) - centre, the boxes are tested about
// C = fl(body + centre): two different roundings of the same point.  With eps = 2^-24 (half an ulp, relative), per axis k
//   |t_k - C_k| <= |e_k| + eps (|t_k - body_k| + |e_k|) + eps (|body_k| + |centre_k|)
//               <= |e_k| (1 + 2 eps) + 3 eps M,      M = max|body_k| + max|centre_k| + rm
// (a candidate has |t_k| <= |body_k| + |centre_k| + |e_k| up to the same roundings, and |e| <= rm (1 + 2 eps) since the
// computed e2 <= rm2).  So the box distance g of a box that holds a candidate obeys |g| <= rm (1 + 4 eps) + 3 sqrt(3) eps M,
// and its computed square D <= |g|^2 (1 + 6 eps).  The test  D * 0.999 <= (rm + S)^2  with the ABSOLUTE slack
//   S = 2^-21 M   (8 eps M > 3 sqrt(3) eps M / sqrt(0.999 (1 + 6 eps)))
// therefore passes for every such box: the factor 0.999 covers the relative terms (1 + 4 eps)^2 (1 + 6 eps) and the
// rounding of (rm + S)^2 itself, S covers the two roundings of the point.  At 4e6 mm from the origin S is 1.9 mm where
// the two roundings differ by up to 0.5 mm.  The comparison is written !(D * 0.999 > thr): a nan on either side (nan
// body, inf - inf in a box of infinite targets) keeps the box.  rm2 = +inf gives thr = +inf: nothing is culled.
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


// Minimum waves per SIMD asked of the compiler (DESIGN.md 3.14 has the resource figures behind the choice).
#ifndef LRM_FOOTHOLD_MISSES_MIN_WAVES
#define LRM_FOOTHOLD_MISSES_MIN_WAVES 4
#endif
__global__ __launch_bounds__(kBlock, LRM_FOOTHOLD_MISSES_MIN_WAVES) void foothold_misses_posed_kernel(
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz, size_t nt,
    const LrmPoseRecord* __restrict__ recs, const LrmPoseFootEntry* __restrict__ fh, uint32_t nposes, uint32_t nlegs,
    const float* __restrict__ boxes /* null = every tile near */, float margin, const int32_t* __restrict__ count_in /* may be null */,
    int32_t* __restrict__ miss_out, float* __restrict__ m2_out /* may be null */, float* __restrict__ shift_x /* all three or none */,
    float* __restrict__ shift_y, float* __restrict__ shift_z, int32_t* __restrict__ near_out /* may be null */) {
    __shared__ float s_qx[kWaves][kQueue], s_qy[kWaves][kQueue], s_qz[kWaves][kQueue];
    __shared__ uint32_t s_qi[kWaves][kQueue];
    __shared__ LrmCircle s_lists[kWaves][LRM_MAX_LEGS][4 * LRM_N_CIRCLES]; // the circle tables of the wave's pose
    __shared__ float s_sphere[kWaves][LRM_MAX_LEGS][4]; // per leg: centre relative to the body, rm2 (-1: leg skipped)
    __shared__ float s_cull[kWaves][LRM_MAX_LEGS][4];   // per leg: C = body + centre, box threshold (rm + S)^2 (-1: leg skipped)
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    float* qx = s_qx[wave];
    float* qy = s_qy[wave];
    float* qz = s_qz[wave];
    uint32_t* qi = s_qi[wave];
    LrmCircle(*my_lists)[4 * LRM_N_CIRCLES] = s_lists[wave];
    float(*my_sphere)[4] = s_sphere[wave];
    float(*my_cull)[4] = s_cull[wave];
    const size_t ntiles = (nt + kTargetTile - 1) / kTargetTile;
    const bool mine = (uint32_t)lane < nlegs;
    const float inf = __builtin_inff();

    for (uint32_t p = blockIdx.x * kWaves + wave; p < nposes; p += gridDim.x * kWaves) { // wave-uniform
        const uint32_t r0 = p * nlegs; // nposes * nlegs < 2^32 (checked by the C ABI)
        const size_t o = (size_t)(mine ? lane : 0) * nposes + p;
        const bool wanted = mine && !(count_in && count_in[o] > 0);
        const uint32_t live = (uint32_t)__ballot(wanted); // bit l: leg l is not skipped
        if (live == 0u) { // every leg skipped: the empty answers, before anything is staged
            if (mine) {
                miss_out[o] = -1;
                if (m2_out) m2_out[o] = inf;
                if (shift_x) shift_x[o] = shift_y[o] = shift_z[o] = __builtin_nanf("");
                if (near_out) near_out[o] = 0;
            }
            continue;
        }
        const LrmPoseRecord& R0 = lrm_fresh(recs[r0]);
        const LrmVec3 body{R0.body_pos[0], R0.body_pos[1], R0.body_pos[2]}; // the same in every record of the pose
        // stage the pose's tables: every lane is done with the previous pose's
        lrm_wave_lds_fence();
        for (uint32_t l = 0; l < nlegs; l++)
            if ((live >> l) & 1u) // wave-uniform
                reinterpret_cast<float*>(my_lists[l])[lane] = reinterpret_cast<const float*>(&recs[r0 + l].head.lists[0][0])[lane];
        if (mine) {
            const LrmPoseFootEntry E = fh[r0 + lane];
            const float rm2 = lrm_foothold_miss_rm2(E.cull_r2, margin);
            // the box slack of the header comment: S = 2^-21 (max|body| + max|centre| + rm)
            const float rm = lrm_sqrtf(E.cull_r2) + margin;
            const float M = (fmaxf(fmaxf(fabsf(body.x), fabsf(body.y)), fabsf(body.z)) +
                             fmaxf(fmaxf(fabsf(E.cull_center[0]), fabsf(E.cull_center[1])), fabsf(E.cull_center[2]))) + rm;
            const float rs = rm + 4.76837158203125e-7f * M;
            my_sphere[lane][0] = E.cull_center[0];
            my_sphere[lane][1] = E.cull_center[1];
            my_sphere[lane][2] = E.cull_center[2];
            my_sphere[lane][3] = wanted ? rm2 : -1.f;
            my_cull[lane][0] = body.x + E.cull_center[0];
            my_cull[lane][1] = body.y + E.cull_center[1];
            my_cull[lane][2] = body.z + E.cull_center[2];
            my_cull[lane][3] = wanted ? rs * rs : -1.f;
        }
        lrm_wave_lds_fence();

        int count = 0;       // survivors waiting in this wave's queue
        uint32_t near_n = 0; // lane l: leg l's misses
        uint64_t key[LRM_MAX_LEGS]; // this lane's best miss per leg (constant indices only: registers)
#pragma unroll
        for (int k = 0; k < LRM_MAX_LEGS; k++) key[k] = kLrmFootholdNone;

        auto process = [&](int m) {
            LrmVec3 t{0.f, 0.f, 0.f};
            uint32_t ti = 0u;
            if (lane < m) {
                t = LrmVec3{qx[lane], qy[lane], qz[lane]};
                ti = qi[lane];
            }
            const LrmVec3 rel{t.x - body.x, t.y - body.y, t.z - body.z};
            for (uint32_t l = 0; l < nlegs; l++) {
                if (!((live >> l) & 1u)) continue; // wave-uniform
                const bool cand = (lane < m) && lrm_foothold_miss_candidate(rel, my_sphere[l], my_sphere[l][3]);
                if (__ballot(cand) == 0ull) continue;
                const LrmPoseRecord& R = lrm_fresh(recs[r0 + l]);
                bool miss = false;
                if (cand) miss = !lrm_reach_global(R.head, my_lists[l], rel);
                const unsigned long long mm = __ballot(miss);
                if (mm == 0ull) continue; // wave-uniform: nobody needs the distance
                if ((uint32_t)lane == l) near_n += (uint32_t)__builtin_popcountll(mm);
                uint64_t kk = kLrmFootholdNone;
                if (miss) {
                    LrmVec3 d = rel;
                    lrm_dist_global(R.head, my_lists[l], d);
                    const float m2 = lrm_foothold_miss_m2(d);
                    if (m2 < inf) kk = lrm_foothold_key(m2, ti);
                }
#pragma unroll
                for (int k = 0; k < LRM_MAX_LEGS; k++)
                    if ((uint32_t)k == l) key[k] = lrm_min_u64(key[k], kk); // l is wave-uniform: one branch taken
            }
        };

        for (size_t tw0 = 0; tw0 < ntiles; tw0 += 64) {
            // lane = tile: near when its box is within (rm + S) of some non-skipped leg's sphere centre
            const size_t tl = tw0 + lane;
            bool tnear = tl < ntiles && !boxes;
            if (boxes && tl < ntiles) {
                const float* tb = boxes + tl * 6;
                for (uint32_t l = 0; l < nlegs; l++) { // wave-uniform
                    if (!((live >> l) & 1u)) continue;
                    tnear = tnear || !(lrm_box_dist2(tb, my_cull[l][0], my_cull[l][1], my_cull[l][2]) * 0.999f > my_cull[l][3]);
                }
            }
            unsigned long long near = __ballot(tnear);
            while (near != 0ull) {
                const int tb = __builtin_ctzll(near);
                near &= near - 1ull;
                const size_t tile = tw0 + tb;
                const size_t t0 = tile * kTargetTile;
                // lane = (chunk of this tile, one of four legs): a chunk is read when its box is within (rm + S) of
                // some non-skipped leg's centre (empty chunks carry an inverted box: infinitely far, unless thr = +inf)
                uint32_t cnear = 0u;
                if (boxes) {
                    const float* cb = boxes + (ntiles + tile * 16 + (lane & 15)) * 6;
                    for (uint32_t l0 = 0; l0 < nlegs; l0 += 4) { // wave-uniform
                        const uint32_t l = l0 + (lane >> 4);
                        bool touch = false;
                        if (l < nlegs && ((live >> l) & 1u))
                            touch = !(lrm_box_dist2(cb, my_cull[l][0], my_cull[l][1], my_cull[l][2]) * 0.999f > my_cull[l][3]);
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
                    // queued iff a candidate of some non-skipped leg (rm2 = -1 for a skipped one: never)
                    const LrmVec3 rel{t.x - body.x, t.y - body.y, t.z - body.z};
                    bool keep = false;
                    for (uint32_t l = 0; l < nlegs; l++) // wave-uniform
                        keep = keep || lrm_foothold_miss_candidate(rel, my_sphere[l], my_sphere[l][3]);
                    keep = keep && ok;
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
            const bool have = best != kLrmFootholdNone; // an eligible miss has m2 < +inf: its key is below ~0
            const uint32_t wi = (uint32_t)best;         // < nt when have
            const LrmFootholdChoice c = lrm_foothold_key_decode(best, have);
            miss_out[o] = c.index;
            if (m2_out) m2_out[o] = c.d2;
            if (near_out) near_out[o] = (int32_t)near_n;
            if (shift_x) { // wave-uniform
                LrmVec3 d{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
                if (have) {
                    // the winner's vector once more, from this lane's own record: strict code, the same bits
                    const LrmPoseRecord& R = recs[r0 + lane];
                    d = LrmVec3{tx[wi] - body.x, ty[wi] - body.y, tz[wi] - body.z};
                    lrm_dist_global(R.head, my_lists[lane], d);
                }
                shift_x[o] = d.x;
                shift_y[o] = d.y;
                shift_z[o] = d.z;
            }
        }
    }
}

} // namespace

hipError_t lrm_launch_foothold_misses_posed(const float* tx, const float* ty, const float* tz, size_t nt, const void* records,
                                            const void* fh_records, size_t nposes, size_t nlegs, float* tile_boxes, float margin,
                                            const int32_t* count_in, int32_t* miss_out, float* miss_m2_out, float* shift_x,
                                            float* shift_y, float* shift_z, int32_t* near_out, hipStream_t st) {
    const LrmWalkLaunch w = lrm_walk_launch(tx, ty, tz, nt, tile_boxes, nposes, kWaves, kMaxGrid, st);
    if (w.err != hipSuccess) return w.err;
    hipLaunchKernelGGL(foothold_misses_posed_kernel, w.grid, dim3(kBlock), 0, st, tx, ty, tz, nt, (const LrmPoseRecord*)records,
                       (const LrmPoseFootEntry*)fh_records, (uint32_t)nposes, (uint32_t)nlegs, w.boxes, margin, count_in, miss_out,
                       miss_m2_out, shift_x, shift_y, shift_z, near_out);
    return hipGetLastError();
}
