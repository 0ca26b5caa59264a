// lrm_footholds.hip -- gfx950 kernel of lrm_footholds_dev: per (body, leg), how many targets the leg can reach and which
// reachable target lies nearest the leg's nominal point.
//
// footholds_wave_kernel is reach_any_wave_kernel (lrm_kernels.hip) without its early exit: a wave owns one body, walks
// the tile boxes (lane = tile) and, inside a near tile, the chunk boxes (lane = chunk), and reads only the 64-target
// chunks whose box touches some leg's bounding sphere, with the next chunk's loads in flight while the current one is
// tested.  Footholds inside the body's reach sphere queue in LDS together with their index; a full batch of 64 is tested
// against every leg whose own sphere it touches.  Per leg, popcount(__ballot(hit)) adds to the count, and every hit lane
// folds the key (d2 bits << 32 | index, lrm_footholds.h) into its own per-leg minimum.  After the last batch the wave
// reduces each leg's key over its 64 lanes, and lane l writes leg l's three outputs: one store per (leg, body), no
// atomics, no second pass.
//
// boxes == null (clouds below the 4096-target threshold of the C ABI): every tile and every chunk counts as near.
//
// Compiled with -ffp-contract=off (see lrm_point.h and lrm_footholds.h).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "lrm_launch.h"
#include "lrm_types.h"
#define LRM_FRESH(L) lrm_fresh(L)
#include "lrm_point.h"
#include "lrm_point_fast.h"
#include "lrm_footholds.h"
#include "lrm_target_walk.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTargetTile = 1024; // the tiles of tile_aabb_kernel (lrm_kernels.hip)
constexpr int kQueue = 128;


#ifndef LRM_FOOTHOLDS_MIN_WAVES
#define LRM_FOOTHOLDS_MIN_WAVES 8 // as LRM_ANY_WAVE_MIN_WAVES: 64 VGPRs + 128-144 B/lane of scratch, config 3 in 1.52 ms; 5 waves (93 VGPRs, no VGPR spill): 1.81 ms
#endif
template <bool kFast>
__global__ __launch_bounds__(kBlock, LRM_FOOTHOLDS_MIN_WAVES) void footholds_wave_kernel(
    const float* __restrict__ bx, const float* __restrict__ by, const float* __restrict__ bz, size_t nb,
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz, size_t nt,
    const LrmCompiledLeg* __restrict__ legs, int nlegs, const float* __restrict__ boxes /* null = every tile near */,
    LrmFootNominal nominal, int32_t* __restrict__ count_out, int32_t* __restrict__ best_out, float* __restrict__ best_d2_out) {
    __shared__ float s_qx[kWaves][kQueue], s_qy[kWaves][kQueue], s_qz[kWaves][kQueue];
    __shared__ uint32_t s_qi[kWaves][kQueue];
    __shared__ LrmCompiledLeg::LeanCircle s_lean[LRM_MAX_LEGS][16];
    __shared__ float s_sphere[LRM_MAX_LEGS][4]; // per-leg bounding sphere: centre (relative to the body), r^2
    __shared__ float s_nom[LRM_MAX_LEGS][3];
    for (int i = threadIdx.x; i < nlegs * 64; i += kBlock)
        reinterpret_cast<float*>(&s_lean[i >> 6][0])[i & 63] = reinterpret_cast<const float*>(&legs[i >> 6].lean[0][0])[i & 63];
    if (threadIdx.x < nlegs * 4)
        s_sphere[threadIdx.x >> 2][threadIdx.x & 3] =
            (threadIdx.x & 3) < 3 ? legs[threadIdx.x >> 2].pair_center[threadIdx.x & 3] : legs[threadIdx.x >> 2].pair_r2;
    if (threadIdx.x == 0) // constant indices: the argument stays in the kernarg segment (a runtime index copies it to scratch)
#pragma unroll
        for (int k = 0; k < LRM_MAX_LEGS * 3; k++) s_nom[k / 3][k % 3] = nominal.v[k / 3][k % 3];
    __syncthreads(); // the only one
    float r2max = 0.f;
    for (int l = 0; l < nlegs; l++) r2max = fmaxf(r2max, legs[l].reach_r2_max);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* qx = s_qx[wave];
    float* qy = s_qy[wave];
    float* qz = s_qz[wave];
    uint32_t* qi = s_qi[wave];
    const size_t ntiles = (nt + kTargetTile - 1) / kTargetTile;

    for (size_t b = (size_t)blockIdx.x * kWaves + wave; b < nb; b += (size_t)gridDim.x * kWaves) {
        const LrmVec3 body{bx[b], by[b], bz[b]};
        int count = 0;        // survivors waiting in this wave's queue
        uint32_t legs_n = 0;  // lane l: leg l's reachable targets
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
            const float rx = t.x - body.x, ry = t.y - body.y, rz = t.z - body.z;
            for (int l = 0; l < nlegs; l++) {
                const float ex = rx - legs[l].pair_center[0], ey = ry - legs[l].pair_center[1], ez = rz - legs[l].pair_center[2];
                const bool inside = (lane < m) && __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex)) <= legs[l].pair_r2;
                if (__ballot(inside) == 0ull) continue;
                bool hit = false;
                if (inside) {
                    if (kFast) hit = lrm_reachable_rotate_leg_filtered(legs[l], &legs[l].lists[0][0], s_lean[l], t, body);
                    else hit = lrm_reachable_rotate_leg(legs[l], &legs[l].lists[0][0], t, body);
                }
                const unsigned long long hm = __ballot(hit);
                if (hm == 0ull) continue; // wave-uniform
                if (lane == l) legs_n += (uint32_t)__builtin_popcountll(hm);
                const uint64_t kk = hit ? lrm_foothold_key(lrm_foothold_d2(t, body, s_nom[l]), ti) : kLrmFootholdNone;
#pragma unroll
                for (int k = 0; k < LRM_MAX_LEGS; k++)
                    if (k == l) key[k] = lrm_min_u64(key[k], kk); // l is wave-uniform: one branch taken
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
                    for (int l0 = 0; l0 < nlegs; l0 += 4) { // wave-uniform
                        const int l = l0 + (lane >> 4);
                        bool touch = false;
                        if (l < nlegs)
                            touch = lrm_box_dist2(cb, body.x + s_sphere[l][0], body.y + s_sphere[l][1], body.z + s_sphere[l][2]) * 0.999f <=
                                    s_sphere[l][3];
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
        lrm_wave_lds_fence(); // the queue is refilled by this wave's next body

        // per leg: the wave's smallest key; lane l keeps leg l's
        uint64_t best = kLrmFootholdNone;
#pragma unroll
        for (int k = 0; k < LRM_MAX_LEGS; k++) {
            if (k >= nlegs) break; // wave-uniform
            const uint64_t v = lrm_wave_min_u64(key[k]);
            if (lane == k) best = v;
        }
        if (lane < nlegs) {
            const size_t o = (size_t)lane * nb + b;
            const LrmFootholdChoice c = lrm_foothold_key_decode(best, legs_n != 0u);
            count_out[o] = (int32_t)legs_n;
            best_out[o] = c.index;
            if (best_d2_out) best_d2_out[o] = c.d2;
        }
    }
}

} // namespace

hipError_t lrm_launch_footholds(const float* bx, const float* by, const float* bz, size_t nb, const float* tx,
                                const float* ty, const float* tz, size_t nt, const LrmCompiledLeg* legs_dev, int nlegs,
                                float* tile_boxes, const LrmFootNominal& nominal, int32_t* count_out, int32_t* best_out,
                                float* best_d2_out, bool fast, hipStream_t st) {
    const LrmWalkLaunch w = lrm_walk_launch(tx, ty, tz, nt, tile_boxes, nb, kWaves, 0 /* a wave per body, no cap */, st);
    if (w.err != hipSuccess) return w.err;
    if (fast)
        hipLaunchKernelGGL(footholds_wave_kernel<true>, w.grid, dim3(kBlock), 0, st, bx, by, bz, nb, tx, ty, tz, nt, legs_dev, nlegs,
                           w.boxes, nominal, count_out, best_out, best_d2_out);
    else
        hipLaunchKernelGGL(footholds_wave_kernel<false>, w.grid, dim3(kBlock), 0, st, bx, by, bz, nb, tx, ty, tz, nt, legs_dev, nlegs,
                           w.boxes, nominal, count_out, best_out, best_d2_out);
    return hipGetLastError();
}
