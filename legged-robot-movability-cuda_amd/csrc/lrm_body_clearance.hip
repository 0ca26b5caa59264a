// lrm_body_clearance.hip -- gfx950 kernel of lrm_body_clearance_posed_dev: per pose of a pose table, how many terrain
// targets stand inside the body volume (a cylinder about the body's z axis, in the BODY frame), which target of the
// column under the body stands highest over the belly plane, and by how much.
//
// With q = t - body[p], v = lrm_qrot(inv_rot of the pose, q) (lrm_body_clearance.h, shared with the host loop):
//   column  in_cylinder(radius, plus_z, floor_z, 0, v);   hit  in_cylinder(radius, plus_z, minus_z, 0, v);
//   height  v.z - minus_z;   answer: the number of hits, the column target with the smallest lrm_clearance_key.
//
// body_clearance_posed_kernel takes the traversal of footholds_posed_traverse (lrm_footholds_posed.hip, which this file
// leaves alone) without its LDS: a wave owns one pose and strides over the rest; lane = tile walks the 1024-target tile
// boxes, lane = chunk the sixteen 64-target chunk boxes of a near tile, and every lane of a near chunk loads its own
// target, with the next near chunk's loads in flight while the current one is tested.  The per-pair work is some
// twenty float operations on nine matrix scalars and three body scalars read once per pose (lrm_fresh: s_load), so
// there is no survivor queue and no staged table: a lane tests what it loaded.  popcount(__ballot(hit)) adds to the
// wave's count, each lane folds one 64-bit key, six __shfl_xor steps reduce the keys, lane 0 stores.  No atomics, no
// __syncthreads, no LDS.  A pose with live_in[p] == 0 is answered before anything else is loaded.
//
// THE CULL SPHERE NEVER DROPS A COLUMN TARGET.  It is about body[p] itself, radius r:
//   - a column target has computed sqrt(vx^2 + vy^2) < radius and floor_z < vz < plus_z, so with
//     zmax = max(|plus_z|, |floor_z|) its |v| < rc (1 + 3 eps), rc = sqrt(radius^2 + zmax^2), eps = 2^-24;
//   - v is the rounded image of q under I + 2 inv_rot, which for |quat|^2 within 1e-5 of 1 changes lengths by less than
//     2e-5 of them (lrm_footholds_posed.h) plus the rounding of the coefficients and of the nine products and sums,
//     below 20 eps |q|: |q| < |v| (1 + 4e-5).  Hence |q| < rc * 1.0001 =: r, roundings of rc and r included.
//   - the box gap is formed as bb - body per axis, q as t - body: rounding is monotone, so for a target inside the box the
//     computed gap e_k <= |q_k| EXACTLY, and the computed square D <= |q|^2 (1 + 3 eps).  Unlike the siblings' spheres
//     (DESIGN.md 3.14, 3.15), whose centre fl(body + centre) is a second rounding of the point the exact test forms as
//     (t - body) - centre, this sphere needs no absolute slack and carries none: thr = r^2.  The factor 0.999 covers the
//     rounding of D and of r^2.
//   The test is written !(D * 0.999 > thr): a nan on either side keeps the box (a nan body gives gaps of 0 through fmaxf,
//   inf - inf in a box of infinite targets a nan D).  An infinite radius or plus_z gives r = +inf, and so does a pose whose leg-0 foothold entry has
//   cull_r2 = +inf (|quat|^2 not within 1e-5 of 1, nan included: v is not a rotation of q): nothing is culled.
//
// boxes == null (clouds below the 4096-target threshold of the C ABI): every tile and every chunk counts as near.
//
// Compiled with -ffp-contract=off (see lrm_point.h).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "lrm_launch.h"
#include "lrm_types.h"
#include "lrm_compile_head.h"
#include "lrm_point.h"
#include "lrm_footholds_posed.h"
#include "lrm_body_clearance.h"
#include "lrm_target_walk.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTargetTile = 1024; // the tiles of tile_aabb_kernel (lrm_kernels.hip)
constexpr unsigned kMaxGrid = 16384; // 65 536 poses in flight; a wave strides over the rest (footholds_posed_kernel's cap)


// Minimum waves per SIMD asked of the compiler.  The kernel needs 32 VGPRs, so 8 waves fit a SIMD whatever is asked; what
// the bound changes is the SGPR budget: asking for 8 leaves 78 SGPRs and spills 16 to VGPR lanes, asking for 4 gives 95
// and spills none.
#ifndef LRM_BODY_CLEARANCE_MIN_WAVES
#define LRM_BODY_CLEARANCE_MIN_WAVES 4
#endif
__global__ __launch_bounds__(kBlock, LRM_BODY_CLEARANCE_MIN_WAVES) void body_clearance_posed_kernel(
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz, size_t nt,
    const LrmPoseRecord* __restrict__ recs, const LrmPoseFootEntry* __restrict__ fh, uint32_t nposes, uint32_t nlegs,
    const float* __restrict__ boxes /* null = every tile near */, float radius, float plus_z, float minus_z, float floor_z,
    const uint8_t* __restrict__ live_in /* may be null */, int32_t* __restrict__ hits_out, int32_t* __restrict__ top_out,
    float* __restrict__ height_out /* may be null */, uint8_t* __restrict__ free_out /* may be null */) {
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const size_t ntiles = (nt + kTargetTile - 1) / kTargetTile;
    const float inf = __builtin_inff();
    // the cylinder's bounding radius about the body origin (header comment); +inf for an uncullable cylinder
    const float zmax = fmaxf(fabsf(plus_z), fabsf(floor_z));
    const float rcyl = lrm_sqrtf(radius * radius + zmax * zmax) * 1.0001f;

    for (uint32_t p = blockIdx.x * kWaves + wave; p < nposes; p += gridDim.x * kWaves) { // wave-uniform
        if (live_in && live_in[p] == 0) { // a skipped pose: the empty answer, before any table is read
            if (lane == 0) {
                hits_out[p] = 0;
                top_out[p] = -1;
                if (height_out) height_out[p] = -inf;
                if (free_out) free_out[p] = 0;
            }
            continue;
        }
        const uint32_t r0 = p * nlegs; // nposes * nlegs < 2^32 (checked by the C ABI); leg 0's record and entry
        const LrmPoseRecord& R0 = lrm_fresh(recs[r0]);
        const LrmVec3 body{R0.body_pos[0], R0.body_pos[1], R0.body_pos[2]}; // the same in every record of the pose
        float m[9];                                                           // and so is inv_rot
#pragma unroll
        for (int k = 0; k < 9; k++) m[k] = R0.head.inv_rot[k];
        const float r = lrm_fresh(fh[r0]).cull_r2 < inf ? rcyl : inf;
        const float thr = r * r;

        uint32_t hits = 0u;               // wave-uniform
        uint64_t key = kLrmClearanceNone; // this lane's highest column target

        for (size_t tw0 = 0; tw0 < ntiles; tw0 += 64) {
            const size_t tl = tw0 + lane; // lane = tile
            unsigned long long near =
                __ballot(tl < ntiles && (!boxes || !(lrm_box_dist2(boxes + tl * 6, body.x, body.y, body.z) * 0.999f > thr)));
            while (near != 0ull) {
                const int tb = __builtin_ctzll(near);
                near &= near - 1ull;
                const size_t tile = tw0 + tb;
                const size_t t0 = tile * kTargetTile;
                // lane = chunk of this tile (empty chunks carry an inverted box: infinitely far, unless thr is +inf)
                uint32_t cnear;
                if (boxes) {
                    cnear = (uint32_t)__ballot(lane < 16 && !(lrm_box_dist2(boxes + (ntiles + tile * 16 + (lane & 15)) * 6, body.x, body.y, body.z) *
                                                                  0.999f > thr)) & 0xffffu;
                } else {
                    const size_t left = nt - t0; // > 0: tile < ntiles
                    const int chunks = left >= (size_t)kTargetTile ? 16 : (int)((left + 63) / 64);
                    cnear = chunks == 16 ? 0xffffu : (1u << chunks) - 1u;
                }
                if (!cnear) continue; // the tile box touches the sphere, no chunk box does
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
                    float h;
                    unsigned in = lrm_clearance_test(m, LrmVec3{t.x - body.x, t.y - body.y, t.z - body.z}, radius, plus_z, minus_z, floor_z, &h);
                    if (!ok) in = 0u;
                    hits += (uint32_t)__builtin_popcountll(__ballot((in & LRM_CLEARANCE_HIT) != 0u));
                    if (in & LRM_CLEARANCE_COLUMN) key = lrm_min_u64(key, lrm_clearance_key(h, ti));
                }
            }
        }

        key = lrm_wave_min_u64(key);
        if (lane == 0) {
            const LrmClearanceTop top = lrm_clearance_key_decode(key);
            hits_out[p] = (int32_t)hits;
            top_out[p] = top.index;
            if (height_out) height_out[p] = top.height;
            if (free_out) free_out[p] = hits == 0u;
        }
    }
}

} // namespace

hipError_t lrm_launch_body_clearance_posed(const float* tx, const float* ty, const float* tz, size_t nt, const void* records,
                                           const void* fh_records, size_t nposes, size_t nlegs, float* tile_boxes, float radius,
                                           float plus_z, float minus_z, float floor_z, const uint8_t* live_in, int32_t* hits_out,
                                           int32_t* top_out, float* height_out, uint8_t* free_out, hipStream_t st) {
    const LrmWalkLaunch w = lrm_walk_launch(tx, ty, tz, nt, tile_boxes, nposes, kWaves, kMaxGrid, st);
    if (w.err != hipSuccess) return w.err;
    hipLaunchKernelGGL(body_clearance_posed_kernel, w.grid, dim3(kBlock), 0, st, tx, ty, tz, nt, (const LrmPoseRecord*)records,
                       (const LrmPoseFootEntry*)fh_records, (uint32_t)nposes, (uint32_t)nlegs, w.boxes, radius, plus_z, minus_z, floor_z,
                       live_in, hits_out, top_out, height_out, free_out);
    return hipGetLastError();
}
