// lrm_foothold_support.hip -- gfx950 kernels of lrm_foothold_support_posed_dev: per (target, leg), how many poses of a
// pose table can put that foot there, and which pose does it best.  The foothold family's traversal with the roles
// swapped: lanes own TARGETS, poses are the thing culled and streamed.
//
// Triple (t, p, l) reaches iff pose p is live (pose_live null or pose_live[p] != 0) and
// reachability_global(t - body[p], legs[l], quats[p]): lrm_reach_global on the pose record, strict arithmetic whatever
// lrm_set_mode says -- lrm_footholds_posed_dev's rule.  Per (l, t): the number of reaching poses and the reaching pose
// with the smallest lrm_foothold_key(d2, p), d2 = lrm_foothold_d2(t, body[p], nominal_w[p, l]) (lrm_footholds.h).
//
// Three launches on one stream, nothing else (no allocation, no host synchronisation):
//  * foothold_support_prepare_kernel: (a) resets the call's accumulators in the support workspace (count 0, key ~0);
//    (b) lane = pose, wave = a chunk of kPoseChunk poses: per (pose, leg) the CULL SPHERE {C = body + centre,
//    thr = (r + S)^2} (16 bytes, for the sphere-against-box test below) and, reduced over the chunk's live poses and all
//    legs by six __shfl_xor steps, the chunk's box of C -/+ (r + S) * 1.001.  A dead pose adds nothing to the box.  A sphere
//    with r2 = +inf or anything non-finite gets thr = +inf and makes its chunk's box (-inf, +inf): never culled.
//  * foothold_support_kernel: a wave owns one 64-target chunk (a target per lane, in registers) and one SLICE of the
//    pose chunks: chunk c belongs to slice c % S, so that the poses near a piece of terrain, which are neighbours in any
//    sensible pose order, spread over all S waves of that piece.  The wave reduces its own targets' box in-wave (it does
//    not touch the pair kernels' per-device box buffer), tests its pose-chunk boxes with lane = pose chunk and a ballot,
//    and visits the survivors in ascending order.  Inside a chunk lane = pose: every lane tests its own pose's nlegs
//    cull spheres against the wave's target box and keeps a leg mask; a second ballot gives the poses to visit, in
//    ascending order, each with its leg mask through readlane.  A visited pose's body and entries sit at wave-uniform
//    addresses (scalars through lrm_fresh); per surviving leg the lane-wise sphere test of footholds_posed_traverse
//    (the same expression) decides which lanes run lrm_reach_global, and the circle tables of the legs with any such lane
//    are staged in the wave's LDS slot first (one float per lane and leg between two wave fences).  Each lane keeps its
//    own count[l] and 64-bit key minimum key[l]; no cross-lane reduction, no queue, no __syncthreads.  At the end a lane
//    adds its non-zero counts with atomicAdd and folds its keys with a 64-bit unsigned atomicMin into the workspace: both
//    order-independent, so the result is bit-deterministic whatever S is.
//  * foothold_support_finish_kernel: a thread per target unpacks the keys into best_pose / best_d2 and forms legs_mask.
//
// Deviation from a scalar sphere-against-box test per visited (pose, leg): gfx950 has no scalar float ALU, so a
// wave-uniform test would occupy the same VALU slots as the 64 lane-wise sphere tests it guards.  The test runs with
// lane = pose instead, 64 poses at once, and whole poses are skipped before any of their scalars are loaded.
//
// ALL BOX TESTS ARE CULLS ONLY AND NEVER DROP A PAIR THE LANE-WISE TEST KEEPS.  The lane-wise test forms
// e = (t - body) - centre and keeps e2 <= r2; the boxes are built about C = fl(body + centre): two roundings of one
// point.  With eps = 2^-24, per axis k (lrm_foothold_misses.hip has the same steps)
//   |t_k - C_k| <= |e_k| (1 + 2 eps) + 3 eps M,   M = max|body_k| + max|centre_k| + r,
// and |e_k| <= r (1 + 2 eps) for a kept pair.
//   - sphere against target box: the box distance g from C obeys |g| <= r (1 + 4 eps) + 3 sqrt(3) eps M and its computed
//     square D <= g^2 (1 + 6 eps); the test keeps unless D * 0.999 > (r + S)^2 with S = 2^-21 M = 8 eps M.
//   - pose-chunk box against target box: per axis the pose box is C_k -/+ h, h = (r + S) * 1.001 >= r (1 + 4 eps) + S, and
//     rounding C_k -/+ h costs at most eps (M + h) < 2.01 eps M, so 3 eps M + 2.01 eps M < S keeps t_k inside.  Minima and
//     maxima over poses, legs and targets are exact; the two boxes are compared per axis, no arithmetic.
// Both comparisons are written negated (!(a > b)): a nan on either side keeps.  4e6 mm from the origin S is 1.9 mm where
// the two roundings differ by up to 0.5 mm.
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
constexpr int kPoseChunk = 64;          // poses per pose-chunk box: one per lane in the second level
constexpr size_t kTargetWaves = 16384;  // waves asked for: two rounds of 8 waves per SIMD on 256 CUs
constexpr size_t kMaxSlices = 32;       // slices of the pose range per target chunk, at most
constexpr size_t kMaxPrepareBlocks = 2048;

struct SupportLayout { // the support workspace, every part 16-byte aligned
    size_t keys, counts, spheres, boxes, bytes;
};
__host__ __device__ inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
inline SupportLayout support_layout(size_t nposes, size_t nlegs, size_t nt) {
    SupportLayout L;
    const size_t npc = (nposes + kPoseChunk - 1) / kPoseChunk;
    L.keys = 0;
    L.counts = L.keys + align16(nlegs * nt * sizeof(uint64_t));
    L.spheres = L.counts + align16(nlegs * nt * sizeof(int32_t));
    L.boxes = L.spheres + nposes * nlegs * 4 * sizeof(float);
    L.bytes = L.boxes + align16(npc * 6 * sizeof(float));
    return L;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ float uniform(float v) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v))); }

__global__ __launch_bounds__(kBlock) void foothold_support_prepare_kernel(
    const LrmPoseRecord* __restrict__ recs, const LrmPoseFootEntry* __restrict__ fh, uint32_t nposes, uint32_t nlegs,
    const uint8_t* __restrict__ pose_live /* may be null */, size_t nacc /* nlegs * nt */, uint64_t* __restrict__ keys,
    int32_t* __restrict__ counts, float4* __restrict__ spheres, float* __restrict__ boxes) {
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < nacc; i += (size_t)gridDim.x * kBlock) {
        keys[i] = kLrmFootholdNone;
        counts[i] = 0;
    }
    const uint32_t npc = (nposes + kPoseChunk - 1) / kPoseChunk;
    const int lane = threadIdx.x & 63;
    const float inf = __builtin_inff();
    for (uint32_t c = blockIdx.x * kWaves + (threadIdx.x >> 6); c < npc; c += gridDim.x * kWaves) { // wave-uniform
        const uint32_t p = c * kPoseChunk + lane; // < 2^31 + 64
        const bool have = p < nposes;
        const bool live = have && (!pose_live || pose_live[p] != 0);
        float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
        bool open = false;
        if (have) {
            const uint32_t r0 = p * nlegs; // nposes * nlegs < 2^32 (checked by the C ABI)
            const float b[3] = {recs[r0].body_pos[0], recs[r0].body_pos[1], recs[r0].body_pos[2]}; // the same in every record of the pose
            const float bm = fmaxf(fmaxf(fabsf(b[0]), fabsf(b[1])), fabsf(b[2]));
            for (uint32_t l = 0; l < nlegs; l++) {
                const LrmPoseFootEntry E = fh[r0 + l];
                const float r = lrm_sqrtf(E.cull_r2);
                const float M = (bm + fmaxf(fmaxf(fabsf(E.cull_center[0]), fabsf(E.cull_center[1])), fabsf(E.cull_center[2]))) + r;
                const float rs = r + 4.76837158203125e-7f * M; // r + S, S = 2^-21 M (header comment)
                const float h = rs * 1.001f;
                const float C[3] = {b[0] + E.cull_center[0], b[1] + E.cull_center[1], b[2] + E.cull_center[2]};
                float thr = rs * rs;
                float l3[3], h3[3];
                bool fin = fabsf(thr) < inf;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    l3[k] = C[k] - h;
                    h3[k] = C[k] + h;
                    fin = fin && fabsf(l3[k]) < inf && fabsf(h3[k]) < inf; // false for nan
                }
                if (!fin) thr = inf;
                spheres[r0 + l] = fin ? make_float4(C[0], C[1], C[2], thr) : make_float4(0.f, 0.f, 0.f, inf);
                if (live) {
                    open = open || !fin;
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        lo[k] = fminf(lo[k], fin ? l3[k] : inf);
                        hi[k] = fmaxf(hi[k], fin ? h3[k] : -inf);
                    }
                }
            }
        }
        const bool any_open = __ballot(open) != 0ull;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            lo[k] = wave_min(lo[k]);
            hi[k] = wave_max(hi[k]);
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                boxes[(size_t)c * 6 + k] = any_open ? -inf : lo[k];
                boxes[(size_t)c * 6 + 3 + k] = any_open ? inf : hi[k];
            }
        }
    }
}

__device__ __forceinline__ float box_dist2(const float* lo, const float* hi, float x, float y, float z) {
    const float ex = fmaxf(fmaxf(lo[0] - x, x - hi[0]), 0.f);
    const float ey = fmaxf(fmaxf(lo[1] - y, y - hi[1]), 0.f);
    const float ez = fmaxf(fmaxf(lo[2] - z, z - hi[2]), 0.f);
    return ex * ex + ey * ey + ez * ez;
}

// Minimum waves per SIMD asked of the compiler (DESIGN.md 3.15 has the resource figures behind the choice).
#ifndef LRM_FOOTHOLD_SUPPORT_MIN_WAVES
#define LRM_FOOTHOLD_SUPPORT_MIN_WAVES 8
#endif
__global__ __launch_bounds__(kBlock, LRM_FOOTHOLD_SUPPORT_MIN_WAVES) void foothold_support_kernel(
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz, size_t nt,
    const LrmPoseRecord* __restrict__ recs, const LrmPoseFootEntry* __restrict__ fh, uint32_t nposes, uint32_t nlegs,
    const uint8_t* __restrict__ pose_live /* may be null */, const float4* __restrict__ spheres, const float* __restrict__ boxes,
    uint32_t slices, uint64_t nwaves, uint64_t* __restrict__ keys, int32_t* __restrict__ counts) {
    __shared__ LrmCircle s_lists[kWaves][LRM_MAX_LEGS][4 * LRM_N_CIRCLES]; // the circle tables of the pose a wave visits
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    LrmCircle(*my_lists)[4 * LRM_N_CIRCLES] = s_lists[wave];
    const uint64_t w = (uint64_t)blockIdx.x * kWaves + wave;
    if (w >= nwaves) return; // wave-uniform; no workgroup barrier anywhere
    const uint64_t tc = w / slices;                // this wave's target chunk
    const uint32_t slice = (uint32_t)(w % slices); // and its share of the pose chunks: c % slices == slice
    const uint32_t npc = (nposes + kPoseChunk - 1) / kPoseChunk;
    const float inf = __builtin_inff(), nan = __builtin_nanf("");

    const size_t ti = (size_t)tc * 64 + lane;
    const bool ok = ti < nt;
    LrmVec3 t{nan, nan, nan}; // a lane past the cloud holds a target that is inside nothing
    if (ok) t = LrmVec3{tx[ti], ty[ti], tz[ti]};
    // this wave's own box: nan coordinates stay out (they reach nothing), infinite ones make it infinite
    float tlo[3], thi[3];
    {
        const float v[3] = {t.x, t.y, t.z};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            tlo[k] = uniform(wave_min(v[k] == v[k] ? v[k] : inf));
            thi[k] = uniform(wave_max(v[k] == v[k] ? v[k] : -inf));
        }
    }

    int32_t count[LRM_MAX_LEGS]; // this lane's target: reaching poses per leg (constant indices only: registers)
    uint64_t key[LRM_MAX_LEGS];  // and the best of them
#pragma unroll
    for (int k = 0; k < LRM_MAX_LEGS; k++) {
        count[k] = 0;
        key[k] = kLrmFootholdNone;
    }

    auto visit = [&](uint32_t p, uint32_t legmask) { // both wave-uniform
        const uint32_t r0 = p * nlegs; // nposes * nlegs < 2^32 (checked by the C ABI)
        const LrmPoseRecord& R0 = lrm_fresh(recs[r0]);
        const LrmVec3 body{R0.body_pos[0], R0.body_pos[1], R0.body_pos[2]}; // the same in every record of the pose
        const LrmVec3 rel{t.x - body.x, t.y - body.y, t.z - body.z};
        uint32_t in_legs = 0u;  // this lane: the legs whose sphere holds its target
        uint32_t any_legs = 0u; // wave-uniform: the legs with such a lane
        for (uint32_t mm = legmask; mm != 0u; mm &= mm - 1u) {
            const uint32_t l = (uint32_t)__builtin_ctz(mm);
            const LrmPoseFootEntry& E = lrm_fresh(fh[r0 + l]);
            const float ex = rel.x - E.cull_center[0], ey = rel.y - E.cull_center[1], ez = rel.z - E.cull_center[2];
            const bool inside = __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex)) <= E.cull_r2; // footholds_posed_traverse's test
            if (__ballot(inside) != 0ull) any_legs |= 1u << l;
            if (inside) in_legs |= 1u << l;
        }
        if (any_legs == 0u) return;
        lrm_wave_lds_fence(); // every lane is done with the previous pose's tables
        for (uint32_t mm = any_legs; mm != 0u; mm &= mm - 1u) {
            const uint32_t l = (uint32_t)__builtin_ctz(mm);
            reinterpret_cast<float*>(my_lists[l])[lane] = reinterpret_cast<const float*>(&recs[r0 + l].head.lists[0][0])[lane];
        }
        lrm_wave_lds_fence();
        for (uint32_t mm = any_legs; mm != 0u; mm &= mm - 1u) {
            const uint32_t l = (uint32_t)__builtin_ctz(mm);
            bool hit = false;
            if ((in_legs >> l) & 1u) {
                const LrmPoseRecord& R = lrm_fresh(recs[r0 + l]);
                hit = lrm_reach_global(R.head, my_lists[l], rel);
            }
            if (__ballot(hit) == 0ull) continue; // wave-uniform
            const LrmPoseFootEntry& E = lrm_fresh(fh[r0 + l]);
            const uint64_t kk = hit ? lrm_foothold_key(lrm_foothold_d2(t, body, E.nominal_w), p) : kLrmFootholdNone;
#pragma unroll
            for (int k = 0; k < LRM_MAX_LEGS; k++)
                if ((uint32_t)k == l) { // l is wave-uniform: one branch taken
                    count[k] += hit ? 1 : 0;
                    key[k] = lrm_min_u64(key[k], kk);
                }
        }
    };

    const uint32_t stride = 64u * slices; // pose chunks one round of the first level covers; npc + stride < 2^32
    for (uint32_t c0 = slice; c0 < npc; c0 += stride) { // wave-uniform
        // lane = pose chunk: kept unless the boxes are apart on some axis (a nan keeps)
        const uint32_t c = c0 + (uint32_t)lane * slices;
        bool keep = false;
        if (c < npc) {
            const float* pb = boxes + (size_t)c * 6;
            keep = !(tlo[0] > pb[3]) && !(thi[0] < pb[0]) && !(tlo[1] > pb[4]) && !(thi[1] < pb[1]) && !(tlo[2] > pb[5]) && !(thi[2] < pb[2]);
        }
        unsigned long long near = __ballot(keep);
        while (near != 0ull) {
            const uint32_t chunk = c0 + (uint32_t)__builtin_ctzll(near) * slices;
            near &= near - 1ull;
            // lane = pose of the chunk: the legs whose cull sphere comes within (r + S) of the wave's target box
            const uint32_t p = chunk * kPoseChunk + lane;
            uint32_t legmask = 0u;
            if (p < nposes && (!pose_live || pose_live[p] != 0)) {
                for (uint32_t l = 0; l < nlegs; l++) { // wave-uniform bound
                    const float4 sp = spheres[p * nlegs + l];
                    if (!(box_dist2(tlo, thi, sp.x, sp.y, sp.z) * 0.999f > sp.w)) legmask |= 1u << l;
                }
            }
            unsigned long long todo = __ballot(legmask != 0u);
            while (todo != 0ull) {
                const int k = __builtin_ctzll(todo);
                todo &= todo - 1ull;
                visit(chunk * kPoseChunk + (uint32_t)k, (uint32_t)__builtin_amdgcn_readlane((int)legmask, k));
            }
        }
    }

    if (ok) {
#pragma unroll
        for (int k = 0; k < LRM_MAX_LEGS; k++) {
            if ((uint32_t)k >= nlegs) break;
            if (count[k] == 0) continue;
            const size_t o = (size_t)k * nt + ti;
            atomicAdd(&counts[o], count[k]);
            atomicMin(reinterpret_cast<unsigned long long*>(&keys[o]), (unsigned long long)key[k]);
        }
    }
}

__global__ __launch_bounds__(kBlock) void foothold_support_finish_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ counts,
                                                                        size_t nt, uint32_t nlegs, int32_t* __restrict__ count_out,
                                                                        int32_t* __restrict__ best_pose_out, float* __restrict__ best_d2_out,
                                                                        uint8_t* __restrict__ legs_mask_out) {
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nt) return;
    uint32_t mask = 0u;
    for (uint32_t l = 0; l < nlegs; l++) {
        const size_t o = (size_t)l * nt + t;
        const int32_t n = counts[o];
        const LrmFootholdChoice c = lrm_foothold_key_decode(keys[o], n != 0);
        count_out[o] = n;
        best_pose_out[o] = c.index;
        if (best_d2_out) best_d2_out[o] = c.d2;
        if (n) mask |= 1u << l;
    }
    if (legs_mask_out) legs_mask_out[t] = (uint8_t)mask;
}

} // namespace

size_t lrm_foothold_support_bytes(size_t nposes, size_t nlegs, size_t nt) { return support_layout(nposes, nlegs, nt).bytes; }

void lrm_foothold_support_grid(size_t nt, size_t nposes, uint64_t out[4]) {
    const size_t ntc = (nt + 63) / 64, npc = (nposes + kPoseChunk - 1) / kPoseChunk;
    size_t s = ntc ? (kTargetWaves + ntc - 1) / ntc : 1;
    if (s > kMaxSlices) s = kMaxSlices;
    if (s > npc) s = npc;
    if (s < 1) s = 1;
    out[0] = kPoseChunk;
    out[1] = s;
    out[2] = (npc + s - 1) / s * kPoseChunk; // the most poses one slice walks: its pose chunks are c % s == slice
    out[3] = (ntc * s + kWaves - 1) / kWaves;
}

hipError_t lrm_launch_foothold_support(const float* tx, const float* ty, const float* tz, size_t nt, const void* records,
                                       const void* fh_records, size_t nposes, size_t nlegs, const uint8_t* pose_live,
                                       void* support_workspace, int32_t* count_out, int32_t* best_pose_out, float* best_d2_out,
                                       uint8_t* legs_mask_out, hipStream_t st) {
    const SupportLayout L = support_layout(nposes, nlegs, nt);
    char* ws = (char*)support_workspace;
    uint64_t* keys = (uint64_t*)(ws + L.keys);
    int32_t* counts = (int32_t*)(ws + L.counts);
    float4* spheres = (float4*)(ws + L.spheres);
    float* boxes = (float*)(ws + L.boxes);
    uint64_t grid[4];
    lrm_foothold_support_grid(nt, nposes, grid);
    const size_t nacc = nlegs * nt, npc = (nposes + kPoseChunk - 1) / kPoseChunk;
    size_t gp = (nacc + kBlock - 1) / kBlock;
    if (gp > kMaxPrepareBlocks) gp = kMaxPrepareBlocks;
    if (gp < (npc + kWaves - 1) / kWaves) gp = (npc + kWaves - 1) / kWaves; // <= 2^23
    hipLaunchKernelGGL(foothold_support_prepare_kernel, dim3((unsigned)gp), dim3(kBlock), 0, st, (const LrmPoseRecord*)records,
                       (const LrmPoseFootEntry*)fh_records, (uint32_t)nposes, (uint32_t)nlegs, pose_live, nacc, keys, counts, spheres, boxes);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (nposes) {
        const uint64_t nwaves = (uint64_t)((nt + 63) / 64) * grid[1];
        hipLaunchKernelGGL(foothold_support_kernel, dim3((unsigned)grid[3]), dim3(kBlock), 0, st, tx, ty, tz, nt, (const LrmPoseRecord*)records,
                           (const LrmPoseFootEntry*)fh_records, (uint32_t)nposes, (uint32_t)nlegs, pose_live, spheres, boxes,
                           (uint32_t)grid[1], nwaves, keys, counts);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(foothold_support_finish_kernel, dim3((unsigned)((nt + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, keys, counts, nt,
                       (uint32_t)nlegs, count_out, best_pose_out, best_d2_out, legs_mask_out);
    return hipGetLastError();
}
