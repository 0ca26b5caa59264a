// lrm_pose_edges.hip -- the gfx950 kernels of lrm_pose_edge_counts_dev and lrm_pose_edges_dev (include/lrm.h): the neighbour
// poses of every pose within a step and a turn, as counts and as a CSR edge list.  The arithmetic is lrm_pose_edges.h's, the
// same the host loop runs.  Compiled with -ffp-contract=off.
//
//  * edges_box_kernel: a wave per chunk of LRM_EDGES_CHUNK consecutive poses; the bounding box of the bodies of the chunk's
//    VALID poses and their number go to the workspace (lo.xyz, n, hi.xyz, 0).  A non-finite body is never valid, so it
//    never enters a box; a chunk without a valid pose has n = 0 and is always culled.
//  * edges_group_box_kernel: a wave per group of LRM_EDGES_ROUND consecutive chunks; the union of their boxes and the sum
//    of their numbers, behind the chunk boxes in the workspace: the second level (measured: DESIGN.md 3.26).
//  * edges_walk_kernel<fill>: a wave owns a chunk, lane = pose p.  It walks the group boxes in ascending order,
//    LRM_EDGES_ROUND per round, one per lane, and ballots the survivors of the exact cull: box gap squared > step2
//    (lrm_edges_box_gap2: a lower bound of every pair's computed d2, so no pair on the threshold is lost; a group box holds
//    its chunks' boxes, so its gap is a lower bound of theirs).  For each surviving group, in ascending order, one round
//    tests its chunk boxes the same way.  For each surviving chunk, in ascending order, the 64 candidate poses are loaded
//    once into the wave's LDS slice (an invalid candidate with x = NaN: its d2 passes no test), and every lane tests them
//    in ascending q by broadcast reads: d2 first, the quaternion only where d2 passes.  Form 0 starts at the wave's own chunk and takes q > p there.  Ascending q falls out of the walk:
//    no sort, no atomics, no workgroup waits for another, and the answer is bit-deterministic.  With fill, lane p stores its
//    k-th neighbour at offsets[p] + k while the segment has room (lrm_edges_room) and nothing anywhere else.
// Every index is checked before an address is formed from it: a box index against the chunk count, a pose index against
// nposes, a list position against the room, which lies inside [0, capacity).  DESIGN.md 3.26.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "lrm_pose_edges.h"
#include "lrm_target_walk.h"

namespace {

constexpr int kBlock = LRM_EDGES_BLOCK;
constexpr int kChunk = LRM_EDGES_CHUNK;
constexpr int kWaves = kBlock / kChunk;
constexpr int kBoxFloats = LRM_EDGES_BOX_FLOATS;
static_assert(kChunk == 64 && LRM_EDGES_ROUND == 64, "a chunk and a walk round are the lanes of a wave");

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

__global__ __launch_bounds__(kBlock) void edges_box_kernel(const LrmEdgesArgs A, float* __restrict__ boxes) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nchunks = (A.nposes + (uint32_t)(kChunk - 1)) / (uint32_t)kChunk; // nposes <= INT32_MAX: no wrap
    const uint32_t chunk = blockIdx.x * (uint32_t)kWaves + (threadIdx.x >> 6);
    if (chunk >= nchunks) return; // the whole wave alike; no workgroup barrier below
    const uint32_t p = chunk * (uint32_t)kChunk + lane;
    float v[8];
    const bool valid = p < A.nposes && lrm_edges_pose(A.quats, A.body, A.pose_live, p, v);
    const float inf = __builtin_inff();
    const float lx = wave_min(valid ? v[0] : inf), ly = wave_min(valid ? v[1] : inf), lz = wave_min(valid ? v[2] : inf);
    const float hx = wave_max(valid ? v[0] : -inf), hy = wave_max(valid ? v[1] : -inf), hz = wave_max(valid ? v[2] : -inf);
    const float n = (float)__popcll(__ballot(valid));
    if (lane == 0u) {
        float4* const out = reinterpret_cast<float4*>(boxes + (size_t)chunk * kBoxFloats);
        out[0] = make_float4(lx, ly, lz, n);
        out[1] = make_float4(hx, hy, hz, 0.f);
    }
}

__global__ __launch_bounds__(kBlock) void edges_group_box_kernel(uint32_t nchunks, float* __restrict__ boxes) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t ngroups = (nchunks + (uint32_t)(LRM_EDGES_ROUND - 1)) / (uint32_t)LRM_EDGES_ROUND;
    const uint32_t group = blockIdx.x * (uint32_t)kWaves + (threadIdx.x >> 6);
    if (group >= ngroups) return; // the whole wave alike; no workgroup barrier below
    const uint32_t chunk = group * (uint32_t)LRM_EDGES_ROUND + lane;
    const float inf = __builtin_inff();
    float4 lo = make_float4(inf, inf, inf, 0.f), hi = make_float4(-inf, -inf, -inf, 0.f);
    if (chunk < nchunks) {
        const float4* const bp = reinterpret_cast<const float4*>(boxes + (size_t)chunk * kBoxFloats);
        lo = bp[0], hi = bp[1]; // an empty chunk holds +inf / -inf and 0
    }
    const float lx = wave_min(lo.x), ly = wave_min(lo.y), lz = wave_min(lo.z);
    const float hx = wave_max(hi.x), hy = wave_max(hi.y), hz = wave_max(hi.z);
    float n = lo.w; // at most 64 x 64: exact
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if (lane == 0u) {
        float4* const out = reinterpret_cast<float4*>(boxes + ((size_t)nchunks + group) * kBoxFloats);
        out[0] = make_float4(lx, ly, lz, n);
        out[1] = make_float4(hx, hy, hz, 0.f);
    }
}

// one lane's cull of box `index` of `boxes` against the wave's own box: true when the box holds a valid pose and its gap
// squared is not above step2
__device__ __forceinline__ bool box_near(const float* own, const float* __restrict__ boxes, size_t index, float step2) {
    const float4* const bp = reinterpret_cast<const float4*>(boxes + index * kBoxFloats);
    const float4 lo = bp[0], hi = bp[1];
    const float other[kBoxFloats] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return lo.w != 0.f && !(lrm_edges_box_gap2(own, other) > step2);
}

template <bool kFill>
__global__ __launch_bounds__(kBlock) void edges_walk_kernel(const LrmEdgesArgs A, const float* __restrict__ boxes, int32_t* __restrict__ count_out,
                                                            const int64_t* __restrict__ offsets, int64_t capacity, int32_t* __restrict__ edge_a_out,
                                                            int32_t* __restrict__ edge_b_out, float* __restrict__ d2_out, float* __restrict__ cos2_out,
                                                            int32_t* __restrict__ written_out) {
    __shared__ float4 s_pose[kWaves][2][kChunk]; // per wave: {x, y, z, n} and the quaternion of the 64 candidates
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t nchunks = (A.nposes + (uint32_t)(kChunk - 1)) / (uint32_t)kChunk;
    const uint32_t ca = blockIdx.x * (uint32_t)kWaves + wave; // wave-uniform
    if (ca >= nchunks) return;                                // no workgroup barrier below
    const uint32_t p = ca * (uint32_t)kChunk + lane;
    float me[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bool valid = p < A.nposes && lrm_edges_pose(A.quats, A.body, A.pose_live, p, me);
    int64_t base = 0, room = 0;
    if (kFill && p < A.nposes) room = lrm_edges_room(offsets, p, capacity, &base);
    float4(*const slice)[kChunk] = s_pose[wave];
    const float* const box_a = boxes + (size_t)ca * kBoxFloats;
    float own[kBoxFloats];
#pragma unroll
    for (int i = 0; i < kBoxFloats; i++) own[i] = box_a[i];
    uint32_t n = 0; // neighbours so far: < nposes
    if (own[3] != 0.f) { // the chunk has a valid pose (wave-uniform)
        const uint32_t ngroups = (nchunks + (uint32_t)(LRM_EDGES_ROUND - 1)) / (uint32_t)LRM_EDGES_ROUND;
        const uint32_t ga = ca / (uint32_t)LRM_EDGES_ROUND; // the wave's own group
        for (uint32_t g0 = A.form ? 0u : (ga & ~(uint32_t)(LRM_EDGES_ROUND - 1)); g0 < ngroups; g0 += LRM_EDGES_ROUND) {
            const uint32_t gb = g0 + lane;
            unsigned long long gm = __ballot(gb < ngroups && (A.form || gb >= ga) && box_near(own, boxes, (size_t)nchunks + gb, A.step2));
            while (gm != 0ull) {
                const uint32_t r0 = (g0 + (uint32_t)(__ffsll((long long)gm) - 1)) * (uint32_t)LRM_EDGES_ROUND; // wave-uniform: the group's first chunk
                gm &= gm - 1ull;
                const uint32_t cb = r0 + lane;
                const bool near = cb < nchunks && (A.form || cb >= ca) && box_near(own, boxes, cb, A.step2);
                unsigned long long m = __ballot(near);
                while (m != 0ull) {
                    const uint32_t cq = r0 + (uint32_t)(__ffsll((long long)m) - 1); // wave-uniform, < nchunks
                    m &= m - 1ull;
                    const uint32_t q0 = cq * (uint32_t)kChunk;
                    float cand[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    const bool cv = q0 + lane < A.nposes && lrm_edges_pose(A.quats, A.body, A.pose_live, q0 + lane, cand);
                    lrm_wave_lds_fence(); // the reads of the chunk before are done
                    slice[0][lane] = make_float4(cv ? cand[0] : __builtin_nanf(""), cand[1], cand[2], cand[3]);
                    slice[1][lane] = make_float4(cand[4], cand[5], cand[6], cand[7]);
                    lrm_wave_lds_fence();
                    // the candidates lane p may pair with: all of another chunk; of its own, q > p (form 0) or q != p (form 1)
                    unsigned long long allow = ~0ull;
                    if (cq == ca) allow = A.form ? ~(1ull << lane) : (lane == 63u ? 0ull : ~0ull << (lane + 1u));
                    if (!valid) allow = 0ull;
    #pragma unroll 8
                    for (uint32_t k = 0; k < (uint32_t)kChunk; k++) {
                        const float4 b = slice[0][k]; // one address for the wave: a broadcast
                        const float d2 = lrm_edges_d2(me[0], me[1], me[2], b.x, b.y, b.z);
                        if (d2 <= A.step2 && ((allow >> k) & 1ull) != 0ull) {
                            const float4 qq = slice[1][k];
                            const float qv[4] = {qq.x, qq.y, qq.z, qq.w};
                            const float c = lrm_edges_dot(me + 4, qv);
                            if (lrm_edges_turn(c, me[3], b.w, A.dot2)) {
                                if (kFill && (int64_t)n < room) {
                                    const int64_t at = base + (int64_t)n; // inside [0, capacity)
                                    edge_a_out[at] = (int32_t)p;
                                    edge_b_out[at] = (int32_t)(q0 + k);
                                    if (d2_out) d2_out[at] = d2;
                                    if (cos2_out) cos2_out[at] = lrm_edges_cos2(c, me[3], b.w);
                                }
                                n++;
                            }
                        }
                    }
                }
            }
        }
    }
    if (p < A.nposes) {
        if (kFill) {
            if (written_out) written_out[p] = (int32_t)((int64_t)n < room ? (int64_t)n : room);
        } else {
            count_out[p] = (int32_t)n;
        }
    }
}

// the chunk boxes, then the group boxes behind them
void launch_boxes(const LrmEdgesArgs& A, const uint64_t plan[4], float* boxes, hipStream_t st) {
    const uint32_t nchunks = (uint32_t)lrm_edges_chunks(A.nposes), ngroups = (uint32_t)lrm_edges_supers(A.nposes);
    hipLaunchKernelGGL(edges_box_kernel, dim3((unsigned)plan[2]), dim3(kBlock), 0, st, A, boxes);
    hipLaunchKernelGGL(edges_group_box_kernel, dim3((ngroups + kWaves - 1) / kWaves), dim3(kBlock), 0, st, nchunks, boxes);
}

} // namespace

hipError_t lrm_launch_pose_edge_counts(const LrmEdgesArgs& A, float* boxes, int32_t* count_out, hipStream_t st) {
    uint64_t plan[4];
    lrm_edges_plan(A.nposes, plan);
    launch_boxes(A, plan, boxes, st);
    hipLaunchKernelGGL(edges_walk_kernel<false>, dim3((unsigned)plan[2]), dim3(kBlock), 0, st, A, (const float*)boxes, count_out,
                       (const int64_t*)nullptr, (int64_t)0, (int32_t*)nullptr, (int32_t*)nullptr, (float*)nullptr, (float*)nullptr,
                       (int32_t*)nullptr);
    return hipGetLastError();
}

hipError_t lrm_launch_pose_edges(const LrmEdgesArgs& A, float* boxes, const int64_t* offsets, int64_t capacity, int32_t* edge_a_out,
                                 int32_t* edge_b_out, float* d2_out, float* cos2_out, int32_t* written_out, hipStream_t st) {
    uint64_t plan[4];
    lrm_edges_plan(A.nposes, plan);
    launch_boxes(A, plan, boxes, st);
    hipLaunchKernelGGL(edges_walk_kernel<true>, dim3((unsigned)plan[2]), dim3(kBlock), 0, st, A, (const float*)boxes, (int32_t*)nullptr, offsets,
                       capacity, edge_a_out, edge_b_out, d2_out, cos2_out, written_out);
    return hipGetLastError();
}
