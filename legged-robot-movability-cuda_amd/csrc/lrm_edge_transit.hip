// lrm_edge_transit.hip -- gfx950 kernel of lrm_edge_transit_posed_dev: per pose transition (edge) and leg, does the planted
// foot stay reachable at S sampled poses between the two ends; per edge whether every planted foot does, and how far the
// body gets before the first one does not.  The path, the evaluation and the per-leg answer are lrm_edge_transit.h's,
// shared with the host loop; this file only spreads them over lanes.
//
// edge_transit_kernel: lane = (edge slot, sample).  A wave holds E = 64 / S edge slots of S adjacent lanes (S = 9: seven
// edges, 63 busy lanes); a workgroup is one wave; the grid is capped and strides over the rest, E edges at a time, so every
// lane of a wave takes the same number of rounds and the ballot and the shuffles below are always whole.
//   Each busy lane of a live edge forms its own sample (quaternion and body) once, then the wave loops over the legs
//   (wave-uniform; the leg's dimensions come from the kernel arguments through scalar loads).  A lane of a planted leg
//   compiles the head of (leg, q_s) -- no table is read or written -- and evaluates its target from it:
//     default: into the lane's own LDS slot.  A slot is 496 bytes: the head's 480 rounded up to an odd number of 16-byte
//       units, so that the slots keep the 16-byte alignment LrmCircle asks for and the 16-byte reads of the circles of 16
//       lanes fall into 16 different units of the 256-byte LDS row.  31 744 bytes per workgroup, five workgroups per CU.
//     -DLRM_TRANSIT_PRIVATE_HEAD: into a local (480 bytes of private memory per lane).  Timed against the default once
//       (DESIGN.md 3.22); the answers are the same.
//   mask: one ballot per leg, shifted and masked to the edge's lanes.  worst: a segmented maximum of the 64-bit key over
//   the edge's lanes in ceil(log2 S) shuffle steps.  The edge's first lane stores the leg's row, and after the last leg the
//   edge's bytes.  No atomics, no __syncthreads, no global scratch; a lane reads no LDS slot but its own.
// No output depends on the mapping.  A dead edge, an unplanted leg, a foot or an end out of range are answered before any
// address is formed from them.
//
// Compiled with -ffp-contract=off (see lrm_point.h).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "lrm_edge_transit.h"

namespace {

constexpr int kBlock = 64;
constexpr unsigned kMaxGrid = 2560; // two rounds of the 256 CUs x 5 resident workgroups; a wave strides over the rest
constexpr int kSlotBytes = 496;
static_assert(kSlotBytes >= (int)sizeof(LrmLegHead) && kSlotBytes % 16 == 0 && (kSlotBytes / 16) % 2 == 1, "LDS slot of a head");

struct TransitLegs { // the legs, by value in the kernarg segment (8 x 56 B)
    LrmLegDimensions l[LRM_MAX_LEGS];
};

__global__ __launch_bounds__(kBlock) void edge_transit_kernel(
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz, uint32_t nt,
    const float* __restrict__ quats, const float* __restrict__ body /* may be null */, uint32_t nposes, const TransitLegs legs,
    uint32_t nlegs, const int32_t* __restrict__ edge_a, const int32_t* __restrict__ edge_b, const int32_t* __restrict__ foot,
    uint32_t nedges, uint32_t S, const uint8_t* __restrict__ live_in /* may be null */, uint64_t* __restrict__ mask_out /* may be null */,
    int32_t* __restrict__ reached_out, int32_t* __restrict__ first_miss_out, int32_t* __restrict__ worst_out /* may be null */,
    float* __restrict__ worst_d2_out /* may be null */, uint8_t* __restrict__ planted_out /* may be null */,
    uint8_t* __restrict__ clear_out /* may be null */, int32_t* __restrict__ advance_out /* may be null */) {
#ifndef LRM_TRANSIT_PRIVATE_HEAD
    __shared__ __attribute__((aligned(16))) unsigned char s_heads[kBlock * kSlotBytes];
    LrmLegHead* const H = reinterpret_cast<LrmLegHead*>(s_heads + threadIdx.x * kSlotBytes);
#else
    LrmLegHead head;
    LrmLegHead* const H = &head;
#endif
    const uint32_t lane = threadIdx.x;
    const uint32_t per_wave = 64u / S;        // edge slots of a wave
    const uint32_t slot = lane / S;           // this lane's edge slot
    const uint32_t s = lane - slot * S;       // and sample
    const uint32_t first = slot * S;          // the first lane of the slot
    const bool busy = slot < per_wave;
    const uint64_t full = lrm_transit_full(S);

    for (uint64_t base = (uint64_t)blockIdx.x * per_wave; base < nedges; base += (uint64_t)gridDim.x * per_wave) { // wave-uniform
        const uint64_t e64 = base + slot;
        const bool have = busy && e64 < nedges;
        const uint32_t e = (uint32_t)e64;
        // ---- the edge and this lane's sample ----
        bool live = false;
        LrmTransitSample smp{};
        if (have) {
            const int32_t a = edge_a[e], b = edge_b[e];
            live = !(live_in && live_in[e] == 0) && a >= 0 && b >= 0 && (uint32_t)a < nposes && (uint32_t)b < nposes;
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
        uint32_t planted_bits = 0u;
        bool all_reach = true;
        int32_t advance = (int32_t)S;
        for (uint32_t l = 0; l < nlegs; l++) { // wave-uniform
            const size_t o = (size_t)l * nedges + e; // < 2^32 (checked by the C ABI)
            int32_t ft = -1;
            if (live) ft = foot[o];
            const bool planted = live && lrm_transit_foot_in_cloud(ft, nt);
            bool reach = false;
            uint64_t key = 0ull;
            if (planted) {
                const LrmVec3 p{tx[ft] - smp.body.x, ty[ft] - smp.body.y, tz[ft] - smp.body.z};
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
                const LrmTransitLeg A = planted ? lrm_transit_leg(mask, key, S) : lrm_transit_leg_unplanted();
                if (mask_out) mask_out[o] = A.mask;
                reached_out[o] = A.reached;
                first_miss_out[o] = A.first_miss;
                if (worst_out) worst_out[o] = A.worst;
                if (worst_d2_out) worst_d2_out[o] = A.worst_d2;
                if (planted) {
                    planted_bits |= 1u << l;
                    all_reach = all_reach && A.first_miss < 0;
                    if (A.first_miss >= 0 && A.first_miss < advance) advance = A.first_miss;
                }
            }
        }
        if (have && s == 0u) {
            if (planted_out) planted_out[e] = (uint8_t)planted_bits;
            if (clear_out) clear_out[e] = live && all_reach;
            if (advance_out) advance_out[e] = live ? advance : 0;
        }
    }
}

// lrm_dbg_edge_transit_samples_dev: one (edge, sample) per lane; out[(e * S + s) * 7 ..] = q_s, body_s; nan for an edge with an
// end out of range
__global__ __launch_bounds__(256) void edge_transit_samples_kernel(const float* __restrict__ quats, const float* __restrict__ body,
                                                                   uint32_t nposes, const int32_t* __restrict__ edge_a,
                                                                   const int32_t* __restrict__ edge_b, uint32_t nedges, uint32_t S,
                                                                   float* __restrict__ out) {
    const uint64_t n = (uint64_t)nedges * S;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint32_t e = (uint32_t)(i / S), s = (uint32_t)(i - (uint64_t)e * S);
        const int32_t a = edge_a[e], b = edge_b[e];
        LrmTransitSample smp;
        for (int k = 0; k < 4; k++) smp.q[k] = __builtin_nanf("");
        smp.body = LrmVec3{smp.q[0], smp.q[0], smp.q[0]};
        if (a >= 0 && b >= 0 && (uint32_t)a < nposes && (uint32_t)b < nposes) {
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
        float* o = out + i * 7;
        for (int k = 0; k < 4; k++) o[k] = smp.q[k];
        o[4] = smp.body.x;
        o[5] = smp.body.y;
        o[6] = smp.body.z;
    }
}

} // namespace

hipError_t lrm_launch_edge_transit_samples(const float* quats, const float* body, size_t nposes, const int32_t* edge_a,
                                           const int32_t* edge_b, size_t nedges, size_t nsamples, float* out, hipStream_t st) {
    size_t g = (nedges * nsamples + 255) / 256;
    if (g > kMaxGrid) g = kMaxGrid;
    hipLaunchKernelGGL(edge_transit_samples_kernel, dim3((unsigned)g), dim3(256), 0, st, quats, body, (uint32_t)nposes, edge_a, edge_b,
                       (uint32_t)nedges, (uint32_t)nsamples, out);
    return hipGetLastError();
}

hipError_t lrm_launch_edge_transit_posed(const float* tx, const float* ty, const float* tz, size_t nt, const float* quats,
                                         const float* body, size_t nposes, const LrmLegDimensions* legs, size_t nlegs,
                                         const int32_t* edge_a, const int32_t* edge_b, size_t nedges, const int32_t* foot,
                                         size_t nsamples, const uint8_t* live_in, uint64_t* mask_out, int32_t* reached_out,
                                         int32_t* first_miss_out, int32_t* worst_out, float* worst_d2_out, uint8_t* planted_out,
                                         uint8_t* clear_out, int32_t* advance_out, hipStream_t st) {
    TransitLegs L{};
    for (size_t k = 0; k < nlegs; k++) L.l[k] = legs[k];
    const size_t per_wave = 64 / nsamples;
    size_t g = (nedges + per_wave - 1) / per_wave;
    if (g > kMaxGrid) g = kMaxGrid;
    hipLaunchKernelGGL(edge_transit_kernel, dim3((unsigned)g), dim3(kBlock), 0, st, tx, ty, tz, (uint32_t)nt, quats, body,
                       (uint32_t)nposes, L, (uint32_t)nlegs, edge_a, edge_b, foot, (uint32_t)nedges, (uint32_t)nsamples, live_in,
                       mask_out, reached_out, first_miss_out, worst_out, worst_d2_out, planted_out, clear_out, advance_out);
    return hipGetLastError();
}
