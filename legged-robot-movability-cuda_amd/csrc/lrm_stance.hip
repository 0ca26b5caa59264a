// lrm_stance.hip -- gfx950 kernel of lrm_stance_stability_dev: per stance (a pose and one chosen foothold per leg) and
// per lift set, the distance of the centre of mass from the nearest edge of the support polygon of the planted feet.
// The arithmetic is lrm_stance.h's, shared with the host loop; this file only spreads it over a wave.
//
// stance_stability_kernel: a wave owns one stance and strides over the rest under a capped grid.  It never walks the
// cloud: it reads one target per leg.
//   phase 1, lane = code i*8 + j: lanes 0..7 load the foot of leg `lane` (index, target, minus the body, validity, plane
//     point); every lane then takes f_i and f_j by __shfl, loops over the eight feet (lane index wave-uniform) for left_ij,
//     forms s_ij and keeps two registers: the packed pair bits and the key's high word.  The diagonal lanes idle.
//   phase 2, lane = lift set (a second round from 64 sets on): the lane forms its planted set S and loops over the 64
//     codes; the pair's two registers come from lane `code` (wave-uniform: a read of one lane into scalars), a pair that
//     takes no part is skipped by a scalar branch, the others cost an and, two compares and a 64-bit minimum.  Codes rise, so
//     a strict comparison keeps the smaller code on ties.  The lane then stores its own margin, edge and stable byte.
// The pose, the quaternion, the body and the centre of mass are wave-uniform.  No LDS, no atomics, no __syncthreads.
// A dead stance (live_in 0, pose out of range, centre of mass not finite) has no valid foot: phase 2 then answers
// -inf / 255 / 0 by the fewer-than-three rule, and nothing of the cloud or the foot array is read.
//
// The lift sets, the centre of mass and the plane sit in the kernel's arguments (LrmStanceParams, 304 bytes): the lane's own
// lift byte is a vector load from the argument segment.
//
// Compiled with -ffp-contract=off (see lrm_point.h).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "lrm_stance.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr unsigned kMaxGrid = 16384; // 65 536 stances in flight; a wave strides over the rest

__global__ __launch_bounds__(kBlock) void stance_stability_kernel(
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz, size_t nt,
    const float* __restrict__ quats, const float* __restrict__ body /* may be null */, uint32_t nposes,
    const int32_t* __restrict__ pose_idx /* may be null */, const int32_t* __restrict__ foot, uint32_t nstances, uint32_t nlegs,
    const LrmStanceParams P, const uint8_t* __restrict__ live_in /* may be null */, float* __restrict__ margin_out,
    uint8_t* __restrict__ edge_out /* may be null */, uint8_t* __restrict__ stable_out, uint8_t* __restrict__ feet_out /* may be null */) {
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int pi = lane >> 3, pj = lane & 7;

    for (uint32_t s = blockIdx.x * kWaves + wave; s < nstances; s += gridDim.x * kWaves) { // wave-uniform
        // ---- the stance: pose, body, centre of mass ----
        const int32_t p = pose_idx ? pose_idx[s] : (int32_t)s;
        bool live = !(live_in && live_in[s] == 0) && p >= 0 && (uint32_t)p < nposes;
        LrmVec3 b{0.f, 0.f, 0.f};
        LrmStancePt c{0.f, 0.f};
        if (live) {
            const float* q4 = quats + (size_t)p * 4;
            const float quat[4] = {q4[0], q4[1], q4[2], q4[3]};
            bool ok;
            c = lrm_stance_com(P, quat, &ok);
            live = ok;
            if (body) b = LrmVec3{body[(size_t)p * 3], body[(size_t)p * 3 + 1], body[(size_t)p * 3 + 2]};
        }

        // ---- phase 1: lanes 0..nlegs-1 load their foot ----
        LrmStancePt f{0.f, 0.f};
        bool valid = false;
        if (live && lane < (int)nlegs) {
            const int32_t ft = foot[(size_t)lane * nstances + s];
            if (lrm_stance_foot_in_cloud(ft, nt)) {
                const LrmVec3 q{tx[ft] - b.x, ty[ft] - b.y, tz[ft] - b.z};
                valid = lrm_stance_foot_valid(q);
                if (valid) f = lrm_stance_project(P, q);
            }
        }
        const uint32_t feet = (uint32_t)__ballot(valid) & 0xffu; // wave-uniform
        // lane = code: the pair (pi, pj)
        const LrmStancePt fi{__shfl(f.x, pi), __shfl(f.y, pi)};
        const LrmStancePt fj{__shfl(f.x, pj), __shfl(f.y, pj)};
        const LrmStanceEdge E = lrm_stance_edge(fi, fj);
        uint32_t left = 0u;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const LrmStancePt fk{__shfl(f.x, k), __shfl(f.y, k)};
            if (((feet >> k) & 1u) && lrm_stance_left(E, fk)) left |= 1u << k;
        }
        const bool on = pi != pj && ((feet >> pi) & 1u) && ((feet >> pj) & 1u) && lrm_stance_edge_usable(E);
        const uint32_t pair = lrm_stance_pair_bits(left, pi, pj, on);
        const uint32_t word = lrm_stance_word(lrm_stance_signed(E, c));

        // ---- phase 2: lane = lift set ----
        for (uint32_t m0 = 0; m0 < P.nmasks; m0 += 64) { // wave-uniform: every lane stays in, so that every lane can be read
            const uint32_t m = m0 + lane;
            const uint32_t S = lrm_stance_planted(feet, m < P.nmasks ? P.lift[m] : 0xffu);
            uint64_t key = kLrmStanceNone;
            for (int code = 0; code < 64; code++) {
                const uint32_t pc = __builtin_amdgcn_readlane(pair, code); // scalars
                if (!(pc & LRM_STANCE_PAIR_ON)) continue;
                const uint32_t wc = __builtin_amdgcn_readlane(word, code);
                const uint64_t kc = lrm_stance_key(wc, (uint32_t)code);
                if (lrm_stance_pair_counts(pc, S) && kc < key) key = kc;
            }
            if (!lrm_stance_stands(S)) key = kLrmStanceNone;
            if (m < P.nmasks) {
                const LrmStanceAnswer A = lrm_stance_key_decode(key);
#ifdef LRM_STANCE_PROBE_COALESCED // timing probe only: a stance-major layout whose stores leave a wave coalesced
                const size_t o = (size_t)s * P.nmasks + m;
#else
                const size_t o = (size_t)m * nstances + s; // < 2^32 (checked by the C ABI)
#endif
                margin_out[o] = A.margin;
                if (edge_out) edge_out[o] = A.edge;
                stable_out[o] = lrm_stance_stable(A.margin, P.min_margin);
            }
        }
        if (feet_out && lane == 0) feet_out[s] = (uint8_t)feet;
    }
}

} // namespace

hipError_t lrm_launch_stance_stability(const float* tx, const float* ty, const float* tz, size_t nt, const float* quats,
                                       const float* body, size_t nposes, const int32_t* pose_idx, const int32_t* foot, size_t nstances,
                                       size_t nlegs, const LrmStanceParams& P, const uint8_t* live_in, float* margin_out,
                                       uint8_t* edge_out, uint8_t* stable_out, uint8_t* feet_out, hipStream_t st) {
    size_t g = (nstances + kWaves - 1) / kWaves;
    if (g > kMaxGrid) g = kMaxGrid;
    hipLaunchKernelGGL(stance_stability_kernel, dim3((unsigned)g), dim3(kBlock), 0, st, tx, ty, tz, nt, quats, body, (uint32_t)nposes,
                       pose_idx, foot, (uint32_t)nstances, (uint32_t)nlegs, P, live_in, margin_out, edge_out, stable_out, feet_out);
    return hipGetLastError();
}
