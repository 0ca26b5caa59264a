// lrm_stance_loads.hip -- gfx950 kernel of lrm_stance_loads_posed_dev: per set (a pose and three joint angles per leg) and
// per lift set, the share of the robot's weight every planted foot carries and the moment of that force about the coxa,
// femur and tibia joints.  The arithmetic is lrm_stance_loads.h's, shared with the host loop; this file only spreads it
// over a wave, on stance_stability_kernel's scheme (lrm_stance.hip).
//
// stance_loads_posed_kernel: a wave owns one set and strides over the rest under a capped grid.  It reads no cloud and no
// body position: the feet are the FK tips relative to the body.
//   phase 1, lane = leg: lanes 0 .. nlegs - 1 read their own two table entries and three angles and run lrm_loads_leg: the
//     three sincos, the joints, the plane point minus the centre of mass and the three lever arms.  A ballot gives the valid
//     legs; the five floats of each of the eight legs are then read out of their lane into scalars (v_readlane), so that
//     every lane holds all forty without a register of its own.
//     Then lane = triple code (56 of the 64 lanes): the barycentric loads of the tripod stage do not depend on the lift set,
//     so each triple i < j < k is computed ONCE per set by its own lane from the feet it takes by __shfl (five registers).
//   phase 2, lane = lift set (a second round from 64 sets on): the lane forms its planted set S and runs the minimum-norm
//     solve and the drop loop of at most five more solves (lrm_loads_min_norm_stages).  Only if some lane of the wave needs
//     the tripod stage -- a rarely taken, wave-uniform branch -- every lane walks the 56 codes: the triple's bits and minimum
//     come from lane `code` into scalars, a triple that does not count is skipped by a scalar branch, the others cost an and,
//     two compares and a select; the winner's three loads come by one __shfl each.  Codes rise, so a strict comparison keeps
//     the first triple on ties.  Then lrm_loads_answer, and the lane stores its own row.  Every loop over legs is unrolled
//     with constant indices: load[8] and tau[8][3] stay in registers.
//     (Unrolling the 56 triples inside the lane instead makes the compiler hoist all of them out of the lift-set loop, as they
//     are wave-uniform: 256 VGPRs + 66 AGPRs and one wave per SIMD.  This form: 126 VGPRs, four waves.)
// The pose, the quaternion and the centre of mass are wave-uniform.  No LDS, no atomics, no __syncthreads, one writer per
// output.  A dead set (live_in 0, pose out of range, centre of mass not finite) reads no table and no angle and stores
// status 0 with the empty answer.
//
// The lift sets, the centre of mass, the plane, `up` and tau_max sit in the kernel's arguments (LrmLoadsParams, 328 bytes).
//
// Compiled with -ffp-contract=off (see lrm_point.h).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "lrm_types.h"
#include "lrm_compile_head.h"
#include "lrm_point.h"
#include "lrm_ik.h"
#include "lrm_stance_loads.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr unsigned kMaxGrid = 16384; // 65 536 sets in flight; a wave strides over the rest
#ifndef LRM_LOADS_LANE_MAX_MASKS      // `make variant FLAGS=-DLRM_LOADS_LANE_MAX_MASKS=n` moves the switch (0: never) for timing
#define LRM_LOADS_LANE_MAX_MASKS 8
#endif
constexpr uint32_t kLaneMaxMasks = LRM_LOADS_LANE_MAX_MASKS; // up to here a lane owns a set (stance_loads_lane_kernel)
constexpr unsigned kLaneMaxGrid = 1024; // 262 144 sets in flight; a lane strides over the rest

__device__ __forceinline__ float read_lane(float v, int l) { return lrm_u2f((uint32_t)__builtin_amdgcn_readlane((int)lrm_f2u(v), l)); }

__global__ __launch_bounds__(kBlock) void stance_loads_posed_kernel(
    const LrmPoseRecord* __restrict__ recs, const LrmIkLeg* __restrict__ iks, const float* __restrict__ quats, uint32_t nposes,
    uint32_t nlegs, const int32_t* __restrict__ pose_idx /* may be null */, uint32_t nsets, const float* __restrict__ coxa,
    const float* __restrict__ femur, const float* __restrict__ tibia, const LrmLoadsParams P,
    const uint8_t* __restrict__ live_in /* may be null */, uint8_t* __restrict__ status_out, uint8_t* __restrict__ holdable_out,
    float* __restrict__ peak_out, uint8_t* __restrict__ peak_at_out /* may be null */, float* __restrict__ load_out /* may be null */,
    float* __restrict__ tau_out /* may be null */) {
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nmasks = P.S.nmasks;
    // this lane's triple (phase 1; the codes do not depend on the set)
    const uint32_t t_bits = lrm_loads_triple_of(lane < LRM_LOADS_TRIPLES ? lane : 0u);
    const uint32_t t_feet = lrm_loads_triple_feet(t_bits);
    const int ti = (int)((t_bits >> 8) & 7u), tj = (int)((t_bits >> 11) & 7u), tk = (int)((t_bits >> 14) & 7u);

    for (uint32_t s = blockIdx.x * kWaves + wave; s < nsets; s += gridDim.x * kWaves) { // wave-uniform
        // ---- the set: pose and centre of mass ----
        const int32_t p = pose_idx ? pose_idx[s] : (int32_t)s;
        bool live = !(live_in && live_in[s] == 0) && p >= 0 && (uint32_t)p < nposes;
        LrmStancePt c{0.f, 0.f};
        if (live) {
            const float* q4 = quats + (size_t)p * 4;
            const float quat[4] = {q4[0], q4[1], q4[2], q4[3]};
            bool ok;
            c = lrm_stance_com(P.S, quat, &ok);
            live = ok;
        }

        // ---- phase 1: lane = leg ----
        LrmLoadsLeg A{0.f, 0.f, {0.f, 0.f, 0.f}};
        bool valid = false;
        if (live && lane < nlegs) {
            const size_t rec = (size_t)p * nlegs + lane;
            const size_t o = (size_t)lane * nsets + s;
            valid = lrm_loads_leg(P, recs[rec].head, iks[rec], c, coxa[o], femur[o], tibia[o], &A);
        }
        const uint32_t feet = (uint32_t)__ballot(valid) & 0xffu; // wave-uniform
        // lane = triple code: the triple's barycentric loads, once per set
        const bool t_live = (feet & t_feet) == t_feet && lane < LRM_LOADS_TRIPLES;
        const LrmLoadsTriple T = lrm_loads_triple(__shfl(A.xi, ti), __shfl(A.eta, ti), __shfl(A.xi, tj), __shfl(A.eta, tj), __shfl(A.xi, tk),
                                                  __shfl(A.eta, tk));
        const uint32_t t_ok = (t_live && T.ok) ? 1u : 0u;
        float xi[8], eta[8], g[8][3];
#pragma unroll
        for (int l = 0; l < 8; l++) {
            xi[l] = read_lane(A.xi, l);
            eta[l] = read_lane(A.eta, l);
            g[l][0] = read_lane(A.g[0], l);
            g[l][1] = read_lane(A.g[1], l);
            g[l][2] = read_lane(A.g[2], l);
        }

        // ---- phase 2: lane = lift set ----
        for (uint32_t m0 = 0; m0 < nmasks; m0 += 64) { // wave-uniform: every lane stays in, so that every lane can be read
            const uint32_t m = m0 + lane;
            const uint32_t S = lrm_stance_planted(feet, m < nmasks ? P.S.lift[m] : 0xffu);
            float load[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            uint8_t st = live ? lrm_loads_min_norm_stages(xi, eta, S, load) : (uint8_t)LRM_LOADS_DEAD;
            if (__any(st == LRM_LOADS_TRIPOD)) { // wave-uniform and rare: the tripod stage chooses among the triples of phase 1
                float best = -1.f;
                int at = -1;
                for (int code = 0; code < LRM_LOADS_TRIPLES; code++) {
                    if (!__builtin_amdgcn_readlane((int)t_ok, code)) continue; // scalars
                    const uint32_t tb = (uint32_t)__builtin_amdgcn_readlane((int)t_bits, code);
                    lrm_loads_triple_offer(tb, true, read_lane(T.mn, code), code, S, &best, &at);
                }
                const int src = at < 0 ? 0 : at;
                const uint32_t tb = (uint32_t)__shfl((int)t_bits, src);
                const float li = __shfl(T.li, src), lj = __shfl(T.lj, src), lk = __shfl(T.lk, src);
                if (st == LRM_LOADS_TRIPOD) {
                    if (at < 0) {
                        lrm_loads_none(S, load);
                        st = LRM_LOADS_NONE;
                    } else {
                        lrm_loads_triple_put(tb, li, lj, lk, load);
                    }
                }
            }
            if (m >= nmasks) continue; // no lane is read below
            float load_o[8], tau_o[8][3];
            const LrmLoadsPeak Q = lrm_loads_answer(P.tau_max, S, st, load, g, load_o, tau_o);
            const size_t o = (size_t)m * nsets + s; // < 2^32 (checked by the C ABI, as are the two below)
            status_out[o] = st;
            holdable_out[o] = Q.holdable;
            peak_out[o] = Q.peak;
            if (peak_at_out) peak_at_out[o] = Q.at;
#pragma unroll
            for (int l = 0; l < 8; l++) {
                if ((uint32_t)l >= nlegs) break; // wave-uniform
                const size_t ol = ((size_t)m * nlegs + (size_t)l) * nsets + s;
                if (load_out) load_out[ol] = load_o[l];
                if (tau_out) {
                    const size_t ot = (((size_t)m * nlegs + (size_t)l) * 3) * nsets + s;
                    tau_out[ot] = tau_o[l][0];
                    tau_out[ot + nsets] = tau_o[l][1];
                    tau_out[ot + 2 * (size_t)nsets] = tau_o[l][2];
                }
            }
        }
    }
}

// stance_loads_lane_kernel: the second mapping, for calls with at most kLaneMaxMasks lift sets: a LANE owns a set, walks its
// legs (unrolled: the arrays stay in registers) and then its lift sets with the host loop's own lrm_loads_solve.  With few
// lift sets the wave-per-set kernel keeps few lanes of 64 busy in phase 2 and pays a wave's trip per set: measured on config 3
//  0.325 / 0.350 ms with 1 / 7 lift sets against this kernel's 0.058 / 0.168 ms; with 64 lift sets this kernel
// takes 0.72 ms against 0.34 ms when loads and torques are not stored.  Adjacent lanes store adjacent sets: coalesced.
// Same functions, same bits.
__global__ __launch_bounds__(kBlock) void stance_loads_lane_kernel(
    const LrmPoseRecord* __restrict__ recs, const LrmIkLeg* __restrict__ iks, const float* __restrict__ quats, uint32_t nposes,
    uint32_t nlegs, const int32_t* __restrict__ pose_idx, uint32_t nsets, const float* __restrict__ coxa, const float* __restrict__ femur,
    const float* __restrict__ tibia, const LrmLoadsParams P, const uint8_t* __restrict__ live_in, uint8_t* __restrict__ status_out,
    uint8_t* __restrict__ holdable_out, float* __restrict__ peak_out, uint8_t* __restrict__ peak_at_out, float* __restrict__ load_out,
    float* __restrict__ tau_out) {
    for (uint32_t s = blockIdx.x * kBlock + threadIdx.x; s < nsets; s += gridDim.x * kBlock) {
        const int32_t p = pose_idx ? pose_idx[s] : (int32_t)s;
        bool live = !(live_in && live_in[s] == 0) && p >= 0 && (uint32_t)p < nposes;
        LrmStancePt c{0.f, 0.f};
        if (live) {
            const float* q4 = quats + (size_t)p * 4;
            const float quat[4] = {q4[0], q4[1], q4[2], q4[3]};
            bool ok;
            c = lrm_stance_com(P.S, quat, &ok);
            live = ok;
        }
        float xi[8], eta[8], g[8][3];
        uint32_t feet = 0u;
#pragma unroll
        for (int l = 0; l < 8; l++) {
            LrmLoadsLeg A{0.f, 0.f, {0.f, 0.f, 0.f}};
            if (live && (uint32_t)l < nlegs) {
                const size_t rec = (size_t)p * nlegs + l;
                const size_t o = (size_t)l * nsets + s;
                if (lrm_loads_leg(P, recs[rec].head, iks[rec], c, coxa[o], femur[o], tibia[o], &A))
                    feet |= 1u << l;
            }
            xi[l] = A.xi, eta[l] = A.eta, g[l][0] = A.g[0], g[l][1] = A.g[1], g[l][2] = A.g[2];
        }
        for (uint32_t m = 0; m < P.S.nmasks; m++) {
            const uint32_t S = lrm_stance_planted(feet, P.S.lift[m]);
            float load[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const uint8_t st = live ? lrm_loads_solve(xi, eta, S, load) : (uint8_t)LRM_LOADS_DEAD;
            float load_o[8], tau_o[8][3];
            const LrmLoadsPeak Q = lrm_loads_answer(P.tau_max, S, st, load, g, load_o, tau_o);
            const size_t o = (size_t)m * nsets + s;
            status_out[o] = st;
            holdable_out[o] = Q.holdable;
            peak_out[o] = Q.peak;
            if (peak_at_out) peak_at_out[o] = Q.at;
#pragma unroll
            for (int l = 0; l < 8; l++) {
                if ((uint32_t)l >= nlegs) break;
                const size_t ol = ((size_t)m * nlegs + (size_t)l) * nsets + s;
                if (load_out) load_out[ol] = load_o[l];
                if (tau_out) {
                    const size_t ot = (((size_t)m * nlegs + (size_t)l) * 3) * nsets + s;
                    tau_out[ot] = tau_o[l][0];
                    tau_out[ot + nsets] = tau_o[l][1];
                    tau_out[ot + 2 * (size_t)nsets] = tau_o[l][2];
                }
            }
        }
    }
}

} // namespace

hipError_t lrm_launch_stance_loads_posed(const void* records, const void* ik_records, const float* quats, size_t nposes, size_t nlegs,
                                         const int32_t* pose_idx, size_t nsets, const float* coxa, const float* femur,
                                         const float* tibia, const LrmLoadsParams& P, const uint8_t* live_in, uint8_t* status_out,
                                         uint8_t* holdable_out, float* peak_out, uint8_t* peak_at_out, float* load_out, float* tau_out,
                                         hipStream_t st) {
    if (P.S.nmasks <= kLaneMaxMasks) {
        size_t gl = (nsets + kBlock - 1) / kBlock;
        if (gl > kLaneMaxGrid) gl = kLaneMaxGrid;
        hipLaunchKernelGGL(stance_loads_lane_kernel, dim3((unsigned)gl), dim3(kBlock), 0, st, (const LrmPoseRecord*)records,
                           (const LrmIkLeg*)ik_records, quats, (uint32_t)nposes, (uint32_t)nlegs, pose_idx, (uint32_t)nsets, coxa, femur, tibia,
                           P, live_in, status_out, holdable_out, peak_out, peak_at_out, load_out, tau_out);
        return hipGetLastError();
    }
    size_t g = (nsets + kWaves - 1) / kWaves;
    if (g > kMaxGrid) g = kMaxGrid;
    hipLaunchKernelGGL(stance_loads_posed_kernel, dim3((unsigned)g), dim3(kBlock), 0, st, (const LrmPoseRecord*)records,
                       (const LrmIkLeg*)ik_records, quats, (uint32_t)nposes, (uint32_t)nlegs, pose_idx, (uint32_t)nsets, coxa, femur, tibia,
                       P, live_in, status_out, holdable_out, peak_out, peak_at_out, load_out, tau_out);
    return hipGetLastError();
}
