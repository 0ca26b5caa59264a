// lrm_stance_loads.h -- the arithmetic of lrm_stance_loads_posed_dev / _cpu (include/lrm.h): what does every planted foot
// of a stance carry, and what must the coxa, femur and tibia joints hold, for every set of lifted legs.  Frictionless point
// contacts that push along `up`, massless legs, weight 1.  One source for the kernel (lrm_stance_loads.hip) and the host
// loop (lrm_capi.cpp): float32 only, no contraction, only + - * /, comparisons, lrm_sincosf and lrm_sqrtf (the last two
// inside lrm_leg_joints), so that both give the same bits.  The joints are lrm_leg_clearance.h's and the plane and the centre
// of mass lrm_stance.h's, which this header includes and leaves alone; everything that decides an output is here, the kernel
// only spreads it over lanes.  Every loop over legs has a constant trip count and constant indices once unrolled: the
// kernel keeps the arrays in registers (no scratch).
#pragma once
#include <stdint.h>
#include "lrm_leg_clearance.h"
#include "lrm_stance.h"

// What travels from the host in the kernel's arguments: lrm_stance.h's parameters (centre of mass, plane, lift sets;
// min_margin is not read), the direction the feet push along and the torque limits.  All checked by the C ABI.
struct LrmLoadsParams {
    LrmStanceParams S;
    float up[3];
    float tau_max[3];
};

// up = u x v, formed once per call; (0, 0, 1) without a plane
LRM_HD void lrm_loads_up(const LrmStanceParams& S, float up[3]) {
    if (!S.on) {
        up[0] = 0.f, up[1] = 0.f, up[2] = 1.f;
        return;
    }
    up[0] = S.u[1] * S.v[2] - S.u[2] * S.v[1];
    up[1] = S.u[2] * S.v[0] - S.u[0] * S.v[2];
    up[2] = S.u[0] * S.v[1] - S.u[1] * S.v[0];
}

LRM_HD float lrm_loads_abs(float x) { return lrm_u2f(lrm_f2u(x) & 0x7fffffffu); }
LRM_HD float lrm_loads_nan() { return lrm_u2f(0x7fc00000u); }
// what is stored of a load or a torque: -0 turned into +0, any nan the canonical quiet nan (sign and payload of a propagated
// nan are not the same on host and device)
LRM_HD float lrm_loads_out(float x) { return x != x ? lrm_loads_nan() : x + 0.f; }

// The linear part of lrm_ik_from_coxa: a DIRECTION of the coxa frame in the caller's frame (no `u.x += L.body`).
LRM_HD LrmVec3 lrm_loads_lin(const LrmLegHead& L, const LrmIkLeg& K, LrmVec3 u) {
    const float buffer = u.x * L.sin_pitch_rev;
    u.x = u.x * L.cos_pitch_rev - u.z * L.sin_pitch_rev;
    u.z = buffer + u.z * L.cos_pitch_rev;
    const float b2 = u.x * -L.sin_body;
    u.x = u.x * L.cos_body - u.y * -L.sin_body;
    u.y = b2 + u.y * L.cos_body;
    const float* m = K.back;
    return LrmVec3{m[0] * u.x + m[1] * u.y + m[2] * u.z, m[3] * u.x + m[4] * u.y + m[5] * u.z,
                   m[6] * u.x + m[7] * u.y + m[8] * u.z};
}

// What phase 1 keeps of a leg: its plane point minus the centre of mass and the three lever arms g_j = up . Lin(col_j), the
// rise of the foot along `up` per radian of joint j (0 coxa, 1 femur, 2 tibia).
struct LrmLoadsLeg {
    float xi, eta;
    float g[3];
};
LRM_HD float lrm_loads_dot_up(const float up[3], LrmVec3 a) { return (up[0] * a.x + up[1] * a.y) + up[2] * a.z; }
// The columns of the tip's Jacobian in the coxa frame, with lrm_leg_joints' sincos arguments and its T (tip_clear == 0).
LRM_HD void lrm_loads_levers(const LrmLegHead& L, const LrmIkLeg& K, const float up[3], float c, float f, float t, float g[3]) {
    float sc, cc, sf, cf, sa, ca;
    lrm_sincosf(c, &sc, &cc);
    lrm_sincosf(f, &sf, &cf);
    lrm_sincosf(f + t, &sa, &ca);
    const float T = !(K.T > 0.f) ? 0.f : K.T;
    const float ts = T * sa, tc = T * ca;
    const float v = K.F * sf + ts, w = K.F * cf + tc, h3 = K.C + w;
    g[0] = lrm_loads_dot_up(up, lrm_loads_lin(L, K, LrmVec3{-sc * h3, cc * h3, 0.f}));
    g[1] = lrm_loads_dot_up(up, lrm_loads_lin(L, K, LrmVec3{-cc * v, -sc * v, w}));
    g[2] = lrm_loads_dot_up(up, lrm_loads_lin(L, K, LrmVec3{-cc * ts, -sc * ts, tc}));
}
// Leg l of a live set with centre of mass c: false = the leg is not valid (nothing of *A is then read)
LRM_HD bool lrm_loads_leg(const LrmLoadsParams& P, const LrmLegHead& L, const LrmIkLeg& K, LrmStancePt c, float coxa, float femur,
                          float tibia, LrmLoadsLeg* A) {
    LrmVec3 J[4];
    lrm_leg_joints(L, K, coxa, femur, tibia, 0.f, J);
    const LrmStancePt f = lrm_stance_project(P.S, J[3]);
    A->xi = f.x - c.x;
    A->eta = f.y - c.y;
    lrm_loads_levers(L, K, P.up, coxa, femur, tibia, A->g);
    return lrm_leg_joints_finite(J);
}

// ---- the loads of one planted set ----
// Stage ALL / DROPPED: the minimum-norm loads of the feet in A (a bit per leg), load_i = (alpha + beta xi_i) + gamma eta_i.
// Returns det > 0 and finite; *neg = some load of A is not >= 0 (a nan counts).  Feet outside A get +0.
LRM_HD bool lrm_loads_min_norm(const float xi[8], const float eta[8], uint32_t A, float load[8], bool* neg) {
    float n = 0.f, sx = 0.f, sy = 0.f, sxx = 0.f, sxy = 0.f, syy = 0.f;
#pragma unroll
    for (int i = 0; i < 8; i++)
        if ((A >> i) & 1u) {
            n = n + 1.f;
            sx = sx + xi[i];
            sy = sy + eta[i];
            sxx = sxx + xi[i] * xi[i];
            sxy = sxy + xi[i] * eta[i];
            syy = syy + eta[i] * eta[i];
        }
    const float c00 = sxx * syy - sxy * sxy, c01 = sxy * sy - sx * syy, c02 = sx * sxy - sxx * sy;
    const float det = (n * c00 + sx * c01) + sy * c02;
    *neg = true;
    if (!(det > 0.f && det < __builtin_inff())) return false; // load[] is then not read
    const float alpha = c00 / det, beta = c01 / det, gamma = c02 / det;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const bool in = (A >> i) & 1u;
        const float w = (alpha + beta * xi[i]) + gamma * eta[i];
        load[i] = in ? w : 0.f;
        bad = bad || (in && !(w >= 0.f));
    }
    *neg = bad;
    return true;
}
// the foot of A with the smallest load: the first foot of A, replaced by a later one only when that is strictly smaller
LRM_HD uint32_t lrm_loads_smallest(const float load[8], uint32_t A) {
    uint32_t at = 8u;
    float best = 0.f;
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (((A >> i) & 1u) && (at == 8u || load[i] < best)) {
            at = (uint32_t)i;
            best = load[i];
        }
    return at;
}
// Stages ALL and DROPPED on the planted set S -> LRM_LOADS_ALL or _DROPPED with load[] as computed (the caller stores
// lrm_loads_out of it); LRM_LOADS_NONE for fewer than three feet (load[] then filled by lrm_loads_none); LRM_LOADS_TRIPOD = the
// tripod stage has to decide (load[] is not to be read).
LRM_HD void lrm_loads_none(uint32_t S, float load[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) load[i] = ((S >> i) & 1u) ? lrm_loads_nan() : 0.f;
}
LRM_HD uint8_t lrm_loads_min_norm_stages(const float xi[8], const float eta[8], uint32_t S, float load[8]) {
    if (__builtin_popcount(S) < 3) {
        lrm_loads_none(S, load);
        return LRM_LOADS_NONE;
    }
    uint32_t A = S;
    uint8_t st = LRM_LOADS_ALL;
    for (;;) { // at most six solves: eight feet down to three
        bool neg;
        if (!lrm_loads_min_norm(xi, eta, A, load, &neg)) break;
        if (!neg) return st;
        if (__builtin_popcount(A) <= 3) break;
        A &= ~(1u << lrm_loads_smallest(load, A));
        st = LRM_LOADS_DROPPED;
    }
    return LRM_LOADS_TRIPOD;
}

// Stage TRIPOD.  The triples i < j < k of eight legs in lexicographic order have the codes 0 .. 55; a triple's numbers do not
// depend on the lift set, so the kernel computes each once per set (lane = code) and a lift set only chooses among them.
#define LRM_LOADS_TRIPLES 56
// code -> bits 0..7 the three feet, bits 8..10 i, 11..13 j, 14..16 k
LRM_HD uint32_t lrm_loads_triple_of(uint32_t code) {
    uint32_t i = 0u, j, c = code;
    while (c >= (7u - i) * (6u - i) / 2u) { // at most five steps
        c -= (7u - i) * (6u - i) / 2u;
        i++;
    }
    j = i + 1u;
    while (c >= 7u - j) { // at most five steps
        c -= 7u - j;
        j++;
    }
    const uint32_t k = j + 1u + c;
    return (1u << i) | (1u << j) | (1u << k) | (i << 8) | (j << 11) | (k << 14);
}
LRM_HD uint32_t lrm_loads_triple_feet(uint32_t tb) { return tb & 0xffu; }
// The barycentric coordinates of the centre of mass (the origin of xi, eta) in the triangle of three feet; ok = the doubled
// area is nonzero and finite and all three are >= 0; mn = the smallest of the three.
struct LrmLoadsTriple {
    float li, lj, lk, mn;
    bool ok;
};
LRM_HD LrmLoadsTriple lrm_loads_triple(float xi, float ei, float xj, float ej, float xk, float ek) {
    LrmLoadsTriple T{0.f, 0.f, 0.f, 0.f, false};
    const float d = (xj - xi) * (ek - ei) - (xk - xi) * (ej - ei);
    if (!(d != 0.f && lrm_stance_finite(d))) return T;
    T.li = (xj * ek - xk * ej) / d;
    T.lj = (xk * ei - xi * ek) / d;
    T.lk = (xi * ej - xj * ei) / d;
    T.ok = T.li >= 0.f && T.lj >= 0.f && T.lk >= 0.f;
    T.mn = T.lj < T.li ? T.lj : T.li;
    T.mn = T.lk < T.mn ? T.lk : T.mn;
    return T;
}
// The fold over the codes in ascending order: a triple of S that is ok replaces the choice iff its mn is strictly larger
// (*best starts at -1, *at at -1): the largest minimum, the first triple on ties.
LRM_HD void lrm_loads_triple_offer(uint32_t tb, bool ok, float mn, int code, uint32_t S, float* best, int* at) {
    const uint32_t f = lrm_loads_triple_feet(tb);
    if (ok && (S & f) == f && mn > *best) {
        *best = mn;
        *at = code;
    }
}
// the chosen triple's loads: its feet in ascending order take li, lj, lk, every other foot +0
LRM_HD void lrm_loads_triple_put(uint32_t tb, float li, float lj, float lk, float load[8]) {
    const uint32_t i = (tb >> 8) & 7u, j = (tb >> 11) & 7u, k = (tb >> 14) & 7u;
#pragma unroll
    for (uint32_t l = 0; l < 8; l++) load[l] = l == i ? li : (l == j ? lj : (l == k ? lk : 0.f));
}
// The three stages, serially (the host loop; the kernel spreads the triples over lanes): -> LRM_LOADS_ALL, _DROPPED, _TRIPOD
// or _NONE; with _NONE the feet of S get nan and the others 0.
LRM_HD uint8_t lrm_loads_solve(const float xi[8], const float eta[8], uint32_t S, float load[8]) {
    const uint8_t st = lrm_loads_min_norm_stages(xi, eta, S, load);
    if (st != LRM_LOADS_TRIPOD) return st;
    float best = -1.f, li = 0.f, lj = 0.f, lk = 0.f;
    int at = -1;
    uint32_t tb_at = 0u;
#pragma unroll // constant feet per iteration: no indexed array is left (stance_loads_lane_kernel, lrm_stance_loads.hip)
    for (int code = 0; code < LRM_LOADS_TRIPLES; code++) {
        const uint32_t tb = lrm_loads_triple_of((uint32_t)code);
        const uint32_t f = lrm_loads_triple_feet(tb);
        if ((S & f) != f) continue;
        const uint32_t i = (tb >> 8) & 7u, j = (tb >> 11) & 7u, k = (tb >> 14) & 7u;
        const LrmLoadsTriple T = lrm_loads_triple(xi[i], eta[i], xi[j], eta[j], xi[k], eta[k]);
        const int before = at;
        lrm_loads_triple_offer(tb, T.ok, T.mn, code, S, &best, &at);
        if (at != before) tb_at = tb, li = T.li, lj = T.lj, lk = T.lk;
    }
    if (at < 0) {
        lrm_loads_none(S, load);
        return LRM_LOADS_NONE;
    }
    lrm_loads_triple_put(tb_at, li, lj, lk, load);
    return LRM_LOADS_TRIPOD;
}

// ---- what a (set, lift set) answers besides the loads ----
struct LrmLoadsPeak {
    float peak;
    uint8_t at, holdable;
};
// What is stored of (set, lift set) with planted feet S, status st and lrm_loads_solve's load[]: load_o and tau_o (a leg
// outside S: +0 and +0; tau = load * g otherwise, stored through lrm_loads_out), the largest |tau_j| / tau_max[j] over the
// feet of S with its code l*4 + j (codes rise and the comparison is strict: the smaller code on ties; a nan ratio never
// wins) and holdable = st in 1..3 and every |tau_j| <= tau_max[j].  st outside 1..3: -inf / 255 / 0.
LRM_HD LrmLoadsPeak lrm_loads_answer(const float tau_max[3], uint32_t S, uint8_t st, const float load[8], const float g[8][3],
                                     float load_o[8], float tau_o[8][3]) {
    LrmLoadsPeak Q{-__builtin_inff(), 255, 0};
    const bool solved = st == LRM_LOADS_ALL || st == LRM_LOADS_DROPPED || st == LRM_LOADS_TRIPOD;
    bool all_ok = solved;
#pragma unroll
    for (int l = 0; l < 8; l++) {
        const bool in = (S >> l) & 1u;
        load_o[l] = in ? lrm_loads_out(load[l]) : 0.f;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const float tau = in ? lrm_loads_out(load[l] * g[l][j]) : 0.f;
            tau_o[l][j] = tau;
            const float a = lrm_loads_abs(tau);
            const float r = a / tau_max[j];
            if (solved && in && r > Q.peak) {
                Q.peak = r;
                Q.at = (uint8_t)(l * 4 + j);
            }
            all_ok = all_ok && (!in || a <= tau_max[j]);
        }
    }
    Q.holdable = all_ok ? 1 : 0;
    return Q;
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// launch function (lrm_stance_loads.hip); only launches.  records / ik_records: the pose and IK tables (entry of (pose, leg)
// at pose * nlegs + leg); angles at [l * nsets + s]; everything is checked by the C ABI: nsets >= 1, nlegs in 1..8, nmasks in
// 1..256, nmasks * nlegs * 3 * nsets < 2^32.  pose_idx, live_in, peak_at_out, load_out, tau_out may be null.
hipError_t lrm_launch_stance_loads_posed(const void* records, const void* ik_records, const float* quats, size_t nposes, size_t nlegs,
                                         const int32_t* pose_idx, size_t nsets, const float* coxa, const float* femur,
                                         const float* tibia, const LrmLoadsParams& P, const uint8_t* live_in, uint8_t* status_out,
                                         uint8_t* holdable_out, float* peak_out, uint8_t* peak_at_out, float* load_out, float* tau_out,
                                         hipStream_t st);
#endif
