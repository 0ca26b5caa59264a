// lrm_stance.h -- the arithmetic of lrm_stance_stability_dev / _cpu (include/lrm.h): does the centre of mass of a stance
// lie over the polygon its planted feet span, and by how much, for every set of lifted legs.  One source for the kernel
// (lrm_stance.hip) and the host loop (lrm_capi.cpp): float32 only, no contraction, only + - * /, comparisons and lrm_sqrtf,
// so that both give the same bits.  Everything that decides an output is here; the kernel only distributes it over lanes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "lrm_compile_head.h"
#include "lrm_point.h"

#define LRM_STANCE_MAX_MASKS 256

struct LrmStancePt {
    float x, y;
};

// What travels from the host in the kernel's arguments: the centre of mass (BODY frame), the plane basis (on == 0: the
// caller's x and y), the lift sets and the margin to beat.  All checked by the C ABI.
struct LrmStanceParams {
    float com[3];
    float u[3], v[3];
    uint32_t on;
    float min_margin;
    uint32_t nmasks;
    uint8_t lift[LRM_STANCE_MAX_MASKS];
};

LRM_HD bool lrm_stance_finite(float v) { return (lrm_f2u(v) & 0x7f800000u) != 0x7f800000u; }

// A point of the caller's frame (relative to body[p]) taken into the plane normal to gravity
LRM_HD LrmStancePt lrm_stance_project(const LrmStanceParams& P, LrmVec3 q) {
    if (!P.on) return LrmStancePt{q.x, q.y};
    return LrmStancePt{(q.x * P.u[0] + q.y * P.u[1]) + q.z * P.u[2], (q.x * P.v[0] + q.y * P.v[1]) + q.z * P.v[2]};
}

// foot index -> usable as an index of the cloud
LRM_HD bool lrm_stance_foot_in_cloud(int32_t foot, size_t nt) { return foot >= 0 && (size_t)foot < nt; }
// q = t[foot] - body[p], already subtracted: the foot is valid iff all three are finite
LRM_HD bool lrm_stance_foot_valid(LrmVec3 q) { return lrm_stance_finite(q.x) && lrm_stance_finite(q.y) && lrm_stance_finite(q.z); }

// The centre of mass in the plane, relative to body[p]: lrm_pose_foothold_entry's nominal_w chain (lrm_footholds_posed.h).
// A zero com is exactly 0 whatever the quaternion (0 * nan would be nan).  *ok = both coordinates finite.
LRM_HD LrmStancePt lrm_stance_com(const LrmStanceParams& P, const float quat[4], bool* ok) {
    LrmVec3 c3{0.f, 0.f, 0.f};
    if (!(P.com[0] == 0.f && P.com[1] == 0.f && P.com[2] == 0.f)) {
        float fwd[9];
        lrm_rot_coefficients(LrmQuat{quat[0], quat[1], quat[2], quat[3]}, fwd);
        c3 = lrm_qrot(fwd, LrmVec3{P.com[0], P.com[1], P.com[2]});
    }
    const LrmStancePt c = lrm_stance_project(P, c3);
    *ok = lrm_stance_finite(c.x) && lrm_stance_finite(c.y);
    return c;
}

// The ordered pair (i, j) of two valid feet: the directed line from a = f_i to f_j.
struct LrmStanceEdge {
    LrmStancePt a, e;
    float len2;
};
LRM_HD LrmStanceEdge lrm_stance_edge(LrmStancePt fi, LrmStancePt fj) {
    LrmStanceEdge E;
    E.a = fi;
    E.e = LrmStancePt{fj.x - fi.x, fj.y - fi.y};
    E.len2 = E.e.x * E.e.x + E.e.y * E.e.y;
    return E;
}
LRM_HD bool lrm_stance_edge_usable(const LrmStanceEdge& E) { return E.len2 > 0.f && E.len2 < __builtin_inff(); }
// the cross product e x (p - a): >= 0 puts p on the line or to its left
LRM_HD float lrm_stance_cross(const LrmStanceEdge& E, LrmStancePt p) { return E.e.x * (p.y - E.a.y) - E.e.y * (p.x - E.a.x); }
LRM_HD bool lrm_stance_left(const LrmStanceEdge& E, LrmStancePt fk) { return lrm_stance_cross(E, fk) >= 0.f; }
// signed distance of the centre of mass from the line, positive to its left
LRM_HD float lrm_stance_signed(const LrmStanceEdge& E, LrmStancePt c) { return lrm_stance_cross(E, c) / lrm_sqrtf(E.len2); }

// What the fold over the lift sets reads of a pair, packed: bits 0..7 left_ij, bits 8..15 the two feet, bit 16 the pair
// takes part (i != j, both feet valid, usable).
#define LRM_STANCE_PAIR_ON 0x10000u
LRM_HD uint32_t lrm_stance_pair_bits(uint32_t left, int i, int j, bool on) {
    return (left & 0xffu) | (((1u << i) | (1u << j)) << 8) | (on ? LRM_STANCE_PAIR_ON : 0u);
}
// Is the pair a counter-clockwise hull edge of the planted feet S: both feet planted, no planted foot to its right
LRM_HD bool lrm_stance_pair_counts(uint32_t bits, uint32_t S) {
    const uint32_t ends = (bits >> 8) & 0xffu;
    return (bits & LRM_STANCE_PAIR_ON) && (S & ends) == ends && (S & ~bits & 0xffu) == 0u;
}

// The high word of a pair's key RISES with s (lrm_body_clearance.h's falls with the height): a nan s counts as -inf, -0 as
// +0; s >= +0 gives bits | 0x80000000, a negative s the complement of its bits.  -inf gives 0x007fffff, +inf 0xff800000.
LRM_HD uint32_t lrm_stance_word(float s) {
    s = s != s ? -__builtin_inff() : s + 0.f;
    const uint32_t u = lrm_f2u(s);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
// 64-bit key of a counting pair: the smallest key is the smallest s, ties the smaller code i*8 + j.  No key of a pair
// equals kLrmStanceNone (its high word would be a nan's).
constexpr uint64_t kLrmStanceNone = ~0ull;
LRM_HD uint64_t lrm_stance_key(uint32_t word, uint32_t code) { return ((uint64_t)word << 32) | code; }
// What a key holds: the margin and its edge code; -inf and 255 for kLrmStanceNone and for a margin of -inf.
struct LrmStanceAnswer {
    float margin;
    uint8_t edge;
};
LRM_HD LrmStanceAnswer lrm_stance_key_decode(uint64_t key) {
    const uint32_t w = (uint32_t)(key >> 32);
    const float inf = __builtin_inff();
    const float m = key == kLrmStanceNone ? -inf : lrm_u2f((w >> 31) ? (w & 0x7fffffffu) : ~w);
    return LrmStanceAnswer{m, (uint8_t)(m == -inf ? 255u : (uint32_t)key & 63u)};
}
// The planted feet of a lift set, and the rule for fewer than three of them
LRM_HD uint32_t lrm_stance_planted(uint32_t valid_feet, uint32_t lift) { return valid_feet & ~lift & 0xffu; }
LRM_HD bool lrm_stance_stands(uint32_t S) { return __builtin_popcount(S) >= 3; }
LRM_HD bool lrm_stance_stable(float margin, float min_margin) { return margin > min_margin; }

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// launch function (lrm_stance.hip); only launches.  Everything is checked by the C ABI: nstances >= 1, nmasks in 1..256,
// nmasks * nstances < 2^32, nt, nposes, nstances <= INT32_MAX.  body, pose_idx, live_in, edge_out, feet_out may be null.
hipError_t lrm_launch_stance_stability(const float* tx, const float* ty, const float* tz, size_t nt, const float* quats,
                                       const float* body, size_t nposes, const int32_t* pose_idx, const int32_t* foot, size_t nstances,
                                       size_t nlegs, const LrmStanceParams& P, const uint8_t* live_in, float* margin_out,
                                       uint8_t* edge_out, uint8_t* stable_out, uint8_t* feet_out, hipStream_t st);
#endif
