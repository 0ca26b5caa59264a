// lrm_compile_head.h -- the strict head of the leg compiler: LrmLegHead (lrm_types.h), built from
// (LegDimensions, quaternion).  One arithmetic for the host compiler (lrm_compile.cpp, the base of every
// LrmCompiledLeg) and the device pose compiler (lrm_posed.hip, one record per (pose, leg)); lrm_toltab_build.h
// is the precedent.  Both fill the same 480 bytes with the same floats.
// Libm: the host calls glibc's cosf / sinf / sincosf / asin exactly as before; the device takes cosf, sinf and
// sincosf from lrm_sincosf (lrm_exact_math.h, glibc's algorithm: tests/test_posed_cpu.py checks it against
// glibc's separate cosf / sinf) and asin from the device libm, whose double result is then rounded to float
// as on the host (the residual double-rounding risk, tests/test_gpu_posed.py).
// Compile without FMA contraction.
#pragma once
#include <math.h>
#include "lrm_exact_math.h"
#include "lrm_types.h"

// One record of the posed queries (lrm_posed.hip): the head of lrm_compile_leg(leg, quat, 1) and the pose's body position.
struct alignas(16) LrmPoseRecord {
    LrmLegHead head;
    float body_pos[3]; // subtracted from the target, component by component (0 when the caller gives none)
    float pad_[5];
};
static_assert(sizeof(LrmPoseRecord) == 512, "pose record size (LRM_POSE_RECORD_BYTES)");

// ---- libm of the head ----
LRM_HD float lrm_head_cosf(float a) {
#if defined(__HIP_DEVICE_COMPILE__)
    float s, c;
    lrm_sincosf(a, &s, &c);
    return c;
#else
    return cosf(a);
#endif
}
LRM_HD float lrm_head_sinf(float a) {
#if defined(__HIP_DEVICE_COMPILE__)
    float s, c;
    lrm_sincosf(a, &s, &c);
    return s;
#else
    return sinf(a);
#endif
}
LRM_HD void lrm_head_sincosf(float a, float* s, float* c) {
#if defined(__HIP_DEVICE_COMPILE__)
    lrm_sincosf(a, s, c);
#else
    sincosf(a, s, c);
#endif
}

struct LrmQuat {
    float x, y, z, w;
};

// qtInvert, unified_math_cuda.cu.h:29-34
LRM_HD LrmQuat lrm_q_invert(LrmQuat q) {
    const float n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
    return LrmQuat{q.x / n2, -q.y / n2, -q.z / n2, -q.w / n2};
}

// qtMultiply, unified_math_cuda.cu.h:40-46
LRM_HD LrmQuat lrm_q_mul(LrmQuat a, LrmQuat b) {
    LrmQuat r;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x;
    r.z = a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w;
    return r;
}

// quatFromVectAngle, unified_math_cuda.cu.h:48-57, for the z axis
LRM_HD LrmQuat lrm_q_about_z(float angle) {
    float s, c;
    lrm_head_sincosf(angle / 2, &s, &c);
    const float mag = lrm_sqrtf(0.f * 0.f + 0.f * 0.f + 1.f * 1.f);
    return LrmQuat{s, c * 0.f / mag, c * 0.f / mag, c * 1.f / mag};
}

// the nine coefficient sums of qtRotate, unified_math_cuda.cu.h:13-27
LRM_HD void lrm_rot_coefficients(LrmQuat q, float m[9]) {
    const float t2 = q.x * q.y, t3 = q.x * q.z, t4 = q.x * q.w;
    const float t5 = -q.y * q.y, t6 = q.y * q.z, t7 = q.y * q.w;
    const float t8 = -q.z * q.z, t9 = q.z * q.w, t10 = -q.w * q.w;
    m[0] = t8 + t10; m[1] = t6 - t4; m[2] = t3 + t7;
    m[3] = t4 + t6;  m[4] = t5 + t10; m[5] = t9 - t2;
    m[6] = t7 - t3;  m[7] = t2 + t9; m[8] = t5 + t8;
}

// pitch component of rpyFromQuat, unified_math_cuda.cu.h:59-83: a double asin rounded to float
LRM_HD float lrm_pitch_of(LrmQuat q) {
    const double sinp = 2 * (q.w * q.y - q.z * q.x); // float product, widened
    if (fabs(sinp) >= 1) return copysignf((float)(M_PI / 2), (float)sinp);
    return (float)asin(sinp);
}

// rotate_leg_data, one_leg_global.cu:48-60: the tibia limits rotated by the pitch of the body orientation seen from the leg
LRM_HD void lrm_rotate_leg(const float quat[4], const LrmLegDimensions& leg, LrmLegDimensions* out) {
    const LrmQuat q{quat[0], quat[1], quat[2], quat[3]};
    const LrmQuat qa = lrm_q_about_z(leg.body_angle);
    const float pitch = lrm_pitch_of(lrm_q_mul(lrm_q_mul(qa, q), lrm_q_invert(qa)));
    *out = leg;
    out->tibia_absolute_pos -= pitch;
    out->tibia_absolute_neg -= pitch;
}

LRM_HD LrmCircle lrm_head_circle(float x, float y, float r, bool attract) { return LrmCircle{x, y, r, attract ? 1.f : 0.f}; }

// circles.cu.h:80-135 + leg_geometry.cu.h:12-50
LRM_HD LrmCircle lrm_head_inner(const LrmLegDimensions& l) {
    const float x = l.femur_length + l.tibia_length * lrm_head_cosf(l.min_angle_tibia);
    const float y = l.tibia_length * lrm_head_sinf(l.min_angle_tibia);
    return lrm_head_circle(0.f, 0.f, lrm_sqrtf(x * x + y * y), false);
}
LRM_HD LrmCircle lrm_head_outer(const LrmLegDimensions& l) {
    return lrm_head_circle(0.f, 0.f, l.tibia_length + l.femur_length, true);
}
LRM_HD LrmCircle lrm_head_from_above(const LrmLegDimensions& l, bool positive) {
    const float a = positive ? l.tibia_absolute_pos : l.tibia_absolute_neg;
    return lrm_head_circle(l.tibia_length * lrm_head_cosf(a), l.tibia_length * lrm_head_sinf(a), l.femur_length, false);
}
LRM_HD LrmCircle lrm_head_winglet(const LrmLegDimensions& l, bool lower_side) {
    const float a = lower_side ? l.min_angle_femur : l.max_angle_femur;
    return lrm_head_circle(lrm_head_cosf(a) * l.femur_length, lrm_head_sinf(a) * l.femur_length, l.tibia_length, false);
}

// The leg-only half of find_region (circles.cu.h:56-68) for a given UpperRegion bit.
struct LrmSideFlags {
    bool femur_limits;       // FemurAngleLimitation
    bool femur_limits_other; // FemurAngleLimitation_other
    float full_sat;          // full_sat_limit
};
LRM_HD LrmSideFlags lrm_side_flags(const LrmLegDimensions& d, bool upper) {
    const float femur_limit = upper ? d.max_angle_femur : d.min_angle_femur;
    const float abs_limit = upper ? d.tibia_absolute_pos : d.tibia_absolute_neg;
    const float femur_limit_o = !upper ? d.max_angle_femur : d.min_angle_femur;
    const float abs_limit_o = !upper ? d.tibia_absolute_pos : d.tibia_absolute_neg;
    LrmSideFlags f;
    f.femur_limits = (!upper) != (femur_limit < abs_limit);
    f.femur_limits_other = (!upper) != (femur_limit_o < abs_limit_o);
    f.full_sat = f.femur_limits ? femur_limit : abs_limit;
    return f;
}

// insert_circles (MegaClamp == 0), circles.cu.h:337-383, for one of the 4 possible regions
LRM_HD void lrm_circle_list(const LrmLegDimensions& l, bool upper, bool fully_ext, LrmCircle out[4]) {
    const LrmSideFlags f = lrm_side_flags(l, upper);
    out[0] = lrm_head_inner(l);
    LrmCircle* tail = out + 1; // [0] fromabove_neg slot, [1] fromabove_pos slot, [2] winglet slot
    tail[0] = lrm_head_from_above(l, false);
    tail[1] = lrm_head_from_above(l, true);
    const int excluded = upper ? 0 : 1;
    if (f.femur_limits_other) tail[excluded] = lrm_head_winglet(l, /*lower_side=*/upper);
    tail[excluded].attract = 0.f;
    const int other = upper ? 1 : 0;
    tail[2] = lrm_head_winglet(l, /*lower_side=*/!upper);
    tail[other].attract = f.femur_limits ? 0.f : 1.f;
    tail[2].attract = f.femur_limits ? 1.f : 0.f;
    if (fully_ext) tail[(tail[other].attract != 0.f) ? other : 2] = lrm_head_outer(l);
}

// insert_intersecv2, circles.cu.h:417-476; the unused slots of xs / ys are set to 0
LRM_HD int lrm_corner_points(const LrmLegDimensions& l, float* xs, float* ys) {
    const double kEps = 0.001; // circles.cu.h:7 (a double literal in the reference)
    const float fem[10] = {l.min_angle_femur, l.min_angle_femur, l.min_angle_femur,
                           l.tibia_absolute_neg - l.min_angle_tibia,
                           l.tibia_absolute_neg - l.max_angle_tibia,
                           l.max_angle_femur, l.max_angle_femur, l.max_angle_femur,
                           l.tibia_absolute_pos - l.min_angle_tibia,
                           l.tibia_absolute_pos - l.min_angle_tibia};
    const float tib[10] = {l.max_angle_tibia, l.min_angle_tibia, l.tibia_absolute_neg - fem[2],
                           l.tibia_absolute_neg - fem[3], l.tibia_absolute_neg - fem[4],
                           l.min_angle_tibia, l.max_angle_tibia, l.tibia_absolute_pos - fem[7],
                           l.tibia_absolute_pos - fem[8], l.tibia_absolute_pos - fem[9]};
    int n = 0;
    for (int i = 0; i < 10; i++) {
        const float f = fem[i], t = tib[i], a = f + t;
        const bool ok = ((double)f < (double)l.max_angle_femur + kEps) && ((double)f > (double)l.min_angle_femur - kEps) &&
                        ((double)t < (double)l.max_angle_tibia + kEps) && ((double)t > (double)l.min_angle_tibia - kEps) &&
                        ((double)a < (double)l.tibia_absolute_pos + kEps) && ((double)a > (double)l.tibia_absolute_neg - kEps);
        if (!ok) continue;
        const float xf = l.femur_length * lrm_head_cosf(f), yf = l.femur_length * lrm_head_sinf(f);
        const float xt = l.tibia_length * lrm_head_cosf(a), yt = l.tibia_length * lrm_head_sinf(a);
        xs[n] = xf + xt;
        ys[n] = yf + yt;
        n++;
    }
    for (int i = n; i < LRM_N_CORNERS; i++) xs[i] = ys[i] = 0.f;
    return n;
}

// The head of lrm_compile_leg(leg_in, quat, apply_leg_rotation): every field of LrmLegHead, written into `out`.
// *leg_out (may be null) receives the leg the rest of the compiler works on.
LRM_HD void lrm_compile_head(const LrmLegDimensions& leg_in, const float quat[4], int apply_leg_rotation, LrmLegHead* out,
                             LrmLegDimensions* leg_out) {
    const float kPi = 3.14159265358979323846264338327950288419716939937510582097f;
    LrmLegDimensions l = leg_in;
    if (apply_leg_rotation) lrm_rotate_leg(quat, leg_in, &l);
    const LrmQuat q{quat[0], quat[1], quat[2], quat[3]};

    for (int u = 0; u < 2; u++)
        for (int fe = 0; fe < 2; fe++) lrm_circle_list(l, u != 0, fe != 0, out->lists[u * 2 + fe]);
    out->n_corners = lrm_corner_points(l, out->corner_x, out->corner_y);

    lrm_rot_coefficients(lrm_q_invert(q), out->inv_rot);
    lrm_rot_coefficients(q, out->fwd_rot);
    lrm_head_sincosf(-l.body_angle, &out->sin_body, &out->cos_body);
    out->body = l.body;
    lrm_head_sincosf(-l.coxa_pitch, &out->sin_pitch, &out->cos_pitch);
    lrm_head_sincosf(l.coxa_pitch, &out->sin_pitch_rev, &out->cos_pitch_rev);
    out->coxa_length = l.coxa_length;
    out->max_coxa = l.max_angle_coxa;
    out->min_coxa = l.min_angle_coxa;
    out->mega_hi = l.max_angle_coxa + kPi / 2;
    out->mega_lo = l.min_angle_coxa - kPi / 2;
    out->coxa_mid = (l.max_angle_coxa + l.min_angle_coxa) / 2;
    // circles.cu.h:52-54 (std::max / std::min)
    const float lo = (l.tibia_absolute_neg < l.min_angle_femur) ? l.min_angle_femur : l.tibia_absolute_neg;
    const float hi = (l.max_angle_femur < l.tibia_absolute_pos) ? l.max_angle_femur : l.tibia_absolute_pos;
    out->region_mid = (lo + hi) / 2;
    out->full_sat[0] = lrm_side_flags(l, false).full_sat;
    out->full_sat[1] = lrm_side_flags(l, true).full_sat;
    // Nothing farther than the stretched leg (+1 mm and 1e-4 relative slack, three orders of
    // magnitude above the float rounding of the strict evaluation) can pass the attractive
    // circle test, so pairs beyond this radius are skipped without changing any result.
    const float reach = l.body + l.coxa_length + l.femur_length + l.tibia_length + 1.0f;
    out->reach_r2_max = reach * reach * 1.0001f;
    if (leg_out) *leg_out = l;
}
