// lrm_footholds_posed.h -- the per-(pose, leg) entry of lrm_footholds_posed_dev's third table: the leg's nominal point
// in the caller's frame and a bounding sphere of everything the leg can reach under the pose.  One arithmetic for the
// device compiler (lrm_footholds_posed.hip) and the host one (lrm_capi.cpp): float32 only, the libm of the head
// (lrm_compile_head.h), no contraction, so that both write the same bytes.  lrm_foothold_d2 (lrm_footholds.h) and
// lrm_ik_compile_pose (lrm_ik.h) are the precedents.
#pragma once
#include "lrm_compile_head.h"
#include "lrm_point.h"

// 32 bytes per (pose, leg) at pose * nlegs + leg (LRM_POSE_FOOTHOLD_BYTES, include/lrm.h)
struct alignas(16) LrmPoseFootEntry {
    float cull_center[3]; // relative to body[pose], caller's frame
    float cull_r2;        // +inf: a sphere that excludes nothing
    float nominal_w[3];   // nominal[leg] taken from the body frame to the caller's frame: qtRotate(quat, nominal)
    float pad;            // 0
};
static_assert(sizeof(LrmPoseFootEntry) == 32, "pose foothold entry size");

// The sphere is lrm_compile.cpp's pair sphere (coxa frame: yaw within the coxa range, within femur + tibia of the femur
// joint in the meridian plane, mirrored points included) taken through the inverse of reachability_global's chain
//   p -> qtInvRotate(quat) -> Rz(-body_angle) -> x -= body -> Rp(-coxa_pitch)
// It depends on the coxa limits and the lengths only, not on the tibia limits that rotate_leg_data changes.
// A quaternion whose |q|^2 is not 1 within 1e-5 (nan and inf included) makes qtInvRotate something else than a
// rotation: the entry then holds centre 0 and r2 = +inf, which excludes nothing, and so does any entry whose
// arithmetic is not finite.  Within 1e-5 the map changes lengths by less than 2e-5 of them: 0.02 mm per metre, inside
// the 1 mm + 1e-4 slack of the radius.
LRM_HD void lrm_pose_foothold_entry(const LrmLegDimensions& leg, const float quat[4], const float* nominal /* 3 floats or null */,
                                    LrmPoseFootEntry* E) {
    const LrmQuat q{quat[0], quat[1], quat[2], quat[3]};
    float fwd[9];
    lrm_rot_coefficients(q, fwd); // the record's fwd_rot
    const LrmVec3 nb{nominal ? nominal[0] : 0.f, nominal ? nominal[1] : 0.f, nominal ? nominal[2] : 0.f};
    const LrmVec3 nw = lrm_qrot(fwd, nb);
    // A zero nominal (NULL included): exactly 0, whatever the quaternion (0 * nan would be nan).  Otherwise a nan (nan or inf quaternion:
    // such a pose reaches nothing) is stored as ONE bit pattern: host and device units give an invalid operation
    // different sign and payload bits, and the tables are compared byte for byte.
    const bool none = nb.x == 0.f && nb.y == 0.f && nb.z == 0.f;
    E->nominal_w[0] = none ? 0.f : nw.x != nw.x ? __builtin_nanf("") : nw.x;
    E->nominal_w[1] = none ? 0.f : nw.y != nw.y ? __builtin_nanf("") : nw.y;
    E->nominal_w[2] = none ? 0.f : nw.z != nw.z ? __builtin_nanf("") : nw.z;
    E->pad = 0.f;

    const float inf = __builtin_inff();
    E->cull_center[0] = E->cull_center[1] = E->cull_center[2] = 0.f;
    E->cull_r2 = inf;
    const float n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
    if (!(fabsf(n2 - 1.0f) <= 1e-5f)) return;
    const float c = leg.coxa_length, L = (leg.femur_length + leg.tibia_length + 1.0f) * 1.0001f;
    const float th = 0.5f * (leg.max_angle_coxa + leg.min_angle_coxa);
    const float al = 0.5f * (leg.max_angle_coxa - leg.min_angle_coxa);
    float rho = 0.f, r2 = (fabsf(c) + L) * (fabsf(c) + L); // the whole ball around the coxa origin
    float sth = 0.f, cth = 1.f;
    if (fabsf(th) <= 8.f && fabsf(al) <= 8.f && c > 0.f) {
        const float ca = lrm_head_cosf(al);
        if (ca > 0.05f) {
            const float lc = fmaxf(L - c, 0.f);
            const float cand[3] = {c, 2.0f * c * L / (lc + (c + L) * ca), c / ca};
            for (int k = 0; k < 3; k++) {
                const float rc = cand[k];
                const float f1 = rc * rc + L * L - c * c + 2.0f * lc * fmaxf(rc - c, 0.f);
                const float f2 = (c + L) * (c + L) - 2.0f * rc * (c + L) * ca + rc * rc;
                const float f = fmaxf(f1, f2);
                if (f < r2) {
                    r2 = f;
                    rho = rc;
                }
            }
            lrm_head_sincosf(th, &sth, &cth);
        }
    }
    // centre: coxa frame -> leg-0 body frame (Rp^T, + body, Rz^T) -> caller's frame (qtRotate(quat, .))
    float sp, cp, sb, cb;
    lrm_head_sincosf(-leg.coxa_pitch, &sp, &cp);
    lrm_head_sincosf(-leg.body_angle, &sb, &cb);
    const float c0 = rho * cth, c1 = rho * sth;
    const float v0 = cp * c0 + leg.body, v1 = c1, v2 = -sp * c0;
    const LrmVec3 u{cb * v0 + sb * v1, cb * v1 - sb * v0, v2};
    const LrmVec3 w = lrm_qrot(fwd, u);
    // + 1 mm and 1e-5 of the offsets: float rounding of the centre, of this arithmetic and of the strict test itself
    const float rr = lrm_sqrtf(fmaxf(r2, 0.f)) + 1.0f + 1e-5f * (fabsf(leg.body) + rho);
    const float out_r2 = rr * rr * 1.0001f;
    const float probe = ((w.x + w.y) + w.z) + out_r2; // nan or inf if any of the four is
    if (!(fabsf(probe) < inf)) return;
    E->cull_center[0] = w.x;
    E->cull_center[1] = w.y;
    E->cull_center[2] = w.z;
    E->cull_r2 = out_r2;
}

// ---- nearest-miss footholds (lrm_foothold_misses_posed_dev / _cpu, lrm_foothold_misses.hip) ----------------------
// One arithmetic for the kernel and the host loop, float32 without contraction: these three functions decide outputs
// (which targets are candidates, and the order of the misses), so the conservative fmaf sphere tests of the other pair
// kernels are NOT a substitute for them.
//
// rm2 of an entry: the square of the entry's radius widened by `margin` (mm).  cull_r2 = +inf or margin = +inf give +inf.
LRM_HD float lrm_foothold_miss_rm2(float cull_r2, float margin) {
    const float rm = lrm_sqrtf(cull_r2) + margin;
    return rm * rm;
}
// Target q = t - body[p] (already subtracted, one f32 subtraction per component) is a candidate of the entry with centre
// `center` iff e2 <= rm2, e = q - center.  A nan e2 is no candidate; rm2 = +inf takes every other target.
LRM_HD bool lrm_foothold_miss_candidate(LrmVec3 q, const float center[3], float rm2) {
    const float ex = q.x - center[0], ey = q.y - center[1], ez = q.z - center[2];
    const float e2 = (ex * ex + ey * ey) + ez * ez;
    return e2 <= rm2;
}
// m2 of a miss: the squared length of its distance_global vector; the miss is eligible iff m2 < +inf (false for nan)
LRM_HD float lrm_foothold_miss_m2(LrmVec3 d) { return (d.x * d.x + d.y * d.y) + d.z * d.z; }
