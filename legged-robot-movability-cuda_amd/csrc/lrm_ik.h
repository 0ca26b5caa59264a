// lrm_ik.h -- per-point inverse / forward kinematics of the 3-DoF yaw-pitch-pitch leg (lrm_ik_*, lrm_fk_*).
//
// One source for the device kernels (lrm_ik.hip) and the CPU entry points (lrm_capi.cpp), compiled with
// -ffp-contract=off like lrm_point.h.  Only lrm_atan2f, lrm_sincosf, lrm_sqrtf (lrm_exact_math.h) and + - * /
// appear, so the host loop and the kernel agree bit for bit.  Every sincos argument is an angle in [-3 pi, 3 pi],
// inside lrm_sincosf's exact range (|x| < 120: the contract at the top of lrm_exact_math.h).
//
// Frames: p (caller's frame) -> qrot(inv_rot) -> rotate by -body_angle -> x -= body -> rotate by -coxa_pitch: the coxa
// frame of lrm_reach_global / lrm_dist_global.  There the tip of (yaw c, femur f, tibia t) is
//   (cos c * (C + F cos f + T cos(f + t)), sin c * (C + ...), F sin f + T sin(f + t))
// with C = coxa_length, F = femur_length, T = tibia_length (the reference's forward_kinematics, one_leg.cu:377-403,
// which stops before the coxa pitch).  lrm_fk_point applies that and the inverse chain (lrm_ik_from_coxa).
//
// IK of point p (DESIGN.md "Joint angles"):
//   goal g = p when lrm_reach_global(p), else g = p - d with d the strict lrm_dist_global vector of p;
//   candidates: yaw atan2(gy, gx) and its mirror atan2(-gy, -gx) in the coxa frame, each clamped to the coxa limits;
//     per yaw plane both knees of the analytic 2-link solve, each re-solved with a violated joint at its limit and
//     then clamped into the limits (lrm_ik_knee);
//   residual of a candidate: |tip - g|, from its in-plane miss and the goal's distance to the (clamped) yaw plane;
//   selection: of the candidates within LRM_IK_NEAR_F of the smallest residual, the one nearest the seed (sum of
//     squared joint differences); ties go to the best-residual candidate, then to the lower candidate number (0 direct
//     yaw / knee +, 1 direct / knee -, 2 mirrored / knee +, 3 mirrored / knee -); a seed with a nan or inf component
//     is replaced by the default one, and a seed can never select a candidate outside the near-best set;
//   status LRM_IK_*: from the chosen tip's distance to p in the caller's frame, in float32 (LRM_IK_TOL_F).
#pragma once
#include "lrm_compile_head.h"
#include "lrm_point.h"

#define LRM_IK_TOL_F 0.002f  // mm: status thresholds (twice the reference's CIRCLE_MARGIN)
#define LRM_IK_REL_F 2.384185791015625e-07f // 2^-22: the float32 resolution of |d| joins the status-2 line far from the leg
#define LRM_IK_NEAR_F 0.001f // mm: candidates this close to the best residual compete on the seed distance
#define LRM_2PI_F 6.28318530717958647692528676655900576839433879875021164195f

// The per-(leg, orientation) constants of the IK, on top of the strict head: the limits of
// rotate_leg_data(quat, leg) and the link lengths.  Small, by value in the kernarg segment.
struct LrmIkLeg {
    float C, F, T;             // coxa_length, femur_length, tibia_length
    float sum2, dif2, ff_tt;   // (F + T)^2, (F - T)^2, F^2 + T^2
    float cmin, cmax;          // coxa (yaw) limits
    float fmin, fmax;          // femur limits
    float tmin, tmax;          // tibia limits
    float aneg, apos;          // femur + tibia: tibia_absolute_neg / _pos of the ROTATED leg
    float f_lo, f_hi;          // femur range where some tibia meets both the tibia and the absolute limits
    float seed[3];             // default seed: mid-range of each joint
    float back[9];             // the inverse of qtInvRotate(quat, .) (row-major): the last step of the FK
    float pad_[4];
};
static_assert(sizeof(LrmIkLeg) == 128, "LrmIkLeg layout");

LRM_HD float lrm_ik_clampf(float x, float lo, float hi) { // comparisons, not fminf/fmaxf: nan stays nan, -0 stays -0
    x = (x < lo) ? lo : x;
    return (x > hi) ? hi : x;
}
LRM_HD float lrm_ik_wrapf(float a) { // [-3 pi, 3 pi] -> [-pi, pi]
    a = (a > LRM_PI_F) ? a - LRM_2PI_F : a;
    return (a < -LRM_PI_F) ? a + LRM_2PI_F : a;
}

// The constants of the leg AFTER rotate_leg_data, from that leg and the head's inv_rot.  The femur range [f_lo, f_hi] is where the tibia interval
// [max(tmin, aneg - f), min(tmax, apos - f)] is not empty.  A leg with no in-limit configuration at all (f_lo > f_hi
// or aneg > apos) keeps the femur's own range: its tibia is clamped into the tibia limits only, the absolute limit is
// then not met, and every point gets status 3 or 4.
// back: the matrix of qtInvRotate(quat, .) is I + 2 inv_rot; its inverse, in double and rounded once, takes the FK back to
// the caller's frame.  For a unit quaternion that is qtRotate(quat, .) up to float32 rounding; the reference does not
// normalise quaternions (several fixtures are not unit), and for those only the inverse makes FK(IK(p)) = p.
// Host (the single-pose calls, lrm_capi.cpp) and device (pose_ik_compile_kernel, lrm_ik_posed.hip): float comparisons,
// float + - * and double + - * / only, all correctly rounded on both sides, so one source gives the same bytes.
LRM_HD void lrm_ik_compile(const LrmLegDimensions& r, const float inv_rot[9], LrmIkLeg* K) {
    K->C = r.coxa_length;
    K->F = r.femur_length;
    K->T = r.tibia_length;
    K->sum2 = (K->F + K->T) * (K->F + K->T);
    K->dif2 = (K->F - K->T) * (K->F - K->T);
    K->ff_tt = K->F * K->F + K->T * K->T;
    K->cmin = r.min_angle_coxa;
    K->cmax = r.max_angle_coxa;
    K->fmin = r.min_angle_femur;
    K->fmax = r.max_angle_femur;
    K->tmin = r.min_angle_tibia;
    K->tmax = r.max_angle_tibia;
    K->aneg = r.tibia_absolute_neg;
    K->apos = r.tibia_absolute_pos;
    float lo = K->aneg - K->tmax, hi = K->apos - K->tmin;
    lo = (K->fmin > lo) ? K->fmin : lo;
    hi = (K->fmax < hi) ? K->fmax : hi;
    if (!(lo <= hi) || !(K->aneg <= K->apos)) {
        lo = K->fmin;
        hi = K->fmax;
    }
    K->f_lo = lo;
    K->f_hi = hi;
    K->seed[0] = 0.5f * (K->cmin + K->cmax);
    K->seed[1] = 0.5f * (K->fmin + K->fmax);
    K->seed[2] = 0.5f * (K->tmin + K->tmax);
    double a[9], inv[9];
    for (int k = 0; k < 9; k++) a[k] = 2.0 * (double)inv_rot[k] + ((k % 4 == 0) ? 1.0 : 0.0);
    inv[0] = a[4] * a[8] - a[5] * a[7];
    inv[1] = a[2] * a[7] - a[1] * a[8];
    inv[2] = a[1] * a[5] - a[2] * a[4];
    inv[3] = a[5] * a[6] - a[3] * a[8];
    inv[4] = a[0] * a[8] - a[2] * a[6];
    inv[5] = a[2] * a[3] - a[0] * a[5];
    inv[6] = a[3] * a[7] - a[4] * a[6];
    inv[7] = a[1] * a[6] - a[0] * a[7];
    inv[8] = a[0] * a[4] - a[1] * a[3];
    const double det = a[0] * inv[0] + a[1] * inv[3] + a[2] * inv[6];
    for (int k = 0; k < 9; k++) K->back[k] = (float)(inv[k] / det);
    K->pad_[0] = K->pad_[1] = K->pad_[2] = K->pad_[3] = 0.f;
}

// The constants of (leg, quat) as the single-pose calls build them: lrm_rotate_leg for the limits, the inv_rot of
// lrm_compile_head.  One entry of the posed IK table (lrm_ik_posed.hip), on the host and on the device; the device can
// differ from the host only where lrm_rotate_leg's double asin does (lrm_compile_head.h).
LRM_HD void lrm_ik_compile_pose(const LrmLegDimensions& leg, const float quat[4], LrmIkLeg* K) {
    LrmLegDimensions r;
    lrm_rotate_leg(quat, leg, &r);
    float inv_rot[9];
    lrm_rot_coefficients(lrm_q_invert(LrmQuat{quat[0], quat[1], quat[2], quat[3]}), inv_rot);
    lrm_ik_compile(r, inv_rot, K);
}

// p (caller's frame) -> coxa frame: the operations of lrm_reach_global + lrm_reach_circles, in their order
LRM_HD LrmVec3 lrm_ik_to_coxa(const LrmLegHead& L, LrmVec3 p) {
    LrmVec3 u = lrm_qrot(L.inv_rot, p);
    const float buffer = u.x * L.sin_body;
    u.x = u.x * L.cos_body - u.y * L.sin_body;
    u.y = buffer + u.y * L.cos_body;
    u.x -= L.body;
    const float b2 = u.x * L.sin_pitch;
    u.x = u.x * L.cos_pitch - u.z * L.sin_pitch;
    u.z = b2 + u.z * L.cos_pitch;
    return u;
}

// coxa frame -> caller's frame: the inverse of lrm_ik_to_coxa
LRM_HD LrmVec3 lrm_ik_from_coxa(const LrmLegHead& L, const LrmIkLeg& K, LrmVec3 u) {
    // place_over_coxa<Reverse>, one_leg.cu:9-24
    const float buffer = u.x * L.sin_pitch_rev;
    u.x = u.x * L.cos_pitch_rev - u.z * L.sin_pitch_rev;
    u.z = buffer + u.z * L.cos_pitch_rev;
    u.x += L.body;
    // z_unrotateInPlace, one_leg_global.cu:33-39
    const float b2 = u.x * -L.sin_body;
    u.x = u.x * L.cos_body - u.y * -L.sin_body;
    u.y = b2 + u.y * L.cos_body;
    const float* m = K.back;
    return LrmVec3{m[0] * u.x + m[1] * u.y + m[2] * u.z, m[3] * u.x + m[4] * u.y + m[5] * u.z,
                   m[6] * u.x + m[7] * u.y + m[8] * u.z};
}

// forward kinematics: joint angles -> tip in the caller's frame
LRM_HD LrmVec3 lrm_fk_point(const LrmLegHead& L, const LrmIkLeg& K, float c, float f, float t) {
    float sc, cc, sf, cf, sa, ca;
    lrm_sincosf(c, &sc, &cc);
    lrm_sincosf(f, &sf, &cf);
    lrm_sincosf(f + t, &sa, &ca);
    const float h = K.C + (K.F * cf + K.T * ca);
    return lrm_ik_from_coxa(L, K, LrmVec3{cc * h, sc * h, K.F * sf + K.T * sa});
}

struct LrmIkCand {
    float c, f, t; // joint angles
    float sc, cc;  // sincos of the yaw
    float h, v;    // tip in the yaw plane, relative to the femur joint
    float e;       // residual |tip - g| (mm)
};

// One knee of the 2-link solve in the yaw plane: goal (px, pz) relative to the femur joint, phi = atan2(pz, px),
// (f, t) the unclamped solution.  A violated femur limit: the femur goes to it and the tibia aims at the goal; then a
// violated tibia limit: the tibia goes to it and the femur is re-solved; then a violated absolute limit: f + t goes
// to it and the femur is re-solved on that face (clamped to where the femur and tibia limits leave it: a corner there).
// Last, the clamp into the limits (femur into [f_lo, f_hi], tibia into its limits
// and [aneg - f, apos - f]) and the residual, with w2 the squared distance of the goal to the plane.
LRM_HD void lrm_ik_knee(const LrmIkLeg& K, float px, float pz, float phi, float w2, float f, float t, LrmIkCand& o) {
    if (f < K.fmin || f > K.fmax) {
        f = lrm_ik_clampf(f, K.fmin, K.fmax);
        float s, c;
        lrm_sincosf(f, &s, &c);
        t = lrm_ik_wrapf(lrm_atan2f(pz - K.F * s, px - K.F * c) - f);
    }
    if (t < K.tmin || t > K.tmax) {
        t = lrm_ik_clampf(t, K.tmin, K.tmax);
        float s, c;
        lrm_sincosf(t, &s, &c);
        f = lrm_ik_wrapf(phi - lrm_atan2f(K.T * s, K.F + K.T * c));
    }
    float a = f + t;
    if (a < K.aneg || a > K.apos) {
        a = lrm_ik_clampf(a, K.aneg, K.apos);
        float s, c;
        lrm_sincosf(a, &s, &c);
        f = lrm_atan2f(pz - K.T * s, px - K.T * c);
        // stay ON the absolute face where the femur or the tibia limit cuts it: the nearest point is then the corner.
        // Clamping f and t separately afterwards (below) would keep the t of the unclamped f and leave the face.
        const float flo = a - K.tmax, fhi = a - K.tmin;
        f = lrm_ik_clampf(f, (K.f_lo > flo) ? K.f_lo : flo, (K.f_hi < fhi) ? K.f_hi : fhi);
        t = a - f;
    }
    f = lrm_ik_clampf(f, K.f_lo, K.f_hi);
    const float lo = K.aneg - f, hi = K.apos - f;
    t = lrm_ik_clampf(t, (K.tmin > lo) ? K.tmin : lo, (K.tmax < hi) ? K.tmax : hi);
    t = lrm_ik_clampf(t, K.tmin, K.tmax); // rounding of aneg - f / apos - f: the tibia limit wins by an ulp of f + t
    float sf, cf, sa, ca;
    lrm_sincosf(f, &sf, &cf);
    lrm_sincosf(f + t, &sa, &ca);
    o.f = f;
    o.t = t;
    o.h = K.F * cf + K.T * ca;
    o.v = K.F * sf + K.T * sa;
    const float ex = px - o.h, ez = pz - o.v;
    o.e = lrm_sqrtf(ex * ex + ez * ez + w2);
}

// Both knees in the plane of yaw candidate `yaw` (already clamped) for the coxa-frame goal g.
LRM_HD void lrm_ik_plane(const LrmIkLeg& K, LrmVec3 g, float yaw, LrmIkCand& kp, LrmIkCand& km) {
    float sc, cc;
    lrm_sincosf(yaw, &sc, &cc);
    const float px = g.x * cc + g.y * sc - K.C;
    const float pz = g.z;
    const float w = g.y * cc - g.x * sc;
    const float w2 = w * w;
    const float r2 = px * px + pz * pz;
    // |knee| = acos((r^2 - F^2 - T^2) / 2FT) in the factored form: no cancellation near full extension
    const float k = (K.sum2 - r2) * (r2 - K.dif2);
    const float tt = lrm_atan2f(lrm_sqrtf(k > 0.f ? k : 0.f), r2 - K.ff_tt);
    const float phi = lrm_atan2f(pz, px);
    float st, ct;
    lrm_sincosf(tt, &st, &ct);
    const float beta = lrm_atan2f(K.T * st, K.F + K.T * ct);
    kp.c = km.c = yaw;
    kp.sc = km.sc = sc;
    kp.cc = km.cc = cc;
    lrm_ik_knee(K, px, pz, phi, w2, lrm_ik_wrapf(phi - beta), tt, kp);
    lrm_ik_knee(K, px, pz, phi, w2, lrm_ik_wrapf(phi + beta), -tt, km);
}

// sel = take ? cand : sel, field by field: a whole-struct conditional copy becomes a select of two stack addresses
// (scratch on the device)
LRM_HD void lrm_ik_take(const LrmIkCand& cand, bool take, LrmIkCand& sel) {
    sel.c = take ? cand.c : sel.c;
    sel.f = take ? cand.f : sel.f;
    sel.t = take ? cand.t : sel.t;
    sel.sc = take ? cand.sc : sel.sc;
    sel.cc = take ? cand.cc : sel.cc;
    sel.h = take ? cand.h : sel.h;
    sel.v = take ? cand.v : sel.v;
    sel.e = take ? cand.e : sel.e;
}

LRM_HD float lrm_ik_seed_dist(const LrmIkCand& cand, LrmVec3 seed) {
    const float dc = cand.c - seed.x, df = cand.f - seed.y, dt = cand.t - seed.z;
    return dc * dc + df * df + dt * dt;
}

// the running selection: cand replaces the current choice when it is within `lim` of the best residual and strictly
// nearer the seed (candidates are offered in candidate-number order)
LRM_HD void lrm_ik_offer(const LrmIkCand& cand, float lim, LrmVec3 seed, LrmIkCand& sel, float& sel_d) {
    const float d = lrm_ik_seed_dist(cand, seed);
    const bool take = cand.e <= lim && d < sel_d;
    lrm_ik_take(cand, take, sel);
    sel_d = take ? d : sel_d;
}

LRM_HD bool lrm_ik_finite(float v) { return (lrm_f2u(v) & 0x7f800000u) != 0x7f800000u; }

// IK of one point.  seed = (coxa, femur, tibia) (K.seed for "no seed").  Writes the angles to ang (x coxa, y femur,
// z tibia) and returns the LRM_IK_* status.
LRM_HD uint8_t lrm_ik_point(const LrmLegHead& L, const LrmCircle* lists, const LrmIkLeg& K, LrmVec3 p, LrmVec3 seed,
                            LrmVec3& ang) {
    const bool reach = lrm_reach_global(L, lists, p);
    LrmVec3 g = p;
    float dn = 0.f;
    if (!reach) { // the goal is the reference's nearest point p - d
        LrmVec3 d = p;
        (void)lrm_dist_global(L, lists, d);
        dn = lrm_norm3(d);
        g.x = p.x - d.x;
        g.y = p.y - d.y;
        g.z = p.z - d.z;
    }
    const LrmVec3 gq = lrm_ik_to_coxa(L, g);
    LrmIkCand c0, c1, c2, c3;
    lrm_ik_plane(K, gq, lrm_ik_clampf(lrm_atan2f(gq.y, gq.x), K.cmin, K.cmax), c0, c1);
    lrm_ik_plane(K, gq, lrm_ik_clampf(lrm_atan2f(-gq.y, -gq.x), K.cmin, K.cmax), c2, c3);
    float best = c0.e;
    best = (c1.e < best) ? c1.e : best;
    best = (c2.e < best) ? c2.e : best;
    best = (c3.e < best) ? c3.e : best;
    const float lim = best + LRM_IK_NEAR_F;
    // The seed only breaks ties among the near-best candidates: the choice starts from the best-residual candidate (the
    // lowest number on equal residuals) and moves only to one strictly nearer the seed.  A seed with a non-finite
    // component is no seed (the default one); a finite seed so far away that every distance overflows keeps the start.
    const bool seed_ok = lrm_ik_finite(seed.x) && lrm_ik_finite(seed.y) && lrm_ik_finite(seed.z);
    if (!seed_ok) seed = LrmVec3{K.seed[0], K.seed[1], K.seed[2]};
    LrmIkCand s = c0;
    lrm_ik_take(c1, c1.e < s.e, s);
    lrm_ik_take(c2, c2.e < s.e, s);
    lrm_ik_take(c3, c3.e < s.e, s);
    float sd = lrm_ik_seed_dist(s, seed);
    lrm_ik_offer(c0, lim, seed, s, sd);
    lrm_ik_offer(c1, lim, seed, s, sd);
    lrm_ik_offer(c2, lim, seed, s, sd);
    lrm_ik_offer(c3, lim, seed, s, sd);
    // status: the chosen tip's distance to p, in the caller's frame (where d is measured)
    const float hx = K.C + s.h;
    const LrmVec3 tip = lrm_ik_from_coxa(L, K, LrmVec3{s.cc * hx, s.sc * hx, s.v});
    const float ex = tip.x - p.x, ey = tip.y - p.y, ez = tip.z - p.z;
    const float ep = lrm_sqrtf(ex * ex + ey * ey + ez * ez);
    uint8_t st = reach ? ((ep <= LRM_IK_TOL_F) ? LRM_IK_REACHED : LRM_IK_MODEL_GAP)
                       : ((ep <= dn + (LRM_IK_TOL_F + dn * LRM_IK_REL_F)) ? LRM_IK_NEAREST : LRM_IK_FAR_GAP);
    const bool ok = lrm_ik_finite(p.x) && lrm_ik_finite(p.y) && lrm_ik_finite(p.z) && lrm_ik_finite(s.c) &&
                    lrm_ik_finite(s.f) && lrm_ik_finite(s.t);
    if (!ok) {
        st = LRM_IK_NONE;
        s.c = s.f = s.t = __builtin_nanf("");
    }
    ang = LrmVec3{s.c, s.f, s.t};
    return st;
}

#if defined(__HIPCC__)
// launch functions (lrm_ik.hip): SoA in and out, `seed_*` null or all three set; only launch
hipError_t lrm_launch_ik(const float* x, const float* y, const float* z, size_t n, const LrmCompiledLeg& L, const LrmIkLeg& K,
                         const float* seed_c, const float* seed_f, const float* seed_t, float* coxa, float* femur, float* tibia,
                         uint8_t* status, hipStream_t st);
hipError_t lrm_launch_fk(const float* coxa, const float* femur, const float* tibia, size_t n, const LrmCompiledLeg& L,
                         const LrmIkLeg& K, float* x, float* y, float* z, hipStream_t st);
#endif
