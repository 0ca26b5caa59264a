/*
 * lrm.h -- C ABI of liblrm.so: the MI355X (gfx950) implementation of the batched 3-DoF
 * (yaw-pitch-pitch) leg reachability / distance path and of the body x target
 * positionability aggregation.
 *
 * Every entry point names the interface of the reference (2lian/Legged-Robot-Movability-Cuda,
 * paths relative to its root) that it replaces.  Plain pointers and sizes only.
 * All functions returning `int` return 0 on success and a negative LRM_E* code on failure;
 * lrm_last_error() then holds a message.  Nothing here ever computes a GPU entry point on
 * the CPU: without a usable HIP device the *_dev / host-buffer GPU calls fail with LRM_ENODEV.
 *
 * Threading.  Streams: the *_dev entry points may be queued on several streams.  Device workspaces (bounding boxes and
 * compiled-leg slots of the pair kernels, doubt queues of LRM_MODE_TOL) are kept per device -- the doubt queues per
 * (device, stream) -- created on first use and reused; a compiled-leg slot is only rewritten after the launch that read
 * it has completed (an event per slot).  The bounding boxes of the pair kernels are one buffer per device: do not run
 * two pair launches on different clouds concurrently on one device.
 * Host threads: these calls may overlap from several threads: the distance and fused calls in every mode, on device or
 * host buffers (host-buffer calls through LRM_HOST_PIPELINE=1 run one at a time), lrm_tol_prepare, lrm_apply_oct* and
 * lrm_dbg_toltab_build (the caches of compiled tables are locked; one device table build runs at a time).  lrm_set_mode
 * is process-wide: a switch in one thread changes the next call of every thread.  The pair kernels (lrm_reach_any_dev,
 * lrm_footholds_dev, lrm_footholds_posed_dev, lrm_foothold_lists_posed_dev, lrm_foothold_edges_posed_dev, lrm_foothold_misses_posed_dev, lrm_body_clearance_posed_dev, lrm_swing_transit_posed_dev (with a foot radius), lrm_positionability*, lrm_any_in_sphere_dev, lrm_any_in_cylinder_dev) share unlocked per-device pools, and
 * lrm_reach_dist_multi its unlocked communicators: call them from one host thread at a time.  lrm_release_workspaces
 * must not overlap any other call.
 * A captured graph that uses a plane table stays valid only while that (leg, orientation) is in the 64-entry table cache
 * and until lrm_release_workspaces.
 *
 * Units: millimetres and radians, float32 arithmetic (reference convention).
 * Quaternions are float[4] = {x,y,z,w} in the reference's own (inconsistent) convention:
 * qtRotate/qtInvert read [0] as the scalar part (identity = {1,0,0,0}, settings.h:51).
 */
#ifndef LRM_H
#define LRM_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LRM_OK 0
#define LRM_EINVAL (-1) /* bad argument (null pointer, length mismatch, too many legs...) */
#define LRM_ENODEV (-2) /* no HIP device / HIP runtime error                               */
#define LRM_ENOMEM (-3) /* device or host allocation failed                               */

/* Arithmetic mode of the GPU kernels.
 * LRM_MODE_STRICT: reference operation order, no FMA contraction, glibc-exact atan2f/sincosf:
 *                  bit-identical to the reference's host path (reachability_kernel_cpu /
 *                  distance_kernel_cpu, one_leg_global.cu:132-147).
 * LRM_MODE_FAST:   the same outputs, bit for bit, faster.  Clouds of >= 2e5 points on legs with a plane table:
 *                  csrc/lrm_point_xtab.h -- every DECISION (clamp target, validity, which yaw candidate) comes
 *                  from the plane table of the tolerance mode with its error bands, every VALUE from the
 *                  reference's own operations in its own order (one exact atan2f, one exact sincosf and one strict
 *                  clamp per evaluated candidate); a point with a decision inside its band is re-evaluated by the
 *                  filtered code in a second small launch.  Otherwise the filtered evaluation
 *                  (csrc/lrm_point_fast.h): decisions with cheap arithmetic plus conservative bands, values that
 *                  reach an output with the strict arithmetic, a decision inside its band re-taken by the strict
 *                  code.  Legs outside the filter's eligibility silently use the strict kernels. */
#define LRM_MODE_STRICT 0
#define LRM_MODE_FAST 1
/* LRM_MODE_TOL:    contract-tolerance mode (csrc/lrm_point_tol.h): the reach mask and the distance's
 *                  validity byte stay bit-identical to LRM_MODE_STRICT; the distance VECTOR is computed with
 *                  FP32 FMA / v_rsq_f32 arithmetic (no atan2f / sincosf / IEEE sqrt) and lands on the same
 *                  boundary feature as the reference's, with the error bound (FROZEN, tests/tolcheck.py)
 *                      |d - d_ref| <= 1e-5 * max(|d_ref|, (|p| + body) / 8)      per point.
 *                  This is a floored reading of "within 1e-5 relative" (BASELINE.json): literally relative for
 *                  every vector longer than 1/8 of the coordinate scale, an absolute bound of about 10 ulp of
 *                  the coordinates (~1e-3 mm at most; measured <= 3e-4 mm) below.  Why a floor: d is a difference
 *                  of float32 positions the reference itself forms after `x -= body` (one_leg.cu:13), so it
 *                  carries ~1e-4 mm of rounding noise in ANY float32 implementation, the reference's own
 *                  -use_fast_math CUDA build included; a purely relative bound is unattainable for
 *                  |d| << 10 mm.  The literal bound |d - d_ref| <= 1e-5 |d_ref| holds for every vector of at
 *                  least 16 mm (asserted on the GPU); the fraction of shorter vectors that miss it is reported by
 *                  bench.py ("tolerance_check").  Callers that need the literal text use LRM_MODE_TOL_REL (below) or LRM_MODE_FAST (tolerance 0).
 *                  Points with any decision inside its error band are re-evaluated by the LRM_MODE_FAST code in a
 *                  second small launch and are bit-identical.  Applies to the distance / fused entry points, host
 *                  buffers (lrm_dist, lrm_reach_dist: the apply_kernel boundary) and device buffers alike;
 *                  reach-only and pair kernels run as in LRM_MODE_FAST.  Legs outside the mode's eligibility use
 *                  LRM_MODE_FAST. */
#define LRM_MODE_TOL 2
/* LRM_MODE_TOL_REL: LRM_MODE_TOL with the LITERAL bound of BASELINE.json on every vector: reach mask and validity byte
 *                  bit-identical, |d - d_ref| <= 1e-5 |d_ref| for every point.  A vector that comes out shorter than
 *                  max(19 mm, 0.034 (|p|_1 + body)) -- the absolute error of the tolerance arithmetic grows with the coordinates --
 *                  has its value chain recomputed with the reference's own operations from the decisions the tolerance
 *                  evaluation took (csrc/lrm_point_xtab.h: lrm_xtab_replay, inside the same kernel: bit-identical, relative
 *                  error 0).  Every longer vector is within 1e-5 relative by LRM_MODE_TOL's own arithmetic (measured 7.6e-6 at
 *                  most, at 17.55 mm under the first threshold of 17 mm; asserted: tests/test_gpu_tol.py).  About 5 % of a cloud filling the leg's bounding cube
 *                  is replayed (+ the 0.5 % of doubtful points of LRM_MODE_TOL through the fix-up launch); a cloud that hugs the
 *                  workspace's surface is replayed whole and runs at about half the speed.  The bench headline. */
#define LRM_MODE_TOL_REL 3

/* LegDimensions, HeaderCPP.h:19-52: 14 x f32 = 56 bytes, this field order. */
typedef struct LrmLegDimensions {
    float body_angle;
    float body;
    float coxa_pitch;
    float coxa_length;
    float tibia_length;
    float femur_length;
    float tibia_absolute_pos;
    float tibia_absolute_neg;
    float max_angle_coxa;
    float min_angle_coxa;
    float max_angle_tibia;
    float min_angle_tibia;
    float max_angle_femur;
    float min_angle_femur;
} LrmLegDimensions;

/* ---- library state ------------------------------------------------------------------ */
const char* lrm_version(void);
const char* lrm_last_error(void);
int lrm_device_count(void);          /* number of HIP devices, 0 if none (never fails)      */
int lrm_set_device(int ordinal);     /* cudaSetDevice analogue; the reference uses device 0 */
int lrm_set_mode(int mode);          /* LRM_MODE_*; process-wide; default LRM_MODE_FAST     */
int lrm_get_mode(void);

/* ---- leg factories: static_variables.cpp:6-93 ---------------------------------------- */
void lrm_leg_factory(float azimut, float body2coxa, float coxa_pitch_deg, float coxa2tibia,
                     float tibia2femur, float femur2tip, float coxa_angle_deg,
                     float femur_angle_deg, float tibia_angle_deg, float tib_abs_pos,
                     float tib_abs_neg, LrmLegDimensions* out);
void lrm_get_M2_leg(float azimut, LrmLegDimensions* out);      /* static_variables.cpp:69-93 */
void lrm_get_moonbot_leg(float azimut, LrmLegDimensions* out); /* static_variables.cpp:44-67 */

/* rotate_leg_data, one_leg_global.cu:48-60 (host helper; also several_leg.cu:743-760) */
void lrm_rotate_leg_data(const float quat[4], const LrmLegDimensions* leg, LrmLegDimensions* out);

/* ---- host-buffer drop-ins ------------------------------------------------------------
 * Replace apply_kernel<float3,LegDimensions,bool|float3> (cross_compiled.cu:33-79) for the
 * kernels reachability_global_kernel / distance_global_kernel (one_leg_global.cu:149-166):
 * device buffers are allocated and freed inside the call, input is copied H2D, a warm-up
 * launch runs, the kernel alone is timed with events, results are copied D2H.
 * xyz is AoS float3 (12-byte stride), mask is one byte per point (C++ bool), *ms receives
 * the kernel-only milliseconds.  `quat` = NULL means the reference's quatTest {1,0,0,0}. */
int lrm_reach(const float* xyz_aos, size_t n, const LrmLegDimensions* leg, const float* quat,
              uint8_t* mask_out, float* ms);
int lrm_dist(const float* xyz_aos, size_t n, const LrmLegDimensions* leg, const float* quat,
             float* dxyz_aos_out, uint8_t* valid_out /* may be NULL */, float* ms);
/* one launch producing both outputs (mask is reachability_global's, not distance's bool) */
int lrm_reach_dist(const float* xyz_aos, size_t n, const LrmLegDimensions* leg, const float* quat,
                   uint8_t* mask_out, float* dxyz_aos_out, float* ms);

/* Host buffers in the reference's on-disk layout: one f32 array per component, as
 * dist_input_t{x,y,z}.bin / out_dist_x{x,y,z}.bin (several_leg.cpp:126-131, :201-219,
 * math_util.cpp:46-89).  Same semantics as lrm_reach / lrm_dist without the AoS detour. */
int lrm_reach_soa(const float* x, const float* y, const float* z, size_t n, const LrmLegDimensions* leg,
                  const float* quat, uint8_t* mask_out, float* ms);
int lrm_dist_soa(const float* x, const float* y, const float* z, size_t n, const LrmLegDimensions* leg,
                 const float* quat, float* dx, float* dy, float* dz, uint8_t* valid_out /* may be NULL */,
                 float* ms);

/* ---- CPU path: apply_reach_cpu / apply_dist_cpu, cross_compiled.cu:163-181 -------------
 * Single-threaded host loops over the same per-point code the kernels run (the reference
 * compiles one `__host__ __device__` source twice in the same way).  These are explicit CPU
 * entry points of the reference API, never a fallback for the GPU ones. */
int lrm_reach_cpu(const float* xyz_aos, size_t n, const LrmLegDimensions* leg, const float* quat,
                  uint8_t* mask_out, double* ms);
int lrm_dist_cpu(const float* xyz_aos, size_t n, const LrmLegDimensions* leg, const float* quat,
                 float* dxyz_aos_out, uint8_t* valid_out /* may be NULL */, double* ms);

/* ---- "RBDL-equivalent" CPU baseline: apply_RBDL, rbdl_benchmark.cpp:18-111 / RBDL_benchmark.h:5 ------
 * The reference times RBDL's Levenberg-Marquardt position IK on the same targets (bench.cpp:158, 3 repeats,
 * setting_bench.h:7).  RBDL is an external, unpinned dependency that is absent here: this is the same iteration
 * (same chain incl. the /400 scaling, max_steps = 10, <= 5 starts) with closed-form kinematics.  PARITY UNPINNED:
 * a timing baseline only; mask_out[i] = the solver converged (no joint limits, no coxa pitch, as the
 * reference's RBDL model).  *ms = chrono milliseconds of the loop. */
int lrm_rbdl_equiv_cpu(const float* xyz_aos, size_t n, const LrmLegDimensions* leg, uint8_t* mask_out, double* ms);

/* ---- device-resident entry points (launch only: no copy of the clouds, the caller synchronises) ----
 * Pointers are device pointers; coordinates are SoA (one f32 array per component: the same
 * layout the reference keeps on disk, several_leg.cpp:126-131).  `stream` is a hipStream_t
 * (NULL = default stream).  `n` need not be a multiple of anything; 16-byte aligned arrays
 * (hipMalloc / torch allocations are) take the vectorised kernels, anything else a scalar
 * variant with identical results.
 * LRM_MODE_STRICT / LRM_MODE_FAST: nothing but the launch (no allocation, no host synchronisation).
 * LRM_MODE_TOL (distance / fused calls): the first call for a (leg, orientation) compiles the mode's tables on the
 * host (~0.3 ms) and builds the plane table for clouds of >= 2e5 points on the device (< 1 ms on the call's stream, one small
 * read-back; LRM_TOLTAB_HOST=1: the host builder, ~30 ms), and allocates the doubt
 * queues of this (device, stream); a later call with a larger n regrows the queues (hipFree + hipMalloc: a device-wide
 * synchronisation).  lrm_tol_prepare does all of that ahead of time, after which the calls only launch -- graph
 * capture and latency-critical loops call it first.  Invariant: the queue words it reserves for n_max are at least what
 * any distance / fused call on n <= n_max points of the same (device, stream) requests, in every mode, with or without the
 * plane table (lrm_dbg_tol_grid reports both; the launch grids are not monotone in n, the requested words are).  The
 * table cache holds 64 (leg, orientation) pairs, least recently used out.  lrm_release_workspaces frees every cached device buffer (queues, tables, the device
 * table builder's scratch, the octree's tables, the pair kernels' boxes and leg slots, the host pipeline's buffers and streams,
 * the multi-device communicators); the next call re-creates what it needs. */
int lrm_tol_prepare(const LrmLegDimensions* leg, const float* quat, size_t n_max, void* stream);
/* Milliseconds the most recent plane-table build of this process took (the table of a (leg, orientation) is built by the first
 * call that needs it, or by lrm_tol_prepare, and cached); -1 when none has been built yet.  bench.py reports it as
 * config.table_build_ms next to ms_per_step. */
int lrm_tol_table_build_ms(float* ms_out);
void lrm_release_workspaces(void);
int lrm_reach_dev(const float* x, const float* y, const float* z, size_t n,
                  const LrmLegDimensions* leg, const float* quat, uint8_t* mask, void* stream);
/* as lrm_reach_dev, plus a wave-ballot bit mask: bit (i & 63) of bits[i >> 6]
 * (ceil(n/64) words; either output may be NULL) */
int lrm_reach_bits_dev(const float* x, const float* y, const float* z, size_t n,
                       const LrmLegDimensions* leg, const float* quat, uint8_t* mask,
                       uint64_t* bits, void* stream);
int lrm_dist_dev(const float* x, const float* y, const float* z, size_t n,
                 const LrmLegDimensions* leg, const float* quat, float* dx, float* dy, float* dz,
                 uint8_t* valid /* may be NULL */, void* stream);
int lrm_reach_dist_dev(const float* x, const float* y, const float* z, size_t n,
                       const LrmLegDimensions* leg, const float* quat, uint8_t* mask, float* dx,
                       float* dy, float* dz, void* stream);
/* as lrm_reach_dist_dev, plus the wave-ballot bit mask of the reach mask (the shard payload
 * of the multi-GPU gather); either mask output may be NULL */
int lrm_reach_dist_bits_dev(const float* x, const float* y, const float* z, size_t n,
                            const LrmLegDimensions* leg, const float* quat, uint8_t* mask,
                            uint64_t* bits, float* dx, float* dy, float* dz, void* stream);
/* AoS device variants (what apply_kernel launches on its device copies) */
int lrm_reach_aos_dev(const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat,
                      uint8_t* mask, void* stream);
int lrm_dist_aos_dev(const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat,
                     float* dxyz, uint8_t* valid /* may be NULL */, void* stream);

/* ---- batched multi-pose queries: N (target, pose, leg) queries in one launch -------------------------------------
 * A pose table quats[nposes][4] (the convention of every `quat` argument above), optionally body[nposes][3], and a leg
 * table legs[nlegs] (nlegs <= LRM_MAX_LEGS, plain legs: rotate_leg_data is applied per pose, as the single-pose calls
 * do).  Query i has the target (x[i], y[i], z[i]), the pose pose_idx[i] and the leg leg_idx[i]; with
 * p = target - body[pose] (f32, component by component; no subtraction when body is NULL):
 *   mask[i]  = reachability_global(p, legs[leg], quats[pose]);
 *   valid[i], (dx, dy, dz)[i] = distance_global(p, legs[leg], quats[pose]).
 * Every byte and every float equals what lrm_reach_dist_dev / lrm_dist_dev return in LRM_MODE_STRICT for that
 * single (leg, quat) on p, whatever lrm_set_mode says: the tolerance modes need a plane table per (leg, orientation)
 * and do not apply to posed queries.  pose_idx == NULL: pose 0 for every query; leg_idx == NULL: leg 0.  A query
 * with an index out of range (pose_idx < 0 or >= nposes, leg_idx >= nlegs) gets mask 0, valid 0 and a nan field.
 * Any of mask / valid / the field (dx, dy, dz: all three or none) may be NULL; with valid and the field NULL only
 * the reach evaluation runs.
 * The workspace (lrm_posed_workspace_bytes, 16-byte aligned device memory) belongs to the caller: one record per
 * (pose, leg), written by lrm_pose_compile_dev on the call's stream from device-resident quaternions and body
 * positions, read by lrm_reach_dist_posed_dev with the same nposes and nlegs.  Both calls only launch (no
 * allocation, no host synchronisation): they can be captured in a graph and replayed with new poses. */
size_t lrm_posed_workspace_bytes(size_t nposes, size_t nlegs);
int lrm_pose_compile_dev(const float* quats /* device, nposes x 4 */, const float* body /* device, nposes x 3, may be NULL */,
                         size_t nposes, const LrmLegDimensions* legs /* host */, size_t nlegs, void* workspace, void* stream);
int lrm_reach_dist_posed_dev(const float* x, const float* y, const float* z, size_t n, const int32_t* pose_idx,
                             const uint8_t* leg_idx, const void* workspace, size_t nposes, size_t nlegs, uint8_t* mask,
                             uint8_t* valid, float* dx, float* dy, float* dz, void* stream);
/* The same queries on the host (xyz and the field AoS float3, host quats / body): a serial loop over the same
 * per-point code, the same out-of-range rule.  *ms = chrono milliseconds of the loop (the records' compile excluded). */
int lrm_reach_dist_posed_cpu(const float* xyz_aos, size_t n, const int32_t* pose_idx, const uint8_t* leg_idx,
                             const float* quats, const float* body, size_t nposes, const LrmLegDimensions* legs,
                             size_t nlegs, uint8_t* mask, uint8_t* valid, float* dxyz_aos, double* ms);

/* ---- joint angles: inverse / forward kinematics of the leg ----------------------------------------------------------
 * The reference answers "reachable?" and "how far?" without joint angles; its only IK is the RBDL benchmark
 * (lrm_rbdl_equiv_cpu: no angles, no limits, no coxa pitch) and its forward_kine_kernel (one_leg.cu:377-414) ignores
 * the coxa pitch.  These calls give the angles (coxa yaw, femur, tibia; radians, the reference's forward_kinematics
 * convention) that put the tip on p, or as near to it as the joint limits allow.
 * Frame chain as distance_global: p -> qtInvRotate(quat) -> rotate by -body_angle -> x -= body -> rotate by
 * -coxa_pitch.  Limits: those of rotate_leg_data(quat, leg): coxa in [min, max], femur in [min, max], tibia in
 * [min, max], femur + tibia in [tibia_absolute_neg, tibia_absolute_pos].  Every returned angle lies within its limits
 * (femur + tibia up to the rounding of one float addition), whatever the status.
 * Goal: p when reachability_global(p), else p - d with d = distance_global(p) (the strict evaluation, whatever
 * lrm_set_mode says).  Of the analytic candidates (yaw direct and mirrored, two knees each, clamped into the limits;
 * csrc/lrm_ik.h) those within 1e-3 mm of the nearest to the goal compete on the distance to the seed (sum of squared
 * joint differences; ties: the best-residual candidate first, then direct yaw before mirrored, knee >= 0 before
 * knee <= 0).  Seed: per point, optional (all three arrays or none); without one, the mid-range of each joint's limits.
 * The seed only breaks ties among those near-best candidates, so it never changes a status: a seed with a nan or inf
 * component counts as no seed (e.g. a previous frame's output where its status was 0), and a finite seed so far away
 * that its distances overflow keeps the best-residual candidate.
 * Quaternion: the statuses assume a unit quaternion (|q| = 1 to float32 rounding).  The reference does not normalise;
 * for a non-unit q, qtRotate(q, .) is not the inverse of qtInvRotate(q, .), distance_global's d is then not the
 * displacement to its nearest point, and status 4 appears at scale.  Normalise before calling.
 * status[i]:
 *   LRM_IK_REACHED   1  reachable (mask 1); the tip is within 2e-3 mm of p
 *   LRM_IK_NEAREST   2  not reachable (mask 0); the tip is at most |d| + 2e-3 mm (+ 2^-22 |d|, the float32
 *                       resolution of |d|: 1.2e-4 mm at 500 mm) from p
 *   LRM_IK_MODEL_GAP 3  mask 1, but no candidate is within 2e-3 mm of p: the circle model calls p reachable where the
 *                       joint limits do not reach; the angles are the best in-limit candidate
 *   LRM_IK_FAR_GAP   4  mask 0, and the best in-limit candidate aimed at p - d is further than that from p (with a unit
 *                       quaternion; see above); the angles are that candidate
 *   LRM_IK_NONE      0  non-finite input (or coordinates beyond ~1e18 mm, where float32 overflows): nan angles
 * Where 3 and 4 occur and what they claim (tests/test_ik_boundary_cpu.py against a float64 search of the limit set):
 * they are reported only where no in-limit tip lies within 1e-3 mm of p.  On the M2 and moonbot legs they occur only
 * within about 1e-2 mm outside a limit face: the circle model's margin calls such a p reachable (3), or puts p - d
 * outside the limit set (4); the returned tip is then the nearest in-limit one to float32 rounding.  Legs of other
 * proportions get them at scale, and there the returned tip need not be the nearest.  Status 4 does not promise that no in-limit configuration is
 * nearer than |d|: where a rotated limit passes +-pi the limit set holds configurations the circle model does not,
 * and an in-limit tip can be nearer than |d| (by 29 mm on the test leg random10).
 * So status in {1, 3} <=> reachability_global's mask.  Decided in float32; the device entry points equal the CPU ones
 * bit for bit (angles, status bytes, FK positions).
 * lrm_fk_*: the tip of (coxa, femur, tibia) in the caller's frame, the exact inverse of the chain above (the
 * reference's forward_kinematics plus coxa pitch, body_angle and quat).
 * *_dev: device pointers, SoA, only launch (no allocation, no host synchronisation: graph-capturable); `stream` a
 * hipStream_t.  *_cpu: AoS float3 (angles {coxa, femur, tibia} per point), serial host loops, *ms = their chrono
 * milliseconds. */
#define LRM_IK_NONE 0
#define LRM_IK_REACHED 1
#define LRM_IK_NEAREST 2
#define LRM_IK_MODEL_GAP 3
#define LRM_IK_FAR_GAP 4
int lrm_ik_dev(const float* x, const float* y, const float* z, size_t n, const LrmLegDimensions* leg, const float* quat,
               const float* seed_c, const float* seed_f, const float* seed_t /* each may be NULL: all or none */,
               float* coxa, float* femur, float* tibia, uint8_t* status, void* stream);
int lrm_fk_dev(const float* coxa, const float* femur, const float* tibia, size_t n, const LrmLegDimensions* leg,
               const float* quat, float* x, float* y, float* z, void* stream);
int lrm_ik_cpu(const float* xyz_aos, size_t n, const LrmLegDimensions* leg, const float* quat,
               const float* seed_aos /* may be NULL */, float* angles_aos, uint8_t* status, double* ms);
int lrm_fk_cpu(const float* angles_aos, size_t n, const LrmLegDimensions* leg, const float* quat, float* xyz_aos,
               double* ms);

/* ---- joint angles per (target, pose, leg): the last step after lrm_footholds_dev ------------------------------------
 * The pose and leg tables of the batched multi-pose queries above, plus a second caller-owned device table of the IK
 * constants: lrm_posed_ik_workspace_bytes (128 B per (pose, leg), 16-byte aligned), written by lrm_pose_ik_compile_dev
 * from the same device-resident quaternions and host legs as lrm_pose_compile_dev, entry of (pose, leg) at
 * pose * nlegs + leg.  Both tables must be compiled for the same nposes and nlegs before a query reads them.
 * lrm_ik_posed_dev: query i takes target target_idx[i] of the nt targets (x, y, z); with target_idx NULL it takes
 * target i, and n > nt is LRM_EINVAL.  p = target - body[pose_idx[i]] (one float32 subtraction per component, as
 * lrm_reach_dist_posed_dev; body as given to lrm_pose_compile_dev).  Angles and status are those of
 * lrm_ik_cpu(p, legs[leg_idx[i]], quats[pose_idx[i]], seed i), bit for bit: same goal, candidates, tie rules, seed
 * rules (seed_c / seed_f / seed_t: all or none, one entry per QUERY) and status thresholds.  pose_idx NULL: pose 0;
 * leg_idx NULL: leg 0.  A query whose pose, leg or target index is out of range (a negative target_idx, such as the -1
 * lrm_footholds_dev writes where nothing is reachable, included) gets status LRM_IK_NONE and nan angles; the kernel
 * clamps every index before it loads and never reads outside its tables.  So best_out of lrm_footholds_dev is a valid
 * target_idx as it stands: with pose_idx[l*nb + b] = b and leg_idx[l*nb + b] = l, one pose per body holding the body
 * position, and the quaternion and legs of that call's frame convention, one launch gives the angles
 * of every chosen foothold.
 * lrm_fk_posed_dev: lrm_fk_dev's tip for (legs[leg], quats[pose]) + body[pose] (one float32 add per component); an
 * out-of-range pose or leg index gives a nan position.
 * All three *_dev calls only launch (no allocation, no host synchronisation: graph-capturable) and do not depend on
 * lrm_set_mode.  *_cpu: the same queries as serial host loops over the same per-point code (AoS float3 targets, seeds,
 * angles and positions; host quats / body, body may be NULL), the same out-of-range rule; *ms = the loop's chrono
 * milliseconds, the tables' compile excluded. */
size_t lrm_posed_ik_workspace_bytes(size_t nposes, size_t nlegs);
int lrm_pose_ik_compile_dev(const float* quats /* device, nposes x 4 */, size_t nposes, const LrmLegDimensions* legs /* host */,
                            size_t nlegs, void* ik_workspace, void* stream);
int lrm_ik_posed_dev(const float* x, const float* y, const float* z, size_t nt,
                     const int32_t* target_idx /* may be NULL */, size_t n,
                     const int32_t* pose_idx, const uint8_t* leg_idx,
                     const void* workspace, const void* ik_workspace, size_t nposes, size_t nlegs,
                     const float* seed_c, const float* seed_f, const float* seed_t /* all or none */,
                     float* coxa, float* femur, float* tibia, uint8_t* status, void* stream);
int lrm_fk_posed_dev(const float* coxa, const float* femur, const float* tibia, size_t n,
                     const int32_t* pose_idx, const uint8_t* leg_idx,
                     const void* workspace, const void* ik_workspace, size_t nposes, size_t nlegs,
                     float* x, float* y, float* z, void* stream);
int lrm_ik_posed_cpu(const float* xyz_aos, size_t nt, const int32_t* target_idx, size_t n, const int32_t* pose_idx,
                     const uint8_t* leg_idx, const float* quats, const float* body, size_t nposes,
                     const LrmLegDimensions* legs, size_t nlegs, const float* seed_aos, float* angles_aos,
                     uint8_t* status, double* ms);
int lrm_fk_posed_cpu(const float* angles_aos, size_t n, const int32_t* pose_idx, const uint8_t* leg_idx,
                     const float* quats, const float* body, size_t nposes, const LrmLegDimensions* legs, size_t nlegs,
                     float* xyz_aos, double* ms);

/* ---- body x target aggregation ---------------------------------------------------------
 * Replaces reach_mem_kernel + launch_opti_mem_reach_kernel (several_leg.cu:92-192) for all
 * legs in ONE launch: out[l*nb + b] = 1 iff some target t satisfies
 * reachable_rotate_leg(t, body b, quat, legs[l]) (several_leg.cu:48-67); otherwise 0 (the
 * whole output is written).  `legs` are used as given (several_leg.cu:743-760 rotates the
 * limits on the host before the launch: use lrm_rotate_leg_data for that).
 * If all_legs_out != NULL it receives the AND over legs per body (agregateReachability,
 * several_leg.cu:681-697, generalised from 4 to nlegs legs). nlegs <= LRM_MAX_LEGS. */
#define LRM_MAX_LEGS 8
int lrm_reach_any_dev(const float* bx, const float* by, const float* bz, size_t nb,
                      const float* tx, const float* ty, const float* tz, size_t nt,
                      const LrmLegDimensions* legs, size_t nlegs, const float* quat,
                      uint8_t* out_leg_body, uint8_t* all_legs_out, void* stream);
/* Per-leg foothold counts and choice, the step between lrm_reach_any_dev and lrm_ik_dev.  Bodies, targets, legs and quat
 * as in lrm_reach_any_dev; pair (b, t, l) is reachable iff reachable_rotate_leg(t, body b, quat, legs[l]).  Every output
 * has nlegs * nb entries at [l*nb + b], all written:
 *   count_out    the number of reachable targets;
 *   best_out     the index of the reachable target with the smallest d2 to the leg's nominal point (ties: the smaller
 *                index), -1 when count is 0;
 *   best_d2_out  (may be NULL) that d2, +inf when count is 0.
 * d2 in float32 without contraction (host and device agree bit for bit): c = body + nominal[l] (one add per component),
 * d = target - c, d2 = (dx*dx + dy*dy) + dz*dz.  nominal: host, nlegs x 3, an offset from the body in the clouds' frame
 * (the leg's neutral foot position, already rotated by the pose); NULL = all zero (nearest the body centre).
 * nt > INT32_MAX or nlegs outside 1..LRM_MAX_LEGS: LRM_EINVAL, checked first; then nb == 0 is a no-op.  The answers do
 * not depend on lrm_set_mode.  lrm_footholds_cpu: AoS float3 clouds, a serial host loop over every (body, leg, target)
 * with the strict test and no culling (the reference the GPU tests compare with); *ms = the loop's time. */
int lrm_footholds_dev(const float* bx, const float* by, const float* bz, size_t nb,
                      const float* tx, const float* ty, const float* tz, size_t nt,
                      const LrmLegDimensions* legs, size_t nlegs, const float* quat,
                      const float* nominal, int32_t* count_out, int32_t* best_out, float* best_d2_out, void* stream);
int lrm_footholds_cpu(const float* bodies_aos, size_t nb, const float* targets_aos, size_t nt,
                      const LrmLegDimensions* legs, size_t nlegs, const float* quat, const float* nominal,
                      int32_t* count_out, int32_t* best_out, float* best_d2_out, double* ms);
/* Foothold counts and choice per (pose, leg) of a pose table: lrm_footholds_dev for bodies that each have their own
 * orientation, with the semantics of the posed calls, so that ONE pose table serves pose compile -> footholds -> IK.
 * The pose table, the leg table and `workspace` are those of lrm_pose_compile_dev.  Pair (pose p, leg l, target t) is
 * reachable iff reachability_global(t - body[p], legs[l], quats[p]) (one float32 subtraction per component): the mask
 * of lrm_reach_dist_posed_cpu, the strict arithmetic whatever lrm_set_mode says.  There is no gravity gate
 * (reachability_global has none), and the legs are used as given: rotate_leg_data happens per pose inside.
 * A third caller-owned device table, lrm_posed_footholds_workspace_bytes (LRM_POSE_FOOTHOLD_BYTES = 32 per (pose, leg),
 * 16-byte aligned), entry of (pose, leg) at pose * nlegs + leg, eight floats:
 *   cull_center[3], cull_r2   a sphere, in the caller's frame relative to body[p], around everything leg l can reach
 *                             under pose p.  Centre 0 and r2 = +inf (a sphere that excludes nothing) when |q|^2 is not 1
 *                             within 1e-5 -- the reference does not normalise, a non-unit, nan or inf q makes qtInvRotate
 *                             something else than a rotation -- or when the leg's numbers are not finite.  It never
 *                             excludes a pair the strict test accepts; with +inf every target of the cloud is tested
 *                             for that pose (nt x nlegs strict tests: one such pose in a large table becomes the
 *                             launch's tail).  Normalise the quaternions before the compile.
 *   nominal_w[3]              nominal[l] (host, nlegs x 3, an offset from the body in the BODY frame; NULL = 0) taken to
 *                             the caller's frame by qtRotate(quats[p], .), the inverse of the rotation
 *                             reachability_global applies to t - body (float32, no contraction)
 *                             A zero nominal gives exactly 0 for every quaternion; otherwise a nan or inf quaternion
 *                             gives nan (one bit pattern), and such a pose reaches nothing.
 *   pad                       0
 * lrm_pose_footholds_compile_dev writes it from the device-resident quaternions lrm_pose_compile_dev reads; it only
 * launches.  lrm_footholds_posed_dev: every output has nlegs * nposes entries at [l*nposes + p], all written:
 *   count_out     the number of reachable targets;
 *   best_out      the reachable target with the smallest d2 (ties: the smaller index), -1 when count is 0;
 *   best_d2_out   (may be NULL) that d2, +inf when count is 0; with c = body[p] + nominal_w (one add per component),
 *                 d = t - c, d2 = (dx*dx + dy*dy) + dz*dz in float32 without contraction, as lrm_footholds_dev;
 *   all_legs_out  (may be NULL, nposes) 1 iff every leg of the pose has count > 0.
 * best_out is a valid target_idx of lrm_ik_posed_dev on the same tables with pose_idx[l*nposes + p] = p and
 * leg_idx[l*nposes + p] = l.  Checked first: nt > INT32_MAX, nlegs outside 1..LRM_MAX_LEGS, nposes > INT32_MAX or more than
 * 2^32 - 1 records give LRM_EINVAL; then nposes == 0 is a no-op; nt == 0 gives count 0, best -1, d2 +inf everywhere.
 * Both tables must have been compiled for the same nposes and nlegs.
 * Threading and streams: lrm_footholds_posed_dev is one of the pair kernels.  It uses their per-device tile-box buffer
 * (clouds of 4096 targets or more) and inherits lrm_footholds_dev's rules: one host thread at a time, and no two pair
 * launches on different clouds concurrently on one device.  The first call for a larger cloud than the buffer holds
 * allocates (not capturable in a graph); every later call only launches, so after one call on a cloud of the largest
 * size both compiles and the query can be captured and replayed with new poses.  Below 4096 targets it always only
 * launches.  It does not use the compiled-leg slots.
 * lrm_footholds_posed_cpu: AoS float3 targets, host quats / body (body may be NULL: 0), a serial loop over every
 * (pose, leg, target) with the strict test and no culling: the reference the GPU tests compare with bit for bit;
 * *ms = the loop's time. */
#define LRM_POSE_FOOTHOLD_BYTES 32
size_t lrm_posed_footholds_workspace_bytes(size_t nposes, size_t nlegs);
int lrm_pose_footholds_compile_dev(const float* quats /* device, nposes x 4 */, size_t nposes, const LrmLegDimensions* legs /* host */,
                                   size_t nlegs, const float* nominal /* host, nlegs x 3, BODY frame, NULL = 0 */,
                                   void* fh_workspace, void* stream);
int lrm_footholds_posed_dev(const float* tx, const float* ty, const float* tz, size_t nt,
                            const void* workspace, const void* fh_workspace, size_t nposes, size_t nlegs,
                            int32_t* count_out, int32_t* best_out, float* best_d2_out /* may be NULL */,
                            uint8_t* all_legs_out /* may be NULL, nposes */, void* stream);
int lrm_footholds_posed_cpu(const float* targets_aos, size_t nt, const float* quats, const float* body, size_t nposes,
                            const LrmLegDimensions* legs, size_t nlegs, const float* nominal, int32_t* count_out,
                            int32_t* best_out, float* best_d2_out, uint8_t* all_legs_out, double* ms);
/* Reachable-foothold LISTS per (pose, leg) in CSR form: the set lrm_footholds_posed_dev counts, written out.  Pose
 * table, leg table, `workspace` and `fh_workspace` are those of lrm_footholds_posed_dev, and a pair (p, l, t) is
 * reachable under the same rule (strict reachability_global(t - body[p], legs[l], quats[p]), whatever lrm_set_mode
 * says).  The two-step CSR: count_out of lrm_footholds_posed_dev -> lrm_foothold_offsets_dev -> this call.
 * lrm_foothold_offsets_dev: offsets_out[0] = 0, offsets_out[k+1] = offsets_out[k] + max(count[k], 0), n + 1 entries,
 * all on the device.  One launch of one workgroup; it never allocates and never synchronises with the host; n up to
 * 2^32 - 1 (more: LRM_EINVAL); n == 0 writes offsets_out[0] = 0 only; NULL pointers give LRM_EINVAL.
 * lrm_foothold_lists_posed_dev / _cpu, with o = l*nposes + p:
 *   segment      base = offsets[o]; room = min(offsets[o+1], (int64)capacity) - base, and 0 if that is negative or base < 0;
 *   idx_out      the reachable targets of (p, l) in ASCENDING index; the first min(count, room) of them at idx_out[base + k];
 *   d2_out       (may be NULL, capacity) at the same positions the d2 of lrm_footholds_posed_dev:
 *                lrm_foothold_d2(t, body[p], nominal_w), float32, no contraction;
 *   written_out  (may be NULL, nlegs*nposes) written_out[o] = min(count, room).
 * No element outside [base, base + room) is ever written, and every other element of idx_out / d2_out keeps its value.
 * ANY offsets array is memory-safe: decreasing, negative and overlapping offsets never cause a write outside the
 * buffers, only a shorter list (overlapping segments hold one of the lists that claim them).  Offsets made by
 * lrm_foothold_offsets_dev from count_out with capacity >= offsets[last] give every list whole; offsets[o] = o*K gives
 * the first K by index of every list.
 * Checked first, as in lrm_footholds_posed_dev: nt > INT32_MAX, nlegs outside 1..LRM_MAX_LEGS, nposes > INT32_MAX or more
 * than 2^32 - 1 records give LRM_EINVAL; NULL offsets or NULL idx_out give LRM_EINVAL.  Then nposes == 0 is a no-op;
 * nt == 0 or capacity == 0 writes written_out = 0 everywhere and nothing else.
 * Threading and streams: lrm_foothold_lists_posed_dev is one of the pair kernels, with lrm_footholds_posed_dev's rules:
 * it uses the per-device tile-box buffer from 4096 targets on, one host thread at a time, no two pair launches on
 * different clouds concurrently on one device; the first call for a larger cloud than the buffer holds allocates, every
 * later call (and every call below 4096 targets) only launches, so compile -> footholds -> offsets -> lists with a
 * fixed capacity can be captured in a graph after one call on a cloud of the largest size.
 * lrm_foothold_lists_posed_cpu: AoS float3 targets, host tables and host offsets, a serial loop over every (pose, leg,
 * target) with the strict test and no culling, like lrm_footholds_posed_cpu: the reference the GPU tests compare with
 * bit for bit; *ms = the loop's time. */
int lrm_foothold_offsets_dev(const int32_t* count, size_t n, int64_t* offsets_out, void* stream);
int lrm_foothold_lists_posed_dev(const float* tx, const float* ty, const float* tz, size_t nt,
                                 const void* workspace, const void* fh_workspace, size_t nposes, size_t nlegs,
                                 const int64_t* offsets /* device, nlegs*nposes + 1 */, size_t capacity,
                                 int32_t* idx_out /* device, capacity */, float* d2_out /* may be NULL, capacity */,
                                 int32_t* written_out /* may be NULL, nlegs*nposes */, void* stream);
int lrm_foothold_lists_posed_cpu(const float* targets_aos, size_t nt, const float* quats, const float* body, size_t nposes,
                                 const LrmLegDimensions* legs, size_t nlegs, const float* nominal,
                                 const int64_t* offsets /* host */, size_t capacity, int32_t* idx_out, float* d2_out,
                                 int32_t* written_out, double* ms);
/* COMMON-foothold counts and choice per pose TRANSITION.  While the body moves from pose a to pose b a stance foot stays
 * planted: its foothold must be reachable from both.  Pose table, leg table, `workspace` and `fh_workspace` are those of
 * lrm_footholds_posed_dev (no new table, no new compile step).  With e an edge, a = edge_a[e], b = edge_b[e] (int32 pose
 * indices, on the device for _dev and on the host for _cpu), triple (e, l, t) is common iff
 *   reachability_global(t - body[a], legs[l], quats[a]) AND reachability_global(t - body[b], legs[l], quats[b]):
 * the strict test on the two pose records, whatever lrm_set_mode says, without a gravity gate -- exactly
 * lrm_footholds_posed_dev's rule, twice.  Every output has nlegs * nedges entries at [l*nedges + e], all written:
 *   count_out     the number of common targets;
 *   best_out      the common target with the smallest d2 (ties: the smaller index), -1 when count is 0;
 *   best_d2_out   (may be NULL) that d2, +inf when count is 0;
 *                 d2 = d2_a + d2_b, ONE float32 add (no contraction) of the two d2 of lrm_footholds_posed_dev, i.e. of
 *                 (t - (body[a] + nominal_w[a,l]))^2 and (t - (body[b] + nominal_w[b,l]))^2: its minimum is the common
 *                 target nearest the midpoint of the leg's two nominal foot positions;
 *   all_legs_out  (may be NULL, nedges) 1 iff every leg has count > 0: the move is feasible with all feet planted AT ITS TWO ENDS;
 *                 lrm_edge_transit_posed_dev tests the poses in between.
 * Consequences: for a == b count and best are lrm_footholds_posed_dev's of that pose and best_d2 is exactly twice its
 * value (x + x is exact); swapping edge_a and edge_b changes no output bit; best_out is a valid target_idx of
 * lrm_ik_posed_dev with pose_idx = either end of the edge.
 * An edge with a or b outside [0, nposes) gives count 0, best -1, d2 +inf, all_legs 0: the kernel checks the indices
 * before it loads any record and never reads outside the tables, so ANY edge_a / edge_b contents are memory-safe.
 * Checked first: nt > INT32_MAX, nlegs outside 1..LRM_MAX_LEGS, nposes > INT32_MAX or more than 2^32 - 1 records, and
 * nedges * nlegs > 2^32 - 1 give LRM_EINVAL; then nedges == 0 is a no-op; NULL edge_a / edge_b / count_out / best_out
 * give LRM_EINVAL; nt == 0 gives count 0, best -1, d2 +inf everywhere.
 * Threading and streams: lrm_foothold_edges_posed_dev is one of the pair kernels, with lrm_footholds_posed_dev's rules:
 * the per-device tile-box buffer from 4096 targets on, one host thread at a time, no two pair launches on different
 * clouds concurrently on one device; the first call for a larger cloud than the buffer holds allocates, every later call
 * (and every call below 4096 targets) only launches, so compile -> footholds -> edges can be captured in a graph after
 * one call on a cloud of the largest size.
 * lrm_foothold_edges_posed_cpu: AoS float3 targets, host tables and host edges, a serial loop over every (edge, leg,
 * target) with both strict tests and no culling: the reference the GPU tests compare with bit for bit; *ms = the loop's
 * time. */
int lrm_foothold_edges_posed_dev(const float* tx, const float* ty, const float* tz, size_t nt,
                                 const void* workspace, const void* fh_workspace, size_t nposes, size_t nlegs,
                                 const int32_t* edge_a, const int32_t* edge_b /* device, nedges */, size_t nedges,
                                 int32_t* count_out, int32_t* best_out, float* best_d2_out /* may be NULL */,
                                 uint8_t* all_legs_out /* may be NULL, nedges */, void* stream);
int lrm_foothold_edges_posed_cpu(const float* targets_aos, size_t nt, const float* quats, const float* body, size_t nposes,
                                 const LrmLegDimensions* legs, size_t nlegs, const float* nominal,
                                 const int32_t* edge_a, const int32_t* edge_b /* host */, size_t nedges,
                                 int32_t* count_out, int32_t* best_out, float* best_d2_out, uint8_t* all_legs_out, double* ms);
/* NEAREST-MISS footholds per (pose, leg): for a leg that reaches nothing, the target that is closest to being reachable
 * and the body translation that would make it so.  Pose table, leg table, `workspace` and `fh_workspace` are those of
 * lrm_footholds_posed_dev (no new table, no new compile step).  One extra scalar, `margin` (mm, float32): margin >= 0 or
 * +inf is accepted, negative or nan gives LRM_EINVAL.  One optional input, count_in (int32, nlegs*nposes, device for _dev
 * and host for _cpu, may be NULL): wherever count_in[o] > 0 that (pose, leg) is skipped and gets the empty answer
 * (entries <= 0, negative ones included, are not skipped).  Pass count_out of lrm_footholds_posed_dev so that only
 * footless legs cost anything.
 * With o = l*nposes + p, E the foothold entry of (p, l) and q = t - body[p] (one float32 subtraction per component, as
 * everywhere in the posed calls), all float32 without contraction, device and host identical:
 *   candidate  target t is a candidate iff e2 <= rm2, with e = q - E.cull_center (one subtraction per component),
 *              e2 = (ex*ex + ey*ey) + ez*ez, rm = sqrtf(E.cull_r2) + margin (correctly rounded), rm2 = rm*rm.
 *              cull_r2 = +inf (non-unit quaternion) or margin = +inf makes every target with a non-nan e2 a candidate.
 *   miss       a candidate with reachability_global(q, legs[l], quats[p]) == 0; its vector is
 *              d = distance_global(q, legs[l], quats[p]): the strict evaluation whatever lrm_set_mode says, the bytes
 *              lrm_reach_dist_posed_cpu returns.  m2 = (dx*dx + dy*dy) + dz*dz.  A miss is eligible iff m2 < +inf
 *              (false for nan).
 * Every output has nlegs * nposes entries at [o], all written:
 *   miss_out     the eligible miss with the smallest (m2, index) -- the m2 bits order like its value, ties go to the
 *                smaller index; -1 when there is none;
 *   miss_m2_out  (may be NULL) that m2, +inf when there is none;
 *   shift_x / shift_y / shift_z  (all three or none; else LRM_EINVAL) that d, nan (the one bit pattern 0x7fc00000) when
 *                there is none.  Translating the body by d at fixed orientation puts the target on the workspace
 *                boundary: t - (body + d) = q - d, the reference's nearest point;
 *   near_out     (may be NULL) the number of misses, eligible or not: the number of distance evaluations the entry cost.
 *                A skipped entry gets 0.
 * Consequences: lrm_reach_dist_posed_* on (miss_out[o], p, l) returns mask 0 and exactly the shift bits; with
 * margin = +inf the answer is the minimum over ALL unreachable targets; a larger margin never gives a larger m2.
 * Checked first, in lrm_footholds_posed_dev's order: nt > INT32_MAX, nlegs outside 1..LRM_MAX_LEGS, nposes > INT32_MAX or
 * more than 2^32 - 1 records, then a bad margin give LRM_EINVAL; then nposes == 0 is a no-op; NULL miss_out gives
 * LRM_EINVAL; nt == 0 gives the empty answer (-1, +inf, nan, 0) everywhere.
 * Threading and streams: lrm_foothold_misses_posed_dev is one of the pair kernels, with lrm_footholds_posed_dev's rules:
 * the per-device tile-box buffer from 4096 targets on, one host thread at a time, no two pair launches on different
 * clouds concurrently on one device; the first call for a larger cloud than the buffer holds allocates, every later call
 * (and every call below 4096 targets) only launches, so compile -> footholds -> foothold_misses(count_in = count_out)
 * can be captured in a graph after one call on a cloud of the largest size.  The box culls keep every candidate: their
 * radius carries an absolute slack of 2^-21 (max|body| + max|centre| + rm) for the different roundings of
 * (t - body) - centre and of body + centre (csrc/lrm_foothold_misses.hip).
 * lrm_foothold_misses_posed_cpu: AoS float3 targets, host tables and a host count_in, a serial loop over every (pose,
 * leg, target) with the same candidate function and the strict code and no box culling: the reference the GPU tests
 * compare with bit for bit; *ms = the loop's time. */
int lrm_foothold_misses_posed_dev(const float* tx, const float* ty, const float* tz, size_t nt,
                                  const void* workspace, const void* fh_workspace, size_t nposes, size_t nlegs,
                                  float margin, const int32_t* count_in /* device, nlegs*nposes, may be NULL */,
                                  int32_t* miss_out, float* miss_m2_out /* may be NULL */,
                                  float* shift_x, float* shift_y, float* shift_z /* all three or none */,
                                  int32_t* near_out /* may be NULL */, void* stream);
int lrm_foothold_misses_posed_cpu(const float* targets_aos, size_t nt, const float* quats, const float* body, size_t nposes,
                                  const LrmLegDimensions* legs, size_t nlegs, float margin,
                                  const int32_t* count_in /* host, may be NULL */, int32_t* miss_out, float* miss_m2_out,
                                  float* shift_x, float* shift_y, float* shift_z, int32_t* near_out, double* ms);
/* Per-TARGET foothold SUPPORT: for every terrain point and leg, how many of the candidate body poses can put that foot
 * there, and which pose does it best -- the foothold queries above with the roles swapped (a contact-first planner, a
 * terrain-usability map).  Pose table, leg table, `workspace` and `fh_workspace` are those of lrm_footholds_posed_dev
 * (no new table, no new compile step).  One optional input, pose_live (uint8, nposes, device for _dev and host for _cpu,
 * may be NULL): pose p is live when pose_live is NULL or pose_live[p] != 0; a dead pose contributes nothing.
 * Triple (t, p, l) is REACHING iff pose p is live and reachability_global(t - body[p], legs[l], quats[p]): the strict
 * test on the pose record, whatever lrm_set_mode says, without a gravity gate -- exactly lrm_footholds_posed_dev's rule.
 * Every float is float32 without contraction, device and host identical.  Outputs with nlegs * nt entries at
 * [l*nt + t], all written:
 *   count_out      the number of reaching poses;
 *   best_pose_out  the reaching pose with the smallest lrm_footholds_posed_dev d2 of that triple,
 *                  d2 = (t - (body[p] + nominal_w[p,l]))^2 -- the same bits -- ties to the smaller pose index; -1 when
 *                  count is 0;
 *   best_d2_out    (may be NULL) that d2, +inf when count is 0;
 * and legs_mask_out[t] (may be NULL, nt bytes): bit l set iff count_out[l*nt + t] > 0 (LRM_MAX_LEGS is 8).
 * Consequences: with pose_live NULL the sum over t of count_out[l, t] equals the sum over p of
 * lrm_footholds_posed_dev's count[l, p]; count_out[l, t] > 0 iff t occurs in some list of leg l of
 * lrm_foothold_lists_posed_dev; for p* = best_pose_out[l, t] the list of (p*, l) contains t with exactly best_d2_out's
 * bits; lrm_ik_posed_dev on (t, p*, l) reports a mask-1 status: LRM_IK_REACHED, or LRM_IK_MODEL_GAP at the few
 * points just outside a limit face (M2 and moonbot: within about 1e-2 mm) that the circle model's margin still calls
 * reachable while no in-limit tip is within 1e-3 mm (see the IK section), never LRM_IK_NONE / NEAREST /
 * FAR_GAP; with pose_live = all_legs_out of lrm_footholds_posed_dev only positionable bodies count.
 * A nan or infinite target reaches nothing.  A pose with a nan body or a non-unit quaternion is handled as in
 * lrm_footholds_posed_dev: its sphere excludes nothing and it is tested against every target.
 * Checked first, in lrm_footholds_posed_dev's order: nt > INT32_MAX, nlegs outside 1..LRM_MAX_LEGS, nposes > INT32_MAX or
 * more than 2^32 - 1 records give LRM_EINVAL; then nt == 0 is a no-op; NULL count_out, best_pose_out or
 * support_workspace give LRM_EINVAL; nposes == 0 writes 0 / -1 / +inf / 0 everywhere (no table is read).
 * support_workspace: lrm_foothold_support_workspace_bytes(nposes, nlegs, nt) bytes of device memory, 16-byte aligned,
 * owned by the caller for the duration of the call; every call rewrites it, no initialisation is needed, and a
 * workspace sized for larger nposes / nt serves smaller ones.  It holds the per-(target, leg) accumulators, one cull
 * sphere per (pose, leg) and one bounding box per 64 poses.
 * Threading and streams: UNLIKE the pair kernels above, lrm_foothold_support_posed_dev does not use the per-device
 * tile-box buffer -- every wave boxes its own 64 targets -- so it does not inherit their rules about one host thread
 * and one cloud at a time: calls with different support workspaces may run concurrently from several threads and
 * streams.  The call allocates nothing and never synchronises with the host; it is three launches on `stream` and can be
 * captured in a graph from its first call.  The pose range is cut into S slices whose partial answers meet through
 * integer atomic add and 64-bit atomic min, both order-independent: the outputs are bit-deterministic.  The box culls
 * keep every reaching triple: they carry an absolute slack of 2^-21 (max|body| + max|centre| + r) for the different
 * roundings of (t - body) - centre and of body + centre (csrc/lrm_foothold_support.hip).
 * lrm_foothold_support_posed_cpu: AoS float3 targets, host tables and a host pose_live, a serial loop over every
 * (target, leg, pose) with the strict test and no culling: the reference the GPU tests compare with bit for bit;
 * *ms = the loop's time. */
size_t lrm_foothold_support_workspace_bytes(size_t nposes, size_t nlegs, size_t nt);
int lrm_foothold_support_posed_dev(const float* tx, const float* ty, const float* tz, size_t nt,
                                   const void* workspace, const void* fh_workspace, size_t nposes, size_t nlegs,
                                   const uint8_t* pose_live /* device, nposes, may be NULL */,
                                   void* support_workspace /* device, caller-owned, 16-byte aligned */,
                                   int32_t* count_out, int32_t* best_pose_out, float* best_d2_out /* may be NULL */,
                                   uint8_t* legs_mask_out /* may be NULL, nt */, void* stream);
int lrm_foothold_support_posed_cpu(const float* targets_aos, size_t nt, const float* quats, const float* body, size_t nposes,
                                   const LrmLegDimensions* legs, size_t nlegs, const float* nominal,
                                   const uint8_t* pose_live /* host, may be NULL */, int32_t* count_out,
                                   int32_t* best_pose_out, float* best_d2_out, uint8_t* legs_mask_out, double* ms);
/* BODY CLEARANCE per pose: does the trunk of a posed body fit over the terrain, how far must it rise if not, and how much
 * ground clearance is left if so.  The reference removes colliding bodies per orientation before it counts anything
 * (eliminateFarAndColliding / eliminateBodyColliding, several_leg.cu:504-630, with in_cylinder of collision.cu.h:12-23 on
 * bodies and targets taken into the orientation's frame); this is that predicate for bodies that each have their own
 * quaternion and position.  Pose table, leg table, `workspace` and `fh_workspace` are those of lrm_footholds_posed_dev (no
 * new table, no new compile step).  Four float32 scalars describe the body volume in the BODY frame, centred on the body
 * origin, the body's z its axis: radius, plus_z (top), minus_z (the belly plane) and floor_z (how far below the body
 * terrain is still looked at).  One optional input, live_in (uint8, nposes, device for _dev and host for _cpu, may be
 * NULL): a pose with live_in[p] == 0 is skipped -- it costs nothing and gets the empty answer with free = 0.
 * For pose p and target t, float32 without contraction, device and host identical:
 *   q = t - body[p]          one subtraction per component, as everywhere in the posed calls;
 *   v = qtInvRotate(quats[p], q)   the strict rotation reachability_global applies, bit for bit: lrm_qrot on the pose
 *                            record's inv_rot (the same in every record of the pose; leg 0's is read);
 *   column(t) = in_cylinder(radius, plus_z, floor_z, 0, v):  sqrtf(vx*vx + vy*vy + 0) < radius, vz < plus_z, vz > floor_z
 *               (norm3df restated as sqrtf of the sum in that order);
 *   hit(t)    = in_cylinder(radius, plus_z, minus_z, 0, v);
 *   height(t) = vz - minus_z, one subtraction; -0 is stored and compared as +0.
 * Every output has nposes entries, all written:
 *   hits_out    (int32) the number of targets with hit;
 *   top_out     (int32) the column target with the largest height, ties to the smaller index; -1 when the column is empty;
 *   height_out  (float, may be NULL) that height, -inf when the column is empty.  A value > 0 is the lift along the body's z
 *               that takes the highest intruder down to the belly plane (stated for exact arithmetic); a value <= 0 means
 *               the belly clears the terrain under it by that much;
 *   free_out    (uint8, may be NULL) 1 iff the pose is live and hits == 0.
 * Consequences: for a live pose hits > 0 iff height > 0 iff free == 0 (a hit is a column target, floor_z <= minus_z, and
 * x - y > 0 iff x > y); with floor_z == minus_z column and hit coincide; with the identity quaternion free_out is the
 * negation of lrm_any_in_cylinder_dev on the same cylinder and centres wherever that byte is defined; a nan or infinite
 * target is in no column; free_out is directly usable as pose_live of lrm_foothold_support_posed_dev, and all_legs_out of
 * lrm_footholds_posed_dev as live_in, so that update -> footholds -> body_clearance(live_in = all_legs) ->
 * foothold_support(pose_live = free) -> ik only counts bodies that stand AND fit.
 * For a pose with a nan body or a non-unit quaternion qtInvRotate is not a rotation: its cull excludes nothing and it is
 * tested against every target, as in lrm_footholds_posed_dev.  Such a pose is recognised by leg 0's foothold entry
 * having cull_r2 = +inf.
 * Checked first, in lrm_footholds_posed_dev's order: nt > INT32_MAX, nlegs outside 1..LRM_MAX_LEGS, nposes > INT32_MAX or
 * more than 2^32 - 1 records, then the scalars give LRM_EINVAL: any of them nan, radius < 0, minus_z or floor_z not finite,
 * floor_z > minus_z, plus_z <= minus_z (radius and plus_z may be +inf).  Then nposes == 0 is a no-op; NULL hits_out or
 * top_out gives LRM_EINVAL; nt == 0 gives 0 / -1 / -inf everywhere, free_out = 1 for every live pose and 0 for a skipped one.
 * Threading and streams: lrm_body_clearance_posed_dev is one of the pair kernels, with lrm_footholds_posed_dev's rules:
 * the per-device tile-box buffer from 4096 targets on, one host thread at a time, no two pair launches on different
 * clouds concurrently on one device; the first call for a larger cloud than the buffer holds allocates, every later call
 * (and every call below 4096 targets) only launches, so compile -> footholds -> body_clearance can be captured in a graph
 * after one call on a cloud of the largest size.  One launch behind the boxes' own; no atomics.  The box culls keep every
 * column target: the cull sphere about body[p] bounds the cylinder (radius, plus_z, floor_z) with slack for |quat|^2 within
 * 1e-5 of 1; its centre is the very point q is formed about, so unlike the foothold spheres it needs no absolute slack
 * far from the origin (csrc/lrm_body_clearance.hip); an infinite radius or plus_z gives the sphere that excludes nothing.
 * lrm_body_clearance_posed_cpu: AoS float3 targets, host tables and a host live_in, a serial loop over every (pose,
 * target) with the same test function and no culling: the reference the GPU tests compare with bit for bit; *ms = the
 * loop's time. */
int lrm_body_clearance_posed_dev(const float* tx, const float* ty, const float* tz, size_t nt,
                                 const void* workspace, const void* fh_workspace, size_t nposes, size_t nlegs,
                                 float radius, float plus_z, float minus_z, float floor_z,
                                 const uint8_t* live_in /* device, nposes, may be NULL */,
                                 int32_t* hits_out, int32_t* top_out, float* height_out /* may be NULL */,
                                 uint8_t* free_out /* may be NULL */, void* stream);
int lrm_body_clearance_posed_cpu(const float* targets_aos, size_t nt, const float* quats, const float* body, size_t nposes,
                                 const LrmLegDimensions* legs, size_t nlegs,
                                 float radius, float plus_z, float minus_z, float floor_z,
                                 const uint8_t* live_in /* host, may be NULL */, int32_t* hits_out, int32_t* top_out,
                                 float* height_out, uint8_t* free_out, double* ms);
/* LEG LINK CLEARANCE per (pose, leg): do the leg's own links fit over the terrain under given joint angles.
 * lrm_footholds_posed_dev says whether a foot reaches the ground and lrm_body_clearance_posed_dev whether the trunk fits;
 * lrm_ik_posed_dev then returns angles that put the foot on the chosen foothold -- and the knee may stand inside a rock.  The
 * reference has no such query (it culls colliding bodies, never legs).  Pose table, leg table, `workspace` and
 * `ik_workspace` are those of lrm_ik_posed_dev (no new table, no new compile step).  coxa / femur / tibia: device float32,
 * nlegs * nposes angles at [l*nposes + p] -- lrm_ik_posed_dev's outputs under the [l*nposes + p] layout of the foothold calls.
 * radius[3] (host): the radii of the capsules about link 0 (coxa), 1 (femur) and 2 (tibia), each >= 0 and finite; a link with
 * radius 0 is not tested at all.  margin >= 0, finite: how far outside a link a target still counts as near.  tip_clear >= 0,
 * finite: how far short of the foot the tibia link stops (without it every stance would collide with its own foothold).
 * live_in (uint8, nposes, device for _dev and host for _cpu, may be NULL): a pose with live_in[p] == 0 is skipped.
 * Everything is float32 without contraction, only + - * /, comparisons, the correctly rounded square root and the sincos
 * of the IK: device and host give the same bits (csrc/lrm_leg_clearance.h is the one source of both).
 * Joints of (p, l) under angles (c, f, t), RELATIVE to body[p], with sc, cc = sincos(c), sf, cf = sincos(f),
 * sa, ca = sincos(f + t), C, F, T the leg's link lengths, T' = T - tip_clear (0 unless T' > 0), from_coxa the last step of
 * lrm_fk_posed_dev's chain:
 *   J0 = from_coxa(0, 0, 0)  the coxa joint;      J1 = from_coxa(cc C, sc C, 0)  the femur joint;
 *   J2 = from_coxa(cc h2, sc h2, F sf), h2 = C + F cf  the knee;
 *   J3 = from_coxa(cc h3, sc h3, F sf + T' sa), h3 = C + (F cf + T' ca)  -- with tip_clear == 0 the bits of lrm_fk_posed_dev's tip
 *   (before the body is added).  Link k runs from A = Jk to B = Jk+1.
 * A leg is VALID iff all twelve coordinates are finite; nan angles (LRM_IK_NONE) and angles outside the sincos range
 * (|x| >= 120) give nan joints.  An invalid leg is SKIPPED: it gets hits 0, links 0, worst -1, pen -inf and DOES NOT BLOCK
 * free_out -- pass live_in = all_legs & body-free so that such legs do not occur in live poses.
 * Target t against link k, q = t - body[p] (one subtraction per component):
 *   ab = B - A; ap = q - A; den = (ab.x ab.x + ab.y ab.y) + ab.z ab.z; num = (ap.x ab.x + ap.y ab.y) + ap.z ab.z;
 *   s = den > 0 ? num / den : 0, then clamped: s = !(s > 0) ? 0 : (s > 1 ? 1 : s);
 *   e = ap - s ab (one multiply, one subtract per component); d = sqrt((e.x e.x + e.y e.y) + e.z e.z);
 *   hit_k = d < radius[k]; near_k = d < radius[k] + margin (the sum formed once per call); pen_k = radius[k] - d (-0 stored
 *   and compared as +0).  A nan d is neither near nor hit.  pen(t) = the largest pen_k over the links with near_k.
 * Outputs with nlegs * nposes entries at [l*nposes + p], all written:
 *   hits_out   (int32) the number of targets with some hit_k;
 *   links_out  (uint8) bit k set iff link k has a hit;
 *   worst_out  (int32) the near target with the largest pen, ties to the smaller index; -1 when no target is near;
 *   pen_out    (float, may be NULL) that pen, -inf when none: > 0 is the depth of the deepest intrusion, <= 0 the
 *              clearance left within the margin;
 * and free_out[p] (uint8, nposes, may be NULL): 1 iff the pose is live and every leg has hits == 0.  A pose with
 * live_in[p] == 0 gets 0 / 0 / -1 / -inf for every leg and free 0.
 * Consequences: pen > 0 iff hits > 0 iff links != 0; with margin == 0 near and hit coincide, so worst is a hit or -1; a nan
 * or infinite target is near nothing; free_out is directly usable as pose_live of lrm_foothold_support_posed_dev:
 * update -> footholds -> body_clearance(live_in = all_legs) -> foothold_support(pose_live = free) -> ik -> leg_clearance.
 * Checked first, in lrm_body_clearance_posed_dev's order: nt > INT32_MAX, nlegs outside 1..LRM_MAX_LEGS, nposes > INT32_MAX
 * or more than 2^32 - 1 records, then the scalars give LRM_EINVAL: any of them nan, a radius, margin or tip_clear negative or
 * not finite (NULL radius too).  Then nposes == 0 is a no-op; NULL hits_out, links_out, worst_out or angle array gives
 * LRM_EINVAL; nt == 0 gives 0 / 0 / -1 / -inf everywhere, free_out = 1 for every live pose and 0 for a skipped one.
 * Threading and streams: lrm_leg_clearance_posed_dev is one of the pair kernels, with lrm_footholds_posed_dev's rules: the
 * per-device tile-box buffer from 4096 targets on, one host thread at a time, no two pair launches on different clouds
 * concurrently on one device; the first call for a larger cloud than the buffer holds allocates, every later call (and every
 * call below 4096 targets) only launches, so update -> footholds -> ik -> leg_clearance can be captured in a graph after one
 * call on a cloud of the largest size.  One launch behind the boxes' own; no atomics.  The box cull keeps every near target:
 * a tile or chunk box is skipped only if on some axis it lies further than (max radius + margin) * 1.0001 + 1e-5 * (the leg
 * box's extent) from the box of the leg's four computed joints, both taken about body[p], so it needs no absolute slack far
 * from the origin and no special case for non-unit quaternions (csrc/lrm_leg_clearance.hip); a margin so large that the
 * inflation overflows culls nothing.
 * lrm_leg_clearance_posed_cpu: AoS float3 targets, host tables, host angles_aos (nlegs * nposes triples {coxa, femur, tibia}
 * at [l*nposes + p]: lrm_ik_posed_cpu's output in that layout) and a host live_in; a serial loop over every (pose, leg,
 * target) with the same functions and no culling: the reference the GPU tests compare with bit for bit; *ms = the loop's time.
 * lrm_leg_joints_posed_dev / _cpu: the joints themselves, for inspection and drawing: joints_out holds nlegs * nposes * 12
 * floats, entry [l*nposes + p] = J0..J3 as x, y, z with body[p] added (one addition per component).  A nan coordinate is stored
 * as the canonical quiet nan 0x7fc00000 (sign and payload of a propagated nan differ between host and device).  Checked first: nlegs >
 * LRM_MAX_LEGS, nposes > INT32_MAX or more than 2^32 - 1 records, tip_clear nan, negative or not finite give LRM_EINVAL; then
 * nposes == 0 or nlegs == 0 is a no-op; NULL arguments give LRM_EINVAL.  The _dev form is one launch, allocates nothing and
 * uses no shared buffer. */
int lrm_leg_clearance_posed_dev(const float* tx, const float* ty, const float* tz, size_t nt,
                                const void* workspace, const void* ik_workspace, size_t nposes, size_t nlegs,
                                const float* coxa, const float* femur, const float* tibia /* device, nlegs*nposes at [l*nposes + p] */,
                                const float radius[3] /* host */, float margin, float tip_clear,
                                const uint8_t* live_in /* device, nposes, may be NULL */,
                                int32_t* hits_out, uint8_t* links_out, int32_t* worst_out, float* pen_out /* may be NULL */,
                                uint8_t* free_out /* nposes, may be NULL */, void* stream);
int lrm_leg_clearance_posed_cpu(const float* targets_aos, size_t nt, const float* quats, const float* body, size_t nposes,
                                const LrmLegDimensions* legs, size_t nlegs, const float* angles_aos,
                                const float radius[3], float margin, float tip_clear,
                                const uint8_t* live_in /* host, may be NULL */, int32_t* hits_out, uint8_t* links_out,
                                int32_t* worst_out, float* pen_out, uint8_t* free_out, double* ms);
int lrm_leg_joints_posed_dev(const float* coxa, const float* femur, const float* tibia, size_t nposes, size_t nlegs,
                             const void* workspace, const void* ik_workspace, float tip_clear,
                             float* joints_out /* device, nlegs*nposes*12 */, void* stream);
int lrm_leg_joints_posed_cpu(const float* angles_aos, const float* quats, const float* body, size_t nposes,
                             const LrmLegDimensions* legs, size_t nlegs, float tip_clear, float* joints_out, double* ms);
/* STATIC STABILITY per stance: does the robot stand, and which legs can it lift.  lrm_footholds_posed_dev says that every leg
 * has a foothold (all_legs), lrm_body_clearance_posed_dev that the trunk fits and lrm_leg_clearance_posed_dev that the legs
 * fit; none of them says that the centre of mass lies over the polygon the chosen footholds span, nor which feet can leave
 * the ground (one leg, a tripod, any subset) with the robot still statically stable.  The reference has no such query (its
 * leg_number_for_stab only counts legs).  No table: the call reads the cloud, the quaternions and the body positions.
 * A STANCE s (of nstances) has a pose p = pose_idx[s] (pose_idx == NULL: p = s) and one foot index per leg,
 * foot[l*nstances + s] (int32): lrm_footholds_posed_dev's best_out as it stands, or lrm_foothold_edges_posed_dev's best_out
 * with pose_idx = edge_a or edge_b.  Everything is float32 without contraction; only + - * /, comparisons and the correctly
 * rounded square root are used: device and host give the same bits (csrc/lrm_stance.h is the one source of both).
 * Foot of leg l: VALID iff 0 <= foot < nt and q = t[foot] - body[p] (one subtraction per component; body == NULL: 0) has
 *   three finite coordinates.  Its plane point is f_l = (q.x, q.y) with plane == NULL (gravity along -z of the caller's
 *   frame); with plane = {u[3], v[3]} (host, six finite floats: a basis of the plane normal to gravity, supplied by the
 *   caller) it is f_l = ((q.x u.x + q.y u.y) + q.z u.z, (q.x v.x + q.y v.y) + q.z v.z).
 * Centre of mass: c3 = qtRotate(quats[p], com) through the coefficient sums of the pose records (the chain of the foothold
 *   table's nominal point), com a host float[3] in the BODY frame; com == NULL or all zero gives exactly 0 whatever the
 *   quaternion.  c3 is projected like a foot: c.  Like the feet, c is relative to body[p].
 * DEAD stance: live_in[s] == 0 (uint8, nstances, device for _dev and host for _cpu, may be NULL), or p outside [0, nposes), or
 *   c not finite.
 * Ordered pairs (i, j), i != j, both feet valid: a = f_i; e = f_j - a; len2 = e.x e.x + e.y e.y; the pair is USABLE iff
 *   len2 > 0 and len2 < inf;
 *   left_ij has bit k set, for every valid foot k, iff e.x (f_k.y - a.y) - e.y (f_k.x - a.x) >= 0 (bits i and j come out set
 *   by the arithmetic);
 *   s_ij = (e.x (c.y - a.y) - e.y (c.x - a.x)) / sqrt(len2); a nan s_ij counts as -inf, -0 is stored and compared as +0.
 * Lift sets: lift (host, uint8, nmasks entries, 1 <= nmasks <= 256); bit l set = leg l is in the air.  The planted set is
 *   S = valid_feet & ~lift[m].  popcount(S) < 3: the margin is -inf.  Otherwise margin = min s_ij over the usable pairs with
 *   i, j in S and (S & ~left_ij) == 0 -- the counter-clockwise hull edges of the planted feet -- ties to the smaller code
 *   i*8 + j; no such pair: -inf.
 * Outputs at [m*nstances + s], all written:
 *   margin_out (float)  > 0: the distance (mm) of the centre of mass from the nearest edge of the support polygon;
 *   edge_out   (uint8, may be NULL) the code i*8 + j of that edge, 255 when the margin is -inf;
 *   stable_out (uint8)  margin > min_margin (min_margin: host float, finite, >= 0);
 * and feet_out[s] (uint8, nstances, may be NULL): the valid-feet bits, 0 for a dead stance.  A dead stance gets
 * -inf / 255 / 0 for every lift set.
 * Consequences: collinear or coincident feet give a margin <= 0, never stable; row m of stable_out is a uint8[nstances],
 * directly usable as live_in / pose_live of the other posed calls (with pose_idx == NULL a stance is a pose):
 * update -> footholds -> stance_stability -> body_clearance(live_in = stable row 0) -> ...; for a centre of mass OUTSIDE
 * the polygon the margin is the most negative half-plane distance, not the Euclidean distance to the polygon; on nearly
 * collinear hull vertices the arithmetic itself decides which edges count.
 * Checked first (all LRM_EINVAL): nlegs outside 1..LRM_MAX_LEGS; nmasks outside 1..256; nt, nposes or nstances > INT32_MAX;
 * nmasks * nstances past 2^32 - 1; NULL lift; a lift bit at or above nlegs; min_margin nan, negative or infinite; a
 * non-finite com or plane value; pose_idx == NULL with nstances > nposes.  Then nstances == 0 is a no-op; NULL foot, quats,
 * margin_out or stable_out (or a NULL cloud with nt > 0) gives LRM_EINVAL; nt == 0 makes every foot invalid.
 * lrm_stance_stability_dev: device pointers are the cloud, quats (nposes x 4), body (nposes x 3, may be NULL), pose_idx, foot,
 * live_in and the outputs; com, plane and lift are host pointers and travel in the kernel's arguments.  ONE launch: no
 * allocation, no host synchronisation, no shared buffer -- it can be captured in a graph and may run concurrently with
 * anything, the pair kernels included, from any host thread.
 * lrm_stance_stability_cpu: AoS float3 targets, host arrays; a serial loop over every (stance, lift set) with the same
 * functions: the reference the GPU tests compare with bit for bit; *ms = the loop's time. */
int lrm_stance_stability_dev(const float* tx, const float* ty, const float* tz, size_t nt,
                             const float* quats /* device, nposes x 4 */, const float* body /* device, nposes x 3, may be NULL */,
                             size_t nposes, const int32_t* pose_idx /* device, nstances, may be NULL */,
                             const int32_t* foot /* device, nlegs*nstances at [l*nstances + s] */, size_t nstances, size_t nlegs,
                             const float* com /* host, 3, may be NULL */, const float* plane /* host, 6, may be NULL */,
                             const uint8_t* lift /* host, nmasks */, size_t nmasks, float min_margin,
                             const uint8_t* live_in /* device, nstances, may be NULL */,
                             float* margin_out, uint8_t* edge_out /* may be NULL */, uint8_t* stable_out,
                             uint8_t* feet_out /* nstances, may be NULL */, void* stream);
int lrm_stance_stability_cpu(const float* targets_aos, size_t nt, const float* quats, const float* body, size_t nposes,
                             const int32_t* pose_idx, const int32_t* foot, size_t nstances, size_t nlegs,
                             const float* com, const float* plane, const uint8_t* lift, size_t nmasks, float min_margin,
                             const uint8_t* live_in /* host, may be NULL */, float* margin_out, uint8_t* edge_out,
                             uint8_t* stable_out, uint8_t* feet_out, double* ms);
/* LEG-LEG SELF CLEARANCE per set: do the legs fit next to each other.  lrm_footholds_posed_dev chooses per leg and
 * lrm_ik_posed_dev solves per leg, so nothing stops two legs from crossing or from choosing the same point;
 * lrm_body_clearance_posed_dev and lrm_leg_clearance_posed_dev test trunk and legs against the TERRAIN only.  This call tests the
 * links of every two DIFFERENT legs against each other (trunk against leg links: lrm_trunk_clearance_posed_dev).  The reference has no such
 * query.  It reads no cloud and no new table: `workspace` and `ik_workspace` are the pose table and the IK table of
 * lrm_leg_clearance_posed_dev; the body position is not read (both legs are relative to the same body).
 * A SET s (of nsets) is a pose p = pose_idx[s] (int32; pose_idx == NULL: p = s) and three angles per leg at [l*nsets + s]:
 * lrm_ik_posed_dev's output under footholds_layout (a set per pose), or under foothold_edges_layout with pose_idx = edge_a or
 * edge_b -- the form lrm_stance_stability_dev takes.  radius[3] (host), margin and tip_clear are lrm_leg_clearance_posed_dev's.
 * Everything is float32 without contraction, only + - * /, comparisons, the correctly rounded square root and the sincos of the
 * IK: device and host give the same bits (csrc/lrm_self_clearance.h is the one source of both).
 * Joints: J0..J3 of (p, l) are lrm_leg_clearance_posed_dev's, tip_clear included.  A leg is VALID iff its twelve coordinates
 *   are finite.  An invalid leg takes part in no pair, gets the empty answer and does not block free_out.
 * Pairs: for legs i < j, both valid, and links ka, kb in 0..2 with radius[ka] != 0 and radius[kb] != 0: segment 1 is link ka
 *   of the leg with the SMALLER index, A1 = J_i[ka], B1 = J_i[ka+1]; segment 2 is A2 = J_j[kb], B2 = J_j[kb+1].  Both legs read
 *   the same d of a pair; it is computed once, in this order.
 * Distance, with dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z and clamp01(x) = !(x > 0) ? 0 : (x > 1 ? 1 : x):
 *   d1 = B1 - A1; d2 = B2 - A2; r = A1 - A2; a = dot(d1,d1); e = dot(d2,d2); f = dot(d2,r); c = dot(d1,r); b = dot(d1,d2);
 *   if !(a > 0) && !(e > 0): s = t = 0;
 *   else if !(a > 0): s = 0; t = clamp01(f / e);
 *   else if !(e > 0): t = 0; s = clamp01(-c / a);
 *   else: den = a*e - b*b; s = den > 0 ? clamp01((b*f - c*e) / den) : 0; tn = b*s + f;
 *         if !(tn > 0): t = 0; s = clamp01(-c / a);  else if tn > e: t = 1; s = clamp01((b - c) / a);  else: t = tn / e;
 *   w = (r + s*d1) - t*d2 per component; d = sqrt(dot(w, w));
 *   then, in this order, the four endpoint distances of lrm_leg_clearance_posed_dev's point-to-link formula (ab the link's
 *   B - A, den = dot(ab, ab)) are folded in: A1 and B1 against segment 2, then A2 and B2 against segment 1, each by
 *   d = dk < d ? dk : d.  Every candidate is a distance between two points of the segments, so d never under-reports; the
 *   fold bounds what the clamped step alone over-reports on nearly parallel links (measured: DESIGN.md 3.20).
 * Per pair: rr = radius[ka] + radius[kb]; hit = d < rr; near = d < rr + margin (the nine sums rr + margin formed once per
 *   call); pen = (rr - d) + 0.  A nan d is neither near nor hit.
 * Outputs per (set, leg) at [l*nsets + s], all written:
 *   hits_out  (int32) the number of pairs with a hit in which leg l is one of the two legs;
 *   with_out  (uint8) bit j set iff some link of l hits some link of leg j;
 *   links_out (uint8) bit k set iff link k of leg l is in a hit;
 *   worst_out (uint8) the near pair of leg l with the largest pen, as code j*9 + own_link*3 + other_link (j the other leg),
 *             ties to the smaller code; 255 when none is near;
 *   pen_out   (float, may be NULL) that pen, -inf when none;
 * and free_out[s] (uint8, nsets, may be NULL): 1 iff the set is live and no leg has a hit.
 * A DEAD set -- live_in[s] == 0 (uint8, nsets, device for _dev and host for _cpu, may be NULL), or p outside [0, nposes) --
 * gets 0 / 0 / 0 / 255 / -inf and free 0; it touches no table and no angle.
 * Consequences: with[i] has bit j set iff with[j] has bit i set; the sum of hits over the legs of a set is even; pen > 0 iff
 * hits > 0 iff with != 0 iff links != 0; with margin == 0 worst is a hit or 255; with nlegs == 1 everything is empty and
 * free = live; free_out is directly a live_in / pose_live of the other posed calls:
 * ... -> ik -> self_clearance -> leg_clearance(live_in = free).
 * Checked first, in lrm_leg_clearance_posed_dev's order and by its rules (all LRM_EINVAL): nlegs outside 1..LRM_MAX_LEGS; nsets
 * or nposes > INT32_MAX, or nlegs * nsets past 2^32 - 1; a radius, margin or tip_clear that is nan, negative or infinite (NULL
 * radius too); pose_idx == NULL with nsets > nposes.  Then nsets == 0 is a no-op; a NULL table, angle array, hits_out,
 * with_out, links_out or worst_out gives LRM_EINVAL.
 * lrm_self_clearance_posed_dev: ONE launch, a wave per set: no allocation, no host synchronisation, no atomics, no shared
 * buffer -- it can be captured in a graph and may run concurrently with anything, the pair kernels included, from any host
 * thread.  Bit-deterministic.
 * lrm_self_clearance_posed_cpu: host quats (nposes x 4), legs and angles_aos (nlegs * nsets triples {coxa, femur, tibia} at
 * [l*nsets + s]: lrm_ik_posed_cpu's output in that layout), host pose_idx and live_in; it compiles its own tables and runs a
 * serial loop over every (set, pair) with the same functions: the reference the GPU tests compare with bit for bit; *ms =
 * the loop's time. */
int lrm_self_clearance_posed_dev(const void* workspace, const void* ik_workspace, size_t nposes, size_t nlegs,
                                 const int32_t* pose_idx /* device, nsets, may be NULL */, size_t nsets,
                                 const float* coxa, const float* femur, const float* tibia /* device, nlegs*nsets at [l*nsets + s] */,
                                 const float radius[3] /* host */, float margin, float tip_clear,
                                 const uint8_t* live_in /* device, nsets, may be NULL */,
                                 int32_t* hits_out, uint8_t* with_out, uint8_t* links_out, uint8_t* worst_out,
                                 float* pen_out /* may be NULL */, uint8_t* free_out /* nsets, may be NULL */, void* stream);
int lrm_self_clearance_posed_cpu(const float* quats, size_t nposes, const LrmLegDimensions* legs, size_t nlegs,
                                 const int32_t* pose_idx /* host, may be NULL */, size_t nsets, const float* angles_aos,
                                 const float radius[3], float margin, float tip_clear,
                                 const uint8_t* live_in /* host, may be NULL */, int32_t* hits_out, uint8_t* with_out,
                                 uint8_t* links_out, uint8_t* worst_out, float* pen_out, uint8_t* free_out, double* ms);
/* TRUNK-LEG CLEARANCE per set: do the legs stay out of the robot's own trunk.  lrm_ik_posed_dev picks among its candidates by
 * residual and seed and sends a joint to its limit where a limit is violated; lrm_self_clearance_posed_dev tests leg against
 * leg and lrm_body_clearance_posed_dev the trunk against the TERRAIN.  This call tests the links of every leg against the trunk
 * itself: the body cylinder of lrm_body_clearance_posed_dev -- trunk_radius, plus_z, minus_z (float32), BODY frame, axis z,
 * centred on the body origin; there is no floor_z.  The reference has no such query.  It reads no cloud, no body position
 * and no new table: `workspace`, `ik_workspace`, nposes, nlegs, pose_idx, nsets, the angles at [l*nsets + s], radius[3] (host),
 * margin, tip_clear and live_in are lrm_self_clearance_posed_dev's, with the same meaning (a set per pose, or per edge with
 * pose_idx = edge_a or edge_b).  links (uint8): bit k set = link k (0 coxa, 1 femur, 2 tibia) is tested; the coxa link starts
 * at the leg's mount on the trunk, so callers usually pass 0b110.  A link with radius[k] == 0 is not tested either.
 * Everything is float32 without contraction, only + - * /, comparisons, the correctly rounded square root and the sincos of the
 * IK: device and host give the same bits (csrc/lrm_trunk_clearance.h is the one source of both).
 * Joints: J0..J3 of (p, l) are lrm_leg_clearance_posed_dev's, relative to the body, tip_clear included.  A leg is VALID iff its
 *   twelve coordinates are finite.  An invalid leg gets the empty answer and does not block free_out.
 * Body frame: each joint is taken into the body frame as lrm_body_clearance_posed_dev takes a target: with m = the pose
 *   record's inv_rot (the coefficient sums of qtInvRotate(quats[p], .)),
 *   v.x = 2 * ((m[0] J.x + m[1] J.y) + m[2] J.z) + J.x, v.y and v.z likewise with m[3..5] and m[6..8].
 * Point to cylinder: for a body-frame point P = (x, y, z), with R = trunk_radius:
 *   rho = sqrt(x*x + y*y); dr = rho > R ? rho - R : 0; dz = z > plus_z ? z - plus_z : (z < minus_z ? minus_z - z : 0);
 *   h(P) = dr*dr + dz*dz -- the squared distance to the solid cylinder, 0 inside, convex along a segment.
 *   (Every comparison with a nan is false, so a nan rho or z counts 0 in its term; the joints of a valid leg are finite.)
 * Link k runs from A = v_k to B = v_(k+1); e = B - A per component; P(u) = A + u*e per component (A.x + u*e.x, ...).
 *   best = h(A); hB = h(B): best = hB < best ? hB : best; [lo, hi] = [0, 1]; then N = 32 rounds (LRM_TRUNK_ROUNDS) of
 *     w = (hi - lo) / 3; m1 = lo + w; m2 = hi - w; h1 = h(P(m1)); h2 = h(P(m2));
 *     best = h1 < best ? h1 : best; best = h2 < best ? h2 : best; if (h1 <= h2) hi = m2; else lo = m1;
 *   d_k = sqrt(best).  Every candidate is the distance of a point of the link, so d never under-reports; what the search
 *   over-reports is measured, not assumed.
 * Per tested link: hit_k = d_k < radius[k]; near_k = d_k < radius[k] + margin (the three sums formed once per call);
 *   pen_k = (radius[k] - d_k) + 0.  A nan d is neither near nor hit.
 * Outputs per (set, leg) at [l*nsets + s], all written:
 *   links_out (uint8) bit k set iff link k hits the trunk;
 *   worst_out (uint8) the near link with the largest pen, ties to the smaller k; 255 when none is near;
 *   pen_out   (float, may be NULL) that pen, -inf when none;
 * and free_out[s] (uint8, nsets, may be NULL): 1 iff the set is live and no valid leg has a hit.
 * A DEAD set -- live_in[s] == 0 (uint8, nsets, device for _dev and host for _cpu, may be NULL), or p outside [0, nposes) --
 * gets 0 / 255 / -inf and free 0; it touches no table and no angle.
 * Consequences: pen > 0 iff links != 0; with margin == 0 worst is a hit or 255; links == 0 (or three radii of 0) gives the
 * empty answer everywhere and free = live; a link wholly inside the cylinder has d = 0 and pen = radius[k]; free_out is
 * directly a live_in / pose_live of the other posed calls:
 * ... -> ik -> trunk_clearance -> self_clearance(live_in = free) -> leg_clearance(live_in = free).
 * Checked first, in lrm_self_clearance_posed_dev's order and by its rules (all LRM_EINVAL): nlegs outside 1..LRM_MAX_LEGS; nsets
 * or nposes > INT32_MAX, or nlegs * nsets past 2^32 - 1; a radius, margin or tip_clear that is nan, negative or infinite (NULL
 * radius too); pose_idx == NULL with nsets > nposes; then a nan or infinite trunk_radius, plus_z or minus_z; trunk_radius < 0;
 * plus_z <= minus_z; a links bit at or above 3.  Then nsets == 0 is a no-op; a NULL table, angle array, links_out or worst_out
 * gives LRM_EINVAL.
 * lrm_trunk_clearance_posed_dev: ONE launch, a lane per (set, leg): no allocation, no host synchronisation, no atomics, no
 * shared buffer -- it can be captured in a graph and may run concurrently with anything, the pair kernels included, from any
 * host thread.  Bit-deterministic; the answer of a leg depends on its own record and angles only.
 * lrm_trunk_clearance_posed_cpu: host quats (nposes x 4), legs and angles_aos (nlegs * nsets triples {coxa, femur, tibia} at
 * [l*nsets + s]), host pose_idx and live_in; it compiles its own tables and runs a serial loop over every (set, leg) with the
 * same functions: the reference the GPU tests compare with bit for bit; *ms = the loop's time. */
int lrm_trunk_clearance_posed_dev(const void* workspace, const void* ik_workspace, size_t nposes, size_t nlegs,
                                  const int32_t* pose_idx /* device, nsets, may be NULL */, size_t nsets,
                                  const float* coxa, const float* femur, const float* tibia /* device, nlegs*nsets at [l*nsets + s] */,
                                  const float radius[3] /* host */, float margin, float tip_clear,
                                  float trunk_radius, float plus_z, float minus_z, uint8_t links,
                                  const uint8_t* live_in /* device, nsets, may be NULL */,
                                  uint8_t* links_out, uint8_t* worst_out, float* pen_out /* may be NULL */,
                                  uint8_t* free_out /* nsets, may be NULL */, void* stream);
int lrm_trunk_clearance_posed_cpu(const float* quats, size_t nposes, const LrmLegDimensions* legs, size_t nlegs,
                                  const int32_t* pose_idx /* host, may be NULL */, size_t nsets, const float* angles_aos,
                                  const float radius[3], float margin, float tip_clear,
                                  float trunk_radius, float plus_z, float minus_z, uint8_t links,
                                  const uint8_t* live_in /* host, may be NULL */, uint8_t* links_out, uint8_t* worst_out,
                                  float* pen_out, uint8_t* free_out, double* ms);
/* PLANTED-FOOT REACH ALONG A POSE TRANSITION: lrm_foothold_edges_posed_dev tests an edge (a, b) at its two ENDS only; a leg's
 * workspace is not convex, so a foothold reachable under pose a and under pose b can be out of reach on the way.  This call
 * samples the way: per (edge, leg) with a planted foot it evaluates nsamples = S poses between a and b (2 <= S <= 64, the ends
 * included) and says at which of them the foot is reachable.  The reference has no such query.  It takes NO workspace and reads
 * no table: the cloud, the quats (nposes x 4) and body (nposes x 3, NULL = 0) that lrm_pose_compile_dev reads (device for _dev),
 * the legs (host, 1..LRM_MAX_LEGS), edge_a / edge_b (int32, nedges), foot (int32, [l*nedges + e]: lrm_foothold_edges_posed_dev's
 * best_out as it stands, -1 = the leg is in the air) and live_in (uint8, nedges, may be NULL).
 * Everything is float32 without contraction, only + - * /, comparisons and the correctly rounded square root on top of the head
 * compiler and the strict evaluation: device and host give the same bits (csrc/lrm_edge_transit.h is the one source of both).
 * Sample s of edge e, with a = edge_a[e], b = edge_b[e], qa = quats[a], qb = quats[b], ba = body[a], bb = body[b]:
 *   u = (float)s / (float)(S - 1); w = 1 - u;
 *   dot = ((qa0*qb0 + qa1*qb1) + qa2*qb2) + qa3*qb3; sg = dot < 0 ? -1 : +1 (a nan dot gives +1);
 *   m_i = w*qa_i + u*(sg*qb_i); n2 = ((m0*m0 + m1*m1) + m2*m2) + m3*m3; q_i = m_i / sqrt(n2);
 *   body_i = ba_i + u*(bb_i - ba_i).
 *   Samples 0 and S-1 are NOT computed this way: they are quats[a], body[a] and quats[b], body[b] themselves, bit for bit and not
 *   normalised, so they equal the posed calls on those poses.  The normalised blend traces the same great arc as slerp (it stays
 *   in the plane of qa and sg*qb); only the speed along the arc differs: slower than slerp near the ends, faster in the middle.
 *   A degenerate interior quaternion (n2 = 0, nan, inf) is evaluated as it comes out.
 * PLANTED: (e, l) is planted iff the edge is live (live_in NULL or live_in[e] != 0), a and b lie in [0, nposes) and
 *   0 <= foot[o] < nt, o = l*nedges + e.  An edge that is not live or has an end out of range is DEAD.
 * Per sample of a planted leg: p_s = t[foot[o]] - body_s (one subtraction per component); r_s = reachability_global(p_s, legs[l],
 *   q_s): the strict evaluation on lrm_compile_head(legs[l], q_s, 1) whatever lrm_set_mode says, exactly as
 *   lrm_reach_dist_posed_* answers a pose with that quaternion and body.  Where r_s = 0, d2_s = (dx*dx + dy*dy) + dz*dz of
 *   distance_global's vector (its validity byte is not consulted); a nan d2 is compared and stored as +inf.
 * Outputs per (edge, leg) at [l*nedges + e], all written:
 *   mask_out       (uint64, may be NULL) bit s = r_s; 0 when not planted;
 *   reached_out    (int32) the number of set bits; -1 when not planted;
 *   first_miss_out (int32) the smallest s with r_s = 0; -1 if none or not planted;
 *   worst_out      (int32, may be NULL) the unreachable sample with the largest d2, ties to the smaller s; -1 if none;
 *   worst_d2_out   (float, may be NULL) that d2; 0 if none;
 * and per edge:
 *   planted_out (uint8, may be NULL) bit l set iff leg l is planted;
 *   clear_out   (uint8, may be NULL) 1 iff the edge is not dead and every planted leg has reached == S.  An edge without a planted
 *               leg is clear: planted_out tells.  The byte is directly a live_in of the other posed calls;
 *   advance_out (int32, may be NULL) the number of leading samples at which every planted leg reaches: the minimum over the
 *               planted legs of first_miss, S where none misses -- how far the body gets before some foot must be lifted.
 *               0 for a dead edge.
 * Consequences: a == b makes every interior sample the pose's own quaternion, normalised (equal to the ends up to rounding), on
 * the pose's own body: the mask is all ones or zero unless the target lies within rounding of the workspace boundary; with foot = lrm_foothold_edges_posed_dev's best, bits 0
 * and S-1 of every planted entry are set; swapping the ends reverses the mask whenever (S-1-s)/(S-1) is the same float as
 * 1 - s/(S-1) for every s (S = 2, 3, 5, 9, 17, 33: S-1 a power of two).
 * Checked first, in this order (all LRM_EINVAL): nlegs outside 1..LRM_MAX_LEGS; nsamples outside 2..64; nt or nposes > INT32_MAX;
 * nedges * nlegs past 2^32 - 1.  Then nedges == 0 is a no-op.  Then a NULL quats, legs, edge_a, edge_b, foot, reached_out or
 * first_miss_out, or a NULL cloud with nt > 0, gives LRM_EINVAL.  nt == 0 plants nothing.  Any contents of edge_a, edge_b and foot
 * are safe: an index is checked before an address is formed from it.
 * lrm_edge_transit_posed_dev: ONE launch, a lane per (edge, sample): no allocation, no host synchronisation, no atomics, no shared
 * buffer, no table -- it can be captured in a graph and may run concurrently with anything from any host thread.
 * Bit-deterministic; the answer of an (edge, leg) depends on its own inputs only.
 * lrm_edge_transit_posed_cpu: AoS targets, host arrays, a serial loop over every (edge, leg, sample) with the same functions: the
 * reference the GPU tests compare with bit for bit; *ms = the loop's time.
 * Chain: update -> footholds -> foothold_edges -> edge_transit -> ik / stance_stability(live_in = clear). */
int lrm_edge_transit_posed_dev(const float* tx, const float* ty, const float* tz, size_t nt, const float* quats /* device */,
                               const float* body /* device, may be NULL */, size_t nposes, const LrmLegDimensions* legs /* host */,
                               size_t nlegs, const int32_t* edge_a, const int32_t* edge_b /* device, nedges */, size_t nedges,
                               const int32_t* foot /* device, nlegs*nedges at [l*nedges + e] */, size_t nsamples,
                               const uint8_t* live_in /* device, nedges, may be NULL */, uint64_t* mask_out /* may be NULL */,
                               int32_t* reached_out, int32_t* first_miss_out, int32_t* worst_out /* may be NULL */,
                               float* worst_d2_out /* may be NULL */, uint8_t* planted_out /* nedges, may be NULL */,
                               uint8_t* clear_out /* nedges, may be NULL */, int32_t* advance_out /* nedges, may be NULL */,
                               void* stream);
int lrm_edge_transit_posed_cpu(const float* targets_aos, size_t nt, const float* quats, const float* body /* may be NULL */,
                               size_t nposes, const LrmLegDimensions* legs, size_t nlegs, const int32_t* edge_a, const int32_t* edge_b,
                               size_t nedges, const int32_t* foot, size_t nsamples, const uint8_t* live_in /* may be NULL */,
                               uint64_t* mask_out, int32_t* reached_out, int32_t* first_miss_out, int32_t* worst_out,
                               float* worst_d2_out, uint8_t* planted_out, uint8_t* clear_out, int32_t* advance_out, double* ms);
/* SWING-FOOT TRANSIT: REACH AND TERRAIN CLEARANCE OF A LIFTED FOOT.  lrm_edge_transit_posed_dev samples a pose transition for the feet
 * that stay planted; this call does it for the leg that is LIFTED: during the step from pose a to pose b the swinging foot leaves
 * target foot_from and lands on target foot_to, along a straight line with a parabolic bump of height `lift` along `up`.  Per
 * (edge, leg) it says at which of the S sampled poses the moving foot is reachable, and which terrain targets stand within
 * foot_radius of the polyline the foot travels along.  The reference has no such query.  No workspace and no table.
 * The cloud, quats, body, legs, edge_a, edge_b, nsamples = S (2..64) and live_in are exactly lrm_edge_transit_posed_dev's.  Further:
 *   foot_from, foot_to (int32, [l*nedges + e], device for _dev): the target on which leg l stands under pose a and the one on which
 *     it lands under pose b.  (e, l) is SWINGING iff the edge is live, a and b lie in [0, nposes) and both indices lie in [0, nt).
 *     from == to is allowed (lift and put down).  A leg with either index outside the cloud (-1, say) is not swinging: callers pass
 *     -1 for the planted legs, which stay lrm_edge_transit_posed_dev's business.
 *   lift (finite, any sign); up (host float[3], NULL = (0, 0, 1), finite, used as given and NOT normalised);
 *   foot_radius (>= 0, finite; 0 = no terrain test at all); margin (>= 0, finite); skip (0..63).
 * Everything is float32 without contraction, only + - * /, comparisons and the correctly rounded square root on top of the head
 * compiler and the strict evaluation: device and host give the same bits (csrc/lrm_swing.h is the one source of both).
 *   A = t[from], B = t[to], D = B - A (one subtraction per component).
 *   Path point of sample s RELATIVE TO A: P_0 = 0, P_{S-1} = D; for an interior sample u = (float)s / (float)(S - 1), w = 1 - u,
 *     h = lift * ((4*u) * w), P_s.c = u*D.c + h*up.c (two multiplications, one addition).
 *   Pose of sample s: lrm_edge_transit_posed_dev's q_s, body_s (the ends are the table's own rows, bit for bit).
 *   Foot of sample s: F_0 = A and F_{S-1} = B themselves, an interior F_s = A + P_s (one addition per component).
 *   p_s = F_s - body_s; r_s and, where it is 0, d2_s as lrm_edge_transit_posed_dev forms them (a nan d2 as +inf).
 * Terrain test, only when foot_radius > 0: segment k runs from P_k to P_{k+1} and is tested for skip <= k < S-1-skip (skip keeps the
 *   take-off and the landing, where the foot is at the ground by definition, out of the test; with 2*skip >= S-1 nothing is tested).
 *   Target i, except i == from and i == to, is tested with q = t_i - A (one subtraction per component) and d_k = the distance of q to
 *   segment k: lrm_leg_clearance_posed_dev's function and clamping rule with a = P_k, ab = P_{k+1} - P_k, den = |ab|^2.
 *   hit = d_k < foot_radius; near = d_k < foot_radius + margin (the sum formed once); pen = foot_radius - d_k (-0 as +0); a nan d is
 *   neither.  If any tested path point P_skip .. P_{S-1-skip} is not finite the leg's terrain part is skipped with the empty answer;
 *   its reach part still decides clear.
 * Outputs per (edge, leg) at [l*nedges + e], all written:
 *   mask_out (uint64, may be NULL), reached_out, first_miss_out, worst_out (may be NULL), worst_d2_out (may be NULL): exactly
 *     lrm_edge_transit_posed_dev's meaning and encodings with "swinging" in place of "planted" (0 / -1 / -1 / -1 / 0 when not);
 *   hits_out    (int32) the number of targets with a hit on some tested segment;
 *   hit_seg_out (int32) the smallest tested k with a hit, -1 if none;
 *   near_out    (int32) the near target with the largest pen (over targets, then over its segments), ties to the smaller index,
 *               -1 if none;
 *   pen_out     (float, may be NULL) that pen, -inf if none;
 *   a leg that is not swinging gets 0 / -1 / -1 / -inf for these four;
 * and per edge:
 *   swinging_out (uint8, may be NULL) bit l set iff leg l is swinging;
 *   clear_out    (uint8, may be NULL) 1 iff the edge is not dead and every swinging leg has reached == S and hits == 0.  The byte is
 *                directly a live_in of the other posed calls.
 * Consequences: with lift = 0, from == to (a finite target) and foot_radius = 0 every reach output equals lrm_edge_transit_posed_*
 * with foot = from, bit for bit (swinging_out = its planted_out, clear_out = its clear_out); hits > 0 iff hit_seg >= 0 iff pen > 0.
 * Checked first, in this order (all LRM_EINVAL): lrm_edge_transit_posed_dev's range checks; a nan or infinite lift, foot_radius or
 * margin; a negative foot_radius or margin; skip > 63; a non-finite up.  Then nedges == 0 is a no-op.  Then a NULL quats, legs, edge_a,
 * edge_b, foot_from, foot_to, reached_out, first_miss_out, hits_out, hit_seg_out or near_out, or a NULL cloud with nt > 0, gives
 * LRM_EINVAL.  nt == 0 lets nothing swing.  Any contents of the index arrays are safe: an index is checked before an address is
 * formed from it.
 * lrm_swing_transit_posed_dev: the reach kernel (a lane per (edge, sample)) and, when something is tested, the terrain kernel (a
 * wave per edge walks the cloud's boxes and culls against the path's box about A; the cull never changes an answer): at most two
 * launches behind the boxes' own, no atomics, bit-deterministic, no host synchronisation.  With foot_radius = 0 no box buffer is
 * read: the call only launches and may run concurrently with anything from any host thread.  With foot_radius > 0 and nt >= 4096 it
 * fills and reads the per-device tile-box buffer and so is one of the PAIR KERNELS, with lrm_footholds_posed_dev's rules: one host
 * thread at a time, no two pair launches on different clouds concurrently on one device, and an allocation only when the cloud is
 * larger than the buffer holds -- after one call on a cloud of the largest size it only launches and can be captured in a graph and
 * replayed with new feet.  It does not use the compiled-leg slots.
 * lrm_swing_transit_posed_cpu: AoS targets, host arrays, a serial loop with the same functions over every (edge, leg, sample) and
 * every (target, segment) WITHOUT any cull: the reference the GPU tests compare with bit for bit; *ms = the loop's time.
 * Chain: update -> footholds -> foothold_edges -> edge_transit -> swing_transit(live_in = clear) -> ik / stance_stability. */
int lrm_swing_transit_posed_dev(const float* tx, const float* ty, const float* tz, size_t nt, const float* quats /* device */,
                                const float* body /* device, may be NULL */, size_t nposes, const LrmLegDimensions* legs /* host */,
                                size_t nlegs, const int32_t* edge_a, const int32_t* edge_b /* device, nedges */, size_t nedges,
                                const int32_t* foot_from, const int32_t* foot_to /* device, nlegs*nedges at [l*nedges + e] */,
                                size_t nsamples, float lift, const float* up /* host float[3], may be NULL */, float foot_radius,
                                float margin, uint32_t skip, const uint8_t* live_in /* device, nedges, may be NULL */,
                                uint64_t* mask_out /* may be NULL */, int32_t* reached_out, int32_t* first_miss_out,
                                int32_t* worst_out /* may be NULL */, float* worst_d2_out /* may be NULL */, int32_t* hits_out,
                                int32_t* hit_seg_out, int32_t* near_out, float* pen_out /* may be NULL */,
                                uint8_t* swinging_out /* nedges, may be NULL */, uint8_t* clear_out /* nedges, may be NULL */,
                                void* stream);
int lrm_swing_transit_posed_cpu(const float* targets_aos, size_t nt, const float* quats, const float* body /* may be NULL */,
                                size_t nposes, const LrmLegDimensions* legs, size_t nlegs, const int32_t* edge_a, const int32_t* edge_b,
                                size_t nedges, const int32_t* foot_from, const int32_t* foot_to, size_t nsamples, float lift,
                                const float* up /* may be NULL */, float foot_radius, float margin, uint32_t skip,
                                const uint8_t* live_in /* may be NULL */, uint64_t* mask_out, int32_t* reached_out,
                                int32_t* first_miss_out, int32_t* worst_out, float* worst_d2_out, int32_t* hits_out, int32_t* hit_seg_out,
                                int32_t* near_out, float* pen_out, uint8_t* swinging_out, uint8_t* clear_out, double* ms);
/* STATIC FOOT LOADS AND JOINT TORQUES per set and lift set: can the actuators hold the stance.  lrm_stance_stability_dev says
 * that the centre of mass lies over the support polygon and lrm_ik_posed_dev gives the joint angles; neither says what every
 * planted foot carries, nor what the coxa, femur and tibia joints must hold when a leg or a tripod is lifted.  The reference has
 * no such query.  THE MODEL: contacts are frictionless points; every planted foot pushes along `up` only; THE LEGS ARE MASSLESS
 * (link weights are ignored: the whole weight acts at the centre of mass); the weight is 1, so loads are fractions of the
 * robot's weight and torques are load x mm -- the caller multiplies both by m g.  The call reads no cloud and no body position
 * (the feet are the FK tips relative to the body): `workspace` and `ik_workspace` are the pose table and the IK table of
 * lrm_self_clearance_posed_dev, and sets, pose_idx, nposes, nlegs and the angles at [l*nsets + s] are that call's; com, plane,
 * lift, nmasks and live_in are lrm_stance_stability_dev's; quats (nposes x 4) is read for the centre of mass only.  Everything
 * is float32 without contraction, only + - * /, comparisons, the correctly rounded square root and the sincos of the IK: device
 * and host give the same bits (csrc/lrm_stance_loads.h is the one source of both).
 * Leg l of set s: J0..J3 are lrm_leg_clearance_posed_dev's joints with tip_clear = 0; the leg is VALID iff its twelve
 *   coordinates are finite; its foot is P = J3 (relative to the body) and its plane point f_l is lrm_stance_stability_dev's
 *   projection of P.  c is that call's centre of mass, and a set is DEAD under that call's rules: live_in[s] == 0, p outside
 *   [0, nposes), or c not finite.  up = (0, 0, 1) with plane == NULL, else u x v = (u.y v.z - u.z v.y, u.z v.x - u.x v.z,
 *   u.x v.y - u.y v.x), formed once per call.  xi_l = f_l.x - c.x, eta_l = f_l.y - c.y.
 * Lever arms: with (sc, cc), (sf, cf), (sa, ca) the sincos of coxa, femur and femur + tibia, C, F, T the link lengths of the
 *   joints (T = 0 unless T > 0), ts = T sa, tc = T ca, v = F sf + ts, w = F cf + tc, h3 = C + w, the columns of the tip's
 *   Jacobian in the coxa frame are col_c = (-sc h3, cc h3, 0), col_f = (-cc v, -sc v, w), col_t = (-cc ts, -sc ts, tc) (the
 *   negation applies to the sine or cosine before the product).  Lin is the coxa-frame-to-caller's-frame chain of the joints
 *   WITHOUT its translation by body_length (a direction, not a point), and g_j = (up.x a.x + up.y a.y) + up.z a.z with
 *   a = Lin(col_j): how fast the foot rises along `up` per radian of joint j.  tau_j = load g_j is the moment of the ground
 *   force about joint j in the angle's positive sense; the actuator holds the opposite.
 * Loads of lift set m: the planted set is S = valid & ~lift[m].  Three stages, in order:
 *   ALL (status 1): over the feet of A = S in ascending leg order the six sums n = sum 1, sx = sum xi, sy = sum eta,
 *     sxx = sum xi xi, sxy = sum xi eta, syy = sum eta eta; c00 = sxx syy - sxy sxy, c01 = sxy sy - sx syy,
 *     c02 = sx sxy - sxx sy, det = (n c00 + sx c01) + sy c02, which must be > 0 and < inf; alpha = c00 / det, beta = c01 / det,
 *     gamma = c02 / det; load_i = (alpha + beta xi_i) + gamma eta_i: the minimum-norm solution of sum load = 1,
 *     sum load xi = 0, sum load eta = 0.  Accepted iff every load >= 0 (a nan is not).
 *   DROPPED (status 2): while the solve is not accepted, its det passed and A has more than three feet, the foot of A with the
 *     smallest load leaves A (the first foot of A, replaced by a later one only if that is strictly smaller: ties to the
 *     smaller leg; a nan is never smaller) and the solve is repeated on A.  Removed feet get load +0.
 *   TRIPOD (status 3), entered when a det fails or three feet remain with a load not >= 0: every triple i < j < k of S (not
 *     of A) in lexicographic order; d = (xi_j - xi_i)(eta_k - eta_i) - (xi_k - xi_i)(eta_j - eta_i) must be nonzero and
 *     finite; l_i = (xi_j eta_k - xi_k eta_j) / d, l_j = (xi_k eta_i - xi_i eta_k) / d, l_k = (xi_i eta_j - xi_j eta_i) / d;
 *     the triple counts iff all three are >= 0; the triple with the largest minimum wins, the first one on ties; the other
 *     feet get +0.
 *   Otherwise -- fewer than three planted feet, or no stage succeeds -- status 4: the feet of S get load and torques nan
 *     (0x7fc00000).  A dead set has status 0 for every m and no planted foot.
 *   Statuses 1..3 mean that an equilibrium with non-negative loads exists (by Caratheodory's theorem the tripod stage finds
 *   one whenever there is one), up to rounding; they do not mean that the loads are the ones a compliant robot settles into.
 * Outputs, all written:
 *   status_out, holdable_out (uint8) at [m*nsets + s]: holdable = status in 1..3 and |tau_j| <= tau_max[j] for every planted
 *             leg and joint; a row of holdable_out is a valid live_in of the other posed calls;
 *   peak_out    (float) at [m*nsets + s]: with status 1..3 the largest |tau_j| / tau_max[j] over the planted legs, else -inf;
 *   peak_at_out (uint8, may be NULL) its code l*4 + j, ties to the smaller code (a nan ratio never wins), 255 with -inf;
 *   load_out    (float, may be NULL) at [(m*nlegs + l)*nsets + s];
 *   tau_out     (float, may be NULL) at [((m*nlegs + l)*3 + j)*nsets + s].
 *   Lifted and invalid legs get load +0 and tau +0; a stored -0 is +0 and a stored nan is 0x7fc00000.
 * tau_max: host float[3] (coxa, femur, tibia), each > 0, +inf allowed (that joint never limits: its ratio is 0, or nan for an
 * infinite torque).
 * Checked first, in this order (all LRM_EINVAL): nlegs outside 1..LRM_MAX_LEGS; nmasks outside 1..256; nposes or nsets >
 * INT32_MAX; nmasks * nlegs * 3 * nsets past 2^32 - 1; NULL lift; a lift bit at or above nlegs; NULL tau_max, or an entry that
 * is nan or <= 0; a non-finite com or plane value; pose_idx == NULL with nsets > nposes.  Then nsets == 0 is a no-op; a NULL
 * table, quats, angle array, status_out, holdable_out or peak_out gives LRM_EINVAL.
 * lrm_stance_loads_posed_dev: ONE launch (with up to eight lift sets a lane per set, from nine on a wave per set and a lane per
 * lift set; the same functions and the same bits either way): no allocation, no host synchronisation, no
 * atomics, no shared buffer -- it can be captured in a graph and may run concurrently with anything, from any host thread.
 * Bit-deterministic.
 * lrm_stance_loads_posed_cpu: host quats, legs and angles_aos (nlegs * nsets triples {coxa, femur, tibia} at [l*nsets + s]);
 * it compiles its own tables and runs a serial loop over every (set, lift set) with the same functions: the reference the GPU
 * tests compare with bit for bit; *ms = the loop's time.
 * Chain: ... -> ik -> stance_loads -> stance_stability / self_clearance(live_in = a holdable row). */
#define LRM_LOADS_DEAD 0
#define LRM_LOADS_ALL 1
#define LRM_LOADS_DROPPED 2
#define LRM_LOADS_TRIPOD 3
#define LRM_LOADS_NONE 4
int lrm_stance_loads_posed_dev(const void* workspace, const void* ik_workspace, const float* quats /* device, nposes x 4 */,
                               size_t nposes, size_t nlegs, const int32_t* pose_idx /* device, nsets, may be NULL */, size_t nsets,
                               const float* coxa, const float* femur, const float* tibia /* device, nlegs*nsets at [l*nsets + s] */,
                               const float* com /* host, 3, may be NULL */, const float* plane /* host, 6, may be NULL */,
                               const uint8_t* lift /* host, nmasks */, size_t nmasks, const float* tau_max /* host, 3 */,
                               const uint8_t* live_in /* device, nsets, may be NULL */, uint8_t* status_out, uint8_t* holdable_out,
                               float* peak_out, uint8_t* peak_at_out /* may be NULL */, float* load_out /* may be NULL */,
                               float* tau_out /* may be NULL */, void* stream);
int lrm_stance_loads_posed_cpu(const float* quats, size_t nposes, const LrmLegDimensions* legs, size_t nlegs,
                               const int32_t* pose_idx /* host, may be NULL */, size_t nsets, const float* angles_aos,
                               const float* com, const float* plane, const uint8_t* lift, size_t nmasks, const float* tau_max,
                               const uint8_t* live_in /* host, may be NULL */, uint8_t* status_out, uint8_t* holdable_out,
                               float* peak_out, uint8_t* peak_at_out, float* load_out, float* tau_out, double* ms);

/* ---- pose-graph routes: cost, hops and predecessor per pose ------------------------------------------------------------
 * New capability: every posed call ends in a byte per pose (all_legs, free, stable, holdable) or per transition (all_legs of
 * lrm_foothold_edges_posed_dev, clear of the transit calls); this call composes them into the answer: which poses the robot
 * can get to from where it stands, in how many steps and at what cost, and through which transition it arrives.  Single- or
 * multi-source shortest routes over the caller's pose graph with INTEGER costs; the answer is bit-deterministic and the same
 * on device and host (csrc/lrm_pose_routes.h is the one source of both).  The reference has no such query.
 * Inputs (device pointers for _dev, host pointers for _cpu):
 *   nposes;  edge_a, edge_b (int32, nedges): the arrays the edge calls take;
 *   edge_live (uint8, nedges, may be NULL): a clear or all_legs byte as it stands, 0 = dead;
 *   pose_live (uint8, nposes, may be NULL): a free, stable or holdable row, 0 = dead;
 *   edge_cost (int32, nedges, may be NULL = 1 for every edge, so that cost equals hops); a negative cost makes the edge dead;
 *   sources (int32, nsources);
 *   direction: 0 an edge serves both ways; 1 a -> b only; 2 b -> a only (with the goal as source: the cost-to-go field and
 *     the next edge towards the goal).
 * USABLE: edge e is usable iff it is live, both ends lie in [0, nposes), both ends are live poses and its cost is >= 0.
 * SOURCE: a pose named in sources is a source iff it is in range and live; duplicates, dead and out-of-range entries are
 *   ignored.
 * KEY of pose v: the lexicographic minimum of (sum of costs, number of arcs) over all walks from a source along arcs of usable
 *   edges whose sum of costs is <= 4 294 967 294.  Costs are integers, so addition is exact, every prefix of a minimal walk is
 *   minimal, and the key is the unique least fixed point of key[v] = min(key[v], key[u] + (w_e, 1)) -- the same in whatever
 *   order the relaxations happen.  Zero-cost cycles and self-loops never lower a key: the arc count is the tie-break.
 * Outputs per pose, all written (each of the four may be NULL, but not all of them):
 *   cost_out      (int64) the sum of costs, -1 if unreachable;
 *   hops_out      (int32) the number of arcs, -1 if unreachable;
 *   pred_edge_out (int32) the smallest usable e that has an arc u -> v with key[u] + (w_e, 1) == key[v]; -1 for a source and
 *                 for an unreachable pose;
 *   pred_pose_out (int32) that arc's u, or -1.  Following pred_pose from any reached pose ends at a source after exactly
 *                 hops steps.
 * Outputs per call: reached_out (int32[1], may be NULL) the number of poses with hops >= 0; done_out (int32[1], _dev only, may
 *   be NULL): >= 1 when the fixed point was proven within `rounds` relaxation launches (the number of launches that did work;
 *   only its sign is a contract), -1 otherwise.  With -1 the per-pose outputs are written and memory-safe but unspecified,
 *   and the workspace holds the state: a further call with resume = 1 and otherwise equal arguments continues from it.  The
 *   fixed point is unique, so the final answer is the same bits however the work was cut.
 * lrm_pose_routes_dev further takes workspace (device, lrm_pose_routes_workspace_bytes(nposes, rounds) bytes, 8-byte aligned:
 *   the 64-bit keys and one flag per launch), rounds (1..4096), resume (0 or 1) and the stream.  It launches init, seed,
 *   `rounds` relax launches and up to three finish launches back to back: no allocation, no host synchronisation, no wait of
 *   one workgroup for another (no grid barrier, no cooperative launch, no loop on memory) -- it can be captured in a graph as
 *   one linear chain.  Relax launch i returns at once when launch i - 1 changed nothing.  Calls on different streams need
 *   different workspaces and outputs.  All atomics are integer min / add.
 * Checked first, in this order (all LRM_EINVAL): direction outside 0..2; rounds outside 1..4096; resume outside 0..1; nposes,
 *   nedges or nsources > INT32_MAX.  Then nposes == 0 is a no-op that still writes reached_out = 0 and done_out = 1.  Then
 *   NULL (or misaligned) workspace; NULL edge_a or edge_b with nedges > 0; NULL sources with nsources > 0; all four per-pose
 *   outputs NULL give LRM_EINVAL.  nedges == 0 and nsources == 0 are valid: only the sources, or nothing, are reached.  Any
 *   contents of edge_a, edge_b and sources are safe: an index is checked before an address is formed from it.
 * lrm_pose_routes_cpu: the same without workspace, rounds, resume and done_out; it always finishes: a binary-heap Dijkstra on
 *   the keys over a counting-sorted arc list, then the predecessor by the rule above in a loop over the edges: the reference
 *   the GPU tests compare with bit for bit; *ms = its time.
 * lrm_dbg_pose_routes_plan: the launch arithmetic of a relax launch on nedges edges, from the function the launch itself
 *   consumes (host only): out = {edges per workgroup C, grid cap G, sweeps per launch K, workgroups launched}.
 * Chain: ... -> foothold_edges -> edge_transit -> swing_transit -> routes(edge_live = clear, pose_live = all_legs). */
size_t lrm_pose_routes_workspace_bytes(size_t nposes, size_t rounds);
int lrm_pose_routes_dev(size_t nposes, const int32_t* edge_a, const int32_t* edge_b, size_t nedges,
                        const uint8_t* edge_live /* may be NULL */, const uint8_t* pose_live /* may be NULL */,
                        const int32_t* edge_cost /* may be NULL */, const int32_t* sources, size_t nsources, int direction,
                        void* workspace, size_t rounds, int resume, int64_t* cost_out, int32_t* hops_out, int32_t* pred_edge_out,
                        int32_t* pred_pose_out, int32_t* reached_out, int32_t* done_out, void* stream);
int lrm_pose_routes_cpu(size_t nposes, const int32_t* edge_a, const int32_t* edge_b, size_t nedges, const uint8_t* edge_live,
                        const uint8_t* pose_live, const int32_t* edge_cost, const int32_t* sources, size_t nsources, int direction,
                        int64_t* cost_out, int32_t* hops_out, int32_t* pred_edge_out, int32_t* pred_pose_out, int32_t* reached_out,
                        double* ms);
int lrm_dbg_pose_routes_plan(size_t nedges, uint64_t out[4]);

/* ---- pose-graph edges: neighbour poses within a step and a turn, in CSR ---------------------------------------------------
 * New capability: every edge call above takes edge_a / edge_b from the caller; these calls build them on the device from the
 * poses alone -- which pose can step to which -- so the chain update -> edges -> footholds -> foothold_edges -> edge_transit
 * -> swing_transit -> routes starts on the device and can be captured in a graph.  The answer is bit-deterministic and the
 * same on device and host (csrc/lrm_pose_edges.h is the one source of both); it does not depend on the order of the poses
 * beyond their labels.  The reference has no such query.
 * Inputs (device pointers for _dev, host pointers for _cpu):
 *   quats (float32, nposes x 4, in storage order q[0..3]);  body (float32, nposes x 3, may be NULL = 0 for every pose);
 *   pose_live (uint8, nposes, may be NULL): 0 = dead;
 *   max_step (host float, mm, >= 0, may be +inf);  min_dot (host float in [0, 1]): the cosine of half the largest turn, 0
 *     disables the turn test.  step2 = max_step*max_step and dot2 = min_dot*min_dot, one float32 product each.
 * All arithmetic is float32 without contraction in the order written here.
 * VALID: pose p is valid iff it is live, its three body coordinates are finite, and
 *   n_p = ((q0*q0 + q1*q1) + q2*q2) + q3*q3 is finite and > 0.
 * NEIGHBOURS: (p, q) with p != q are neighbours iff both are valid and
 *   d2 = (dx*dx + dy*dy) + dz*dz <= step2, with dx = body[q].x - body[p].x and so on, and
 *   c*c >= dot2 * (n_p * n_q), with c = ((p0*q0 + p1*q1) + p2*q2) + p3*q3.
 *   Every comparison with a NaN is false (so two poses whose n_p * n_q overflows are never neighbours).  q and -q are the
 *   same orientation: the test uses c*c.  The relation is SYMMETRIC BIT FOR BIT: x_q - x_p is the exact negative of
 *   x_p - x_q, and c and n_p * n_q do not depend on which pose is named first; d2 and cos2 of (p, q) are those of (q, p).
 * form: 0 row p holds the neighbours q > p, so every unordered pair appears once (what lrm_pose_routes_dev with
 *   direction = 0 wants); 1 row p holds all neighbours q != p, an adjacency list: the exact symmetrisation of form 0.
 * The two-step CSR: lrm_pose_edge_counts_dev -> lrm_foothold_offsets_dev -> lrm_pose_edges_dev.
 *   count_out    (int32, nposes) the number of entries of row p;
 *   segment      base = offsets[p]; room = min(offsets[p+1], (int64)capacity) - base, and 0 if that is negative or base < 0
 *                (lrm_foothold_lists_posed_dev's rule);
 *   edge_a_out, edge_b_out (int32, capacity) row p's neighbours in ASCENDING q, the first min(count, room) of them at
 *                base + k: edge_a_out = p, edge_b_out = q;
 *   d2_out       (float32, capacity, may be NULL) at the same positions the d2 above;
 *   cos2_out     (float32, capacity, may be NULL) (c*c) / (n_p*n_q), one IEEE division: the squared cosine of half the turn;
 *   written_out  (int32, nposes, may be NULL) written_out[p] = min(count, room).
 * No element outside [base, base + room) is ever written, and every other element keeps its value.  ANY offsets array is
 * memory-safe: decreasing, negative and overlapping offsets never cause a write outside the buffers, only a shorter row.
 * With offsets made from count_out and capacity >= offsets[nposes] every row is whole and the edge list is sorted by (a, b).
 * THE LAUNCH-ONLY IDIOM: prefill edge_a_out with -1, pass a fixed capacity to lrm_pose_edges_dev, and pass that capacity as
 * nedges to the edge calls: every one of them treats an end outside [0, nposes) as a dead edge, so the tail beyond
 * offsets[nposes] is inert and the chain needs no read-back of offsets[nposes].
 * lrm_pose_edges_workspace_bytes(nposes): the bytes of `workspace` (device, 16-byte aligned): one bounding box per chunk of
 *   64 consecutive poses and one per 64 chunks.  Both device calls launch their own box kernels, so neither depends on the
 *   other having run; they make no allocation and no host synchronisation, no workgroup waits for another, there are no
 *   atomics, and both can be captured in a graph.  Calls on different streams need different workspaces.  The cull by the boxes is exact (the gap of
 *   two boxes, squared and summed in d2's order, is a lower bound of every pair's computed d2), so the answer does not depend
 *   on how tight the boxes are; a cloud in Morton order (lrm_morton_order) makes them tight and the call fast.
 * Checked first, in this order (all LRM_EINVAL): form outside 0..1; nposes > INT32_MAX; max_step NaN or negative; min_dot NaN
 *   or outside [0, 1].  Then nposes == 0 is a no-op.  Then NULL quats, workspace (or one not 16-byte aligned), count_out
 *   (counts call), offsets, edge_a_out or edge_b_out (fill call) give LRM_EINVAL.  Then capacity == 0 writes written_out = 0
 *   everywhere and nothing else.
 * lrm_pose_edges_cpu: the same with host pointers and no workspace, counts and lists in one call: count_out may be NULL;
 *   offsets may be NULL when only the counts are asked for (then count_out must not be NULL and the list arguments are not
 *   read); with offsets, edge_a_out and edge_b_out must not be NULL.  A serial loop over every pair with no culling: the
 *   reference the GPU tests compare with bit for bit; *ms = the loop's time.
 * lrm_dbg_pose_edges_plan: the launch arithmetic of the count and fill kernels on nposes poses, from the function the launch
 *   itself consumes (host only): out = {poses per chunk, boxes per walk round, workgroups, block}.
 * Chain: update -> pose_edges -> footholds -> foothold_edges -> edge_transit -> swing_transit -> routes. */
size_t lrm_pose_edges_workspace_bytes(size_t nposes);
int lrm_pose_edge_counts_dev(const float* quats, const float* body /* may be NULL */, size_t nposes,
                             const uint8_t* pose_live /* may be NULL */, float max_step, float min_dot, int form, void* workspace,
                             int32_t* count_out, void* stream);
int lrm_pose_edges_dev(const float* quats, const float* body /* may be NULL */, size_t nposes,
                       const uint8_t* pose_live /* may be NULL */, float max_step, float min_dot, int form, void* workspace,
                       const int64_t* offsets /* device, nposes + 1 */, size_t capacity, int32_t* edge_a_out, int32_t* edge_b_out,
                       float* d2_out /* may be NULL */, float* cos2_out /* may be NULL */, int32_t* written_out /* may be NULL */,
                       void* stream);
int lrm_pose_edges_cpu(const float* quats, const float* body, size_t nposes, const uint8_t* pose_live, float max_step, float min_dot,
                       int form, int32_t* count_out /* may be NULL */, const int64_t* offsets /* host, may be NULL: counts only */,
                       size_t capacity, int32_t* edge_a_out, int32_t* edge_b_out, float* d2_out, float* cos2_out,
                       int32_t* written_out, double* ms);
int lrm_dbg_pose_edges_plan(size_t nposes, uint64_t out[4]);
/* host-buffer form of robot_full_struct's pipeline (several_leg.cu:326-877; AoS in, as its
 * Array<float3> arguments); quats is nquat x 4; body_mask_out[b] = 1 iff for SOME orientation
 * EVERY leg (limits rotated per orientation, bodies and targets rotated by the quaternion) has a
 * reachable target.  reference_culls != 0 additionally applies multi_rot_estimator's culls: the
 * one-time spheres (r = 60 collision, r = 400 far body / far target, :413-502) and the
 * per-orientation cylinder pair of eliminateFarAndColliding (:504-559).  reference_culls == 2 applies only the
 * per-orientation pair: for callers that shard the bodies over several GPUs and evaluate the one-time culls
 * themselves (the far-target cull depends on ALL surviving bodies; lrm_amd/shard.py).  *ms = kernel time. */
int lrm_positionability(const float* bodies_aos, size_t nb, const float* targets_aos, size_t nt,
                        const LrmLegDimensions* legs, size_t nlegs, const float* quats,
                        size_t nquat, int reference_culls, uint8_t* body_mask_out, float* ms);

/* lrm_positionability's orientation sweep on clouds that already live on the device (SoA float32), device-resident
 * masks in and out: no copies of the clouds, no reordering (feed Morton-ordered clouds).  reference_culls: 0 none, 2 the
 * per-orientation cylinder culls (the caller has applied multi_rot_estimator's one-time culls, several_leg.cu:413-502,
 * as the sharded drivers do).  active_in (device, may be NULL = every body): bodies with 0 are not tested;
 * accepted_out[nb] (device).  Null stream; returns when the device has finished; *ms = the sweep's kernel time. */
int lrm_positionability_dev(const float* bx, const float* by, const float* bz, size_t nb, const float* tx, const float* ty,
                            const float* tz, size_t nt, const LrmLegDimensions* legs, size_t nlegs, const float* quats,
                            size_t nquat, int reference_culls, const uint8_t* active_in, uint8_t* accepted_out, float* ms);
/* Morton (Z-curve) order of a host cloud: order_out[k] = index of the k-th point along the curve.
 * The pair kernels (lrm_reach_any_dev, lrm_any_in_*_dev) skip whole 1024-target tiles by bounding
 * box; feeding them clouds (and centres / bodies) in this order makes the boxes compact in any
 * orientation.  Results do not depend on the order.  lrm_positionability does this itself. */
int lrm_morton_order(const float* xyz_aos, size_t n, uint64_t* order_out);

/* in_sphere / in_cylinder any-reductions: launch_optimized_mem_in_sphere /
 * launch_optimized_mem_in_cylinder (collision.cu:68-98, :148-168):
 * out[c] = 1 iff some target lies in the sphere / cylinder centred on centre c. */
int lrm_any_in_sphere_dev(const float* cx, const float* cy, const float* cz, size_t nc,
                          const float* tx, const float* ty, const float* tz, size_t nt,
                          float radius, uint8_t* out, void* stream);
int lrm_any_in_cylinder_dev(const float* cx, const float* cy, const float* cz, size_t nc,
                            const float* tx, const float* ty, const float* tz, size_t nt,
                            float radius, float plus_z, float minus_z, uint8_t* out, void* stream);

/* ---- octree-culled positionability: apply_oct, several_leg_octree.cu:391-488 ----------------
 * Breadth-first refinement of the body-position box: per level every child box is tested against
 * every foothold (and the orientation samples for small boxes) with distance_global for each
 * mounted leg (validity_child, several_leg_octree.cu:19-151); valid leaves' centres are returned
 * in depth-first child order (extractValidAsArray, octree_util.cu:128-180).  The compile-time knobs
 * of settings.h:15-46 are a struct here; lrm_octree_default_settings() fills in the committed
 * values (root box +-5000 mm, MINBOXSIZE 100, 3x3x3 orientation samples, 4 legs mounted every
 * pi/4, LegNumberForStab 4, MAX_DEPTH 1).  Level-synchronous flat arrays replace the reference's
 * device-side cudaMalloc and kernel-launching kernels. */
typedef struct LrmOctreeSettings {
    float box_center[3];        /* settings.h:24 BoxCenter        */
    float box_size[3];          /* settings.h:26 BoxSize (half)   */
    float min_box;              /* settings.h:17 MINBOXSIZE       */
    float enable_rot_below;     /* settings.h:33 EnableRotBelow   */
    float convex_radius;        /* settings.h:34 convexRadius     */
    int32_t angle_sample[3];    /* settings.h:35 AngleSample      */
    float angle_minmax[6];      /* settings.h:38 AngleMinMax      */
    int32_t leg_count;          /* settings.h:41 LegCount         */
    float leg_mount[8];         /* settings.h:42 LegMount         */
    int32_t leg_number_for_stab;/* settings.h:46 LegNumberForStab */
    int32_t max_depth;          /* settings.h:15 MAX_DEPTH        */
} LrmOctreeSettings;
void lrm_octree_default_settings(LrmOctreeSettings* out);
/* footholds: AoS float3 (Array<float3> input of apply_oct); centers_out: room for `capacity` float3;
 * *n_out = number of valid leaves (if > capacity the call fails with LRM_EINVAL and *n_out tells the
 * size to retry with); settings = NULL -> defaults; *ms = kernel time.
 * From 3e5 footholds on (LRM_MODE_FAST) the work items' decisions come from the plane tables of the (leg, orientation) pairs, built
 * on the device on the first call that meets a pair (~0.4 ms each) and kept for the process; the tree is the same. */
int lrm_apply_oct(const float* footholds_aos, size_t n, const LrmLegDimensions* dim,
                  const LrmOctreeSettings* settings, float* centers_out, size_t capacity, size_t* n_out,
                  float* ms);
/* The same tree on several GPUs, one process each (the reference is single-device).  `exchange(flags, n, user)` must
 * replace flags[0..n) by their element-wise BITWISE OR over all ranks and return 0 (non-zero: the call fails); it is
 * called by every rank once with n = 1 before the first level and once per level.  A rank that fails locally still
 * enters the exchange its peers wait in with 0xffffffff in every word, and a rank that reads 0xffffffff fails too.
 * lrm_apply_oct_sharded: every rank holds all footholds, the children of a level are dealt round-robin to the ranks.
 * lrm_apply_oct_partitioned(_dev): every rank holds ITS part of the footholds (any disjoint split of the cloud; a
 *   spatial one keeps the work local) and evaluates every child against it -- a child's flags are ORs over
 *   footholds, so the OR over the ranks is exact: BASELINE config 5 without a replica of the 1e8-point cloud per GPU.
 * Every rank returns all valid leaves. */
typedef int (*LrmOctExchange)(uint32_t* flags, size_t n, void* user);
int lrm_apply_oct_sharded(const float* footholds_aos, size_t n, const LrmLegDimensions* dim,
                          const LrmOctreeSettings* settings, float* centers_out, size_t capacity, size_t* n_out,
                          float* ms, int rank, int world, LrmOctExchange exchange, void* user);
int lrm_apply_oct_partitioned(const float* local_footholds_aos, size_t n_local, const LrmLegDimensions* dim,
                              const LrmOctreeSettings* settings, float* centers_out, size_t capacity, size_t* n_out,
                              float* ms, LrmOctExchange exchange, void* user);
int lrm_apply_oct_partitioned_dev(const float* fx, const float* fy, const float* fz, size_t n_local, const LrmLegDimensions* dim,
                                  const LrmOctreeSettings* settings, float* centers_out, size_t capacity, size_t* n_out,
                                  float* ms, LrmOctExchange exchange, void* user);
/* The same with the footholds already on the device, one array per component (the layout of the other *_dev entry points;
 * the reference has no such call: apply_oct uploads its Array<float3> every time, several_leg_octree.cu:408-414).  The arrays
 * are read only (a sorted copy is made).  rank / world / exchange as lrm_apply_oct_sharded (0, 1, NULL, NULL on one GPU). */
int lrm_apply_oct_dev(const float* fx, const float* fy, const float* fz, size_t n, const LrmLegDimensions* dim,
                      const LrmOctreeSettings* settings, float* centers_out, size_t capacity, size_t* n_out, float* ms,
                      int rank, int world, LrmOctExchange exchange, void* user);
const char* lrm_octree_last_error(void);
/* Trace of the octree calls of this thread (tests): after lrm_dbg_oct_trace(1) every evaluated child of every level is
 * recorded as 12 floats {c[3], h[3], parent h[3], flag bits the kernel returned (1 reach, 2 leaf, 4 edge),
 * parent_valid + 2 * rotations + 4 * skipped, depth}; lrm_dbg_oct_trace_read copies them (out may be NULL to ask for
 * the count); lrm_dbg_oct_trace(0) stops and clears. */
int lrm_dbg_oct_trace(int enable);
int lrm_dbg_oct_trace_read(float* out, size_t capacity_records, size_t* n_out);
/* What an octree call launches for a level of nc children on nf footholds under the LRM_OCT_* switches of the environment,
 * from the function the launch itself consumes (host only, no device needed): out = {kernel (0 every foothold, 1 chunked),
 * grid.x, grid.y, tiles per round, workgroups per child ("splits"; both 0 for kernel 0), 1 if the level goes through the
 * deferred queue (as when the plane tables and the queue exist), tiles of the cloud, threads per workgroup}.  nc = 0 is
 * LRM_EINVAL.  tests/test_octree_cases_cpu.py holds it against the restatement the boundary suite is built on. */
int lrm_dbg_oct_plan(size_t nc, size_t nf, uint64_t out[8]);

/* ---- several GPUs behind the apply_kernel boundary (one process, one host thread) ------------------------------
 * New capability: the reference runs on device 0 only (several_leg.cu:800; apply_kernel cross_compiled.cu:33-79).
 * lrm_shard_bounds: owner `rank` of `world` gets items [lo, hi) of n, boundaries multiples of `align` (64 for point
 *   clouds: no 64-point ballot word straddles two owners); ceil(n / world) rounded up to `align` per owner, the last
 *   owners may be short or empty.  The Python side (lrm_amd.shard.shard_bounds) uses the same arithmetic.
 * lrm_reach_dist_multi: lrm_reach_dist with the cloud cut into those shards over `ndev` devices (`devices`: their
 *   ordinals, NULL = 0 .. ndev-1): per device one stream, its slice of the input, the fused kernels of the current
 *   mode, the reach bytes packed into ballot words; the words are all-gathered with RCCL (ncclCommInitAll once per
 *   device set + one grouped ncclAllGather per call; librccl.so is opened on first use with ndev > 1), so that every
 *   device holds the bit-packed mask of the whole cloud (BASELINE config 4's exchange step).  mask_out[n] /
 *   dxyz_out[3 n] as lrm_reach_dist; bits_out: NULL or ceil(n / 64) words, the gathered mask as devices[0] holds it;
 *   ms_per_dev: NULL or [ndev] kernel milliseconds per device.  lrm_multi_release frees the cached communicators. */
int lrm_shard_bounds(size_t n, int world, int rank, size_t align, size_t* lo_out, size_t* hi_out);
int lrm_reach_dist_multi(const float* xyz_aos, size_t n, const LrmLegDimensions* leg, const float* quat, int ndev,
                         const int* devices, uint8_t* mask_out, float* dxyz_out, uint64_t* bits_out, float* ms_per_dev);
void lrm_multi_release(void);

/* ---- diagnostics -------------------------------------------------------------------------
 * The glibc-exact atan2f / sincosf of the strict kernels (csrc/lrm_exact_math.h) applied to
 * arrays: at2[i] = atan2f(a[i], b[i]); (sn[i], cs[i]) = sincosf(a[i]).  Host build and device
 * build; tests compare the host build with the platform libm and the device build with the host build. */
int lrm_dbg_exact_math_host(const float* a, const float* b, size_t n, float* at2, float* sn, float* cs);
int lrm_dbg_exact_math_dev(const float* a, const float* b, size_t n, float* at2, float* sn, float* cs,
                           void* stream);
/* Block checksums of the same header's one-argument functions over float bit patterns (csrc/lrm_dbg_math.h), for comparing
 * the device build with the host build on EVERY float.  The 2^32 patterns u form 65536 blocks of 65536: block b holds
 * u = b * 65536 + j.  fn: 0 lrm_atanf(x), 1 the sine, 2 the cosine of lrm_sincosf(x).  With r(u) the result's bits, every nan
 * replaced by 0x7fc00000, sums_out[k] = sum_j r(u) * (2 j + 1) mod 2^64 of block first_block + k, k < nblocks: the weights are
 * odd, so one wrong result in a block changes its sum.  first_block + nblocks <= 65536; nblocks == 0 writes nothing.  Host:
 * at most 16 threads (LRM_DBG_MATH_THREADS sets fewer).  Device: sums_out is device memory, one workgroup per block, one
 * launch on `stream`. */
int lrm_dbg_exact_math_sums_host(int fn, uint32_t first_block, uint32_t nblocks, uint64_t* sums_out);
int lrm_dbg_exact_math_sums_dev(int fn, uint32_t first_block, uint32_t nblocks, uint64_t* sums_out, void* stream);
/* The link-pair distance of lrm_self_clearance_posed_dev (csrc/lrm_self_clearance.h) on n hand-made segment pairs: segs holds
 * 12 floats per pair, A1, B1, A2, B2 as x, y, z; out[i] = d of pair i.  Host build and device build (one pair per lane); the
 * tests hold the branchy distance to the text above on them. */
int lrm_dbg_link_pair_dist_host(const float* segs, size_t n, float* out);
int lrm_dbg_link_pair_dist_dev(const float* segs, size_t n, float* out, void* stream);
/* The link-to-cylinder distance of lrm_trunk_clearance_posed_dev (csrc/lrm_trunk_clearance.h) on n hand-made links in the BODY
 * frame: segs holds 6 floats per link, A and B as x, y, z; out[i] = d of link i against the cylinder (trunk_radius, plus_z,
 * minus_z), which is not checked here.  Host build and device build (one link per lane); the tests hold the search to the text
 * above on them and measure it against float64. */
int lrm_dbg_trunk_link_dist_host(const float* segs, size_t n, float trunk_radius, float plus_z, float minus_z, float* out);
int lrm_dbg_trunk_link_dist_dev(const float* segs, size_t n, float trunk_radius, float plus_z, float minus_z, float* out, void* stream);
/* The sampled path of lrm_edge_transit_posed_dev (csrc/lrm_edge_transit.h) on its own: out holds 7 floats per (edge, sample) at
 * [(e*nsamples + s)*7]: the quaternion q_s and the body position body_s the call evaluates; nan for an edge with an end outside
 * [0, nposes).  body may be NULL (= 0).  Host build and device build (one sample per lane); the tests hold the path to the
 * text above and measure it against a float64 model. */
int lrm_dbg_edge_transit_samples_host(const float* quats, const float* body, size_t nposes, const int32_t* edge_a, const int32_t* edge_b,
                                      size_t nedges, size_t nsamples, float* out);
int lrm_dbg_edge_transit_samples_dev(const float* quats, const float* body, size_t nposes, const int32_t* edge_a, const int32_t* edge_b,
                                     size_t nedges, size_t nsamples, float* out, void* stream);
/* The device's correctly rounded square root (csrc/lrm_exact_math.h, lrm_sqrtf) against the
 * compiler's IEEE sqrtf on ALL 2^32 float bit patterns: writes the number of patterns whose results
 * differ bitwise (nan payloads included) and the first such pattern.  Synchronous. */
int lrm_dbg_sqrt_check_dev(uint64_t* mismatches_out, uint32_t* first_bad_out);

/* The pose records lrm_pose_compile_dev writes (host quats / body here), made by the host compiler: nposes x nlegs
 * records of lrm_posed_workspace_bytes(1, 1) bytes, each the first 480 bytes of the host's compiled leg for
 * (leg, quat) followed by the body position.  The device's records must be the same bytes (tests/test_gpu_posed.py). */
int lrm_dbg_pose_compile_host(const float* quats, const float* body, size_t nposes, const LrmLegDimensions* legs, size_t nlegs,
                              void* records_out);
/* The foothold table lrm_pose_footholds_compile_dev writes (host quats here), made on the host by the same function
 * (csrc/lrm_footholds_posed.h): nposes x nlegs x LRM_POSE_FOOTHOLD_BYTES bytes.  The device table equals it byte for byte. */
int lrm_dbg_pose_footholds_compile_host(const float* quats, size_t nposes, const LrmLegDimensions* legs, size_t nlegs,
                                        const float* nominal, void* entries_out);
/* The IK table lrm_pose_ik_compile_dev writes (host quats here), made on the host by the code of the single-pose calls:
 * nposes x nlegs entries of lrm_posed_ik_workspace_bytes(1, 1) bytes.  The device's must be the same bytes
 * (tests/test_gpu_ik_posed.py). */
int lrm_dbg_pose_ik_compile_host(const float* quats, size_t nposes, const LrmLegDimensions* legs, size_t nlegs,
                                 void* records_out);
/* The first 480 bytes (the part the strict per-point code reads) of the leg compiler's block for (leg, quat), apply_leg_rotation = 1. */
int lrm_dbg_compile_leg_head(const LrmLegDimensions* leg, const float* quat, void* out480);

/* The filtered (LRM_MODE_FAST) per-point evaluation run on the host WITHOUT its strict
 * fallback, plus the per-point "uncertain" flags that would trigger the fallback.  Any output
 * pointer may be NULL.  Fails with LRM_EINVAL for a leg the filter does not support. */
int lrm_dbg_fast_host(const float* xyz_aos, size_t n, const LrmLegDimensions* leg, const float* quat,
                      uint8_t* mask_out, uint8_t* mask_uncertain_out, float* dxyz_aos_out,
                      uint8_t* valid_out, uint8_t* dist_uncertain_out);
/* The contract-tolerance evaluation (LRM_MODE_TOL, csrc/lrm_point_tol.h) on the host WITHOUT the bit-exact
 * re-evaluation of its doubtful points: mask_out = reach / validity flag, doubt_out = LRM_TD_* bits (0: the
 * outputs are final).  Fails with LRM_EINVAL for a leg the mode does not support. */
int lrm_dbg_tol_host(const float* xyz_aos, size_t n, const LrmLegDimensions* leg, const float* quat,
                     uint8_t* mask_out, float* dxyz_aos_out, uint32_t* doubt_out);
/* As lrm_dbg_tol_host with the plane table with deferred decisions (csrc/lrm_toltab.cpp) in place of the full plane
 * evaluation; doubt bit 0x100 = a cell without an answer.  stats_out[5] (or NULL): rows, validity rows, refined cells, bytes,
 * points whose second yaw candidate had to be evaluated (its lower bound did not exclude it). */
int lrm_dbg_toltab_host(const float* xyz_aos, size_t n, const LrmLegDimensions* leg, const float* quat,
                        uint8_t* mask_out, float* dxyz_out, uint32_t* doubt_out, uint32_t* stats_out);
/* The bit-exact table-guided evaluation (csrc/lrm_point_xtab.h: decisions from the plane table, values in the reference's
 * operation order) on the host, WITHOUT the re-evaluation of its doubtful points: every point with doubt 0 carries the mask and
 * the vector of lrm_reach_cpu / lrm_dist_cpu bit for bit (tests/test_xtab_cpu.py).  stats_out[2] (or NULL): points whose
 * second value chain ran, table bytes. */
int lrm_dbg_xtab_host(const float* xyz_aos, size_t n, const LrmLegDimensions* leg, const float* quat,
                      uint8_t* mask_out, float* dxyz_out, uint32_t* doubt_out, uint32_t* stats_out);
/* LRM_MODE_TOL_REL's two steps on the host: the tolerance evaluation with the plane table, then -- for every point without doubt --
 * the strict replay of the winner's value chain from the decisions the first step took (csrc/lrm_point_xtab.h: lrm_xtab_replay):
 * those vectors equal lrm_dist_cpu bit for bit (tests/test_xtab_cpu.py).  A point in doubt keeps the tolerance vector. */
int lrm_dbg_replay_host(const float* xyz_aos, size_t n, const LrmLegDimensions* leg, const float* quat,
                        uint8_t* mask_out, float* dxyz_out, uint32_t* doubt_out);
/* The plane table of (leg, quat) as the HOST builder (device = 0: csrc/lrm_toltab.cpp) or the DEVICE builder (device = 1:
 * csrc/lrm_toltab_dev.hip, on the current device) makes it: its bytes into out[cap] (when they fit; out may be NULL), its size, the
 * build's milliseconds.  The two must agree byte for byte (tests/test_gpu_toltab.py). */
int lrm_dbg_toltab_build(const LrmLegDimensions* leg, const float* quat, int device, uint8_t* out, size_t cap, size_t* size_out,
                         float* ms_out);
/* The plane table's lower bound of the in-plane distance at n plane points xz[2 n] (abscissa - coxa_length, z), next to the
 * full plane evaluation there: distance sqrt(du^2 + dz^2), validity, doubt bits.  The bound must not exceed the distance
 * of an invalid point and must be 0 at a valid one (tests/test_tol_cpu.py). */
int lrm_dbg_toltab_bounds(const float* xz, size_t n, const LrmLegDimensions* leg, const float* quat, float* lb_out,
                          float* dist_out, uint8_t* valid_out, uint32_t* doubt_out);
/* Counting build only (csrc: -DLRM_PAIR_COUNT, tools/c3_evidence.py): what the wave-per-body pair kernel evaluated since the
 * last call: out[0] full (leg, target) evaluations, [1] leg bounding-sphere tests, [2] footholds inside a body's reach sphere,
 * [3] footholds loaded.  LRM_EINVAL in an ordinary build. */
int lrm_dbg_pair_counts(uint64_t out[4]);
/* After a distance / fused call on device buffers in LRM_MODE_TOL: the points of that call, how many of them its main
 * kernel queued for the bit-exact fix-up launch, and how many workgroups overflowed their queue segment (all their
 * points are re-evaluated).  Synchronises that device. */
int lrm_dbg_tol_queue_counts(uint64_t* n_points, uint64_t* n_queued, uint64_t* n_overflowed);
/* The launch grids of the distance / fused calls for n points, from the functions the launches themselves call (host only, no
 * device needed): out[0] workgroups of the table kernels of LRM_MODE_TOL and LRM_MODE_FAST, out[1] workgroups of the table
 * kernel of LRM_MODE_TOL_REL, out[2] workgroups of the tolerance kernel without a plane table; out[3] the queue words (uint32)
 * a call with the plane table requests, out[4] those a call without it requests, out[5] the words lrm_tol_prepare(n) reserves
 * (before its allocation slack).  A workgroup has 256 threads; a grid of b workgroups strides by 256 b points per round.
 * tests/test_grid_cpu.py checks lrm_tol_prepare's invariant with it, tests/test_gpu_shapes.py aims at the grids' transitions. */
int lrm_dbg_tol_grid(size_t n, uint64_t out[6]);
/* The launch shape of lrm_foothold_support_posed_dev for nt targets and nposes poses, from the function the launch itself
 * calls (host only, no device needed; a function of nt and nposes alone): out[0] poses per pose chunk (one bounding box
 * each), out[1] the slices S the pose range is cut into per 64-target chunk, out[2] the most poses one slice walks (slice s
 * takes the pose chunks c with c % S == s), out[3] workgroups of the traversal (4 waves each, one (target chunk, slice)
 * per wave).  tests/test_gpu_foothold_support.py takes its boundaries from it. */
int lrm_dbg_foothold_support_grid(size_t nt, size_t nposes, uint64_t out[4]);
/* 1 if (leg, quat) is eligible for LRM_MODE_TOL, else 0 */
int lrm_dbg_tol_ok(const LrmLegDimensions* leg, const float* quat);
/* The per-leg bounding sphere the pair kernels use to skip batches of footholds:
 * out4 = {cx, cy, cz (relative to the body position), squared radius}.  Tests check that every
 * pair the strict reachable_rotate_leg accepts lies inside. */
int lrm_dbg_pair_sphere(const LrmLegDimensions* leg, const float* quat, float* out4);

/* The reach mask the fused filtered kernel derives from its distance evaluation
 * (lrm_reach_from_dist, csrc/lrm_point_fast.h), WITHOUT the strict fallback, and the per-point
 * doubt flag that would trigger it. */
int lrm_dbg_fused_reach_host(const float* xyz_aos, size_t n, const LrmLegDimensions* leg, const float* quat,
                             uint8_t* mask_out, uint8_t* doubt_out);

#ifdef __cplusplus
}
#endif
#endif /* LRM_H */
