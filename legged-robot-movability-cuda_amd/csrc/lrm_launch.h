// lrm_launch.h -- kernel launch functions (lrm_kernels.hip) used by the C ABI (lrm_capi.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include "lrm_types.h"

hipError_t lrm_launch_warmup(size_t n, hipStream_t st);
hipError_t lrm_launch_reach_soa(const float* x, const float* y, const float* z, size_t n,
                                const LrmCompiledLeg& L, uint8_t* mask, uint64_t* bits, bool fast, hipStream_t st);
// op: 1 = distance (mask = distance's validity byte, may be null), 2 = reach mask + distance
hipError_t lrm_launch_dist_soa(int op, const float* x, const float* y, const float* z, size_t n,
                               const LrmCompiledLeg& L, uint8_t* mask, uint64_t* bits, float* dx, float* dy,
                               float* dz, bool fast, hipStream_t st);
// LRM_MODE_TOL (lrm_tol_kernels.hip): the tolerance kernel + the fix-up of its doubtful points, two launches on
// `st`.  workspace: lrm_tol_queue_words(n) uint32 of device memory owned by the caller for the duration of both
// launches (contents are rewritten by every call; no initialisation needed).
#ifndef LRM_TOL_SEG_CAP
#define LRM_TOL_SEG_CAP 128 // doubt slots per workgroup of the main kernel (768 points): 17 %.  32 overflowed on the reference's planar bench grid (7 % in doubt: it contains the coxa axis and the symmetry plane)
#endif
#define LRM_TOL_SEG_CAP_WORDS LRM_TOL_SEG_CAP
#ifndef LRM_TOL_TAB_SEG_CAP
#define LRM_TOL_TAB_SEG_CAP 256 // doubt slots per workgroup of the table kernel (1536 points): 17 %
#endif
// flags of the tolerance-mode launches (bits 0 and 1 are LRM_TOL_SELFTEST's)
#define LRM_TOLF_SHORT 4u     // LRM_MODE_TOL_REL: every vector shorter than LRM_TOL_REL_MM is queued for the bit-exact fix-up
#ifndef LRM_TOL_REL_MM
#define LRM_TOL_REL_MM 19.0f  // the literal bound |d - d_ref| <= 1e-5 |d_ref| is asserted from 16 mm on (17 mm until the third campaign of round 4 found 7.6e-6 at 17.55 mm: the threshold and the band count below went up by an eighth, 0.9 us per 1e7 points)
#endif
#ifndef LRM_TOL_REL_BANDS
#define LRM_TOL_REL_BANDS 2250.0f // ... and from 2250 decision bands on (34 mm at |p|_1 + body = 1 m): the error grows with the coordinates
#endif
size_t lrm_tol_queue_words(size_t n);
hipError_t lrm_launch_dist_tol_aos(int op, const float* xyz, size_t n, const LrmCompiledLeg& L, const LrmTolLeg& TL, uint8_t* mask,
                                   float* dxyz, uint32_t* workspace, uint32_t flags, hipStream_t st);
hipError_t lrm_launch_dist_tol(int op, const float* x, const float* y, const float* z, size_t n, const LrmCompiledLeg& L,
                               const LrmTolLeg& TL, uint8_t* mask, uint64_t* bits, float* dx, float* dy, float* dz,
                               uint32_t* workspace, uint32_t flags, hipStream_t st);
// Table variant (dist_tab_kernel + the same fix-up): tab_dev = device copy of lrm_build_tol_tab's table for TL.
size_t lrm_tol_tab_queue_words(size_t n);
size_t lrm_tol_tab_segments(size_t n, bool rel); // the workspace starts with one count per segment (rel: LRM_MODE_TOL_REL's grid)
// workgroups of the main kernel for n points: [0] the table kernels of LRM_MODE_TOL / LRM_MODE_FAST, [1] the table kernel of
// LRM_MODE_TOL_REL, [2] the staged kernel without a table (lrm_dbg_tol_grid)
void lrm_tol_grid(size_t n, size_t blocks_out[3]);
struct LrmXtabLeg; // lrm_point_xtab.h
hipError_t lrm_launch_dist_tab(int op, const float* x, const float* y, const float* z, size_t n, const LrmCompiledLeg& L,
                               const LrmTolLeg& TL, const LrmXtabLeg& X, const uint8_t* tab_dev, uint8_t* mask, uint64_t* bits, float* dx, float* dy,
                               float* dz, uint32_t* workspace, uint32_t flags, hipStream_t st);
hipError_t lrm_launch_dist_tab_aos(int op, const float* xyz, size_t n, const LrmCompiledLeg& L, const LrmTolLeg& TL, const LrmXtabLeg& X, const uint8_t* tab_dev,
                                   uint8_t* mask, float* dxyz, uint32_t* workspace, uint32_t flags, hipStream_t st);
// LRM_MODE_FAST through the plane table (dist_xtab_kernel, lrm_point_xtab.h: decisions from the table, values in the reference's
// order, bit-identical to LRM_MODE_STRICT) + tol_fixup_kernel for its doubtful points.  Workspace: lrm_tol_tab_queue_words(n).
hipError_t lrm_launch_dist_xtab(int op, const float* x, const float* y, const float* z, size_t n, const LrmCompiledLeg& L, const LrmXtabLeg& X,
                                const uint8_t* tab_dev, uint8_t* mask, uint64_t* bits, float* dx, float* dy, float* dz, uint32_t* workspace, hipStream_t st);
hipError_t lrm_launch_dist_xtab_aos(int op, const float* xyz, size_t n, const LrmCompiledLeg& L, const LrmXtabLeg& X, const uint8_t* tab_dev,
                                    uint8_t* mask, float* dxyz, uint32_t* workspace, hipStream_t st);
hipError_t lrm_launch_reach_aos(const float* xyz, size_t n, const LrmCompiledLeg& L, uint8_t* mask, bool fast,
                                hipStream_t st);
hipError_t lrm_launch_dist_aos(int op, const float* xyz, size_t n, const LrmCompiledLeg& L, uint8_t* mask,
                               float* dxyz, bool fast, hipStream_t st);
hipError_t lrm_launch_reach_any(const float* bx, const float* by, const float* bz, size_t nb, const float* tx,
                                const float* ty, const float* tz, size_t nt, const LrmCompiledLeg* legs_dev,
                                int nlegs, float* tile_boxes /* 17 x ntiles x 6 floats of workspace, or null */,
                                bool boxes_ready /* the workspace already holds this cloud's boxes */,
                                const uint8_t* body_active /* null = all */, uint8_t* out_leg_body,
                                uint8_t* all_legs_out, bool fast, hipStream_t st);
// tile_aabb_kernel alone: the two-level boxes of a target cloud (17 x ntiles x 6 floats of workspace, as above)
hipError_t lrm_launch_tile_boxes(const float* tx, const float* ty, const float* tz, size_t nt, float* tile_boxes, hipStream_t st);
// The prologue of the launchers whose waves each walk the whole target cloud for one of n items (bodies, poses, edges):
// the cloud's boxes into tile_boxes when there is a workspace and a cloud; boxes = what the kernel gets (null = every tile
// near); grid = workgroups of `waves` items, at most max_grid of them when that is not 0 (a wave strides over the rest).
struct LrmWalkLaunch {
    hipError_t err;
    const float* boxes;
    dim3 grid;
};
inline LrmWalkLaunch lrm_walk_launch(const float* tx, const float* ty, const float* tz, size_t nt, float* tile_boxes, size_t n,
                                     unsigned waves, unsigned max_grid, hipStream_t st) {
    hipError_t err = hipSuccess;
    if (tile_boxes && nt) err = lrm_launch_tile_boxes(tx, ty, tz, nt, tile_boxes, st);
    size_t g = (n + waves - 1) / waves;
    if (max_grid && g > max_grid) g = max_grid;
    return LrmWalkLaunch{err, nt ? tile_boxes : nullptr, dim3((unsigned)g)};
}
// lrm_footholds_dev (lrm_footholds.hip): outputs [nlegs * nb] at l * nb + b; best_d2_out may be null; tile_boxes null =
// no culling (small clouds), otherwise workspace that this call fills with the cloud's boxes first
struct LrmFootNominal; // lrm_footholds.h
hipError_t lrm_launch_footholds(const float* bx, const float* by, const float* bz, size_t nb, const float* tx,
                                const float* ty, const float* tz, size_t nt, const LrmCompiledLeg* legs_dev, int nlegs,
                                float* tile_boxes, const LrmFootNominal& nominal, int32_t* count_out, int32_t* best_out,
                                float* best_d2_out, bool fast, hipStream_t st);
// lrm_pose_footholds_compile_dev / lrm_footholds_posed_dev (lrm_footholds_posed.hip).  fh_records: nposes x nlegs
// LrmPoseFootEntry (lrm_footholds_posed.h) at pose * nlegs + leg, next to the pose records of lrm_posed.hip.  Outputs
// [nlegs * nposes] at l * nposes + p and all_legs_out[nposes]; best_d2_out and all_legs_out may be null; tile_boxes as above.
hipError_t lrm_launch_pose_footholds_compile(const float* quats, size_t nposes, const LrmLegDimensions* legs, size_t nlegs,
                                             const LrmFootNominal& nominal, void* fh_records, hipStream_t st);
hipError_t lrm_launch_footholds_posed(const float* tx, const float* ty, const float* tz, size_t nt, const void* records,
                                      const void* fh_records, size_t nposes, size_t nlegs, float* tile_boxes, int32_t* count_out,
                                      int32_t* best_out, float* best_d2_out, uint8_t* all_legs_out, hipStream_t st);
// lrm_foothold_lists_posed_dev / lrm_foothold_offsets_dev (lrm_footholds_posed.hip): the same tables and tile_boxes;
// offsets: device, nlegs * nposes + 1; d2_out and written_out may be null.  The kernel clamps every segment to
// [0, capacity) before it stores.
hipError_t lrm_launch_foothold_lists_posed(const float* tx, const float* ty, const float* tz, size_t nt, const void* records,
                                           const void* fh_records, size_t nposes, size_t nlegs, float* tile_boxes,
                                           const int64_t* offsets, size_t capacity, int32_t* idx_out, float* d2_out,
                                           int32_t* written_out, hipStream_t st);
hipError_t lrm_launch_foothold_offsets(const int32_t* count, size_t n, int64_t* offsets_out, hipStream_t st);
// lrm_foothold_edges_posed_dev (lrm_footholds_posed.hip): the same tables and tile_boxes; edge_a / edge_b: device, nedges
// pose indices of any value (the kernel checks them); outputs [nlegs * nedges] at l * nedges + e and all_legs_out[nedges];
// best_d2_out and all_legs_out may be null.  nedges * nlegs < 2^32 (checked by the C ABI).
hipError_t lrm_launch_foothold_edges_posed(const float* tx, const float* ty, const float* tz, size_t nt, const void* records,
                                           const void* fh_records, size_t nposes, size_t nlegs, float* tile_boxes,
                                           const int32_t* edge_a, const int32_t* edge_b, size_t nedges, int32_t* count_out,
                                           int32_t* best_out, float* best_d2_out, uint8_t* all_legs_out, hipStream_t st);
// lrm_foothold_misses_posed_dev (lrm_foothold_misses.hip): the same tables and tile_boxes; margin >= 0 or +inf (checked by
// the C ABI); count_in: device, nlegs * nposes, or null; outputs [nlegs * nposes] at l * nposes + p; miss_m2_out, the three
// shift arrays (all or none) and near_out may be null.
hipError_t lrm_launch_foothold_misses_posed(const float* tx, const float* ty, const float* tz, size_t nt, const void* records,
                                            const void* fh_records, size_t nposes, size_t nlegs, float* tile_boxes, float margin,
                                            const int32_t* count_in, int32_t* miss_out, float* miss_m2_out, float* shift_x,
                                            float* shift_y, float* shift_z, int32_t* near_out, hipStream_t st);
// lrm_foothold_support_posed_dev (lrm_foothold_support.hip): the same tables, NO tile_boxes (a wave boxes its own 64
// targets); pose_live: device, nposes, or null; support_workspace: lrm_foothold_support_bytes(nposes, nlegs, nt) bytes,
// 16-byte aligned, rewritten by every call; outputs [nlegs * nt] at l * nt + t and legs_mask_out[nt]; best_d2_out and
// legs_mask_out may be null.  nposes == 0: the empty answers, no record is read.  Three launches on `st`.
size_t lrm_foothold_support_bytes(size_t nposes, size_t nlegs, size_t nt);
// out[0] poses per pose chunk, [1] slices S of the pose range per target chunk, [2] the most poses one slice walks,
// [3] workgroups of the traversal (4 waves each; wave w takes target chunk w / S and the pose chunks c with c % S == w % S)
void lrm_foothold_support_grid(size_t nt, size_t nposes, uint64_t out[4]);
hipError_t lrm_launch_foothold_support(const float* tx, const float* ty, const float* tz, size_t nt, const void* records,
                                       const void* fh_records, size_t nposes, size_t nlegs, const uint8_t* pose_live,
                                       void* support_workspace, int32_t* count_out, int32_t* best_pose_out, float* best_d2_out,
                                       uint8_t* legs_mask_out, hipStream_t st);
// lrm_body_clearance_posed_dev (lrm_body_clearance.hip): the same tables and tile_boxes; the four scalars are checked by the
// C ABI (floor_z <= minus_z < plus_z, radius >= 0, radius and plus_z may be +inf); live_in: device, nposes, or null;
// outputs [nposes]; height_out and free_out may be null.  Reads leg 0's record and foothold entry of every live pose.
hipError_t lrm_launch_body_clearance_posed(const float* tx, const float* ty, const float* tz, size_t nt, const void* records,
                                           const void* fh_records, size_t nposes, size_t nlegs, float* tile_boxes, float radius,
                                           float plus_z, float minus_z, float floor_z, const uint8_t* live_in, int32_t* hits_out,
                                           int32_t* top_out, float* height_out, uint8_t* free_out, hipStream_t st);
hipError_t lrm_launch_any_in_shape(int shape, const float* cx, const float* cy, const float* cz, size_t nc,
                                   const float* tx, const float* ty, const float* tz, size_t nt, float radius,
                                   float plus_z, float minus_z, float* tile_boxes /* workspace or null */,
                                   bool boxes_ready, uint8_t* out, hipStream_t st);
hipError_t lrm_launch_sqrt_check(unsigned long long* counters_dev /* [2]: mismatches, first bad pattern + 1 */,
                                 hipStream_t st);
hipError_t lrm_launch_exact_math(const float* a, const float* b, size_t n, float* at2, float* sn, float* cs,
                                 hipStream_t st);
// lrm_dbg_math.hip: sums_dev[k] = the checksum (lrm_dbg_math.h) of block first_block + k, k < nblocks; one workgroup per block
hipError_t lrm_launch_exact_math_sums(int fn, uint32_t first_block, uint32_t nblocks, uint64_t* sums_dev, hipStream_t st);
hipError_t lrm_launch_rotate_soa(const float* sx, const float* sy, const float* sz, size_t n, const LrmCompiledLeg* rot_dev,
                                 float* dx, float* dy, float* dz, hipStream_t st);
hipError_t lrm_launch_sweep_update(const uint8_t* all_legs, const uint8_t* cyl_validate, const uint8_t* cyl_eliminate,
                                   int use_culls, size_t nb, uint8_t* active, uint8_t* accepted, hipStream_t st);
// evaluation counters of reach_any_wave_kernel in a -DLRM_PAIR_COUNT build (read and reset); hipErrorNotSupported otherwise
hipError_t lrm_pair_counts(unsigned long long out[4]);

// The plane table built on the device (lrm_toltab_dev.hip): 0 ok (*tab_dev_out = a fresh hipMalloc-ed table, the caller's), 1 this
// leg has no table, 2 the device builder does not take this leg or has no memory for its scratch (use lrm_build_tol_tab), < 0 a
// negated hipError_t.  Serialised by a lock of its own, taken after the caller's.
int lrm_build_tol_tab_dev(const LrmTolLeg& L, hipStream_t st, uint8_t** tab_dev_out, size_t* bytes_out, float* ms_out);
void lrm_toltab_dev_release();
// frees the octree's table cache (lrm_octree.hip); for lrm_release_workspaces
void lrm_octree_release();

// Batched multi-pose queries (lrm_posed.hip).  records: nposes x nlegs LrmPoseRecord (lrm_compile_head.h), record of
// (pose, leg) at pose * nlegs + leg.  lrm_launch_posed: op by outputs -- mask set: reach; valid or dx set: distance.
hipError_t lrm_launch_pose_compile(const float* quats, const float* body, size_t nposes, const LrmLegDimensions* legs,
                                   size_t nlegs, void* records, hipStream_t st);
hipError_t lrm_launch_posed(const float* x, const float* y, const float* z, size_t n, const int32_t* pose_idx,
                            const uint8_t* leg_idx, const void* records, size_t nposes, size_t nlegs, uint8_t* mask,
                            uint8_t* valid, float* dx, float* dy, float* dz, hipStream_t st);

// Joint angles per (target, pose, leg) (lrm_ik_posed.hip).  ik_records: nposes x nlegs LrmIkLeg (lrm_ik.h), entry of
// (pose, leg) at pose * nlegs + leg, next to the pose records above.  target_idx null: query i takes target i.
hipError_t lrm_launch_pose_ik_compile(const float* quats, size_t nposes, const LrmLegDimensions* legs, size_t nlegs, void* ik_records,
                                      hipStream_t st);
hipError_t lrm_launch_ik_posed(const float* x, const float* y, const float* z, size_t nt, const int32_t* target_idx, size_t n,
                               const int32_t* pose_idx, const uint8_t* leg_idx, const void* records, const void* ik_records,
                               size_t nposes, size_t nlegs, const float* seed_c, const float* seed_f, const float* seed_t,
                               float* coxa, float* femur, float* tibia, uint8_t* status, hipStream_t st);
hipError_t lrm_launch_fk_posed(const float* coxa, const float* femur, const float* tibia, size_t n, const int32_t* pose_idx,
                               const uint8_t* leg_idx, const void* records, const void* ik_records, size_t nposes, size_t nlegs,
                               float* x, float* y, float* z, hipStream_t st);
