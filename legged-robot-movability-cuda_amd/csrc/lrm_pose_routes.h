// lrm_pose_routes.h -- the arithmetic of lrm_pose_routes_dev / _cpu (include/lrm.h): shortest routes over the caller's pose
// graph with integer costs.  One source for the kernels (lrm_pose_routes.hip) and the host loop (lrm_capi.cpp): which edge is
// usable, which way its arcs run, the 64-bit key and its capped add, and the launch arithmetic.  Integers only, so device
// and host agree bit for bit, and the answer does not depend on the order in which arcs are relaxed.
//
// THE KEY of a pose is (sum of costs) << 32 | (number of arcs): one unsigned 64-bit compare is the lexicographic compare of the
// definition, and one 64-bit atomic min relaxes an arc.  All-ones is "not reached".  A stored key always belongs to a walk
// without a repeated pose (a walk that returns to a pose offers it a key above the one it had when the walk left it, and
// keys only fall), so the arc count stays below nposes <= INT32_MAX and never carries into the cost.
#pragma once
#include <stdint.h>
#include "lrm_types.h"

#ifndef LRM_ROUTES_SWEEPS
#define LRM_ROUTES_SWEEPS 4 // K: sweeps a workgroup makes over its chunk per launch, at most (it stops at the first that changes nothing); measured: DESIGN.md 3.25
#endif
#ifndef LRM_ROUTES_EDGES_PER_LANE
#define LRM_ROUTES_EDGES_PER_LANE 4 // edges a lane keeps in registers; C = 256 lanes x this; measured: DESIGN.md 3.25
#endif
#define LRM_ROUTES_BLOCK 256
#define LRM_ROUTES_CHUNK (LRM_ROUTES_BLOCK * LRM_ROUTES_EDGES_PER_LANE) // C: edges per workgroup and chunk
#define LRM_ROUTES_MAX_GRID 1024   // G: workgroups of a relax launch, at most (a workgroup strides over further chunks)
#define LRM_ROUTES_FINISH_GRID 256 // workgroups of the init and finish launches, at most (a lane strides over further items)
#define LRM_ROUTES_MAX_ROUNDS 4096

#define LRM_ROUTES_UNREACHED 0xffffffffffffffffull
#define LRM_ROUTES_COST_CAP 4294967294ull // the largest sum of costs a route may have
#define LRM_ROUTES_DEAD 0xffffffffu       // the cost of an edge that is not usable: no arc

// key + (w, 1) with the cap: LRM_ROUTES_UNREACHED when the sum of costs would exceed LRM_ROUTES_COST_CAP (an unreached tail
// has cost field 2^32 - 1 and lands there too).  w <= INT32_MAX.
LRM_HD uint64_t lrm_routes_step(uint64_t key, uint32_t w) {
    const uint64_t c = (key >> 32) + (uint64_t)w;
    if (c > LRM_ROUTES_COST_CAP) return LRM_ROUTES_UNREACHED;
    return (c << 32) | (uint64_t)((uint32_t)key + 1u);
}

// a live pose in range: an index is checked before an address is formed from it
LRM_HD bool lrm_routes_pose(int32_t p, uint32_t nposes, const uint8_t* pose_live) {
    return p >= 0 && (uint32_t)p < nposes && !(pose_live && pose_live[p] == 0);
}

// Edge e as arcs: *u -> *v, and *v -> *u too when direction == 0; direction 2 swaps the ends.  Returns the cost, or
// LRM_ROUTES_DEAD for an edge that is not usable (then *u = *v = 0).
LRM_HD uint32_t lrm_routes_edge(size_t e, const int32_t* edge_a, const int32_t* edge_b, const uint8_t* edge_live, const uint8_t* pose_live,
                                const int32_t* edge_cost, uint32_t nposes, int direction, int32_t* u, int32_t* v) {
    *u = 0, *v = 0;
    if (edge_live && edge_live[e] == 0) return LRM_ROUTES_DEAD;
    const int32_t a = edge_a[e], b = edge_b[e];
    if (!lrm_routes_pose(a, nposes, pose_live) || !lrm_routes_pose(b, nposes, pose_live)) return LRM_ROUTES_DEAD;
    const int32_t w = edge_cost ? edge_cost[e] : 1;
    if (w < 0) return LRM_ROUTES_DEAD;
    *u = direction == 2 ? b : a;
    *v = direction == 2 ? a : b;
    return (uint32_t)w;
}

// The launch arithmetic of a relax launch on nedges edges: out = {C, G, K, workgroups launched}.
inline void lrm_routes_plan(size_t nedges, uint64_t out[4]) {
    const uint64_t chunks = ((uint64_t)nedges + LRM_ROUTES_CHUNK - 1) / LRM_ROUTES_CHUNK;
    out[0] = LRM_ROUTES_CHUNK;
    out[1] = LRM_ROUTES_MAX_GRID;
    out[2] = LRM_ROUTES_SWEEPS;
    out[3] = chunks < LRM_ROUTES_MAX_GRID ? chunks : LRM_ROUTES_MAX_GRID;
}

// the workspace: nposes keys, then rounds + 1 flags (flag[0] is the init launch's, flag[i] relax launch i's)
inline size_t lrm_routes_workspace_bytes(size_t nposes, size_t rounds) { return nposes * sizeof(uint64_t) + (rounds + 1) * sizeof(uint32_t); }

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// what the launches take; everything is checked by the C ABI (nposes >= 1, the counts <= INT32_MAX, rounds in 1..4096,
// direction in 0..2, not all four per-pose outputs null)
struct LrmRoutesArgs {
    uint32_t nposes, nedges, nsources;
    const int32_t *edge_a, *edge_b, *edge_cost, *sources;
    const uint8_t *edge_live, *pose_live;
    int direction;
    int64_t* cost_out;
    int32_t *hops_out, *pred_edge_out, *pred_pose_out, *reached_out, *done_out;
};
// launch function (lrm_pose_routes.hip); only launches: init, `rounds` relax launches, up to three finish launches
hipError_t lrm_launch_pose_routes(const LrmRoutesArgs& A, void* workspace, uint32_t rounds, int resume, hipStream_t st);
// nposes == 0: *reached_out = 0, *done_out = 1 (either may be null)
hipError_t lrm_launch_pose_routes_empty(int32_t* reached_out, int32_t* done_out, hipStream_t st);
#endif
