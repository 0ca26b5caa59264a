// lrm_pose_routes.hip -- the gfx950 kernels of lrm_pose_routes_dev (include/lrm.h): shortest routes over the pose graph by
// chaotic relaxation of 64-bit keys (lrm_pose_routes.h) with atomic min.  No kernel waits for another workgroup: there is no
// grid barrier, no cooperative launch and no loop on memory; every loop is bounded by a constant or an argument.  What one
// workgroup must see of another's work it sees across a kernel boundary.
//
// The launches of one call, all on the caller's stream: init (keys all-ones, flags, the reached count), seed (key 0 for the
// sources), `rounds` relax launches, then finish: per pose (cost, hops, reached, done), per edge (the smallest tight edge
// per pose by a 32-bit atomic min) and per pose again (the predecessor pose from that edge).
//
// TERMINATION.  Relax launch i reads flag[i-1], which launch i-1 completed; 0 there means launch i-1 changed no key, and the
// whole grid returns.  A workgroup that lowers any key stores 1 to flag[i].  If launch i changed nothing, the keys were
// constant while it ran, and every load in it read what earlier launches had completed -- the kernel boundary makes that
// visible, whatever the caches do -- so every arc was checked against the true keys: the fixed point is proven.  WITHIN a
// launch nothing is assumed of the caches (a CU's L1 is never refreshed by another CU's stores, the L2s of the XCDs are not
// coherent with each other): the loads are agent-scope atomic loads, and a load that is stale all the same can only read a
// key that is too large, since keys only fall.  That delays progress and never gives a wrong key: the atomic min decides at
// the memory, and "changed" is what it returns.  DESIGN.md 3.25.
#include "lrm_pose_routes.h"

namespace {

constexpr int kBlock = LRM_ROUTES_BLOCK;
constexpr int kPerLane = LRM_ROUTES_EDGES_PER_LANE;
constexpr uint32_t kChunk = LRM_ROUTES_CHUNK;
constexpr int kSweeps = LRM_ROUTES_SWEEPS;

__device__ __forceinline__ uint64_t key_load(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// true iff this min lowered the key
__device__ __forceinline__ bool key_min(uint64_t* p, uint64_t c) {
    return __hip_atomic_fetch_min(p, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > c;
}

// keys all-ones (not with resume), flag[0] = 1 and flag[1..rounds] = 0, the reached count 0
__global__ __launch_bounds__(kBlock) void routes_init_kernel(uint64_t* __restrict__ keys, uint32_t* __restrict__ flags, uint32_t nposes,
                                                             uint32_t rounds, int resume, int32_t* __restrict__ reached_out) {
    const uint32_t i0 = blockIdx.x * kBlock + threadIdx.x, stride = gridDim.x * kBlock;
    if (!resume)
        for (uint32_t i = i0; i < nposes; i += stride) keys[i] = LRM_ROUTES_UNREACHED;
    for (uint32_t i = i0; i <= rounds; i += stride) flags[i] = i == 0u ? 1u : 0u;
    if (i0 == 0u && reached_out) *reached_out = 0;
}

// key 0 for every source that is in range and live (a launch of its own: behind the all-ones of every other lane)
__global__ __launch_bounds__(kBlock) void routes_seed_kernel(uint64_t* __restrict__ keys, uint32_t nposes, const int32_t* __restrict__ sources,
                                                             uint32_t nsources, const uint8_t* __restrict__ pose_live) {
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < nsources; i += gridDim.x * kBlock) {
        const int32_t s = sources[i];
        if (lrm_routes_pose(s, nposes, pose_live)) keys[s] = 0ull;
    }
}

// Relax launch `launch` (1..rounds).  A workgroup takes chunks blockIdx.x, blockIdx.x + gridDim.x, ... of kChunk edges; per
// chunk a lane validates its kPerLane edges once, keeps (u, v, w) in registers and sweeps over them up to kSweeps times.
// s_token: the one LDS word.  A wave with a change stores the sweep's number there; two barriers keep the next sweep's
// store behind every wave's read.  Every branch around a barrier is uniform over the workgroup.
__global__ __launch_bounds__(kBlock) void routes_relax_kernel(uint64_t* keys, uint32_t* flags, uint32_t launch, const LrmRoutesArgs A) {
    __shared__ uint32_t s_token;
    if (__hip_atomic_load(flags + (launch - 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return; // the whole grid alike
    const uint32_t tid = threadIdx.x;
    if (tid == 0u) s_token = 0u;
    __syncthreads();
    const uint32_t nchunks = (A.nedges + kChunk - 1u) / kChunk; // nedges <= INT32_MAX: no wrap
    uint32_t token = 0u;
    bool wg_changed = false;
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        int32_t u[kPerLane], v[kPerLane];
        uint32_t w[kPerLane];
#pragma unroll
        for (int j = 0; j < kPerLane; j++) {
            const uint32_t e = chunk * kChunk + (uint32_t)j * kBlock + tid; // < nedges + kChunk < 2^32
            u[j] = 0, v[j] = 0, w[j] = LRM_ROUTES_DEAD;
            if (e < A.nedges) w[j] = lrm_routes_edge(e, A.edge_a, A.edge_b, A.edge_live, A.pose_live, A.edge_cost, A.nposes, A.direction, &u[j], &v[j]);
        }
        for (int s = 0; s < kSweeps; s++) {
            bool changed = false;
#pragma unroll
            for (int j = 0; j < kPerLane; j++) {
                if (w[j] == LRM_ROUTES_DEAD) continue;
                const uint64_t ku = key_load(keys + u[j]), kv = key_load(keys + v[j]);
                const uint64_t c = lrm_routes_step(ku, w[j]);
                if (c < kv) {
                    changed |= key_min(keys + v[j], c);
                } else if (A.direction == 0) { // the arc back; never lower where the arc forth was (c > ku)
                    const uint64_t r = lrm_routes_step(kv, w[j]);
                    if (r < ku) changed |= key_min(keys + u[j], r);
                }
            }
            ++token;
            if (__ballot(changed) != 0ull && (tid & 63u) == 0u) s_token = token;
            __syncthreads();
            const bool any = s_token == token;
            __syncthreads();
            if (!any) break;
            wg_changed = true;
        }
    }
    if (wg_changed && tid == 0u) __hip_atomic_store(flags + launch, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Finish, a lane per pose: the key unpacked; -1 into the array the edge pass takes its minimum in (pred_edge_out, or
// pred_pose_out when only that is asked for); the reached count (a ballot per wave, one integer add); workgroup 0 finds
// done = the first relax launch that changed nothing.
__global__ __launch_bounds__(kBlock) void routes_finish_pose_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ flags,
                                                                    uint32_t rounds, const LrmRoutesArgs A) {
    __shared__ uint32_t s_first;
    int32_t* const slot = A.pred_edge_out ? A.pred_edge_out : A.pred_pose_out;
    const uint32_t n64 = (A.nposes + 63u) & ~63u; // whole waves enter the ballot
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < n64; p += gridDim.x * kBlock) {
        bool reached = false;
        if (p < A.nposes) {
            const uint64_t k = keys[p];
            reached = k != LRM_ROUTES_UNREACHED;
            if (A.cost_out) A.cost_out[p] = reached ? (int64_t)(k >> 32) : (int64_t)-1;
            if (A.hops_out) A.hops_out[p] = reached ? (int32_t)(uint32_t)k : -1;
            if (slot) slot[p] = -1;
        }
        const unsigned long long b = __ballot(reached);
        if (A.reached_out && b != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(A.reached_out, (int32_t)__popcll(b));
    }
    if (blockIdx.x == 0u && A.done_out) {
        if (threadIdx.x == 0u) s_first = 0xffffffffu;
        __syncthreads();
        for (uint32_t i = 1u + threadIdx.x; i <= rounds; i += kBlock)
            if (flags[i] == 0u) {
                atomicMin(&s_first, i);
                break;
            }
        __syncthreads();
        if (threadIdx.x == 0u) *A.done_out = s_first == 0xffffffffu ? -1 : (int32_t)s_first;
    }
}

// Finish, a lane per edge: e into slot[v] by an unsigned 32-bit min for every tight arc u -> v of a usable edge; all-ones is
// the -1 of the pass before.
__global__ __launch_bounds__(kBlock) void routes_finish_edge_kernel(const uint64_t* __restrict__ keys, const LrmRoutesArgs A) {
    uint32_t* const slot = reinterpret_cast<uint32_t*>(A.pred_edge_out ? A.pred_edge_out : A.pred_pose_out);
    for (uint32_t e = blockIdx.x * kBlock + threadIdx.x; e < A.nedges; e += gridDim.x * kBlock) {
        int32_t u, v;
        const uint32_t w = lrm_routes_edge(e, A.edge_a, A.edge_b, A.edge_live, A.pose_live, A.edge_cost, A.nposes, A.direction, &u, &v);
        if (w == LRM_ROUTES_DEAD) continue;
        const uint64_t ku = keys[u], kv = keys[v];
        if (kv != LRM_ROUTES_UNREACHED && lrm_routes_step(ku, w) == kv) atomicMin(slot + v, e);
        else if (A.direction == 0 && ku != LRM_ROUTES_UNREACHED && lrm_routes_step(kv, w) == ku) atomicMin(slot + u, e);
    }
}

// Finish, a lane per pose: the tail of the chosen edge's tight arc.  With pred_edge_out null the edge sits in pred_pose_out
// itself and is replaced in place (a lane reads and writes its own entry only).
__global__ __launch_bounds__(kBlock) void routes_finish_pred_kernel(const LrmRoutesArgs A) {
    const int32_t* const slot = A.pred_edge_out ? A.pred_edge_out : A.pred_pose_out;
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < A.nposes; p += gridDim.x * kBlock) {
        const int32_t e = slot[p];
        int32_t from = -1;
        if (e >= 0 && (uint32_t)e < A.nedges) { // an edge the pass before stored: its ends are in range
            const int32_t a = A.edge_a[e], b = A.edge_b[e];
            from = (A.direction != 2 && (uint32_t)b == p) ? a : b;
        }
        A.pred_pose_out[p] = from;
    }
}

__global__ void routes_empty_kernel(int32_t* reached_out, int32_t* done_out) {
    if (reached_out) *reached_out = 0;
    if (done_out) *done_out = 1;
}

unsigned grid_for(size_t n, unsigned cap) {
    size_t g = (n + kBlock - 1) / kBlock;
    if (g < 1) g = 1;
    return (unsigned)(g > cap ? cap : g);
}

} // namespace

hipError_t lrm_launch_pose_routes(const LrmRoutesArgs& A, void* workspace, uint32_t rounds, int resume, hipStream_t st) {
    uint64_t* const keys = static_cast<uint64_t*>(workspace);
    uint32_t* const flags = reinterpret_cast<uint32_t*>(keys + A.nposes);
    const size_t ninit = A.nposes > rounds + 1u ? A.nposes : rounds + 1u;
    hipLaunchKernelGGL(routes_init_kernel, dim3(grid_for(ninit, LRM_ROUTES_FINISH_GRID)), dim3(kBlock), 0, st, keys, flags, A.nposes, rounds,
                       resume, A.reached_out);
    if (!resume && A.nsources)
        hipLaunchKernelGGL(routes_seed_kernel, dim3(grid_for(A.nsources, LRM_ROUTES_FINISH_GRID)), dim3(kBlock), 0, st, keys, A.nposes,
                           A.sources, A.nsources, A.pose_live);
    uint64_t plan[4];
    lrm_routes_plan(A.nedges, plan);
    if (plan[3]) // no edge: flag[1] stays 0, done = 1
        for (uint32_t i = 1; i <= rounds; i++)
            hipLaunchKernelGGL(routes_relax_kernel, dim3((unsigned)plan[3]), dim3(kBlock), 0, st, keys, flags, i, A);
    hipLaunchKernelGGL(routes_finish_pose_kernel, dim3(grid_for(A.nposes, LRM_ROUTES_FINISH_GRID)), dim3(kBlock), 0, st, keys, flags, rounds, A);
    if (A.pred_edge_out || A.pred_pose_out) {
        if (A.nedges)
            hipLaunchKernelGGL(routes_finish_edge_kernel, dim3(grid_for(A.nedges, LRM_ROUTES_MAX_GRID)), dim3(kBlock), 0, st, keys, A);
        if (A.pred_pose_out)
            hipLaunchKernelGGL(routes_finish_pred_kernel, dim3(grid_for(A.nposes, LRM_ROUTES_FINISH_GRID)), dim3(kBlock), 0, st, A);
    }
    return hipGetLastError();
}

hipError_t lrm_launch_pose_routes_empty(int32_t* reached_out, int32_t* done_out, hipStream_t st) {
    hipLaunchKernelGGL(routes_empty_kernel, dim3(1), dim3(1), 0, st, reached_out, done_out);
    return hipGetLastError();
}
