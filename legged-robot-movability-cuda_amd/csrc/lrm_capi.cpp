// lrm_capi.cpp -- the extern "C" boundary of liblrm.so (include/lrm.h).
#include "../../include/lrm.h"
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <map>
#include <mutex>
#include <thread>
#include <string>
#include <utility>
#include <vector>
#include "lrm_compile.h"
#include "lrm_compile_head.h"
#include "lrm_footholds.h"
#include "lrm_footholds_posed.h"
#include "lrm_body_clearance.h"
#include "lrm_leg_clearance.h"
#include "lrm_stance.h"
#include "lrm_self_clearance.h"
#include "lrm_trunk_clearance.h"
#include "lrm_edge_transit.h"
#include "lrm_swing.h"
#include "lrm_stance_loads.h"
#include "lrm_pose_routes.h"
#include "lrm_pose_edges.h"
#include "lrm_ik.h"
#include "lrm_dbg_math.h"
#include "lrm_launch.h"
#include "lrm_point.h"
#include "lrm_point_fast.h"
#include "lrm_point_tol.h"
#include "lrm_point_xtab.h"

namespace {

thread_local std::string g_err;
// Process-wide, as documented in lrm.h; atomic so that a helper thread (the host pipeline's) or a second caller thread reads a whole value.
std::atomic<int> g_mode{LRM_MODE_FAST}; // bit-identical to LRM_MODE_STRICT (tests/test_gpu_parity.py runs both)
bool tol_mode() { const int m = g_mode; return m == LRM_MODE_TOL || m == LRM_MODE_TOL_REL; }
uint32_t tol_flags() { return g_mode == LRM_MODE_TOL_REL ? LRM_TOLF_SHORT : 0u; }
const float kQuatTest[4] = {1.f, 0.f, 0.f, 0.f}; // settings.h:51

int fail(int code, const char* what) {
    g_err = what;
    return code;
}
int hip_fail(hipError_t e, const char* where) {
    g_err = std::string(where) + ": " + hipGetErrorString(e);
    return (e == hipErrorOutOfMemory) ? LRM_ENOMEM : LRM_ENODEV;
}
#define HIP_TRY(expr, where)                              \
    do {                                                  \
        hipError_t e_ = (expr);                           \
        if (e_ != hipSuccess) return hip_fail(e_, where); \
    } while (0)

const float* quat_or_default(const float* q) { return q ? q : kQuatTest; }

// ---- table-guided modes: plumbing ---------------------------------------------------------------
// One lock around the process-wide caches below (table cache with LRU eviction, queue workspaces, the statistic of the last
// call, the host pipeline's buffers), held while a call queues its launches: as lrm.h states, host threads may overlap the
// distance and fused calls in every mode (host or device buffers), lrm_tol_prepare, lrm_apply_oct* and lrm_dbg_toltab_build,
// and a table is never freed under a launch that is being queued.  The pair kernels' pools (g_pools) and the multi-device
// communicators (g_multi) are not locked: those calls stay on one host thread.  lrm_release_workspaces must not overlap any
// other call.
std::recursive_mutex g_cache_mu;
// The tolerance block of a (leg, quaternion) costs a few hundred microseconds of host geometry (arc
// intersections + their verification, lrm_compile_tol): a small cache keyed by the 18 input floats.
struct TolKey {
    float v[18];
    bool operator<(const TolKey& o) const { return std::memcmp(v, o.v, sizeof v) < 0; }
};
struct TolEntry {
    LrmTolLeg tl;
    LrmXtabLeg xl;                 // the strict value chain's constants (lrm_point_xtab.h)
    std::vector<uint8_t> tab;      // the plane table (lrm_build_tol_tab), built on first use
    int tab_state = 0;             // 0 not built yet, 1 built, -1 this leg has none (too many rows)
    float tab_build_ms = 0.f;      // what building it cost (host wall clock, or the device build's events)
    std::map<int, uint8_t*> tab_dev;
    uint64_t last_use = 0;
};
uint64_t g_tol_clock = 0;
std::map<TolKey, TolEntry> g_tol_cache;
float g_last_tab_build_ms = -1.f; // lrm_dbg_last_table_build_ms
TolEntry& tol_entry(const LrmLegDimensions& leg, const float* quat, const LrmCompiledLeg& L) {
    TolKey k;
    std::memcpy(k.v, &leg, 14 * sizeof(float));
    std::memcpy(k.v + 14, quat, 4 * sizeof(float));
    auto it = g_tol_cache.find(k);
    if (it != g_tol_cache.end()) {
        it->second.last_use = ++g_tol_clock;
        return it->second;
    }
    if (g_tol_cache.size() >= 64) { // a sweep over many orientations: the least recently used pair goes (hipFree waits for the device)
        auto old = g_tol_cache.begin();
        for (auto jt = g_tol_cache.begin(); jt != g_tol_cache.end(); ++jt)
            if (jt->second.last_use < old->second.last_use) old = jt;
        for (auto& d : old->second.tab_dev) (void)hipFree(d.second);
        g_tol_cache.erase(old);
    }
    TolEntry& e = g_tol_cache[k];
    e.last_use = ++g_tol_clock;
    lrm_compile_tol(L, &e.tl);
    lrm_make_xtab_leg(L, e.tl, &e.xl);
    return e;
}
// where the last tolerance-mode launch left its per-segment doubt counts, for lrm_dbg_tol_queue_counts
struct TolLast {
    int dev = -1;
    const uint32_t* counts = nullptr; // device: one count per queue segment of the main kernel
    size_t blocks = 0, n = 0;         // segments, points
    uint32_t cap = 0;                 // slots per segment
} g_tol_last;
// Device workspace of the doubt queues (rewritten by every call), one per (device, stream) in use, grown on demand.  Streams come
// and go (a caller rotating streams; lrm_reach_dist_multi's per-call streams drop theirs explicitly): the map keeps the
// kMaxWorkspaces most recently used entries, and an entry is looked up by the stream's address only while that stream lives.
struct TolWorkspace {
    uint32_t* p = nullptr;
    size_t words = 0;
    uint64_t last_use = 0;
};
constexpr size_t kMaxWorkspaces = 16;
std::map<std::pair<int, void*>, TolWorkspace> g_tol_ws;
void tol_workspace_free(TolWorkspace& w) {
    if (w.p && g_tol_last.counts == w.p) g_tol_last = TolLast{}; // the statistic of the last call goes with its workspace
    if (w.p) (void)hipFree(w.p); // synchronises with whatever still uses it
    w = TolWorkspace{};
}
// the workspace of a stream that is about to be destroyed (call on its device, after the stream has drained)
void tol_workspace_drop(int dev, void* stream) {
    std::lock_guard<std::recursive_mutex> g(g_cache_mu);
    auto it = g_tol_ws.find(std::make_pair(dev, stream));
    if (it == g_tol_ws.end()) return;
    tol_workspace_free(it->second);
    g_tol_ws.erase(it);
}
int tol_workspace(size_t words, void* stream, uint32_t** out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev), "hipGetDevice");
    const auto key = std::make_pair(dev, stream);
    if (g_tol_ws.find(key) == g_tol_ws.end() && g_tol_ws.size() >= kMaxWorkspaces) { // the least recently used entry goes
        auto old = g_tol_ws.begin();
        for (auto jt = g_tol_ws.begin(); jt != g_tol_ws.end(); ++jt)
            if (jt->second.last_use < old->second.last_use) old = jt;
        int cur = dev;
        (void)hipSetDevice(old->first.first);
        tol_workspace_free(old->second);
        (void)hipSetDevice(cur);
        g_tol_ws.erase(old);
    }
    TolWorkspace& w = g_tol_ws[key];
    w.last_use = ++g_tol_clock;
    if (words > w.words) {
        tol_workspace_free(w);
        w.last_use = g_tol_clock;
        void* p = nullptr;
        const size_t want = words + words / 4;
        HIP_TRY(hipMalloc(&p, want * sizeof(uint32_t)), "hipMalloc tolerance-mode queues");
        w.p = static_cast<uint32_t*>(p);
        w.words = want;
    }
    *out = w.p;
    return LRM_OK;
}
// The queue words lrm_tol_prepare(n_max) reserves: at least what a call of any mode on n <= n_max points requests, with or without
// the plane table (both word counts are monotone in n), so that those calls never regrow the workspace.
size_t tol_prepare_words(size_t n_max) { return std::max(lrm_tol_tab_queue_words(n_max), lrm_tol_queue_words(n_max)); }
// The table kernels (dist_tab_kernel, dist_xtab_kernel) are the default of their modes from LRM_TOLTAB_MIN_POINTS points on
// (below, a call is launch-bound and the single launch of the kernels without a table wins); LRM_TOL_TABLE=0 in the
// environment keeps the kernels without a table (A/B runs).
#ifndef LRM_TOLTAB_MIN_POINTS
#define LRM_TOLTAB_MIN_POINTS 200000
#endif
// LRM_TOL_TABLE: "0" never, "2" for every size (tests), anything else / unset: from LRM_TOLTAB_MIN_POINTS points on
bool tol_tab_wanted(size_t n) {
    const char* e = std::getenv("LRM_TOL_TABLE");
    if (e && e[0] == '0') return false;
    if (e && e[0] == '2') return n > 0;
    return n >= (size_t)LRM_TOLTAB_MIN_POINTS;
}
// LRM_MODE_FAST takes the table-guided bit-exact kernel (dist_xtab_kernel) wherever the tolerance mode would take its table
// kernel; LRM_XTAB=0 keeps the filtered kernel of rounds 1-3 (A/B runs, and the reference the new kernel is tested against).
bool xtab_wanted(size_t n) {
    const char* e = std::getenv("LRM_XTAB");
    if (e && e[0] == '0') return false;
    return tol_tab_wanted(n);
}
// The table of E on the current device, or null (no table for this leg); rc != LRM_OK on a HIP error.  Built by the device
// builder (lrm_toltab_dev.hip, on `stream`: < 1 ms) unless LRM_TOLTAB_HOST=1 asks for the host builder or the device builder
// declines the leg (the host builder's ~30 ms + an upload); the two give the same bytes (tests/test_gpu_toltab.py).
bool toltab_host_wanted() {
    const char* e = std::getenv("LRM_TOLTAB_HOST");
    return e && e[0] == '1';
}
int tol_tab_device(TolEntry& E, void* stream, const uint8_t** out) {
    *out = nullptr;
    if (E.tab_state < 0) return LRM_OK;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev), "hipGetDevice");
    uint8_t*& td = E.tab_dev[dev];
    if (!td) {
        bool host = toltab_host_wanted() || !E.tab.empty();
        if (!host) {
            uint8_t* t = nullptr;
            size_t bytes = 0;
            float ms = 0.f;
            const int rc = lrm_build_tol_tab_dev(E.tl, (hipStream_t)stream, &t, &bytes, &ms);
            if (rc < 0) return hip_fail((hipError_t)(-rc), "plane table (device build)");
            if (rc == 1) { E.tab_state = -1; return LRM_OK; }
            if (rc == 0) {
                td = t;
                E.tab_state = 1;
                E.tab_build_ms = ms;
                g_last_tab_build_ms = ms;
            } else host = true; // the device builder declines this leg
        }
        if (host) {
            if (E.tab.empty()) {
                const auto t0 = std::chrono::steady_clock::now();
                E.tab_state = lrm_build_tol_tab(E.tl, &E.tab) ? 1 : -1;
                E.tab_build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
                g_last_tab_build_ms = E.tab_build_ms;
                if (E.tab_state < 0) { E.tab.clear(); return LRM_OK; }
            }
            void* p = nullptr;
            HIP_TRY(hipMalloc(&p, E.tab.size()), "hipMalloc plane table");
            td = static_cast<uint8_t*>(p);
            HIP_TRY(hipMemcpy(td, E.tab.data(), E.tab.size(), hipMemcpyHostToDevice), "hipMemcpy plane table");
        }
    }
    *out = td;
    return LRM_OK;
}
// distance / fused launch in the current mode, SoA (xyz_aos null) or the float3 arrays of the apply_kernel boundary (xyz_aos set:
// x, y, z, bits, dy, dz unused, dx = the float3 output).  op: 1 distance, 2 reach + distance
int launch_dist_any(int op, const float* xyz_aos, const float* x, const float* y, const float* z, size_t n, const LrmLegDimensions& leg,
                    const float* quat, const LrmCompiledLeg& L, uint8_t* mask, uint64_t* bits, float* dx, float* dy,
                    float* dz, void* stream) {
    std::lock_guard<std::recursive_mutex> g(g_cache_mu);
    const int mode = g_mode;
    hipStream_t st = (hipStream_t)stream;
    const bool tolm = mode == LRM_MODE_TOL || mode == LRM_MODE_TOL_REL;
    // 32-bit point indices in the table kernels (n + one grid stride < 2^32; LRM_MODE_TOL_REL keeps bit 31 of a queue record for a flag)
    const bool fits = n < (mode == LRM_MODE_TOL_REL ? 0x80000000ull : 0xc0000000ull);
    if ((tolm || (mode == LRM_MODE_FAST && xtab_wanted(n))) && L.fast_ok && fits) {
        TolEntry& E = tol_entry(leg, quat, L);
        const LrmTolLeg& TL = E.tl;
        if (TL.tol_ok) {
            const uint8_t* tab = nullptr;
            if (tol_tab_wanted(n)) {
                const int rc = tol_tab_device(E, stream, &tab);
                if (rc != LRM_OK) return rc;
            }
            if (tolm || tab) {
                uint32_t* w = nullptr;
                const int rc = tol_workspace(tab ? lrm_tol_tab_queue_words(n) : lrm_tol_queue_words(n), stream, &w);
                if (rc != LRM_OK) return rc;
                if (!tolm) {
                    if (xyz_aos) HIP_TRY(lrm_launch_dist_xtab_aos(op, xyz_aos, n, L, E.xl, tab, mask, dx, w, st), "table-guided bit-exact launch");
                    else HIP_TRY(lrm_launch_dist_xtab(op, x, y, z, n, L, E.xl, tab, mask, bits, dx, dy, dz, w, st), "table-guided bit-exact launch");
                } else if (tab) {
                    if (xyz_aos) HIP_TRY(lrm_launch_dist_tab_aos(op, xyz_aos, n, L, TL, E.xl, tab, mask, dx, w, tol_flags(), st), "tolerance-mode (table) launch");
                    else HIP_TRY(lrm_launch_dist_tab(op, x, y, z, n, L, TL, E.xl, tab, mask, bits, dx, dy, dz, w, tol_flags(), st), "tolerance-mode (table) launch");
                } else {
                    if (xyz_aos) HIP_TRY(lrm_launch_dist_tol_aos(op, xyz_aos, n, L, TL, mask, dx, w, tol_flags(), st), "tolerance-mode launch");
                    else HIP_TRY(lrm_launch_dist_tol(op, x, y, z, n, L, TL, mask, bits, dx, dy, dz, w, tol_flags(), st), "tolerance-mode launch");
                }
                int dev = 0;
                (void)hipGetDevice(&dev);
                // the workspace starts with one count per segment
                if (tab) g_tol_last = TolLast{dev, w, lrm_tol_tab_segments(n, mode == LRM_MODE_TOL_REL), n, (uint32_t)LRM_TOL_TAB_SEG_CAP};
                else g_tol_last = TolLast{dev, w, lrm_tol_queue_words(n) / (4 * LRM_TOL_SEG_CAP_WORDS + 4), n, (uint32_t)LRM_TOL_SEG_CAP_WORDS};
                return LRM_OK;
            }
        }
    }
    g_tol_last = TolLast{}; // this call ran the kernels without a table and without a queue: no queue statistic
    if (xyz_aos) HIP_TRY(lrm_launch_dist_aos(op, xyz_aos, n, L, mask, dx, mode != LRM_MODE_STRICT, st), "Kernel launch");
    else HIP_TRY(lrm_launch_dist_soa(op, x, y, z, n, L, mask, bits, dx, dy, dz, mode != LRM_MODE_STRICT, st), "distance launch");
    return LRM_OK;
}
int launch_dist_mode(int op, const float* x, const float* y, const float* z, size_t n, const LrmLegDimensions& leg,
                     const float* quat, const LrmCompiledLeg& L, uint8_t* mask, uint64_t* bits, float* dx, float* dy,
                     float* dz, void* stream) {
    return launch_dist_any(op, nullptr, x, y, z, n, leg, quat, L, mask, bits, dx, dy, dz, stream);
}
// distance / fused launch on the float3 arrays of the apply_kernel boundary in the current mode
int launch_dist_aos_mode(int op, const float* xyz, size_t n, const LrmLegDimensions& leg, const float* quat, const LrmCompiledLeg& L,
                         uint8_t* mask, float* dxyz, void* stream) {
    return launch_dist_any(op, xyz, nullptr, nullptr, nullptr, n, leg, quat, L, mask, nullptr, dxyz, nullptr, nullptr, stream);
}

// RAII device buffer for the host-buffer entry points
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
    template <class T> T* as() { return static_cast<T*>(p); }
};

struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    ~Events() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

// ---- pipelined host boundary (opt-in: LRM_HOST_PIPELINE=1) ---------------------------------------------------------
// apply_kernel (cross_compiled.cu:41-77) allocates, copies the whole input, runs the kernel, copies the whole output and
// frees, one after the other; for 1e7 fused points that is 16 ms of which 0.1-0.3 ms are kernels.  Where the time goes on
// this box (tools/pcie_probe.cpp, profiles/r03_pcie_probe.txt): a copy from / to memory the runtime has seen before runs
// at 56 GB/s, but the caller's output arrays are fresh (`new float3[n]`, bench.cpp:125-131): a copy INTO never-touched
// pages runs at 10 GB/s (one page fault per 4 KB, taken by the single thread that stages the copy) -- 13 of the 16 ms.
// With the pipeline the call keeps its device buffers, a few pinned staging slots and a handful of helper threads per
// device, and cuts the cloud into chunks (LRM_HOST_PIPELINE_CHUNK points, default 2^19: 6 MB in, 6.5 MB out; 2^20: 5.8 ms instead of 4.7):
//     kIn threads:   caller's input chunk -> pinned slot (memcpy) -> device (async DMA)
//     caller thread: the kernels of a chunk as soon as its input has landed
//     kOut threads:  device -> pinned slot (async DMA) -> caller's output arrays (memcpy: the page faults of the fresh
//                    arrays are taken by several threads at once, and overlap the DMA of the other chunks)
// Results are the same bytes as without the pipeline (same kernels on sub-ranges; the tolerance mode's fix-up is per
// launch anyway).  Returned ms = the sum of the chunks' kernel times (HIP events on the compute stream).
// Three streams in all (compute, H2D, D2H): ROCm maps streams onto a handful of hardware queues, and with one stream per
// helper thread a copy ended up queued behind another stream's event wait -- 6 ms stalls in one run out of two.  The
// helper threads of a direction share its stream and wait on their own events.
constexpr int kPipeIn = 4, kPipeOut = 4;
struct HostPipe {
    hipStream_t s_k = nullptr, s_in = nullptr, s_out = nullptr;
    hipEvent_t ev_slot_in[kPipeIn] = {}, ev_slot_out[kPipeOut] = {};
    void *d_in = nullptr, *d_mask = nullptr, *d_out = nullptr;
    size_t cap = 0;        // points the device buffers hold
    size_t slot_chunk = 0; // points a pinned slot holds
    void *pin_in[kPipeIn] = {}, *pin_out[kPipeOut] = {}, *pin_mask[kPipeOut] = {};
    std::vector<hipEvent_t> ev_in, ev_k0, ev_k1;
};
std::map<int, HostPipe> g_host_pipe; // per device ordinal; lives until lrm_release_workspaces()
size_t host_pipeline_chunk() {
    const char* e = std::getenv("LRM_HOST_PIPELINE_CHUNK");
    const long v = e ? std::atol(e) : 0;
    return v >= 4096 ? ((size_t)v + 63) & ~(size_t)63 : (size_t)1 << 19;
}
bool host_pipeline_enabled() {
    const char* e = std::getenv("LRM_HOST_PIPELINE");
    return e && e[0] == '1';
}
void host_pipe_free(HostPipe& P) {
    for (void* p : {P.d_in, P.d_mask, P.d_out})
        if (p) (void)hipFree(p);
    for (int k = 0; k < kPipeIn; k++) {
        if (P.pin_in[k]) (void)hipHostFree(P.pin_in[k]);
        if (P.ev_slot_in[k]) (void)hipEventDestroy(P.ev_slot_in[k]);
    }
    for (int k = 0; k < kPipeOut; k++) {
        if (P.pin_out[k]) (void)hipHostFree(P.pin_out[k]);
        if (P.pin_mask[k]) (void)hipHostFree(P.pin_mask[k]);
        if (P.ev_slot_out[k]) (void)hipEventDestroy(P.ev_slot_out[k]);
    }
    for (hipStream_t st : {P.s_k, P.s_in, P.s_out})
        if (st) (void)hipStreamDestroy(st);
    for (auto* v : {&P.ev_in, &P.ev_k0, &P.ev_k1})
        for (hipEvent_t e : *v) (void)hipEventDestroy(e);
    P = HostPipe{};
}
int host_apply_pipelined(int op, const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat,
                         uint8_t* mask_out, float* dxyz_out, float* ms, const LrmCompiledLeg& L) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev), "hipGetDevice");
    HostPipe& P = g_host_pipe[dev];
    const bool want_mask = (op != 1) || mask_out;
    const size_t chunk = host_pipeline_chunk();
    if (!P.s_k) {
        HIP_TRY(hipStreamCreateWithFlags(&P.s_k, hipStreamNonBlocking), "hipStreamCreate");
        HIP_TRY(hipStreamCreateWithFlags(&P.s_in, hipStreamNonBlocking), "hipStreamCreate");
        HIP_TRY(hipStreamCreateWithFlags(&P.s_out, hipStreamNonBlocking), "hipStreamCreate");
        for (int k = 0; k < kPipeIn; k++) HIP_TRY(hipEventCreateWithFlags(&P.ev_slot_in[k], hipEventDisableTiming), "hipEventCreate");
        for (int k = 0; k < kPipeOut; k++) HIP_TRY(hipEventCreateWithFlags(&P.ev_slot_out[k], hipEventDisableTiming), "hipEventCreate");
    }
    if (chunk > P.slot_chunk) {
        for (int k = 0; k < kPipeIn; k++) {
            if (P.pin_in[k]) (void)hipHostFree(P.pin_in[k]);
            P.pin_in[k] = nullptr;
        }
        for (int k = 0; k < kPipeOut; k++) {
            if (P.pin_out[k]) (void)hipHostFree(P.pin_out[k]);
            if (P.pin_mask[k]) (void)hipHostFree(P.pin_mask[k]);
            P.pin_out[k] = P.pin_mask[k] = nullptr;
        }
        P.slot_chunk = 0;
        for (int k = 0; k < kPipeIn; k++) HIP_TRY(hipHostMalloc(&P.pin_in[k], chunk * 3 * sizeof(float), hipHostMallocDefault), "hipHostMalloc staging");
        for (int k = 0; k < kPipeOut; k++) {
            HIP_TRY(hipHostMalloc(&P.pin_out[k], chunk * 3 * sizeof(float), hipHostMallocDefault), "hipHostMalloc staging");
            HIP_TRY(hipHostMalloc(&P.pin_mask[k], chunk, hipHostMallocDefault), "hipHostMalloc staging");
        }
        P.slot_chunk = chunk;
    }
    if (n > P.cap) {
        for (void** p : {&P.d_in, &P.d_mask, &P.d_out}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
        P.cap = 0;
        HIP_TRY(hipMalloc(&P.d_in, n * 3 * sizeof(float)), "hipMalloc gpu_in.elements");
        HIP_TRY(hipMalloc(&P.d_mask, n), "hipMalloc gpu_out.elements");
        HIP_TRY(hipMalloc(&P.d_out, n * 3 * sizeof(float)), "hipMalloc gpu_out.elements");
        P.cap = n;
    }
    const size_t nchunks = (n + chunk - 1) / chunk;
    while (P.ev_in.size() < nchunks) {
        hipEvent_t a = nullptr, b = nullptr, c = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&a, hipEventDisableTiming), "hipEventCreate");
        HIP_TRY(hipEventCreate(&b), "hipEventCreate");
        HIP_TRY(hipEventCreate(&c), "hipEventCreate");
        P.ev_in.push_back(a);
        P.ev_k0.push_back(b);
        P.ev_k1.push_back(c);
    }
    float* d_in = static_cast<float*>(P.d_in);
    uint8_t* d_mask = static_cast<uint8_t*>(P.d_mask);
    float* d_out = static_cast<float*>(P.d_out);
    // hand-over between the host threads: in_ready[c] = chunk c's "input landed" event is recorded; k_issued = chunks whose
    // kernels are queued (their "kernels done" event recorded)
    std::mutex mu, mu_in, mu_out;
    std::condition_variable cv;
    std::vector<char> in_ready(nchunks, 0);
    size_t k_issued = 0;
    hipError_t err_copy = hipSuccess;
    bool abort = false;
    auto fail_copy = [&](hipError_t e) {
        std::lock_guard<std::mutex> g(mu);
        if (err_copy == hipSuccess) err_copy = e;
        abort = true;
        cv.notify_all();
    };
    const bool dbg = std::getenv("LRM_HOST_PIPELINE_DEBUG") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(); };
    std::vector<std::thread> helpers;
    for (int k = 0; k < kPipeIn; k++)
        helpers.emplace_back([&, k] {
            hipError_t e = hipSetDevice(dev);
            for (size_t c = (size_t)k; c < nchunks && e == hipSuccess; c += kPipeIn) {
                { std::lock_guard<std::mutex> g(mu); if (abort) return; }
                const size_t lo = c * chunk, cnt = std::min(chunk, n - lo);
                const double t0 = since();
                std::memcpy(P.pin_in[k], xyz + 3 * lo, cnt * 3 * sizeof(float));
                const double t1 = since();
                {   // one thread at a time queues on the shared stream: copy + its two events stay together
                    std::lock_guard<std::mutex> q(mu_in);
                    e = hipMemcpyAsync(d_in + 3 * lo, P.pin_in[k], cnt * 3 * sizeof(float), hipMemcpyHostToDevice, P.s_in);
                    if (e == hipSuccess) e = hipEventRecord(P.ev_in[c], P.s_in);
                    if (e == hipSuccess) e = hipEventRecord(P.ev_slot_in[k], P.s_in);
                }
                if (dbg) std::fprintf(stderr, "  in[%d] chunk %zu: memcpy %.2f-%.2f ms\n", k, c, t0, t1);
                if (e == hipSuccess) {
                    std::lock_guard<std::mutex> g(mu);
                    in_ready[c] = 1;
                    cv.notify_all();
                }
                if (e == hipSuccess) e = hipEventSynchronize(P.ev_slot_in[k]); // the slot is free again
            }
            if (e != hipSuccess) fail_copy(e);
        });
    for (int k = 0; k < kPipeOut; k++)
        helpers.emplace_back([&, k] {
            hipError_t e = hipSetDevice(dev);
            for (size_t c = (size_t)k; c < nchunks && e == hipSuccess; c += kPipeOut) {
                {
                    std::unique_lock<std::mutex> g(mu);
                    cv.wait(g, [&] { return k_issued > c || abort; });
                    if (abort) return;
                }
                const size_t lo = c * chunk, cnt = std::min(chunk, n - lo);
                const bool mask_here = want_mask && mask_out, field_here = op != 0;
                {
                    std::lock_guard<std::mutex> q(mu_out);
                    e = hipStreamWaitEvent(P.s_out, P.ev_k1[c], 0);
                    if (e == hipSuccess && mask_here) e = hipMemcpyAsync(P.pin_mask[k], d_mask + lo, cnt, hipMemcpyDeviceToHost, P.s_out);
                    if (e == hipSuccess && field_here) e = hipMemcpyAsync(P.pin_out[k], d_out + 3 * lo, cnt * 3 * sizeof(float), hipMemcpyDeviceToHost, P.s_out);
                    if (e == hipSuccess) e = hipEventRecord(P.ev_slot_out[k], P.s_out);
                }
                const double t0 = since();
                if (e == hipSuccess) e = hipEventSynchronize(P.ev_slot_out[k]);
                const double t1 = since();
                if (e == hipSuccess) {
                    if (mask_here) std::memcpy(mask_out + lo, P.pin_mask[k], cnt);
                    if (field_here) std::memcpy(dxyz_out + 3 * lo, P.pin_out[k], cnt * 3 * sizeof(float));
                }
                if (dbg) std::fprintf(stderr, "  out[%d] chunk %zu: D2H wait %.2f-%.2f, memcpy to the caller's arrays until %.2f ms\n", k, c, t0, t1, since());
            }
            if (e != hipSuccess) fail_copy(e);
        });
    int rc = LRM_OK;
    hipError_t err_k = hipSuccess;
    for (size_t c = 0; c < nchunks; c++) {
        {
            std::unique_lock<std::mutex> g(mu);
            cv.wait(g, [&] { return in_ready[c] || abort; });
            if (abort) break;
        }
        const size_t lo = c * chunk, cnt = std::min(chunk, n - lo);
        err_k = hipStreamWaitEvent(P.s_k, P.ev_in[c], 0);
        if (err_k == hipSuccess) err_k = hipEventRecord(P.ev_k0[c], P.s_k);
        if (err_k == hipSuccess) {
            if (op == 0) err_k = lrm_launch_reach_aos(d_in + 3 * lo, cnt, L, d_mask + lo, g_mode != LRM_MODE_STRICT, P.s_k);
            else rc = launch_dist_aos_mode(op, d_in + 3 * lo, cnt, *leg, quat_or_default(quat), L, want_mask ? d_mask + lo : nullptr, d_out + 3 * lo, P.s_k);
        }
        if (err_k == hipSuccess && rc == LRM_OK) err_k = hipEventRecord(P.ev_k1[c], P.s_k);
        std::lock_guard<std::mutex> g(mu);
        if (err_k != hipSuccess || rc != LRM_OK) abort = true;
        else k_issued = c + 1;
        cv.notify_all();
        if (abort) break;
    }
    const double t_launched = since();
    for (auto& t : helpers) t.join();
    if (dbg) std::fprintf(stderr, "host pipeline: %zu chunks of %zu points; kernels queued after %.2f ms, helpers done after %.2f ms\n", nchunks, chunk, t_launched, since());
    if (rc != LRM_OK) return rc;
    HIP_TRY(err_k, "Kernel launch");
    HIP_TRY(err_copy, "hipMemcpy (pipelined)");
    HIP_TRY(hipStreamSynchronize(P.s_k), "hipStreamSynchronize");
    float total = 0.f;
    for (size_t c = 0; c < nchunks; c++) {
        float e = 0.f;
        HIP_TRY(hipEventElapsedTime(&e, P.ev_k0[c], P.ev_k1[c]), "hipEventElapsedTime");
        total += e;
    }
    if (ms) *ms = total;
    return LRM_OK;
}

// host-buffer skeleton of apply_kernel (cross_compiled.cu:33-79)
// op: 0 reach, 1 dist, 2 reach+dist
int host_apply(int op, const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat,
               uint8_t* mask_out, float* dxyz_out, float* ms) {
    if (!leg || (n && !xyz)) return fail(LRM_EINVAL, "null input");
    if ((op == 0 || op == 2) && n && !mask_out) return fail(LRM_EINVAL, "null mask output");
    if ((op == 1 || op == 2) && n && !dxyz_out) return fail(LRM_EINVAL, "null distance output");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(LRM_ENODEV, "no HIP device");
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    if (host_pipeline_enabled() && n >= 2 * host_pipeline_chunk()) {
        // one pipelined call at a time: its buffers, pinned slots, streams and events are per device (g_host_pipe).  Its helper
        // threads take no library lock, and the caller's own launches take g_cache_mu again (recursive).
        std::lock_guard<std::recursive_mutex> g(g_cache_mu);
        return host_apply_pipelined(op, xyz, n, leg, quat, mask_out, dxyz_out, ms, L);
    }
    DevBuf d_in, d_mask, d_out;
    HIP_TRY(d_in.alloc(n * 3 * sizeof(float)), "hipMalloc gpu_in.elements");
    const bool want_mask = (op != 1) || mask_out;
    if (want_mask) HIP_TRY(d_mask.alloc(n), "hipMalloc gpu_out.elements");
    if (op != 0) HIP_TRY(d_out.alloc(n * 3 * sizeof(float)), "hipMalloc gpu_out.elements");
    HIP_TRY(hipMemcpy(d_in.p, xyz, n * 3 * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy gpu_in.elements");
    HIP_TRY(lrm_launch_warmup(n, nullptr), "warm-up launch");
    Events ev;
    HIP_TRY(hipEventCreate(&ev.a), "hipEventCreate");
    HIP_TRY(hipEventCreate(&ev.b), "hipEventCreate");
    HIP_TRY(hipEventRecord(ev.a, nullptr), "hipEventRecord");
    if (n) {
        if (op == 0) HIP_TRY(lrm_launch_reach_aos(d_in.as<float>(), n, L, d_mask.as<uint8_t>(), g_mode != LRM_MODE_STRICT, nullptr), "Kernel launch");
        else {
            const int rc = launch_dist_aos_mode(op, d_in.as<float>(), n, *leg, quat_or_default(quat), L, want_mask ? d_mask.as<uint8_t>() : nullptr,
                                                d_out.as<float>(), nullptr);
            if (rc != LRM_OK) return rc;
        }
    }
    HIP_TRY(hipEventRecord(ev.b, nullptr), "hipEventRecord");
    HIP_TRY(hipEventSynchronize(ev.b), "Kernel launch");
    float elapsed = 0.f;
    HIP_TRY(hipEventElapsedTime(&elapsed, ev.a, ev.b), "hipEventElapsedTime");
    if (want_mask && mask_out) HIP_TRY(hipMemcpy(mask_out, d_mask.p, n, hipMemcpyDeviceToHost), "hipMemcpy gpu_out.elements");
    if (op != 0) HIP_TRY(hipMemcpy(dxyz_out, d_out.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy gpu_out.elements");
    HIP_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
    if (ms) *ms = elapsed;
    return LRM_OK;
}

} // namespace

namespace {
// Morton (Z-curve) order of an AoS cloud: indices sorted by the interleaved 10-bit cell
// coordinates of the bounding box.  Consecutive points are then spatially compact in ANY
// orientation, which is what the tile bounding-box skipping of the pair kernels needs (a raster
// row stops being a thin box as soon as the cloud is yawed).  "Any target" / per-body results do
// not depend on the order, so sorting changes no output.
std::vector<size_t> morton_order(const float* aos, const std::vector<size_t>& idx) {
    const size_t n = idx.size();
    std::vector<size_t> order(idx);
    if (n < 2) return order;
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    for (size_t i : idx)
        for (int a = 0; a < 3; a++) {
            const float v = aos[3 * i + a];
            if (v < lo[a]) lo[a] = v;
            if (v > hi[a]) hi[a] = v;
        }
    auto spread = [](uint32_t v) { // 10 bits -> every third bit
        v &= 0x3ffu;
        v = (v | (v << 16)) & 0x030000ffu;
        v = (v | (v << 8)) & 0x0300f00fu;
        v = (v | (v << 4)) & 0x030c30c3u;
        v = (v | (v << 2)) & 0x09249249u;
        return v;
    };
    std::vector<uint32_t> key(n), key2(n);
    for (size_t k = 0; k < n; k++) {
        uint32_t kk = 0;
        for (int a = 0; a < 3; a++) {
            const float span = hi[a] - lo[a];
            float t = span > 0.f ? (aos[3 * idx[k] + a] - lo[a]) / span : 0.f;
            if (!(t >= 0.f)) t = 0.f; // nan / below
            if (t > 1.f) t = 1.f;
            kk |= spread((uint32_t)(t * 1023.f)) << a;
        }
        key[k] = kk;
    }
    // stable LSD radix sort on the 30-bit key, three 10-bit passes (equal keys keep the order of `idx`):
    // lrm_morton_order on 1e5 points: 2.3 ms against 5.5 ms with std::sort on (key, index) pairs
    std::vector<size_t> order2(n);
    for (int pass = 0; pass < 3; pass++) {
        size_t count[1025] = {0};
        const int shift = 10 * pass;
        for (size_t k = 0; k < n; k++) count[((key[k] >> shift) & 1023u) + 1]++;
        for (int b = 0; b < 1024; b++) count[b + 1] += count[b];
        for (size_t k = 0; k < n; k++) {
            const size_t dst = count[(key[k] >> shift) & 1023u]++;
            key2[dst] = key[k];
            order2[dst] = order[k];
        }
        key.swap(key2);
        order.swap(order2);
    }
    return order;
}
} // namespace

// Morton order for other translation units (lrm_octree.hip)
void lrm_host_morton_order(const float* xyz_aos, size_t n, std::vector<size_t>* order) {
    std::vector<size_t> idx(n);
    for (size_t i = 0; i < n; i++) idx[i] = i;
    *order = morton_order(xyz_aos, idx);
}

extern "C" {

const char* lrm_version(void) { return "lrm-mi355x 0.1 (gfx950)"; }
const char* lrm_last_error(void) { return g_err.c_str(); }

int lrm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
int lrm_set_device(int ordinal) {
    HIP_TRY(hipSetDevice(ordinal), "hipSetDevice");
    return LRM_OK;
}
int lrm_set_mode(int mode) {
    if (mode != LRM_MODE_STRICT && mode != LRM_MODE_FAST && mode != LRM_MODE_TOL && mode != LRM_MODE_TOL_REL) return fail(LRM_EINVAL, "unknown mode");
    g_mode = mode;
    return LRM_OK;
}
int lrm_get_mode(void) { return g_mode; }

void lrm_leg_factory(float azimut, float body2coxa, float coxa_pitch_deg, float coxa2tibia, float tibia2femur,
                     float femur2tip, float coxa_angle_deg, float femur_angle_deg, float tibia_angle_deg,
                     float tib_abs_pos, float tib_abs_neg, LrmLegDimensions* out) {
    lrm_host_leg_factory(azimut, body2coxa, coxa_pitch_deg, coxa2tibia, tibia2femur, femur2tip, coxa_angle_deg,
                         femur_angle_deg, tibia_angle_deg, tib_abs_pos, tib_abs_neg, out);
}
void lrm_get_M2_leg(float azimut, LrmLegDimensions* out) {
    lrm_host_leg_factory(azimut, 181, -45, 65.5f, 129, 135, 60.0f, 90.0f, 120.0f, -5, -5, out);
}
void lrm_get_moonbot_leg(float azimut, LrmLegDimensions* out) {
    lrm_host_leg_factory(azimut, 181, 0, 65.5f, 129, 160, 60.0f, 90.0f, 120.0f, -5, -5, out);
}
void lrm_rotate_leg_data(const float quat[4], const LrmLegDimensions* leg, LrmLegDimensions* out) {
    lrm_host_rotate_leg_data(quat, *leg, out);
}

int lrm_reach(const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat, uint8_t* mask_out,
              float* ms) {
    return host_apply(0, xyz, n, leg, quat, mask_out, nullptr, ms);
}
int lrm_dist(const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat, float* dxyz_out,
             uint8_t* valid_out, float* ms) {
    return host_apply(1, xyz, n, leg, quat, valid_out, dxyz_out, ms);
}
int lrm_reach_dist(const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat, uint8_t* mask_out,
                   float* dxyz_out, float* ms) {
    return host_apply(2, xyz, n, leg, quat, mask_out, dxyz_out, ms);
}

// Host buffers in the reference's ON-DISK layout (one f32 array per component,
// several_leg.cpp:126-131, :201-219): straight to the SoA kernels, no AoS detour
// (threeArrays2float3Arr, math_util.cpp:92, disappears).  op: 0 reach, 1 dist, 2 both.
namespace {
int host_apply_soa(int op, const float* x, const float* y, const float* z, size_t n, const LrmLegDimensions* leg,
                   const float* quat, uint8_t* mask_out, float* dx, float* dy, float* dz, float* ms) {
    if (!leg || (n && (!x || !y || !z))) return fail(LRM_EINVAL, "null input");
    if ((op == 0 || op == 2) && n && !mask_out) return fail(LRM_EINVAL, "null mask output");
    if ((op == 1 || op == 2) && n && (!dx || !dy || !dz)) return fail(LRM_EINVAL, "null distance output");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(LRM_ENODEV, "no HIP device");
    if (n == 0) { if (ms) *ms = 0.f; return LRM_OK; }
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    const size_t pad = (n + 3) & ~(size_t)3; // keeps the three component arrays 16-byte aligned
    DevBuf d_in, d_mask, d_out;
    HIP_TRY(d_in.alloc(3 * pad * sizeof(float)), "hipMalloc gpu_in.elements");
    const bool want_mask = (op != 1) || mask_out;
    if (want_mask) HIP_TRY(d_mask.alloc(n), "hipMalloc gpu_out.elements");
    if (op != 0) HIP_TRY(d_out.alloc(3 * pad * sizeof(float)), "hipMalloc gpu_out.elements");
    float* I = d_in.as<float>();
    HIP_TRY(hipMemcpy(I, x, n * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy x");
    HIP_TRY(hipMemcpy(I + pad, y, n * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy y");
    HIP_TRY(hipMemcpy(I + 2 * pad, z, n * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy z");
    HIP_TRY(lrm_launch_warmup(n, nullptr), "warm-up launch");
    Events ev;
    HIP_TRY(hipEventCreate(&ev.a), "hipEventCreate");
    HIP_TRY(hipEventCreate(&ev.b), "hipEventCreate");
    HIP_TRY(hipEventRecord(ev.a, nullptr), "hipEventRecord");
    const bool fast = g_mode != LRM_MODE_STRICT;
    float* O = d_out.as<float>();
    if (op == 0) HIP_TRY(lrm_launch_reach_soa(I, I + pad, I + 2 * pad, n, L, d_mask.as<uint8_t>(), nullptr, fast, nullptr), "Kernel launch");
    else {
        const int rc = launch_dist_mode(op, I, I + pad, I + 2 * pad, n, *leg, quat_or_default(quat), L,
                                        want_mask ? d_mask.as<uint8_t>() : nullptr, nullptr, O, O + pad, O + 2 * pad, nullptr);
        if (rc != LRM_OK) return rc;
    }
    HIP_TRY(hipEventRecord(ev.b, nullptr), "hipEventRecord");
    HIP_TRY(hipEventSynchronize(ev.b), "Kernel launch");
    float elapsed = 0.f;
    HIP_TRY(hipEventElapsedTime(&elapsed, ev.a, ev.b), "hipEventElapsedTime");
    if (want_mask && mask_out) HIP_TRY(hipMemcpy(mask_out, d_mask.p, n, hipMemcpyDeviceToHost), "hipMemcpy mask");
    if (op != 0) {
        HIP_TRY(hipMemcpy(dx, O, n * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy dx");
        HIP_TRY(hipMemcpy(dy, O + pad, n * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy dy");
        HIP_TRY(hipMemcpy(dz, O + 2 * pad, n * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy dz");
    }
    if (ms) *ms = elapsed;
    return LRM_OK;
}
} // namespace

int lrm_reach_soa(const float* x, const float* y, const float* z, size_t n, const LrmLegDimensions* leg,
                  const float* quat, uint8_t* mask_out, float* ms) {
    return host_apply_soa(0, x, y, z, n, leg, quat, mask_out, nullptr, nullptr, nullptr, ms);
}
int lrm_dist_soa(const float* x, const float* y, const float* z, size_t n, const LrmLegDimensions* leg,
                 const float* quat, float* dx, float* dy, float* dz, uint8_t* valid_out, float* ms) {
    return host_apply_soa(1, x, y, z, n, leg, quat, valid_out, dx, dy, dz, ms);
}

// apply_reach_cpu / apply_dist_cpu (cross_compiled.cu:163-181): chrono-timed serial loops
int lrm_reach_cpu(const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat, uint8_t* mask_out,
                  double* ms) {
    if (!leg || (n && (!xyz || !mask_out))) return fail(LRM_EINVAL, "null argument");
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    const auto t0 = std::chrono::high_resolution_clock::now();
    for (size_t i = 0; i < n; i++)
        mask_out[i] = lrm_reach_global(L, &L.lists[0][0], LrmVec3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]});
    const auto t1 = std::chrono::high_resolution_clock::now();
    if (ms) *ms = std::chrono::duration<double>(t1 - t0).count() * 1000.0;
    return LRM_OK;
}
int lrm_dist_cpu(const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat, float* dxyz_out,
                 uint8_t* valid_out, double* ms) {
    if (!leg || (n && (!xyz || !dxyz_out))) return fail(LRM_EINVAL, "null argument");
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    const auto t0 = std::chrono::high_resolution_clock::now();
    for (size_t i = 0; i < n; i++) {
        LrmVec3 p{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        const bool v = lrm_dist_global(L, &L.lists[0][0], p);
        dxyz_out[3 * i] = p.x;
        dxyz_out[3 * i + 1] = p.y;
        dxyz_out[3 * i + 2] = p.z;
        if (valid_out) valid_out[i] = v;
    }
    const auto t1 = std::chrono::high_resolution_clock::now();
    if (ms) *ms = std::chrono::duration<double>(t1 - t0).count() * 1000.0;
    return LRM_OK;
}

// ---- device-resident entry points ------------------------------------------------------
int lrm_reach_bits_dev(const float* x, const float* y, const float* z, size_t n, const LrmLegDimensions* leg,
                       const float* quat, uint8_t* mask, uint64_t* bits, void* stream) {
    if (!leg || (n && (!x || !y || !z || (!mask && !bits)))) return fail(LRM_EINVAL, "null argument");
    if (n == 0) return LRM_OK;
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    HIP_TRY(lrm_launch_reach_soa(x, y, z, n, L, mask, bits, g_mode != LRM_MODE_STRICT, (hipStream_t)stream), "reach launch");
    return LRM_OK;
}
int lrm_reach_dev(const float* x, const float* y, const float* z, size_t n, const LrmLegDimensions* leg,
                  const float* quat, uint8_t* mask, void* stream) {
    return lrm_reach_bits_dev(x, y, z, n, leg, quat, mask, nullptr, stream);
}
int lrm_dist_dev(const float* x, const float* y, const float* z, size_t n, const LrmLegDimensions* leg,
                 const float* quat, float* dx, float* dy, float* dz, uint8_t* valid, void* stream) {
    if (!leg || (n && (!x || !y || !z || !dx || !dy || !dz))) return fail(LRM_EINVAL, "null argument");
    if (n == 0) return LRM_OK;
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    return launch_dist_mode(1, x, y, z, n, *leg, quat_or_default(quat), L, valid, nullptr, dx, dy, dz, stream);
}
int lrm_reach_dist_bits_dev(const float* x, const float* y, const float* z, size_t n,
                            const LrmLegDimensions* leg, const float* quat, uint8_t* mask, uint64_t* bits,
                            float* dx, float* dy, float* dz, void* stream) {
    if (!leg || (n && (!x || !y || !z || (!mask && !bits) || !dx || !dy || !dz)))
        return fail(LRM_EINVAL, "null argument");
    if (n == 0) return LRM_OK;
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    return launch_dist_mode(2, x, y, z, n, *leg, quat_or_default(quat), L, mask, bits, dx, dy, dz, stream);
}
int lrm_reach_dist_dev(const float* x, const float* y, const float* z, size_t n, const LrmLegDimensions* leg,
                       const float* quat, uint8_t* mask, float* dx, float* dy, float* dz, void* stream) {
    if (n && !mask) return fail(LRM_EINVAL, "null argument");
    return lrm_reach_dist_bits_dev(x, y, z, n, leg, quat, mask, nullptr, dx, dy, dz, stream);
}
int lrm_reach_aos_dev(const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat, uint8_t* mask,
                      void* stream) {
    if (!leg || (n && (!xyz || !mask))) return fail(LRM_EINVAL, "null argument");
    if (n == 0) return LRM_OK;
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    HIP_TRY(lrm_launch_reach_aos(xyz, n, L, mask, g_mode != LRM_MODE_STRICT, (hipStream_t)stream), "reach launch");
    return LRM_OK;
}
int lrm_dist_aos_dev(const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat, float* dxyz,
                     uint8_t* valid, void* stream) {
    if (!leg || (n && (!xyz || !dxyz))) return fail(LRM_EINVAL, "null argument");
    if (n == 0) return LRM_OK;
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    return launch_dist_aos_mode(1, xyz, n, *leg, quat_or_default(quat), L, valid, dxyz, stream);
}

// ---- batched multi-pose queries (lrm_posed.hip) ------------------------------------------
namespace {
int posed_args(size_t nposes, size_t nlegs, const LrmLegDimensions* legs) {
    if (nlegs > LRM_MAX_LEGS) return fail(LRM_EINVAL, "posed queries: nlegs > LRM_MAX_LEGS");
    if (nposes > (size_t)INT32_MAX) return fail(LRM_EINVAL, "posed queries: nposes does not fit the int32 pose index");
    if (nposes * nlegs > (size_t)UINT32_MAX) return fail(LRM_EINVAL, "posed queries: more than 2^32 - 1 (pose, leg) records");
    if (nlegs && !legs) return fail(LRM_EINVAL, "null argument");
    return LRM_OK;
}
// the host pose compiler: record (pose, leg) at pose * nlegs + leg, as pose_compile_kernel writes it
void host_pose_records(const float* quats, const float* body, size_t nposes, const LrmLegDimensions* legs, size_t nlegs,
                       LrmPoseRecord* out) {
    for (size_t p = 0; p < nposes; p++)
        for (size_t l = 0; l < nlegs; l++) {
            LrmPoseRecord& r = out[p * nlegs + l];
            std::memset(&r, 0, sizeof r);
            lrm_compile_head(legs[l], quats + 4 * p, 1, &r.head, (LrmLegDimensions*)nullptr);
            for (int k = 0; k < 3; k++) r.body_pos[k] = body ? body[3 * p + k] : 0.f;
        }
}
} // namespace

size_t lrm_posed_workspace_bytes(size_t nposes, size_t nlegs) { return nposes * nlegs * sizeof(LrmPoseRecord); }

int lrm_pose_compile_dev(const float* quats, const float* body, size_t nposes, const LrmLegDimensions* legs, size_t nlegs,
                         void* workspace, void* stream) {
    int rc = posed_args(nposes, nlegs, legs);
    if (rc != LRM_OK) return rc;
    if (nposes == 0 || nlegs == 0) return LRM_OK;
    if (!quats || !workspace) return fail(LRM_EINVAL, "null argument");
    if ((uintptr_t)workspace & 15) return fail(LRM_EINVAL, "posed queries: the workspace must be 16-byte aligned");
    HIP_TRY(lrm_launch_pose_compile(quats, body, nposes, legs, nlegs, workspace, (hipStream_t)stream), "pose compile launch");
    return LRM_OK;
}

int lrm_reach_dist_posed_dev(const float* x, const float* y, const float* z, size_t n, const int32_t* pose_idx,
                             const uint8_t* leg_idx, const void* workspace, size_t nposes, size_t nlegs, uint8_t* mask,
                             uint8_t* valid, float* dx, float* dy, float* dz, void* stream) {
    if (nlegs > LRM_MAX_LEGS) return fail(LRM_EINVAL, "posed queries: nlegs > LRM_MAX_LEGS");
    if (nposes > (size_t)INT32_MAX) return fail(LRM_EINVAL, "posed queries: nposes does not fit the int32 pose index");
    if (nposes * nlegs > (size_t)UINT32_MAX) return fail(LRM_EINVAL, "posed queries: more than 2^32 - 1 (pose, leg) records");
    if (n == 0) return LRM_OK;
    if (nposes == 0 || nlegs == 0) return fail(LRM_EINVAL, "posed queries: no pose or no leg for n > 0 queries");
    if (!workspace) return fail(LRM_EINVAL, "posed queries: null workspace");
    if ((uintptr_t)workspace & 15) return fail(LRM_EINVAL, "posed queries: the workspace must be 16-byte aligned");
    if (!x || !y || !z) return fail(LRM_EINVAL, "null argument");
    if (!dx != !dy || !dx != !dz) return fail(LRM_EINVAL, "posed queries: give all three field components or none");
    if (!mask && !valid && !dx) return fail(LRM_EINVAL, "posed queries: no output");
    HIP_TRY(lrm_launch_posed(x, y, z, n, pose_idx, leg_idx, workspace, nposes, nlegs, mask, valid, dx, dy, dz,
                             (hipStream_t)stream),
            "posed launch");
    return LRM_OK;
}

int lrm_reach_dist_posed_cpu(const float* xyz, size_t n, const int32_t* pose_idx, const uint8_t* leg_idx, const float* quats,
                             const float* body, size_t nposes, const LrmLegDimensions* legs, size_t nlegs, uint8_t* mask,
                             uint8_t* valid, float* dxyz, double* ms) {
    int rc = posed_args(nposes, nlegs, legs);
    if (rc != LRM_OK) return rc;
    if (n == 0) return LRM_OK;
    if (nposes == 0 || nlegs == 0) return fail(LRM_EINVAL, "posed queries: no pose or no leg for n > 0 queries");
    if (!xyz || !quats) return fail(LRM_EINVAL, "null argument");
    if (!mask && !valid && !dxyz) return fail(LRM_EINVAL, "posed queries: no output");
    std::vector<LrmPoseRecord> recs(nposes * nlegs);
    host_pose_records(quats, body, nposes, legs, nlegs, recs.data());
    const auto t0 = std::chrono::high_resolution_clock::now();
    for (size_t i = 0; i < n; i++) {
        const int32_t pi = pose_idx ? pose_idx[i] : 0;
        const uint32_t li = leg_idx ? leg_idx[i] : 0u;
        if (pi < 0 || (size_t)pi >= nposes || li >= nlegs) { // out of range: mask 0, valid 0, nan field
            if (mask) mask[i] = 0;
            if (valid) valid[i] = 0;
            if (dxyz) dxyz[3 * i] = dxyz[3 * i + 1] = dxyz[3 * i + 2] = std::nanf("");
            continue;
        }
        const LrmPoseRecord& R = recs[(size_t)pi * nlegs + li];
        const LrmLegHead& L = R.head;
        LrmVec3 p{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        p.x -= R.body_pos[0];
        p.y -= R.body_pos[1];
        p.z -= R.body_pos[2];
        if (mask) mask[i] = lrm_reach_global(L, &R.head.lists[0][0], p);
        if (valid || dxyz) {
            const bool v = lrm_dist_global(L, &R.head.lists[0][0], p);
            if (valid) valid[i] = v;
            if (dxyz) {
                dxyz[3 * i] = p.x;
                dxyz[3 * i + 1] = p.y;
                dxyz[3 * i + 2] = p.z;
            }
        }
    }
    const auto t1 = std::chrono::high_resolution_clock::now();
    if (ms) *ms = std::chrono::duration<double>(t1 - t0).count() * 1000.0;
    return LRM_OK;
}

int lrm_dbg_pose_compile_host(const float* quats, const float* body, size_t nposes, const LrmLegDimensions* legs, size_t nlegs,
                              void* records_out) {
    int rc = posed_args(nposes, nlegs, legs);
    if (rc != LRM_OK) return rc;
    if (nposes == 0 || nlegs == 0) return LRM_OK;
    if (!quats || !records_out) return fail(LRM_EINVAL, "null argument");
    host_pose_records(quats, body, nposes, legs, nlegs, (LrmPoseRecord*)records_out);
    return LRM_OK;
}

int lrm_dbg_compile_leg_head(const LrmLegDimensions* leg, const float* quat, void* out480) {
    if (!leg || !out480) return fail(LRM_EINVAL, "null argument");
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    std::memcpy(out480, &L, sizeof(LrmLegHead));
    return LRM_OK;
}

// ---- joint angles (lrm_ik.h, lrm_ik.hip) --------------------------------------------------
// The strict head of lrm_compile_leg(leg, quat, 1) and the IK constants of rotate_leg_data(quat, leg): the reach and
// distance part reads the compiled leg the strict calls use, the IK part its own small block.
namespace {
void ik_compile(const LrmLegDimensions& leg, const float* quat, LrmCompiledLeg* L, LrmIkLeg* K) {
    lrm_compile_leg(leg, quat_or_default(quat), 1, L);
    LrmLegDimensions r;
    lrm_host_rotate_leg_data(quat_or_default(quat), leg, &r);
    lrm_ik_compile(r, L->inv_rot, K);
}
} // namespace

int lrm_ik_dev(const float* x, const float* y, const float* z, size_t n, const LrmLegDimensions* leg, const float* quat,
               const float* seed_c, const float* seed_f, const float* seed_t, float* coxa, float* femur, float* tibia,
               uint8_t* status, void* stream) {
    if (!leg) return fail(LRM_EINVAL, "null argument");
    if (!seed_c != !seed_f || !seed_c != !seed_t) return fail(LRM_EINVAL, "ik: give all three seed arrays or none");
    if (n && (!x || !y || !z || !coxa || !femur || !tibia || !status)) return fail(LRM_EINVAL, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(LRM_ENODEV, "no HIP device");
    if (n == 0) return LRM_OK;
    LrmCompiledLeg L;
    LrmIkLeg K;
    ik_compile(*leg, quat, &L, &K);
    HIP_TRY(lrm_launch_ik(x, y, z, n, L, K, seed_c, seed_f, seed_t, coxa, femur, tibia, status, (hipStream_t)stream), "ik launch");
    return LRM_OK;
}

int lrm_fk_dev(const float* coxa, const float* femur, const float* tibia, size_t n, const LrmLegDimensions* leg,
               const float* quat, float* x, float* y, float* z, void* stream) {
    if (!leg || (n && (!coxa || !femur || !tibia || !x || !y || !z))) return fail(LRM_EINVAL, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(LRM_ENODEV, "no HIP device");
    if (n == 0) return LRM_OK;
    LrmCompiledLeg L;
    LrmIkLeg K;
    ik_compile(*leg, quat, &L, &K);
    HIP_TRY(lrm_launch_fk(coxa, femur, tibia, n, L, K, x, y, z, (hipStream_t)stream), "fk launch");
    return LRM_OK;
}

int lrm_ik_cpu(const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat, const float* seed,
               float* angles, uint8_t* status, double* ms) {
    if (!leg || (n && (!xyz || !angles || !status))) return fail(LRM_EINVAL, "null argument");
    LrmCompiledLeg L;
    LrmIkLeg K;
    ik_compile(*leg, quat, &L, &K);
    const LrmVec3 dseed{K.seed[0], K.seed[1], K.seed[2]};
    const auto t0 = std::chrono::high_resolution_clock::now();
    for (size_t i = 0; i < n; i++) {
        const LrmVec3 s = seed ? LrmVec3{seed[3 * i], seed[3 * i + 1], seed[3 * i + 2]} : dseed;
        LrmVec3 a;
        status[i] = lrm_ik_point(L, &L.lists[0][0], K, LrmVec3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]}, s, a);
        angles[3 * i] = a.x;
        angles[3 * i + 1] = a.y;
        angles[3 * i + 2] = a.z;
    }
    const auto t1 = std::chrono::high_resolution_clock::now();
    if (ms) *ms = std::chrono::duration<double>(t1 - t0).count() * 1000.0;
    return LRM_OK;
}

int lrm_fk_cpu(const float* angles, size_t n, const LrmLegDimensions* leg, const float* quat, float* xyz, double* ms) {
    if (!leg || (n && (!angles || !xyz))) return fail(LRM_EINVAL, "null argument");
    LrmCompiledLeg L;
    LrmIkLeg K;
    ik_compile(*leg, quat, &L, &K);
    const auto t0 = std::chrono::high_resolution_clock::now();
    for (size_t i = 0; i < n; i++) {
        const LrmVec3 p = lrm_fk_point(L, K, angles[3 * i], angles[3 * i + 1], angles[3 * i + 2]);
        xyz[3 * i] = p.x;
        xyz[3 * i + 1] = p.y;
        xyz[3 * i + 2] = p.z;
    }
    const auto t1 = std::chrono::high_resolution_clock::now();
    if (ms) *ms = std::chrono::duration<double>(t1 - t0).count() * 1000.0;
    return LRM_OK;
}

// ---- joint angles per (target, pose, leg) (lrm_ik_posed.hip) -------------------------------
namespace {
int ik_posed_tables(size_t nposes, size_t nlegs) {
    if (nlegs > LRM_MAX_LEGS) return fail(LRM_EINVAL, "posed queries: nlegs > LRM_MAX_LEGS");
    if (nposes > (size_t)INT32_MAX) return fail(LRM_EINVAL, "posed queries: nposes does not fit the int32 pose index");
    if (nposes * nlegs > (size_t)UINT32_MAX) return fail(LRM_EINVAL, "posed queries: more than 2^32 - 1 (pose, leg) records");
    return LRM_OK;
}
int ik_posed_targets(size_t nt, const int32_t* target_idx, size_t n) {
    if (nt > (size_t)INT32_MAX) return fail(LRM_EINVAL, "posed ik: nt does not fit the int32 target index");
    if (!target_idx && n > nt) return fail(LRM_EINVAL, "posed ik: n > nt without target_idx");
    return LRM_OK;
}
void host_pose_ik_records(const float* quats, size_t nposes, const LrmLegDimensions* legs, size_t nlegs, LrmIkLeg* out) {
    for (size_t p = 0; p < nposes; p++)
        for (size_t l = 0; l < nlegs; l++) lrm_ik_compile_pose(legs[l], quats + 4 * p, &out[p * nlegs + l]);
}
} // namespace

size_t lrm_posed_ik_workspace_bytes(size_t nposes, size_t nlegs) { return nposes * nlegs * sizeof(LrmIkLeg); }

int lrm_pose_ik_compile_dev(const float* quats, size_t nposes, const LrmLegDimensions* legs, size_t nlegs, void* ik_workspace,
                            void* stream) {
    int rc = posed_args(nposes, nlegs, legs);
    if (rc != LRM_OK) return rc;
    if (nposes == 0 || nlegs == 0) return LRM_OK;
    if (!quats || !ik_workspace) return fail(LRM_EINVAL, "null argument");
    if ((uintptr_t)ik_workspace & 15) return fail(LRM_EINVAL, "posed ik: the ik workspace must be 16-byte aligned");
    HIP_TRY(lrm_launch_pose_ik_compile(quats, nposes, legs, nlegs, ik_workspace, (hipStream_t)stream), "pose ik compile launch");
    return LRM_OK;
}

int lrm_dbg_pose_ik_compile_host(const float* quats, size_t nposes, const LrmLegDimensions* legs, size_t nlegs, void* records_out) {
    int rc = posed_args(nposes, nlegs, legs);
    if (rc != LRM_OK) return rc;
    if (nposes == 0 || nlegs == 0) return LRM_OK;
    if (!quats || !records_out) return fail(LRM_EINVAL, "null argument");
    host_pose_ik_records(quats, nposes, legs, nlegs, (LrmIkLeg*)records_out);
    return LRM_OK;
}

int lrm_ik_posed_dev(const float* x, const float* y, const float* z, size_t nt, const int32_t* target_idx, size_t n,
                     const int32_t* pose_idx, const uint8_t* leg_idx, const void* workspace, const void* ik_workspace, size_t nposes,
                     size_t nlegs, const float* seed_c, const float* seed_f, const float* seed_t, float* coxa, float* femur,
                     float* tibia, uint8_t* status, void* stream) {
    int rc = ik_posed_tables(nposes, nlegs);
    if (rc == LRM_OK) rc = ik_posed_targets(nt, target_idx, n);
    if (rc != LRM_OK) return rc;
    if (!seed_c != !seed_f || !seed_c != !seed_t) return fail(LRM_EINVAL, "posed ik: give all three seed arrays or none");
    if (n == 0) return LRM_OK;
    if (nposes == 0 || nlegs == 0) return fail(LRM_EINVAL, "posed queries: no pose or no leg for n > 0 queries");
    if (!workspace || !ik_workspace) return fail(LRM_EINVAL, "posed ik: null workspace");
    if (((uintptr_t)workspace | (uintptr_t)ik_workspace) & 15) return fail(LRM_EINVAL, "posed ik: the workspaces must be 16-byte aligned");
    if ((nt && (!x || !y || !z)) || !coxa || !femur || !tibia || !status) return fail(LRM_EINVAL, "null argument");
    HIP_TRY(lrm_launch_ik_posed(x, y, z, nt, target_idx, n, pose_idx, leg_idx, workspace, ik_workspace, nposes, nlegs, seed_c, seed_f,
                                seed_t, coxa, femur, tibia, status, (hipStream_t)stream),
            "posed ik launch");
    return LRM_OK;
}

int lrm_fk_posed_dev(const float* coxa, const float* femur, const float* tibia, size_t n, const int32_t* pose_idx,
                     const uint8_t* leg_idx, const void* workspace, const void* ik_workspace, size_t nposes, size_t nlegs, float* x,
                     float* y, float* z, void* stream) {
    int rc = ik_posed_tables(nposes, nlegs);
    if (rc != LRM_OK) return rc;
    if (n == 0) return LRM_OK;
    if (nposes == 0 || nlegs == 0) return fail(LRM_EINVAL, "posed queries: no pose or no leg for n > 0 queries");
    if (!workspace || !ik_workspace) return fail(LRM_EINVAL, "posed fk: null workspace");
    if (((uintptr_t)workspace | (uintptr_t)ik_workspace) & 15) return fail(LRM_EINVAL, "posed fk: the workspaces must be 16-byte aligned");
    if (!coxa || !femur || !tibia || !x || !y || !z) return fail(LRM_EINVAL, "null argument");
    HIP_TRY(lrm_launch_fk_posed(coxa, femur, tibia, n, pose_idx, leg_idx, workspace, ik_workspace, nposes, nlegs, x, y, z,
                                (hipStream_t)stream),
            "posed fk launch");
    return LRM_OK;
}

int lrm_ik_posed_cpu(const float* xyz, size_t nt, const int32_t* target_idx, size_t n, const int32_t* pose_idx,
                     const uint8_t* leg_idx, const float* quats, const float* body, size_t nposes, const LrmLegDimensions* legs,
                     size_t nlegs, const float* seed, float* angles, uint8_t* status, double* ms) {
    int rc = posed_args(nposes, nlegs, legs);
    if (rc == LRM_OK) rc = ik_posed_targets(nt, target_idx, n);
    if (rc != LRM_OK) return rc;
    if (n == 0) return LRM_OK;
    if (nposes == 0 || nlegs == 0) return fail(LRM_EINVAL, "posed queries: no pose or no leg for n > 0 queries");
    if ((nt && !xyz) || !quats || !angles || !status) return fail(LRM_EINVAL, "null argument");
    std::vector<LrmPoseRecord> recs(nposes * nlegs);
    std::vector<LrmIkLeg> iks(nposes * nlegs);
    host_pose_records(quats, body, nposes, legs, nlegs, recs.data());
    host_pose_ik_records(quats, nposes, legs, nlegs, iks.data());
    const auto t0 = std::chrono::high_resolution_clock::now();
    for (size_t i = 0; i < n; i++) {
        const int32_t pi = pose_idx ? pose_idx[i] : 0;
        const uint32_t li = leg_idx ? leg_idx[i] : 0u;
        const int64_t ti = target_idx ? (int64_t)target_idx[i] : (int64_t)i;
        if (pi < 0 || (size_t)pi >= nposes || li >= nlegs || ti < 0 || (size_t)ti >= nt) { // out of range: status 0, nan angles
            status[i] = LRM_IK_NONE;
            angles[3 * i] = angles[3 * i + 1] = angles[3 * i + 2] = std::nanf("");
            continue;
        }
        const LrmPoseRecord& R = recs[(size_t)pi * nlegs + li];
        const LrmIkLeg& K = iks[(size_t)pi * nlegs + li];
        LrmVec3 p{xyz[3 * ti], xyz[3 * ti + 1], xyz[3 * ti + 2]};
        p.x -= R.body_pos[0];
        p.y -= R.body_pos[1];
        p.z -= R.body_pos[2];
        const LrmVec3 s = seed ? LrmVec3{seed[3 * i], seed[3 * i + 1], seed[3 * i + 2]} : LrmVec3{K.seed[0], K.seed[1], K.seed[2]};
        LrmVec3 a;
        status[i] = lrm_ik_point(R.head, &R.head.lists[0][0], K, p, s, a);
        angles[3 * i] = a.x;
        angles[3 * i + 1] = a.y;
        angles[3 * i + 2] = a.z;
    }
    const auto t1 = std::chrono::high_resolution_clock::now();
    if (ms) *ms = std::chrono::duration<double>(t1 - t0).count() * 1000.0;
    return LRM_OK;
}

int lrm_fk_posed_cpu(const float* angles, size_t n, const int32_t* pose_idx, const uint8_t* leg_idx, const float* quats,
                     const float* body, size_t nposes, const LrmLegDimensions* legs, size_t nlegs, float* xyz, double* ms) {
    int rc = posed_args(nposes, nlegs, legs);
    if (rc != LRM_OK) return rc;
    if (n == 0) return LRM_OK;
    if (nposes == 0 || nlegs == 0) return fail(LRM_EINVAL, "posed queries: no pose or no leg for n > 0 queries");
    if (!angles || !quats || !xyz) return fail(LRM_EINVAL, "null argument");
    std::vector<LrmPoseRecord> recs(nposes * nlegs);
    std::vector<LrmIkLeg> iks(nposes * nlegs);
    host_pose_records(quats, body, nposes, legs, nlegs, recs.data());
    host_pose_ik_records(quats, nposes, legs, nlegs, iks.data());
    const auto t0 = std::chrono::high_resolution_clock::now();
    for (size_t i = 0; i < n; i++) {
        const int32_t pi = pose_idx ? pose_idx[i] : 0;
        const uint32_t li = leg_idx ? leg_idx[i] : 0u;
        if (pi < 0 || (size_t)pi >= nposes || li >= nlegs) {
            xyz[3 * i] = xyz[3 * i + 1] = xyz[3 * i + 2] = std::nanf("");
            continue;
        }
        const LrmPoseRecord& R = recs[(size_t)pi * nlegs + li];
        LrmVec3 p = lrm_fk_point(R.head, iks[(size_t)pi * nlegs + li], angles[3 * i],
                                 angles[3 * i + 1], angles[3 * i + 2]);
        p.x += R.body_pos[0];
        p.y += R.body_pos[1];
        p.z += R.body_pos[2];
        xyz[3 * i] = p.x;
        xyz[3 * i + 1] = p.y;
        xyz[3 * i + 2] = p.z;
    }
    const auto t1 = std::chrono::high_resolution_clock::now();
    if (ms) *ms = std::chrono::duration<double>(t1 - t0).count() * 1000.0;
    return LRM_OK;
}

// ---- body x target aggregation ---------------------------------------------------------
namespace {
// Library-owned device workspaces of the pair kernels, ONE SET PER DEVICE (a process that walks over several GPUs
// keeps them all; nothing is leaked or overwritten on a device switch):
//   boxes  the bounding boxes of the target cloud (6 floats per 1024-target tile and per 64-target chunk), grown on
//          demand: the first call for a larger cloud allocates (not capturable in a graph), later calls only launch;
//   legs   kLegSlots slots of LRM_MAX_LEGS compiled legs for in-flight launches, handed out round-robin; a slot is
//          rewritten only after the event recorded behind the launch that last read it has completed, so launches
//          queued on several streams never see each other's legs.
constexpr int kLegSlots = 16;
struct DevicePool {
    float* boxes = nullptr;
    size_t boxes_cap = 0; // tiles
    LrmCompiledLeg* legs = nullptr;
    hipEvent_t slot_done[kLegSlots] = {};
    unsigned next_slot = 0;
};
std::map<int, DevicePool> g_pools;
int device_pool(DevicePool** out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev), "hipGetDevice");
    *out = &g_pools[dev];
    return LRM_OK;
}
int tile_boxes(size_t nt, float** out) {
    const size_t ntiles = (nt + 1023) / 1024 * 17; // one box per tile + 16 chunk boxes per tile
    DevicePool* P = nullptr;
    int rc = device_pool(&P);
    if (rc != LRM_OK) return rc;
    if (ntiles > P->boxes_cap) {
        if (P->boxes) (void)hipFree(P->boxes); // synchronises with launches that still read it
        P->boxes = nullptr;
        P->boxes_cap = 0;
        void* p = nullptr;
        const size_t cap = ntiles + ntiles / 2 + 16;
        HIP_TRY(hipMalloc(&p, cap * 6 * sizeof(float)), "hipMalloc tile boxes");
        P->boxes = static_cast<float*>(p);
        P->boxes_cap = cap;
    }
    *out = P->boxes;
    return LRM_OK;
}
// a free slot for the legs of one launch; leg_slot_used() records the event behind that launch
int leg_slot(LrmCompiledLeg** out, hipEvent_t** done) {
    DevicePool* P = nullptr;
    int rc = device_pool(&P);
    if (rc != LRM_OK) return rc;
    if (!P->legs) {
        void* p = nullptr;
        HIP_TRY(hipMalloc(&p, sizeof(LrmCompiledLeg) * LRM_MAX_LEGS * kLegSlots), "hipMalloc leg pool");
        P->legs = static_cast<LrmCompiledLeg*>(p);
    }
    const unsigned slot = P->next_slot++ % kLegSlots;
    if (P->slot_done[slot]) HIP_TRY(hipEventSynchronize(P->slot_done[slot]), "hipEventSynchronize leg slot");
    else HIP_TRY(hipEventCreateWithFlags(&P->slot_done[slot], hipEventDisableTiming), "hipEventCreate leg slot");
    *out = P->legs + (size_t)slot * LRM_MAX_LEGS;
    *done = &P->slot_done[slot];
    return LRM_OK;
}
} // namespace

namespace {
int reach_any_impl(const float* bx, const float* by, const float* bz, size_t nb, const float* tx, const float* ty,
                   const float* tz, size_t nt, const LrmLegDimensions* legs, size_t nlegs, const float* quat,
                   const uint8_t* body_active, bool boxes_ready, uint8_t* out_leg_body, uint8_t* all_legs_out, void* stream);
int any_in_shape_impl(int shape, const float* cx, const float* cy, const float* cz, size_t nc, const float* tx,
                      const float* ty, const float* tz, size_t nt, float radius, float plus_z, float minus_z,
                      bool boxes_ready, uint8_t* out, void* stream);
}

int lrm_reach_any_dev(const float* bx, const float* by, const float* bz, size_t nb, const float* tx,
                      const float* ty, const float* tz, size_t nt, const LrmLegDimensions* legs, size_t nlegs,
                      const float* quat, uint8_t* out_leg_body, uint8_t* all_legs_out, void* stream) {
    return reach_any_impl(bx, by, bz, nb, tx, ty, tz, nt, legs, nlegs, quat, nullptr, false, out_leg_body, all_legs_out, stream);
}

namespace {
int reach_any_impl(const float* bx, const float* by, const float* bz, size_t nb, const float* tx, const float* ty,
                   const float* tz, size_t nt, const LrmLegDimensions* legs, size_t nlegs, const float* quat,
                   const uint8_t* body_active, bool boxes_ready, uint8_t* out_leg_body, uint8_t* all_legs_out, void* stream) {
    if (!legs || nlegs == 0 || nlegs > LRM_MAX_LEGS) return fail(LRM_EINVAL, "nlegs must be 1..LRM_MAX_LEGS");
    if (!out_leg_body || (nb && (!bx || !by || !bz)) || (nt && (!tx || !ty || !tz)))
        return fail(LRM_EINVAL, "null argument");
    if (nb == 0) return LRM_OK;
    LrmCompiledLeg host_legs[LRM_MAX_LEGS];
    for (size_t l = 0; l < nlegs; l++) lrm_compile_leg(legs[l], quat_or_default(quat), 0, &host_legs[l]);
    LrmCompiledLeg* dev_legs = nullptr;
    hipEvent_t* slot_done = nullptr;
    int rc = leg_slot(&dev_legs, &slot_done);
    if (rc != LRM_OK) return rc;
    HIP_TRY(hipMemcpyAsync(dev_legs, host_legs, sizeof(LrmCompiledLeg) * nlegs, hipMemcpyHostToDevice,
                           (hipStream_t)stream), "hipMemcpyAsync legs");
    // pageable-source async copies are staged by the runtime before returning, so host_legs may die
    bool fast = g_mode != LRM_MODE_STRICT;
    for (size_t l = 0; l < nlegs; l++) fast = fast && host_legs[l].fast_ok;
    float* boxes = nullptr;
    if (nt >= 4096) { // below that the whole cloud is a handful of tiles: nothing to skip
        rc = tile_boxes(nt, &boxes);
        if (rc != LRM_OK) return rc;
    }
    HIP_TRY(lrm_launch_reach_any(bx, by, bz, nb, tx, ty, tz, nt, dev_legs, (int)nlegs, boxes, boxes_ready && boxes, body_active,
                                 out_leg_body, all_legs_out, fast, (hipStream_t)stream), "reach_any launch");
    HIP_TRY(hipEventRecord(*slot_done, (hipStream_t)stream), "hipEventRecord leg slot"); // the slot is free again after this launch
    return LRM_OK;
}
} // namespace

// ---- per-leg foothold counts and choice (lrm_footholds_dev / lrm_footholds_cpu) --------------
namespace {
// the argument checks of both forms, in reach_any_impl's order; the range checks come before any early return
int footholds_args(size_t nt, const LrmLegDimensions* legs, size_t nlegs, const float* nominal, LrmFootNominal* nom) {
    if (nt > (size_t)INT32_MAX) return fail(LRM_EINVAL, "nt must be at most INT32_MAX");
    if (!legs || nlegs == 0 || nlegs > LRM_MAX_LEGS) return fail(LRM_EINVAL, "nlegs must be 1..LRM_MAX_LEGS");
    for (int l = 0; l < LRM_MAX_LEGS; l++)
        for (int a = 0; a < 3; a++) nom->v[l][a] = (nominal && (size_t)l < nlegs) ? nominal[3 * l + a] : 0.f;
    return LRM_OK;
}
} // namespace

int lrm_footholds_dev(const float* bx, const float* by, const float* bz, size_t nb, const float* tx, const float* ty,
                      const float* tz, size_t nt, const LrmLegDimensions* legs, size_t nlegs, const float* quat,
                      const float* nominal, int32_t* count_out, int32_t* best_out, float* best_d2_out, void* stream) {
    LrmFootNominal nom;
    int rc = footholds_args(nt, legs, nlegs, nominal, &nom);
    if (rc != LRM_OK) return rc;
    if (!count_out || !best_out || (nb && (!bx || !by || !bz)) || (nt && (!tx || !ty || !tz)))
        return fail(LRM_EINVAL, "null argument");
    if (nb == 0) return LRM_OK;
    LrmCompiledLeg host_legs[LRM_MAX_LEGS];
    for (size_t l = 0; l < nlegs; l++) lrm_compile_leg(legs[l], quat_or_default(quat), 0, &host_legs[l]);
    LrmCompiledLeg* dev_legs = nullptr;
    hipEvent_t* slot_done = nullptr;
    rc = leg_slot(&dev_legs, &slot_done);
    if (rc != LRM_OK) return rc;
    HIP_TRY(hipMemcpyAsync(dev_legs, host_legs, sizeof(LrmCompiledLeg) * nlegs, hipMemcpyHostToDevice,
                           (hipStream_t)stream), "hipMemcpyAsync legs");
    // the filtered test gives the strict test's bit (as in reach_any_impl): the answers do not depend on the mode
    bool fast = g_mode != LRM_MODE_STRICT;
    for (size_t l = 0; l < nlegs; l++) fast = fast && host_legs[l].fast_ok;
    float* boxes = nullptr;
    if (nt >= 4096) { // below that every tile is read (reach_any_impl's threshold)
        rc = tile_boxes(nt, &boxes);
        if (rc != LRM_OK) return rc;
    }
    HIP_TRY(lrm_launch_footholds(bx, by, bz, nb, tx, ty, tz, nt, dev_legs, (int)nlegs, boxes, nom, count_out, best_out,
                                 best_d2_out, fast, (hipStream_t)stream), "footholds launch");
    HIP_TRY(hipEventRecord(*slot_done, (hipStream_t)stream), "hipEventRecord leg slot"); // the slot is free again after this launch
    return LRM_OK;
}

int lrm_footholds_cpu(const float* bodies, size_t nb, const float* targets, size_t nt, const LrmLegDimensions* legs,
                      size_t nlegs, const float* quat, const float* nominal, int32_t* count_out, int32_t* best_out,
                      float* best_d2_out, double* ms) {
    LrmFootNominal nom;
    const int rc = footholds_args(nt, legs, nlegs, nominal, &nom);
    if (rc != LRM_OK) return rc;
    if (nb && (!bodies || !count_out || !best_out)) return fail(LRM_EINVAL, "null argument");
    if (nt && !targets) return fail(LRM_EINVAL, "null argument");
    LrmCompiledLeg L[LRM_MAX_LEGS];
    for (size_t l = 0; l < nlegs; l++) lrm_compile_leg(legs[l], quat_or_default(quat), 0, &L[l]);
    const auto t0 = std::chrono::high_resolution_clock::now();
    for (size_t b = 0; b < nb; b++) {
        const LrmVec3 body{bodies[3 * b], bodies[3 * b + 1], bodies[3 * b + 2]};
        for (size_t l = 0; l < nlegs; l++) {
            int32_t count = 0;
            uint64_t best = kLrmFootholdNone;
            for (size_t t = 0; t < nt; t++) {
                const LrmVec3 p{targets[3 * t], targets[3 * t + 1], targets[3 * t + 2]};
                if (!lrm_reachable_rotate_leg(L[l], &L[l].lists[0][0], p, body)) continue;
                count++;
                const uint64_t key = lrm_foothold_key(lrm_foothold_d2(p, body, nom.v[l]), (uint32_t)t);
                if (key < best) best = key;
            }
            const size_t o = l * nb + b;
            count_out[o] = count;
            best_out[o] = count ? (int32_t)(uint32_t)best : -1;
            if (best_d2_out) {
                const uint32_t hi = (uint32_t)(best >> 32);
                float d2;
                std::memcpy(&d2, &hi, sizeof d2);
                best_d2_out[o] = count ? d2 : INFINITY;
            }
        }
    }
    const auto t1 = std::chrono::high_resolution_clock::now();
    if (ms) *ms = std::chrono::duration<double>(t1 - t0).count() * 1000.0;
    return LRM_OK;
}

// ---- foothold counts and choice per (pose, leg) (lrm_footholds_posed.hip) --------------------
namespace {
// the range checks of the posed foothold calls, before any early return
int footholds_posed_args(size_t nt, size_t nposes, size_t nlegs) {
    if (nt > (size_t)INT32_MAX) return fail(LRM_EINVAL, "nt must be at most INT32_MAX");
    if (nlegs == 0 || nlegs > LRM_MAX_LEGS) return fail(LRM_EINVAL, "nlegs must be 1..LRM_MAX_LEGS");
    if (nposes > (size_t)INT32_MAX) return fail(LRM_EINVAL, "posed queries: nposes does not fit the int32 pose index");
    if (nposes * nlegs > (size_t)UINT32_MAX) return fail(LRM_EINVAL, "posed queries: more than 2^32 - 1 (pose, leg) records");
    return LRM_OK;
}
// the box workspace of a cloud whose kernel culls: null below 4096 targets, where every tile is read (reach_any_impl's threshold)
int cull_boxes(size_t nt, float** boxes) {
    *boxes = nullptr;
    return nt >= 4096 ? tile_boxes(nt, boxes) : LRM_OK;
}
// the wall time of the scope it lives in, to *ms (may be null) when the scope ends
struct ScopeMs {
    double* ms;
    std::chrono::high_resolution_clock::time_point t0 = std::chrono::high_resolution_clock::now();
    ~ScopeMs() {
        if (ms) *ms = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count() * 1000.0;
    }
};
void host_pose_foothold_entries(const float* quats, size_t nposes, const LrmLegDimensions* legs, size_t nlegs, const float* nominal,
                                LrmPoseFootEntry* out) {
    for (size_t p = 0; p < nposes; p++)
        for (size_t l = 0; l < nlegs; l++) lrm_pose_foothold_entry(legs[l], quats + 4 * p, nominal ? nominal + 3 * l : nullptr, &out[p * nlegs + l]);
}
} // namespace

size_t lrm_posed_footholds_workspace_bytes(size_t nposes, size_t nlegs) { return nposes * nlegs * sizeof(LrmPoseFootEntry); }

int lrm_pose_footholds_compile_dev(const float* quats, size_t nposes, const LrmLegDimensions* legs, size_t nlegs, const float* nominal,
                                   void* fh_workspace, void* stream) {
    int rc = posed_args(nposes, nlegs, legs);
    if (rc != LRM_OK) return rc;
    if (nposes == 0 || nlegs == 0) return LRM_OK;
    if (!quats || !fh_workspace) return fail(LRM_EINVAL, "null argument");
    if ((uintptr_t)fh_workspace & 15) return fail(LRM_EINVAL, "posed footholds: the foothold workspace must be 16-byte aligned");
    LrmFootNominal nom;
    for (int l = 0; l < LRM_MAX_LEGS; l++)
        for (int a = 0; a < 3; a++) nom.v[l][a] = (nominal && (size_t)l < nlegs) ? nominal[3 * l + a] : 0.f;
    HIP_TRY(lrm_launch_pose_footholds_compile(quats, nposes, legs, nlegs, nom, fh_workspace, (hipStream_t)stream),
            "pose footholds compile launch");
    return LRM_OK;
}

int lrm_dbg_pose_footholds_compile_host(const float* quats, size_t nposes, const LrmLegDimensions* legs, size_t nlegs,
                                        const float* nominal, void* entries_out) {
    int rc = posed_args(nposes, nlegs, legs);
    if (rc != LRM_OK) return rc;
    if (nposes == 0 || nlegs == 0) return LRM_OK;
    if (!quats || !entries_out) return fail(LRM_EINVAL, "null argument");
    host_pose_foothold_entries(quats, nposes, legs, nlegs, nominal, (LrmPoseFootEntry*)entries_out);
    return LRM_OK;
}

int lrm_footholds_posed_dev(const float* tx, const float* ty, const float* tz, size_t nt, const void* workspace,
                            const void* fh_workspace, size_t nposes, size_t nlegs, int32_t* count_out, int32_t* best_out,
                            float* best_d2_out, uint8_t* all_legs_out, void* stream) {
    int rc = footholds_posed_args(nt, nposes, nlegs);
    if (rc != LRM_OK) return rc;
    if (nposes == 0) return LRM_OK;
    if (!workspace || !fh_workspace || !count_out || !best_out || (nt && (!tx || !ty || !tz))) return fail(LRM_EINVAL, "null argument");
    if (((uintptr_t)workspace | (uintptr_t)fh_workspace) & 15)
        return fail(LRM_EINVAL, "posed footholds: the workspaces must be 16-byte aligned");
    float* boxes;
    rc = cull_boxes(nt, &boxes);
    if (rc != LRM_OK) return rc;
    HIP_TRY(lrm_launch_footholds_posed(tx, ty, tz, nt, workspace, fh_workspace, nposes, nlegs, boxes, count_out, best_out, best_d2_out,
                                       all_legs_out, (hipStream_t)stream), "posed footholds launch");
    return LRM_OK;
}

int lrm_footholds_posed_cpu(const float* targets, size_t nt, const float* quats, const float* body, size_t nposes,
                            const LrmLegDimensions* legs, size_t nlegs, const float* nominal, int32_t* count_out, int32_t* best_out,
                            float* best_d2_out, uint8_t* all_legs_out, double* ms) {
    int rc = footholds_posed_args(nt, nposes, nlegs);
    if (rc != LRM_OK) return rc;
    if (!legs) return fail(LRM_EINVAL, "null argument");
    if (nposes == 0) return LRM_OK;
    if (!quats || !count_out || !best_out || (nt && !targets)) return fail(LRM_EINVAL, "null argument");
    std::vector<LrmPoseRecord> recs(nposes * nlegs);
    host_pose_records(quats, body, nposes, legs, nlegs, recs.data());
    std::vector<LrmPoseFootEntry> ent(nposes * nlegs);
    host_pose_foothold_entries(quats, nposes, legs, nlegs, nominal, ent.data());
    const ScopeMs timer{ms};
    for (size_t p = 0; p < nposes; p++) {
        bool all = true;
        for (size_t l = 0; l < nlegs; l++) {
            const LrmPoseRecord& R = recs[p * nlegs + l];
            const LrmLegHead& L = R.head;
            const LrmVec3 b{R.body_pos[0], R.body_pos[1], R.body_pos[2]};
            int32_t count = 0;
            uint64_t best = kLrmFootholdNone;
            for (size_t t = 0; t < nt; t++) { // every target: the sphere of the entry is not consulted
                const LrmVec3 tg{targets[3 * t], targets[3 * t + 1], targets[3 * t + 2]};
                const LrmVec3 rel{tg.x - b.x, tg.y - b.y, tg.z - b.z};
                if (!lrm_reach_global(L, &R.head.lists[0][0], rel)) continue;
                count++;
                const uint64_t key = lrm_foothold_key(lrm_foothold_d2(tg, b, ent[p * nlegs + l].nominal_w), (uint32_t)t);
                if (key < best) best = key;
            }
            const size_t o = l * nposes + p;
            count_out[o] = count;
            const LrmFootholdChoice choice = lrm_foothold_key_decode(best, count != 0);
            best_out[o] = choice.index;
            if (best_d2_out) best_d2_out[o] = choice.d2;
            all = all && count > 0;
        }
        if (all_legs_out) all_legs_out[p] = all;
    }
    return LRM_OK;
}

// ---- reachable-foothold lists per (pose, leg) in CSR form (lrm_footholds_posed.hip) -----------
int lrm_foothold_offsets_dev(const int32_t* count, size_t n, int64_t* offsets_out, void* stream) {
    if (n > (size_t)UINT32_MAX) return fail(LRM_EINVAL, "foothold offsets: more than 2^32 - 1 counts");
    if (!offsets_out || (n && !count)) return fail(LRM_EINVAL, "null argument");
    HIP_TRY(lrm_launch_foothold_offsets(count, n, offsets_out, (hipStream_t)stream), "foothold offsets launch");
    return LRM_OK;
}

int lrm_foothold_lists_posed_dev(const float* tx, const float* ty, const float* tz, size_t nt, const void* workspace,
                                 const void* fh_workspace, size_t nposes, size_t nlegs, const int64_t* offsets, size_t capacity,
                                 int32_t* idx_out, float* d2_out, int32_t* written_out, void* stream) {
    int rc = footholds_posed_args(nt, nposes, nlegs);
    if (rc != LRM_OK) return rc;
    if (!offsets || !idx_out) return fail(LRM_EINVAL, "null argument");
    if (nposes == 0) return LRM_OK;
    if (!workspace || !fh_workspace || (nt && (!tx || !ty || !tz))) return fail(LRM_EINVAL, "null argument");
    if (((uintptr_t)workspace | (uintptr_t)fh_workspace) & 15)
        return fail(LRM_EINVAL, "posed footholds: the workspaces must be 16-byte aligned");
    if (nt == 0 || capacity == 0) { // every list is empty or has no room: nothing but written_out
        if (written_out)
            HIP_TRY(hipMemsetAsync(written_out, 0, nposes * nlegs * sizeof(int32_t), (hipStream_t)stream), "hipMemsetAsync written_out");
        return LRM_OK;
    }
    float* boxes;
    rc = cull_boxes(nt, &boxes);
    if (rc != LRM_OK) return rc;
    HIP_TRY(lrm_launch_foothold_lists_posed(tx, ty, tz, nt, workspace, fh_workspace, nposes, nlegs, boxes, offsets, capacity, idx_out,
                                            d2_out, written_out, (hipStream_t)stream), "posed foothold lists launch");
    return LRM_OK;
}

int lrm_foothold_lists_posed_cpu(const float* targets, size_t nt, const float* quats, const float* body, size_t nposes,
                                 const LrmLegDimensions* legs, size_t nlegs, const float* nominal, const int64_t* offsets,
                                 size_t capacity, int32_t* idx_out, float* d2_out, int32_t* written_out, double* ms) {
    int rc = footholds_posed_args(nt, nposes, nlegs);
    if (rc != LRM_OK) return rc;
    if (!offsets || !idx_out || !legs) return fail(LRM_EINVAL, "null argument");
    if (nposes == 0) return LRM_OK;
    if (!quats || (nt && !targets)) return fail(LRM_EINVAL, "null argument");
    if (nt == 0 || capacity == 0) {
        if (written_out) std::memset(written_out, 0, nposes * nlegs * sizeof(int32_t));
        if (ms) *ms = 0.0;
        return LRM_OK;
    }
    std::vector<LrmPoseRecord> recs(nposes * nlegs);
    host_pose_records(quats, body, nposes, legs, nlegs, recs.data());
    std::vector<LrmPoseFootEntry> ent(nposes * nlegs);
    host_pose_foothold_entries(quats, nposes, legs, nlegs, nominal, ent.data());
    const int64_t cap = capacity > (size_t)INT64_MAX ? INT64_MAX : (int64_t)capacity;
    const ScopeMs timer{ms};
    for (size_t p = 0; p < nposes; p++) {
        for (size_t l = 0; l < nlegs; l++) {
            const LrmPoseRecord& R = recs[p * nlegs + l];
            const LrmLegHead& L = R.head;
            const LrmVec3 b{R.body_pos[0], R.body_pos[1], R.body_pos[2]};
            const size_t o = l * nposes + p;
            const int64_t base = offsets[o], end = offsets[o + 1] < cap ? offsets[o + 1] : cap;
            const int64_t room = (base >= 0 && end > base) ? end - base : 0;
            int64_t n = 0; // reachable so far
            for (size_t t = 0; t < nt; t++) { // every target: the sphere of the entry is not consulted
                const LrmVec3 tg{targets[3 * t], targets[3 * t + 1], targets[3 * t + 2]};
                const LrmVec3 rel{tg.x - b.x, tg.y - b.y, tg.z - b.z};
                if (!lrm_reach_global(L, &R.head.lists[0][0], rel)) continue;
                if (n < room) {
                    idx_out[base + n] = (int32_t)t;
                    if (d2_out) d2_out[base + n] = lrm_foothold_d2(tg, b, ent[p * nlegs + l].nominal_w);
                }
                n++;
            }
            if (written_out) written_out[o] = (int32_t)(n < room ? n : room);
        }
    }
    return LRM_OK;
}

// ---- common-foothold counts and choice per pose transition (lrm_footholds_posed.hip) -----------
namespace {
// the range checks of both forms, before any early return
int foothold_edges_args(size_t nt, size_t nposes, size_t nlegs, size_t nedges) {
    const int rc = footholds_posed_args(nt, nposes, nlegs);
    if (rc != LRM_OK) return rc;
    if (nedges > (size_t)UINT32_MAX / nlegs) return fail(LRM_EINVAL, "foothold edges: more than 2^32 - 1 (edge, leg) outputs");
    return LRM_OK;
}
} // namespace

int lrm_foothold_edges_posed_dev(const float* tx, const float* ty, const float* tz, size_t nt, const void* workspace,
                                 const void* fh_workspace, size_t nposes, size_t nlegs, const int32_t* edge_a, const int32_t* edge_b,
                                 size_t nedges, int32_t* count_out, int32_t* best_out, float* best_d2_out, uint8_t* all_legs_out,
                                 void* stream) {
    int rc = foothold_edges_args(nt, nposes, nlegs, nedges);
    if (rc != LRM_OK) return rc;
    if (nedges == 0) return LRM_OK;
    if (!edge_a || !edge_b || !count_out || !best_out || (nt && (!tx || !ty || !tz))) return fail(LRM_EINVAL, "null argument");
    if (nposes && (!workspace || !fh_workspace)) return fail(LRM_EINVAL, "null argument"); // without poses no record is ever read
    if (((uintptr_t)workspace | (uintptr_t)fh_workspace) & 15)
        return fail(LRM_EINVAL, "posed footholds: the workspaces must be 16-byte aligned");
    float* boxes;
    rc = cull_boxes(nt, &boxes);
    if (rc != LRM_OK) return rc;
    HIP_TRY(lrm_launch_foothold_edges_posed(tx, ty, tz, nt, workspace, fh_workspace, nposes, nlegs, boxes, edge_a, edge_b, nedges,
                                            count_out, best_out, best_d2_out, all_legs_out, (hipStream_t)stream),
            "posed foothold edges launch");
    return LRM_OK;
}

int lrm_foothold_edges_posed_cpu(const float* targets, size_t nt, const float* quats, const float* body, size_t nposes,
                                 const LrmLegDimensions* legs, size_t nlegs, const float* nominal, const int32_t* edge_a,
                                 const int32_t* edge_b, size_t nedges, int32_t* count_out, int32_t* best_out, float* best_d2_out,
                                 uint8_t* all_legs_out, double* ms) {
    int rc = foothold_edges_args(nt, nposes, nlegs, nedges);
    if (rc != LRM_OK) return rc;
    if (!legs) return fail(LRM_EINVAL, "null argument");
    if (nedges == 0) return LRM_OK;
    if (!edge_a || !edge_b || !count_out || !best_out || (nposes && !quats) || (nt && !targets)) return fail(LRM_EINVAL, "null argument");
    std::vector<LrmPoseRecord> recs(nposes * nlegs);
    std::vector<LrmPoseFootEntry> ent(nposes * nlegs);
    if (nposes) {
        host_pose_records(quats, body, nposes, legs, nlegs, recs.data());
        host_pose_foothold_entries(quats, nposes, legs, nlegs, nominal, ent.data());
    }
    const ScopeMs timer{ms};
    for (size_t e = 0; e < nedges; e++) {
        const int64_t a = edge_a[e], b = edge_b[e];
        const bool valid = a >= 0 && b >= 0 && (uint64_t)a < nposes && (uint64_t)b < nposes;
        bool all = valid;
        for (size_t l = 0; l < nlegs; l++) {
            int32_t count = 0;
            uint64_t best = kLrmFootholdNone;
            if (valid) {
                const LrmPoseRecord& RA = recs[(size_t)a * nlegs + l];
                const LrmPoseRecord& RB = recs[(size_t)b * nlegs + l];
                const LrmLegHead& LA = RA.head;
                const LrmLegHead& LB = RB.head;
                const LrmVec3 ba{RA.body_pos[0], RA.body_pos[1], RA.body_pos[2]}, bb{RB.body_pos[0], RB.body_pos[1], RB.body_pos[2]};
                for (size_t t = 0; t < nt; t++) { // every target: no sphere is consulted
                    const LrmVec3 tg{targets[3 * t], targets[3 * t + 1], targets[3 * t + 2]};
                    const LrmVec3 rel_a{tg.x - ba.x, tg.y - ba.y, tg.z - ba.z}, rel_b{tg.x - bb.x, tg.y - bb.y, tg.z - bb.z};
                    if (!lrm_reach_global(LA, &RA.head.lists[0][0], rel_a) || !lrm_reach_global(LB, &RB.head.lists[0][0], rel_b)) continue;
                    count++;
                    const float d2 = lrm_foothold_d2(tg, ba, ent[(size_t)a * nlegs + l].nominal_w) +
                                     lrm_foothold_d2(tg, bb, ent[(size_t)b * nlegs + l].nominal_w); // one f32 add, no contraction
                    const uint64_t key = lrm_foothold_key(d2, (uint32_t)t);
                    if (key < best) best = key;
                }
            }
            const size_t o = l * nedges + e;
            count_out[o] = count;
            const LrmFootholdChoice choice = lrm_foothold_key_decode(best, count != 0);
            best_out[o] = choice.index;
            if (best_d2_out) best_d2_out[o] = choice.d2;
            all = all && count > 0;
        }
        if (all_legs_out) all_legs_out[e] = all;
    }
    return LRM_OK;
}

// ---- nearest-miss footholds per (pose, leg): target and body shift (lrm_foothold_misses.hip) -----------
namespace {
// lrm_footholds_posed_dev's range checks, then the margin's, before any early return
int foothold_misses_args(size_t nt, size_t nposes, size_t nlegs, float margin) {
    const int rc = footholds_posed_args(nt, nposes, nlegs);
    if (rc != LRM_OK) return rc;
    if (!(margin >= 0.f)) return fail(LRM_EINVAL, "foothold misses: margin must be >= 0 or +inf"); // negative and nan
    return LRM_OK;
}
} // namespace

int lrm_foothold_misses_posed_dev(const float* tx, const float* ty, const float* tz, size_t nt, const void* workspace,
                                  const void* fh_workspace, size_t nposes, size_t nlegs, float margin, const int32_t* count_in,
                                  int32_t* miss_out, float* miss_m2_out, float* shift_x, float* shift_y, float* shift_z,
                                  int32_t* near_out, void* stream) {
    int rc = foothold_misses_args(nt, nposes, nlegs, margin);
    if (rc != LRM_OK) return rc;
    if (nposes == 0) return LRM_OK;
    if (!workspace || !fh_workspace || !miss_out || (nt && (!tx || !ty || !tz))) return fail(LRM_EINVAL, "null argument");
    if (!shift_x != !shift_y || !shift_x != !shift_z) return fail(LRM_EINVAL, "foothold misses: give all three shift components or none");
    if (((uintptr_t)workspace | (uintptr_t)fh_workspace) & 15)
        return fail(LRM_EINVAL, "posed footholds: the workspaces must be 16-byte aligned");
    float* boxes;
    rc = cull_boxes(nt, &boxes);
    if (rc != LRM_OK) return rc;
    HIP_TRY(lrm_launch_foothold_misses_posed(tx, ty, tz, nt, workspace, fh_workspace, nposes, nlegs, boxes, margin, count_in, miss_out,
                                             miss_m2_out, shift_x, shift_y, shift_z, near_out, (hipStream_t)stream),
            "posed foothold misses launch");
    return LRM_OK;
}

int lrm_foothold_misses_posed_cpu(const float* targets, size_t nt, const float* quats, const float* body, size_t nposes,
                                  const LrmLegDimensions* legs, size_t nlegs, float margin, const int32_t* count_in,
                                  int32_t* miss_out, float* miss_m2_out, float* shift_x, float* shift_y, float* shift_z,
                                  int32_t* near_out, double* ms) {
    int rc = foothold_misses_args(nt, nposes, nlegs, margin);
    if (rc != LRM_OK) return rc;
    if (!legs) return fail(LRM_EINVAL, "null argument");
    if (nposes == 0) return LRM_OK;
    if (!quats || !miss_out || (nt && !targets)) return fail(LRM_EINVAL, "null argument");
    if (!shift_x != !shift_y || !shift_x != !shift_z) return fail(LRM_EINVAL, "foothold misses: give all three shift components or none");
    std::vector<LrmPoseRecord> recs(nposes * nlegs);
    host_pose_records(quats, body, nposes, legs, nlegs, recs.data());
    std::vector<LrmPoseFootEntry> ent(nposes * nlegs);
    host_pose_foothold_entries(quats, nposes, legs, nlegs, nullptr, ent.data()); // the sphere does not depend on the nominal point
    const ScopeMs timer{ms};
    for (size_t p = 0; p < nposes; p++) {
        for (size_t l = 0; l < nlegs; l++) {
            const size_t o = l * nposes + p;
            const LrmPoseRecord& R = recs[p * nlegs + l];
            const LrmLegHead& L = R.head;
            const LrmPoseFootEntry& E = ent[p * nlegs + l];
            const LrmVec3 b{R.body_pos[0], R.body_pos[1], R.body_pos[2]};
            int32_t near = 0;
            uint64_t best = kLrmFootholdNone;
            LrmVec3 best_d{std::nanf(""), std::nanf(""), std::nanf("")};
            if (!(count_in && count_in[o] > 0)) { // a skipped entry keeps the empty answer
                const float rm2 = lrm_foothold_miss_rm2(E.cull_r2, margin);
                for (size_t t = 0; t < nt; t++) { // every target: no box is consulted
                    const LrmVec3 q{targets[3 * t] - b.x, targets[3 * t + 1] - b.y, targets[3 * t + 2] - b.z};
                    if (!lrm_foothold_miss_candidate(q, E.cull_center, rm2)) continue;
                    if (lrm_reach_global(L, &R.head.lists[0][0], q)) continue;
                    near++;
                    LrmVec3 d = q;
                    lrm_dist_global(L, &R.head.lists[0][0], d);
                    const float m2 = lrm_foothold_miss_m2(d);
                    if (!(m2 < INFINITY)) continue;
                    const uint64_t key = lrm_foothold_key(m2, (uint32_t)t);
                    if (key < best) {
                        best = key;
                        best_d = d;
                    }
                }
            }
            const bool have = best != kLrmFootholdNone;
            const LrmFootholdChoice choice = lrm_foothold_key_decode(best, have);
            miss_out[o] = choice.index;
            if (miss_m2_out) miss_m2_out[o] = choice.d2;
            if (shift_x) {
                shift_x[o] = best_d.x;
                shift_y[o] = best_d.y;
                shift_z[o] = best_d.z;
            }
            if (near_out) near_out[o] = near;
        }
    }
    return LRM_OK;
}

// ---- per-target foothold support: which poses reach each target, per leg (lrm_foothold_support.hip) -----------
size_t lrm_foothold_support_workspace_bytes(size_t nposes, size_t nlegs, size_t nt) { return lrm_foothold_support_bytes(nposes, nlegs, nt); }

int lrm_dbg_foothold_support_grid(size_t nt, size_t nposes, uint64_t out[4]) {
    if (!out) return fail(LRM_EINVAL, "null argument");
    lrm_foothold_support_grid(nt, nposes, out);
    return LRM_OK;
}

int lrm_foothold_support_posed_dev(const float* tx, const float* ty, const float* tz, size_t nt, const void* workspace,
                                   const void* fh_workspace, size_t nposes, size_t nlegs, const uint8_t* pose_live,
                                   void* support_workspace, int32_t* count_out, int32_t* best_pose_out, float* best_d2_out,
                                   uint8_t* legs_mask_out, void* stream) {
    int rc = footholds_posed_args(nt, nposes, nlegs);
    if (rc != LRM_OK) return rc;
    if (nt == 0) return LRM_OK;
    if (!count_out || !best_pose_out || !support_workspace || !tx || !ty || !tz) return fail(LRM_EINVAL, "null argument");
    if (nposes && (!workspace || !fh_workspace)) return fail(LRM_EINVAL, "null argument"); // without poses no record is ever read
    if (((uintptr_t)workspace | (uintptr_t)fh_workspace | (uintptr_t)support_workspace) & 15)
        return fail(LRM_EINVAL, "foothold support: the workspaces must be 16-byte aligned");
    HIP_TRY(lrm_launch_foothold_support(tx, ty, tz, nt, workspace, fh_workspace, nposes, nlegs, pose_live, support_workspace, count_out,
                                        best_pose_out, best_d2_out, legs_mask_out, (hipStream_t)stream),
            "foothold support launch");
    return LRM_OK;
}

int lrm_foothold_support_posed_cpu(const float* targets, size_t nt, const float* quats, const float* body, size_t nposes,
                                   const LrmLegDimensions* legs, size_t nlegs, const float* nominal, const uint8_t* pose_live,
                                   int32_t* count_out, int32_t* best_pose_out, float* best_d2_out, uint8_t* legs_mask_out, double* ms) {
    int rc = footholds_posed_args(nt, nposes, nlegs);
    if (rc != LRM_OK) return rc;
    if (!legs) return fail(LRM_EINVAL, "null argument");
    if (nt == 0) return LRM_OK;
    if (!count_out || !best_pose_out || !targets || (nposes && !quats)) return fail(LRM_EINVAL, "null argument");
    std::vector<LrmPoseRecord> recs(nposes * nlegs);
    std::vector<LrmPoseFootEntry> ent(nposes * nlegs);
    if (nposes) {
        host_pose_records(quats, body, nposes, legs, nlegs, recs.data());
        host_pose_foothold_entries(quats, nposes, legs, nlegs, nominal, ent.data());
    }
    const ScopeMs timer{ms};
    for (size_t t = 0; t < nt; t++) {
        const LrmVec3 tg{targets[3 * t], targets[3 * t + 1], targets[3 * t + 2]};
        uint8_t mask = 0;
        for (size_t l = 0; l < nlegs; l++) {
            int32_t count = 0;
            uint64_t best = kLrmFootholdNone;
            for (size_t p = 0; p < nposes; p++) { // every pose: no sphere and no box is consulted
                if (pose_live && !pose_live[p]) continue;
                const LrmPoseRecord& R = recs[p * nlegs + l];
                const LrmLegHead& L = R.head;
                const LrmVec3 b{R.body_pos[0], R.body_pos[1], R.body_pos[2]};
                const LrmVec3 rel{tg.x - b.x, tg.y - b.y, tg.z - b.z};
                if (!lrm_reach_global(L, &R.head.lists[0][0], rel)) continue;
                count++;
                const uint64_t key = lrm_foothold_key(lrm_foothold_d2(tg, b, ent[p * nlegs + l].nominal_w), (uint32_t)p);
                if (key < best) best = key;
            }
            const size_t o = l * nt + t;
            count_out[o] = count;
            const LrmFootholdChoice choice = lrm_foothold_key_decode(best, count != 0);
            best_pose_out[o] = choice.index;
            if (best_d2_out) best_d2_out[o] = choice.d2;
            if (count) mask |= (uint8_t)(1u << l);
        }
        if (legs_mask_out) legs_mask_out[t] = mask;
    }
    return LRM_OK;
}

// ---- body clearance per pose: terrain hits, worst point and lift (lrm_body_clearance.hip) -----------
namespace {
// lrm_footholds_posed_dev's range checks, then the four scalars', before any early return
int body_clearance_args(size_t nt, size_t nposes, size_t nlegs, float radius, float plus_z, float minus_z, float floor_z) {
    const int rc = footholds_posed_args(nt, nposes, nlegs);
    if (rc != LRM_OK) return rc;
    if (radius != radius || plus_z != plus_z || minus_z != minus_z || floor_z != floor_z)
        return fail(LRM_EINVAL, "body clearance: nan scalar");
    if (radius < 0.f) return fail(LRM_EINVAL, "body clearance: radius must be >= 0 or +inf");
    if (!(std::fabs(minus_z) < INFINITY) || !(std::fabs(floor_z) < INFINITY))
        return fail(LRM_EINVAL, "body clearance: minus_z and floor_z must be finite");
    if (floor_z > minus_z) return fail(LRM_EINVAL, "body clearance: floor_z must not lie above minus_z");
    if (plus_z <= minus_z) return fail(LRM_EINVAL, "body clearance: plus_z must lie above minus_z");
    return LRM_OK;
}
} // namespace

int lrm_body_clearance_posed_dev(const float* tx, const float* ty, const float* tz, size_t nt, const void* workspace,
                                 const void* fh_workspace, size_t nposes, size_t nlegs, float radius, float plus_z, float minus_z,
                                 float floor_z, const uint8_t* live_in, int32_t* hits_out, int32_t* top_out, float* height_out,
                                 uint8_t* free_out, void* stream) {
    int rc = body_clearance_args(nt, nposes, nlegs, radius, plus_z, minus_z, floor_z);
    if (rc != LRM_OK) return rc;
    if (nposes == 0) return LRM_OK;
    if (!workspace || !fh_workspace || !hits_out || !top_out || (nt && (!tx || !ty || !tz))) return fail(LRM_EINVAL, "null argument");
    if (((uintptr_t)workspace | (uintptr_t)fh_workspace) & 15)
        return fail(LRM_EINVAL, "posed footholds: the workspaces must be 16-byte aligned");
    float* boxes;
    rc = cull_boxes(nt, &boxes);
    if (rc != LRM_OK) return rc;
    HIP_TRY(lrm_launch_body_clearance_posed(tx, ty, tz, nt, workspace, fh_workspace, nposes, nlegs, boxes, radius, plus_z, minus_z, floor_z,
                                            live_in, hits_out, top_out, height_out, free_out, (hipStream_t)stream),
            "posed body clearance launch");
    return LRM_OK;
}

int lrm_body_clearance_posed_cpu(const float* targets, size_t nt, const float* quats, const float* body, size_t nposes,
                                 const LrmLegDimensions* legs, size_t nlegs, float radius, float plus_z, float minus_z, float floor_z,
                                 const uint8_t* live_in, int32_t* hits_out, int32_t* top_out, float* height_out, uint8_t* free_out,
                                 double* ms) {
    int rc = body_clearance_args(nt, nposes, nlegs, radius, plus_z, minus_z, floor_z);
    if (rc != LRM_OK) return rc;
    if (!legs) return fail(LRM_EINVAL, "null argument");
    if (nposes == 0) return LRM_OK;
    if (!quats || !hits_out || !top_out || (nt && !targets)) return fail(LRM_EINVAL, "null argument");
    std::vector<LrmPoseRecord> recs(nposes); // leg 0's record of every pose: inv_rot and body_pos are the same in all of them
    host_pose_records(quats, body, nposes, legs, 1, recs.data());
    const ScopeMs timer{ms};
    for (size_t p = 0; p < nposes; p++) {
        const LrmPoseRecord& R = recs[p];
        const bool live = !(live_in && !live_in[p]);
        int32_t hits = 0;
        uint64_t best = kLrmClearanceNone;
        if (live) { // a skipped pose keeps the empty answer
            for (size_t t = 0; t < nt; t++) { // every target: no sphere and no box is consulted
                const LrmVec3 q{targets[3 * t] - R.body_pos[0], targets[3 * t + 1] - R.body_pos[1], targets[3 * t + 2] - R.body_pos[2]};
                float h;
                const unsigned in = lrm_clearance_test(R.head.inv_rot, q, radius, plus_z, minus_z, floor_z, &h);
                if (in & LRM_CLEARANCE_HIT) hits++;
                if (in & LRM_CLEARANCE_COLUMN) {
                    const uint64_t key = lrm_clearance_key(h, (uint32_t)t);
                    if (key < best) best = key;
                }
            }
        }
        const LrmClearanceTop top = lrm_clearance_key_decode(best);
        hits_out[p] = hits;
        top_out[p] = top.index;
        if (height_out) height_out[p] = top.height;
        if (free_out) free_out[p] = live && hits == 0;
    }
    return LRM_OK;
}

// ---- leg link clearance per (pose, leg): terrain hits on the leg's links (lrm_leg_clearance.hip) -----------
namespace {
int leg_scalar_ok(float v, const char* what) { // >= 0 and finite
    if (v != v) return fail(LRM_EINVAL, "leg clearance: nan scalar");
    if (v < 0.f || !(v < INFINITY)) return fail(LRM_EINVAL, what);
    return LRM_OK;
}
// the capsule scalars of the leg clearance and the self clearance calls: a radius array, every radius, margin and tip_clear
// >= 0 and finite; a nan anywhere is reported first
int leg_capsule_args(const float* radius, float margin, float tip_clear) {
    if (!radius) return fail(LRM_EINVAL, "null argument");
    for (int k = 0; k < 3; k++)
        if (radius[k] != radius[k]) return fail(LRM_EINVAL, "leg clearance: nan scalar");
    if (margin != margin || tip_clear != tip_clear) return fail(LRM_EINVAL, "leg clearance: nan scalar");
    int rc = LRM_OK;
    for (int k = 0; k < 3 && rc == LRM_OK; k++) rc = leg_scalar_ok(radius[k], "leg clearance: every radius must be >= 0 and finite");
    if (rc == LRM_OK) rc = leg_scalar_ok(margin, "leg clearance: margin must be >= 0 and finite");
    if (rc == LRM_OK) rc = leg_scalar_ok(tip_clear, "leg clearance: tip_clear must be >= 0 and finite");
    return rc;
}
// lrm_footholds_posed_dev's range checks, then the scalars', before any early return
int leg_clearance_args(size_t nt, size_t nposes, size_t nlegs, const float* radius, float margin, float tip_clear) {
    const int rc = footholds_posed_args(nt, nposes, nlegs);
    return rc != LRM_OK ? rc : leg_capsule_args(radius, margin, tip_clear);
}
} // namespace

int lrm_leg_clearance_posed_dev(const float* tx, const float* ty, const float* tz, size_t nt, const void* workspace,
                                const void* ik_workspace, size_t nposes, size_t nlegs, const float* coxa, const float* femur,
                                const float* tibia, const float radius[3], float margin, float tip_clear, const uint8_t* live_in,
                                int32_t* hits_out, uint8_t* links_out, int32_t* worst_out, float* pen_out, uint8_t* free_out,
                                void* stream) {
    int rc = leg_clearance_args(nt, nposes, nlegs, radius, margin, tip_clear);
    if (rc != LRM_OK) return rc;
    if (nposes == 0) return LRM_OK;
    if (!workspace || !ik_workspace || !hits_out || !links_out || !worst_out || !coxa || !femur || !tibia || (nt && (!tx || !ty || !tz)))
        return fail(LRM_EINVAL, "null argument");
    if (((uintptr_t)workspace | (uintptr_t)ik_workspace) & 15) return fail(LRM_EINVAL, "posed ik: the workspaces must be 16-byte aligned");
    float* boxes;
    rc = cull_boxes(nt, &boxes);
    if (rc != LRM_OK) return rc;
    HIP_TRY(lrm_launch_leg_clearance_posed(tx, ty, tz, nt, workspace, ik_workspace, nposes, nlegs, boxes, coxa, femur, tibia, radius, margin,
                                           tip_clear, live_in, hits_out, links_out, worst_out, pen_out, free_out, (hipStream_t)stream),
            "posed leg clearance launch");
    return LRM_OK;
}

int lrm_leg_clearance_posed_cpu(const float* targets, size_t nt, const float* quats, const float* body, size_t nposes,
                                const LrmLegDimensions* legs, size_t nlegs, const float* angles, const float radius[3], float margin,
                                float tip_clear, const uint8_t* live_in, int32_t* hits_out, uint8_t* links_out, int32_t* worst_out,
                                float* pen_out, uint8_t* free_out, double* ms) {
    int rc = leg_clearance_args(nt, nposes, nlegs, radius, margin, tip_clear);
    if (rc != LRM_OK) return rc;
    if (!legs) return fail(LRM_EINVAL, "null argument");
    if (nposes == 0) return LRM_OK;
    if (!quats || !angles || !hits_out || !links_out || !worst_out || (nt && !targets)) return fail(LRM_EINVAL, "null argument");
    std::vector<LrmPoseRecord> recs(nposes * nlegs);
    std::vector<LrmIkLeg> iks(nposes * nlegs);
    host_pose_records(quats, body, nposes, legs, nlegs, recs.data());
    host_pose_ik_records(quats, nposes, legs, nlegs, iks.data());
    const float reach[3] = {radius[0] + margin, radius[1] + margin, radius[2] + margin};
    const ScopeMs timer{ms};
    for (size_t p = 0; p < nposes; p++) {
        const bool live = !(live_in && !live_in[p]);
        bool pose_free = live;
        for (size_t l = 0; l < nlegs; l++) {
            const LrmPoseRecord& R = recs[p * nlegs + l];
            const size_t o = l * nposes + p;
            int32_t hits = 0;
            unsigned links = 0u;
            uint64_t best = kLrmLegClearanceNone;
            LrmVec3 J[4];
            if (live) lrm_leg_joints(R.head, iks[p * nlegs + l], angles[3 * o], angles[3 * o + 1],
                                     angles[3 * o + 2], tip_clear, J);
            if (live && lrm_leg_joints_finite(J)) { // a skipped pose and a skipped leg keep the empty answer
                LrmLegLinks S;
                lrm_leg_links(J, &S);
                for (size_t t = 0; t < nt; t++) { // every target: no box is consulted
                    const LrmVec3 q{targets[3 * t] - R.body_pos[0], targets[3 * t + 1] - R.body_pos[1], targets[3 * t + 2] - R.body_pos[2]};
                    float pen = 0.f;
                    const unsigned in = lrm_leg_clearance_test(S, radius, reach, q, &pen);
                    if (in & 7u) hits++;
                    links |= in & 7u;
                    if (in & LRM_LEG_NEAR) {
                        const uint64_t key = lrm_leg_clearance_key(pen, (uint32_t)t);
                        if (key < best) best = key;
                    }
                }
            }
            const LrmLegClearanceWorst worst = lrm_leg_clearance_key_decode(best);
            hits_out[o] = hits;
            links_out[o] = (uint8_t)links;
            worst_out[o] = worst.index;
            if (pen_out) pen_out[o] = worst.pen;
            pose_free = pose_free && hits == 0;
        }
        if (free_out) free_out[p] = pose_free;
    }
    return LRM_OK;
}

int lrm_leg_joints_posed_dev(const float* coxa, const float* femur, const float* tibia, size_t nposes, size_t nlegs,
                             const void* workspace, const void* ik_workspace, float tip_clear, float* joints_out, void* stream) {
    int rc = ik_posed_tables(nposes, nlegs);
    if (rc == LRM_OK) rc = leg_scalar_ok(tip_clear, "leg clearance: tip_clear must be >= 0 and finite");
    if (rc != LRM_OK) return rc;
    if (nposes == 0 || nlegs == 0) return LRM_OK;
    if (!workspace || !ik_workspace || !coxa || !femur || !tibia || !joints_out) return fail(LRM_EINVAL, "null argument");
    if (((uintptr_t)workspace | (uintptr_t)ik_workspace) & 15) return fail(LRM_EINVAL, "posed ik: the workspaces must be 16-byte aligned");
    HIP_TRY(lrm_launch_leg_joints_posed(coxa, femur, tibia, nposes, nlegs, workspace, ik_workspace, tip_clear, joints_out,
                                        (hipStream_t)stream),
            "posed leg joints launch");
    return LRM_OK;
}

int lrm_leg_joints_posed_cpu(const float* angles, const float* quats, const float* body, size_t nposes, const LrmLegDimensions* legs,
                             size_t nlegs, float tip_clear, float* joints_out, double* ms) {
    int rc = posed_args(nposes, nlegs, legs);
    if (rc == LRM_OK) rc = leg_scalar_ok(tip_clear, "leg clearance: tip_clear must be >= 0 and finite");
    if (rc != LRM_OK) return rc;
    if (nposes == 0 || nlegs == 0) return LRM_OK;
    if (!angles || !quats || !joints_out) return fail(LRM_EINVAL, "null argument");
    std::vector<LrmPoseRecord> recs(nposes * nlegs);
    std::vector<LrmIkLeg> iks(nposes * nlegs);
    host_pose_records(quats, body, nposes, legs, nlegs, recs.data());
    host_pose_ik_records(quats, nposes, legs, nlegs, iks.data());
    const ScopeMs timer{ms};
    for (size_t p = 0; p < nposes; p++)
        for (size_t l = 0; l < nlegs; l++) {
            const LrmPoseRecord& R = recs[p * nlegs + l];
            const size_t o = l * nposes + p;
            LrmVec3 J[4];
            lrm_leg_joints(R.head, iks[p * nlegs + l], angles[3 * o], angles[3 * o + 1],
                           angles[3 * o + 2], tip_clear, J);
            for (int k = 0; k < 4; k++) {
                joints_out[o * 12 + 3 * k] = lrm_leg_joint_out(J[k].x, R.body_pos[0]);
                joints_out[o * 12 + 3 * k + 1] = lrm_leg_joint_out(J[k].y, R.body_pos[1]);
                joints_out[o * 12 + 3 * k + 2] = lrm_leg_joint_out(J[k].z, R.body_pos[2]);
            }
        }
    return LRM_OK;
}

// ---- static stability per stance: support-polygon margin per lift set (lrm_stance.hip) -----------
namespace {
// every range and scalar check, before any early return; fills *P
int stance_args(size_t nt, size_t nposes, const int32_t* pose_idx, size_t nstances, size_t nlegs, const float* com, const float* plane,
                const uint8_t* lift, size_t nmasks, float min_margin, LrmStanceParams* P) {
    if (nlegs < 1 || nlegs > LRM_MAX_LEGS) return fail(LRM_EINVAL, "stance stability: nlegs must be 1..LRM_MAX_LEGS");
    if (nmasks < 1 || nmasks > LRM_STANCE_MAX_MASKS) return fail(LRM_EINVAL, "stance stability: nmasks must be 1..256");
    if (nt > (size_t)INT32_MAX || nposes > (size_t)INT32_MAX || nstances > (size_t)INT32_MAX)
        return fail(LRM_EINVAL, "stance stability: nt, nposes and nstances must not exceed INT32_MAX");
    if ((uint64_t)nmasks * (uint64_t)nstances > 0xffffffffull) return fail(LRM_EINVAL, "stance stability: more than 2^32 - 1 answers");
    if (!lift) return fail(LRM_EINVAL, "null argument");
    for (size_t m = 0; m < nmasks; m++)
        if (lift[m] >> nlegs) return fail(LRM_EINVAL, "stance stability: a lift set names a leg at or above nlegs");
    if (min_margin != min_margin || min_margin < 0.f || !(min_margin < INFINITY))
        return fail(LRM_EINVAL, "stance stability: min_margin must be >= 0 and finite");
    for (int k = 0; k < 3; k++)
        if (com && !lrm_stance_finite(com[k])) return fail(LRM_EINVAL, "stance stability: com must be finite");
    for (int k = 0; k < 6; k++)
        if (plane && !lrm_stance_finite(plane[k])) return fail(LRM_EINVAL, "stance stability: plane must be finite");
    if (!pose_idx && nstances > nposes) return fail(LRM_EINVAL, "stance stability: without pose_idx, stance s takes pose s: nstances <= nposes");
    *P = LrmStanceParams{};
    for (int k = 0; k < 3; k++) {
        P->com[k] = com ? com[k] : 0.f;
        P->u[k] = plane ? plane[k] : 0.f;
        P->v[k] = plane ? plane[3 + k] : 0.f;
    }
    P->on = plane ? 1u : 0u;
    P->min_margin = min_margin;
    P->nmasks = (uint32_t)nmasks;
    for (size_t m = 0; m < nmasks; m++) P->lift[m] = lift[m];
    return LRM_OK;
}
} // namespace

int lrm_stance_stability_dev(const float* tx, const float* ty, const float* tz, size_t nt, const float* quats, const float* body,
                             size_t nposes, const int32_t* pose_idx, const int32_t* foot, size_t nstances, size_t nlegs, const float* com,
                             const float* plane, const uint8_t* lift, size_t nmasks, float min_margin, const uint8_t* live_in,
                             float* margin_out, uint8_t* edge_out, uint8_t* stable_out, uint8_t* feet_out, void* stream) {
    LrmStanceParams P;
    const int rc = stance_args(nt, nposes, pose_idx, nstances, nlegs, com, plane, lift, nmasks, min_margin, &P);
    if (rc != LRM_OK) return rc;
    if (nstances == 0) return LRM_OK;
    if (!foot || !quats || !margin_out || !stable_out || (nt && (!tx || !ty || !tz))) return fail(LRM_EINVAL, "null argument");
    HIP_TRY(lrm_launch_stance_stability(tx, ty, tz, nt, quats, body, nposes, pose_idx, foot, nstances, nlegs, P, live_in, margin_out,
                                        edge_out, stable_out, feet_out, (hipStream_t)stream),
            "stance stability launch");
    return LRM_OK;
}

int lrm_stance_stability_cpu(const float* targets, size_t nt, const float* quats, const float* body, size_t nposes,
                             const int32_t* pose_idx, const int32_t* foot, size_t nstances, size_t nlegs, const float* com,
                             const float* plane, const uint8_t* lift, size_t nmasks, float min_margin, const uint8_t* live_in,
                             float* margin_out, uint8_t* edge_out, uint8_t* stable_out, uint8_t* feet_out, double* ms) {
    LrmStanceParams P;
    const int rc = stance_args(nt, nposes, pose_idx, nstances, nlegs, com, plane, lift, nmasks, min_margin, &P);
    if (rc != LRM_OK) return rc;
    if (nstances == 0) return LRM_OK;
    if (!foot || !quats || !margin_out || !stable_out || (nt && !targets)) return fail(LRM_EINVAL, "null argument");
    const ScopeMs timer{ms};
    for (size_t s = 0; s < nstances; s++) {
        const int64_t p = pose_idx ? (int64_t)pose_idx[s] : (int64_t)s;
        bool live = !(live_in && !live_in[s]) && p >= 0 && (uint64_t)p < nposes;
        LrmStancePt c{0.f, 0.f};
        if (live) c = lrm_stance_com(P, quats + 4 * p, &live);
        LrmStancePt f[LRM_MAX_LEGS] = {};
        uint32_t feet = 0u;
        for (size_t l = 0; live && l < nlegs; l++) {
            const int32_t ft = foot[l * nstances + s];
            if (!lrm_stance_foot_in_cloud(ft, nt)) continue;
            const float* t = targets + 3 * (size_t)ft;
            const float* b = body ? body + 3 * p : nullptr;
            const LrmVec3 q{t[0] - (b ? b[0] : 0.f), t[1] - (b ? b[1] : 0.f), t[2] - (b ? b[2] : 0.f)};
            if (!lrm_stance_foot_valid(q)) continue;
            f[l] = lrm_stance_project(P, q);
            feet |= 1u << l;
        }
        // every ordered pair of valid feet, once per stance
        uint32_t pair[64];
        uint32_t word[64];
        for (int i = 0; i < 8; i++)
            for (int j = 0; j < 8; j++) {
                const int code = i * 8 + j;
                pair[code] = 0u;
                word[code] = 0u;
                if (i == j || !((feet >> i) & 1u) || !((feet >> j) & 1u)) continue;
                const LrmStanceEdge E = lrm_stance_edge(f[i], f[j]);
                uint32_t left = 0u;
                for (int k = 0; k < 8; k++)
                    if (((feet >> k) & 1u) && lrm_stance_left(E, f[k])) left |= 1u << k;
                pair[code] = lrm_stance_pair_bits(left, i, j, lrm_stance_edge_usable(E));
                word[code] = lrm_stance_word(lrm_stance_signed(E, c));
            }
        for (size_t m = 0; m < nmasks; m++) { // every (stance, lift set)
            const uint32_t S = lrm_stance_planted(feet, P.lift[m]);
            uint64_t key = kLrmStanceNone;
            for (int code = 0; code < 64 && lrm_stance_stands(S); code++) {
                if (!lrm_stance_pair_counts(pair[code], S)) continue;
                const uint64_t kc = lrm_stance_key(word[code], (uint32_t)code);
                if (kc < key) key = kc;
            }
            const LrmStanceAnswer A = lrm_stance_key_decode(key);
            const size_t o = m * nstances + s;
            margin_out[o] = A.margin;
            if (edge_out) edge_out[o] = A.edge;
            stable_out[o] = lrm_stance_stable(A.margin, P.min_margin);
        }
        if (feet_out) feet_out[s] = (uint8_t)feet;
    }
    return LRM_OK;
}

// ---- leg-leg self clearance per set: link pairs of different legs (lrm_self_clearance.hip) -----------
namespace {
// leg_clearance_args' order and rules without the cloud: the ranges, the scalars, then the set-to-pose rule
int self_clearance_args(size_t nposes, size_t nlegs, const int32_t* pose_idx, size_t nsets, const float* radius, float margin,
                        float tip_clear) {
    if (nlegs == 0 || nlegs > LRM_MAX_LEGS) return fail(LRM_EINVAL, "nlegs must be 1..LRM_MAX_LEGS");
    if (nposes > (size_t)INT32_MAX || nsets > (size_t)INT32_MAX)
        return fail(LRM_EINVAL, "self clearance: nposes and nsets must not exceed INT32_MAX");
    if ((uint64_t)nlegs * (uint64_t)nsets > 0xffffffffull) return fail(LRM_EINVAL, "self clearance: more than 2^32 - 1 (set, leg) answers");
    const int rc = leg_capsule_args(radius, margin, tip_clear); // the capsules are lrm_leg_clearance_posed_dev's: one check, its messages
    if (rc != LRM_OK) return rc;
    if (!pose_idx && nsets > nposes) return fail(LRM_EINVAL, "self clearance: without pose_idx, set s takes pose s: nsets <= nposes");
    return LRM_OK;
}
} // namespace

int lrm_self_clearance_posed_dev(const void* workspace, const void* ik_workspace, size_t nposes, size_t nlegs, const int32_t* pose_idx,
                                 size_t nsets, const float* coxa, const float* femur, const float* tibia, const float radius[3],
                                 float margin, float tip_clear, const uint8_t* live_in, int32_t* hits_out, uint8_t* with_out,
                                 uint8_t* links_out, uint8_t* worst_out, float* pen_out, uint8_t* free_out, void* stream) {
    const int rc = self_clearance_args(nposes, nlegs, pose_idx, nsets, radius, margin, tip_clear);
    if (rc != LRM_OK) return rc;
    if (nsets == 0) return LRM_OK;
    if (!workspace || !ik_workspace || !coxa || !femur || !tibia || !hits_out || !with_out || !links_out || !worst_out)
        return fail(LRM_EINVAL, "null argument");
    if (((uintptr_t)workspace | (uintptr_t)ik_workspace) & 15) return fail(LRM_EINVAL, "posed ik: the workspaces must be 16-byte aligned");
    HIP_TRY(lrm_launch_self_clearance_posed(workspace, ik_workspace, nposes, nlegs, pose_idx, nsets, coxa, femur, tibia, radius, margin,
                                            tip_clear, live_in, hits_out, with_out, links_out, worst_out, pen_out, free_out,
                                            (hipStream_t)stream),
            "posed self clearance launch");
    return LRM_OK;
}

int lrm_self_clearance_posed_cpu(const float* quats, size_t nposes, const LrmLegDimensions* legs, size_t nlegs, const int32_t* pose_idx,
                                 size_t nsets, const float* angles, const float radius[3], float margin, float tip_clear,
                                 const uint8_t* live_in, int32_t* hits_out, uint8_t* with_out, uint8_t* links_out, uint8_t* worst_out,
                                 float* pen_out, uint8_t* free_out, double* ms) {
    const int rc = self_clearance_args(nposes, nlegs, pose_idx, nsets, radius, margin, tip_clear);
    if (rc != LRM_OK) return rc;
    if (nsets == 0) return LRM_OK;
    if (!legs || (nposes && !quats) || !angles || !hits_out || !with_out || !links_out || !worst_out) return fail(LRM_EINVAL, "null argument");
    std::vector<LrmPoseRecord> recs(nposes * nlegs);
    std::vector<LrmIkLeg> iks(nposes * nlegs);
    host_pose_records(quats, nullptr, nposes, legs, nlegs, recs.data()); // the body position is not read
    host_pose_ik_records(quats, nposes, legs, nlegs, iks.data());
    const LrmSelfRadii R = lrm_self_radii(radius, margin);
    const uint32_t npairs = lrm_self_npairs((uint32_t)nlegs);
    const ScopeMs timer{ms};
    for (size_t s = 0; s < nsets; s++) {
        const int64_t p = pose_idx ? (int64_t)pose_idx[s] : (int64_t)s;
        const bool live = !(live_in && !live_in[s]) && p >= 0 && (uint64_t)p < nposes;
        LrmVec3 J[LRM_MAX_LEGS][4];
        uint32_t legs_ok = 0u;
        for (size_t l = 0; live && l < nlegs; l++) { // the joints once per (set, leg)
            const size_t o = l * nsets + s;
            lrm_leg_joints(recs[p * nlegs + l].head, iks[p * nlegs + l], angles[3 * o],
                           angles[3 * o + 1], angles[3 * o + 2], tip_clear, J[l]);
            if (lrm_leg_joints_finite(J[l])) legs_ok |= 1u << l;
        }
        LrmSelfLeg A[LRM_MAX_LEGS];
        for (size_t l = 0; l < nlegs; l++) A[l] = lrm_self_leg_empty();
        for (uint32_t code = 0; live && code < npairs; code++) { // every pair once; both legs read the same d
            const uint32_t pk = lrm_self_pair_of(code);
            const uint32_t i = lrm_self_pair_i(pk), j = lrm_self_pair_j(pk), ka = lrm_self_pair_ka(pk), kb = lrm_self_pair_kb(pk);
            if (!((legs_ok >> i) & 1u) || !((legs_ok >> j) & 1u) || !((R.tested >> (ka * 3u + kb)) & 1u)) continue;
            const float d = lrm_self_pair_dist(J[i][ka], J[i][ka + 1], J[j][kb], J[j][kb + 1]);
            float pen = 0.f;
            const unsigned bits = lrm_self_clearance_test(d, R.rr[ka * 3u + kb], R.reach[ka * 3u + kb], &pen);
            if (!bits) continue;
            lrm_self_leg_take(&A[i], i, pk, bits, pen);
            lrm_self_leg_take(&A[j], j, pk, bits, pen);
        }
        bool set_free = live;
        for (size_t l = 0; l < nlegs; l++) {
            const size_t o = l * nsets + s;
            const LrmSelfWorst W = lrm_self_key_decode(A[l].key);
            hits_out[o] = A[l].hits;
            with_out[o] = (uint8_t)A[l].with;
            links_out[o] = (uint8_t)A[l].links;
            worst_out[o] = W.code;
            if (pen_out) pen_out[o] = W.pen;
            set_free = set_free && A[l].hits == 0;
        }
        if (free_out) free_out[s] = set_free;
    }
    return LRM_OK;
}

// ---- trunk-leg clearance per set: leg links against the body cylinder (lrm_trunk_clearance.hip) -----------
namespace {
// self_clearance_args' order and rules, then the cylinder and the link mask
int trunk_clearance_args(size_t nposes, size_t nlegs, const int32_t* pose_idx, size_t nsets, const float* radius, float margin,
                         float tip_clear, float trunk_radius, float plus_z, float minus_z, uint8_t links) {
    const int rc = self_clearance_args(nposes, nlegs, pose_idx, nsets, radius, margin, tip_clear);
    if (rc != LRM_OK) return rc;
    if (!lrm_ik_finite(trunk_radius) || !lrm_ik_finite(plus_z) || !lrm_ik_finite(minus_z))
        return fail(LRM_EINVAL, "trunk clearance: trunk_radius, plus_z and minus_z must be finite");
    if (trunk_radius < 0.f) return fail(LRM_EINVAL, "trunk clearance: trunk_radius must be >= 0");
    if (plus_z <= minus_z) return fail(LRM_EINVAL, "trunk clearance: plus_z must exceed minus_z");
    if (links >> 3) return fail(LRM_EINVAL, "trunk clearance: links has bits 0..2 only (coxa, femur, tibia link)");
    return LRM_OK;
}
} // namespace

int lrm_trunk_clearance_posed_dev(const void* workspace, const void* ik_workspace, size_t nposes, size_t nlegs, const int32_t* pose_idx,
                                  size_t nsets, const float* coxa, const float* femur, const float* tibia, const float radius[3],
                                  float margin, float tip_clear, float trunk_radius, float plus_z, float minus_z, uint8_t links,
                                  const uint8_t* live_in, uint8_t* links_out, uint8_t* worst_out, float* pen_out, uint8_t* free_out,
                                  void* stream) {
    const int rc = trunk_clearance_args(nposes, nlegs, pose_idx, nsets, radius, margin, tip_clear, trunk_radius, plus_z, minus_z, links);
    if (rc != LRM_OK) return rc;
    if (nsets == 0) return LRM_OK;
    if (!workspace || !ik_workspace || !coxa || !femur || !tibia || !links_out || !worst_out) return fail(LRM_EINVAL, "null argument");
    if (((uintptr_t)workspace | (uintptr_t)ik_workspace) & 15) return fail(LRM_EINVAL, "posed ik: the workspaces must be 16-byte aligned");
    HIP_TRY(lrm_launch_trunk_clearance_posed(workspace, ik_workspace, nposes, nlegs, pose_idx, nsets, coxa, femur, tibia, radius, margin,
                                             tip_clear, trunk_radius, plus_z, minus_z, links, live_in, links_out, worst_out, pen_out,
                                             free_out, (hipStream_t)stream),
            "posed trunk clearance launch");
    return LRM_OK;
}

int lrm_trunk_clearance_posed_cpu(const float* quats, size_t nposes, const LrmLegDimensions* legs, size_t nlegs, const int32_t* pose_idx,
                                  size_t nsets, const float* angles, const float radius[3], float margin, float tip_clear,
                                  float trunk_radius, float plus_z, float minus_z, uint8_t links, const uint8_t* live_in,
                                  uint8_t* links_out, uint8_t* worst_out, float* pen_out, uint8_t* free_out, double* ms) {
    const int rc = trunk_clearance_args(nposes, nlegs, pose_idx, nsets, radius, margin, tip_clear, trunk_radius, plus_z, minus_z, links);
    if (rc != LRM_OK) return rc;
    if (nsets == 0) return LRM_OK;
    if (!legs || (nposes && !quats) || !angles || !links_out || !worst_out) return fail(LRM_EINVAL, "null argument");
    std::vector<LrmPoseRecord> recs(nposes * nlegs);
    std::vector<LrmIkLeg> iks(nposes * nlegs);
    host_pose_records(quats, nullptr, nposes, legs, nlegs, recs.data()); // the body position is not read
    host_pose_ik_records(quats, nposes, legs, nlegs, iks.data());
    const LrmTrunkRadii R = lrm_trunk_radii(radius, margin, links);
    const LrmTrunk C{trunk_radius, plus_z, minus_z};
    const ScopeMs timer{ms};
    for (size_t s = 0; s < nsets; s++) {
        const int64_t p = pose_idx ? (int64_t)pose_idx[s] : (int64_t)s;
        const bool live = !(live_in && !live_in[s]) && p >= 0 && (uint64_t)p < nposes;
        bool set_free = live;
        for (size_t l = 0; l < nlegs; l++) {
            const size_t o = l * nsets + s;
            LrmTrunkLeg A = lrm_trunk_leg_empty();
            if (live) {
                const LrmPoseRecord& rec = recs[p * nlegs + l];
                LrmVec3 J[4];
                lrm_leg_joints(rec.head, iks[p * nlegs + l], angles[3 * o], angles[3 * o + 1],
                               angles[3 * o + 2], tip_clear, J);
                if (lrm_leg_joints_finite(J)) A = lrm_trunk_leg(C, R, rec.head.inv_rot, J);
            }
            links_out[o] = (uint8_t)A.links;
            worst_out[o] = (uint8_t)A.worst;
            if (pen_out) pen_out[o] = A.pen;
            set_free = set_free && A.links == 0u;
        }
        if (free_out) free_out[s] = set_free;
    }
    return LRM_OK;
}

// ---- diagnostics: lrm_trunk_clearance.h's link distance on arrays (host build / device build) -----------
int lrm_dbg_trunk_link_dist_host(const float* segs, size_t n, float trunk_radius, float plus_z, float minus_z, float* out) {
    if (n && (!segs || !out)) return fail(LRM_EINVAL, "null argument");
    const LrmTrunk C{trunk_radius, plus_z, minus_z};
    for (size_t i = 0; i < n; i++) {
        const float* g = segs + 6 * i;
        out[i] = lrm_trunk_link_dist(C, LrmVec3{g[0], g[1], g[2]}, LrmVec3{g[3], g[4], g[5]});
    }
    return LRM_OK;
}
int lrm_dbg_trunk_link_dist_dev(const float* segs, size_t n, float trunk_radius, float plus_z, float minus_z, float* out, void* stream) {
    if (n && (!segs || !out)) return fail(LRM_EINVAL, "null argument");
    if (n == 0) return LRM_OK;
    HIP_TRY(lrm_launch_trunk_link_dist(segs, n, trunk_radius, plus_z, minus_z, out, (hipStream_t)stream), "trunk link distance launch");
    return LRM_OK;
}

// ---- planted-foot reach along pose transitions: sampled motion per edge (lrm_edge_transit.hip) -----------
namespace {
// the range checks of both forms, before any early return
int edge_transit_args(size_t nt, size_t nposes, size_t nlegs, size_t nedges, size_t nsamples) {
    if (nlegs < 1 || nlegs > LRM_MAX_LEGS) return fail(LRM_EINVAL, "edge transit: nlegs must be 1..LRM_MAX_LEGS");
    if (nsamples < 2 || nsamples > LRM_TRANSIT_MAX_SAMPLES) return fail(LRM_EINVAL, "edge transit: nsamples must be 2..64");
    if (nt > (size_t)INT32_MAX || nposes > (size_t)INT32_MAX) return fail(LRM_EINVAL, "edge transit: nt and nposes must not exceed INT32_MAX");
    if (nedges > (size_t)UINT32_MAX / nlegs) return fail(LRM_EINVAL, "edge transit: more than 2^32 - 1 (edge, leg) outputs");
    return LRM_OK;
}
} // namespace

int lrm_edge_transit_posed_dev(const float* tx, const float* ty, const float* tz, size_t nt, const float* quats, const float* body,
                               size_t nposes, const LrmLegDimensions* legs, size_t nlegs, const int32_t* edge_a, const int32_t* edge_b,
                               size_t nedges, const int32_t* foot, size_t nsamples, const uint8_t* live_in, uint64_t* mask_out,
                               int32_t* reached_out, int32_t* first_miss_out, int32_t* worst_out, float* worst_d2_out,
                               uint8_t* planted_out, uint8_t* clear_out, int32_t* advance_out, void* stream) {
    const int rc = edge_transit_args(nt, nposes, nlegs, nedges, nsamples);
    if (rc != LRM_OK) return rc;
    if (nedges == 0) return LRM_OK;
    if (!quats || !legs || !edge_a || !edge_b || !foot || !reached_out || !first_miss_out || (nt && (!tx || !ty || !tz)))
        return fail(LRM_EINVAL, "null argument");
    HIP_TRY(lrm_launch_edge_transit_posed(tx, ty, tz, nt, quats, body, nposes, legs, nlegs, edge_a, edge_b, nedges, foot, nsamples, live_in,
                                          mask_out, reached_out, first_miss_out, worst_out, worst_d2_out, planted_out, clear_out,
                                          advance_out, (hipStream_t)stream),
            "edge transit launch");
    return LRM_OK;
}

int lrm_edge_transit_posed_cpu(const float* targets, size_t nt, const float* quats, const float* body, size_t nposes,
                               const LrmLegDimensions* legs, size_t nlegs, const int32_t* edge_a, const int32_t* edge_b, size_t nedges,
                               const int32_t* foot, size_t nsamples, const uint8_t* live_in, uint64_t* mask_out, int32_t* reached_out,
                               int32_t* first_miss_out, int32_t* worst_out, float* worst_d2_out, uint8_t* planted_out,
                               uint8_t* clear_out, int32_t* advance_out, double* ms) {
    const int rc = edge_transit_args(nt, nposes, nlegs, nedges, nsamples);
    if (rc != LRM_OK) return rc;
    if (nedges == 0) return LRM_OK;
    if (!quats || !legs || !edge_a || !edge_b || !foot || !reached_out || !first_miss_out || (nt && !targets))
        return fail(LRM_EINVAL, "null argument");
    const uint32_t S = (uint32_t)nsamples;
    LrmLegHead H;
    const ScopeMs timer{ms};
    for (size_t e = 0; e < nedges; e++) {
        const int64_t a = edge_a[e], b = edge_b[e];
        const bool live = !(live_in && !live_in[e]) && a >= 0 && b >= 0 && (uint64_t)a < nposes && (uint64_t)b < nposes;
        LrmVec3 ba{0.f, 0.f, 0.f}, bb{0.f, 0.f, 0.f};
        if (live && body) {
            ba = LrmVec3{body[3 * a], body[3 * a + 1], body[3 * a + 2]};
            bb = LrmVec3{body[3 * b], body[3 * b + 1], body[3 * b + 2]};
        }
        uint32_t planted_bits = 0u;
        bool all_reach = true;
        int32_t advance = (int32_t)S;
        for (size_t l = 0; l < nlegs; l++) {
            const size_t o = l * nedges + e;
            LrmTransitLeg A = lrm_transit_leg_unplanted();
            if (live && lrm_transit_foot_in_cloud(foot[o], (uint32_t)nt)) {
                const float* t = targets + 3 * (size_t)foot[o];
                uint64_t mask = 0ull, key = 0ull;
                for (uint32_t s = 0; s < S; s++) {
                    const LrmTransitSample smp = lrm_transit_sample(quats + 4 * a, quats + 4 * b, ba, bb, s, S);
                    const LrmVec3 p{t[0] - smp.body.x, t[1] - smp.body.y, t[2] - smp.body.z};
                    float d2 = 0.f;
                    if (lrm_transit_eval(legs[l], smp.q, p, &H, &d2)) {
                        mask |= 1ull << s;
                    } else {
                        const uint64_t k = lrm_transit_key(d2, s);
                        if (k > key) key = k;
                    }
                }
                A = lrm_transit_leg(mask, key, S);
                planted_bits |= 1u << l;
                all_reach = all_reach && A.first_miss < 0;
                if (A.first_miss >= 0 && A.first_miss < advance) advance = A.first_miss;
            }
            if (mask_out) mask_out[o] = A.mask;
            reached_out[o] = A.reached;
            first_miss_out[o] = A.first_miss;
            if (worst_out) worst_out[o] = A.worst;
            if (worst_d2_out) worst_d2_out[o] = A.worst_d2;
        }
        if (planted_out) planted_out[e] = (uint8_t)planted_bits;
        if (clear_out) clear_out[e] = live && all_reach;
        if (advance_out) advance_out[e] = live ? advance : 0;
    }
    return LRM_OK;
}

// ---- swing-foot transit: reach and terrain clearance of a lifted foot per (edge, leg) (lrm_swing.hip) -----------
namespace {
// edge_transit's range checks, then the scalars', before any early return; *upv receives up or its default (0, 0, 1)
int swing_transit_args(size_t nt, size_t nposes, size_t nlegs, size_t nedges, size_t nsamples, float lift, const float* up,
                       float foot_radius, float margin, uint32_t skip, float upv[3]) {
    const int rc = edge_transit_args(nt, nposes, nlegs, nedges, nsamples);
    if (rc != LRM_OK) return rc;
    if (!std::isfinite(lift) || !std::isfinite(foot_radius) || !std::isfinite(margin))
        return fail(LRM_EINVAL, "swing transit: lift, foot_radius and margin must be finite");
    if (foot_radius < 0.f || margin < 0.f) return fail(LRM_EINVAL, "swing transit: foot_radius and margin must be >= 0");
    if (skip > LRM_SWING_MAX_SKIP) return fail(LRM_EINVAL, "swing transit: skip must be 0..63");
    upv[0] = upv[1] = 0.f;
    upv[2] = 1.f;
    if (up) {
        for (int k = 0; k < 3; k++) upv[k] = up[k];
        if (!std::isfinite(up[0]) || !std::isfinite(up[1]) || !std::isfinite(up[2])) return fail(LRM_EINVAL, "swing transit: up must be finite");
    }
    return LRM_OK;
}
} // namespace

int lrm_swing_transit_posed_dev(const float* tx, const float* ty, const float* tz, size_t nt, const float* quats, const float* body,
                                size_t nposes, const LrmLegDimensions* legs, size_t nlegs, const int32_t* edge_a, const int32_t* edge_b,
                                size_t nedges, const int32_t* foot_from, const int32_t* foot_to, size_t nsamples, float lift,
                                const float* up, float foot_radius, float margin, uint32_t skip, const uint8_t* live_in,
                                uint64_t* mask_out, int32_t* reached_out, int32_t* first_miss_out, int32_t* worst_out,
                                float* worst_d2_out, int32_t* hits_out, int32_t* hit_seg_out, int32_t* near_out, float* pen_out,
                                uint8_t* swinging_out, uint8_t* clear_out, void* stream) {
    float upv[3];
    int rc = swing_transit_args(nt, nposes, nlegs, nedges, nsamples, lift, up, foot_radius, margin, skip, upv);
    if (rc != LRM_OK) return rc;
    if (nedges == 0) return LRM_OK;
    if (!quats || !legs || !edge_a || !edge_b || !foot_from || !foot_to || !reached_out || !first_miss_out || !hits_out || !hit_seg_out ||
        !near_out || (nt && (!tx || !ty || !tz)))
        return fail(LRM_EINVAL, "null argument");
    float* boxes = nullptr; // foot_radius == 0: no terrain test, no box buffer, the call only launches
    if (foot_radius > 0.f) {
        rc = cull_boxes(nt, &boxes);
        if (rc != LRM_OK) return rc;
    }
    HIP_TRY(lrm_launch_swing_transit_posed(tx, ty, tz, nt, quats, body, nposes, legs, nlegs, edge_a, edge_b, nedges, foot_from, foot_to,
                                           nsamples, lift, upv, foot_radius, margin, skip, boxes, live_in, mask_out, reached_out,
                                           first_miss_out, worst_out, worst_d2_out, hits_out, hit_seg_out, near_out, pen_out, swinging_out,
                                           clear_out, (hipStream_t)stream),
            "swing transit launch");
    return LRM_OK;
}

int lrm_swing_transit_posed_cpu(const float* targets, size_t nt, const float* quats, const float* body, size_t nposes,
                                const LrmLegDimensions* legs, size_t nlegs, const int32_t* edge_a, const int32_t* edge_b, size_t nedges,
                                const int32_t* foot_from, const int32_t* foot_to, size_t nsamples, float lift, const float* up,
                                float foot_radius, float margin, uint32_t skip, const uint8_t* live_in, uint64_t* mask_out,
                                int32_t* reached_out, int32_t* first_miss_out, int32_t* worst_out, float* worst_d2_out, int32_t* hits_out,
                                int32_t* hit_seg_out, int32_t* near_out, float* pen_out, uint8_t* swinging_out, uint8_t* clear_out,
                                double* ms) {
    float upv[3];
    const int rc = swing_transit_args(nt, nposes, nlegs, nedges, nsamples, lift, up, foot_radius, margin, skip, upv);
    if (rc != LRM_OK) return rc;
    if (nedges == 0) return LRM_OK;
    if (!quats || !legs || !edge_a || !edge_b || !foot_from || !foot_to || !reached_out || !first_miss_out || !hits_out || !hit_seg_out ||
        !near_out || (nt && !targets))
        return fail(LRM_EINVAL, "null argument");
    const uint32_t S = (uint32_t)nsamples;
    const LrmVec3 U{upv[0], upv[1], upv[2]};
    const LrmSwingRange range = lrm_swing_range(S, skip);
    const bool terrain = foot_radius > 0.f && range.k0 < range.k1;
    const float reach = foot_radius + margin;
    LrmLegHead H;
    LrmVec3 P[LRM_TRANSIT_MAX_SAMPLES];
    LrmSwingSeg seg[LRM_TRANSIT_MAX_SAMPLES];
    const ScopeMs timer{ms};
    for (size_t e = 0; e < nedges; e++) {
        const int64_t a = edge_a[e], b = edge_b[e];
        const bool live = !(live_in && !live_in[e]) && a >= 0 && b >= 0 && (uint64_t)a < nposes && (uint64_t)b < nposes;
        LrmVec3 ba{0.f, 0.f, 0.f}, bb{0.f, 0.f, 0.f};
        if (live && body) {
            ba = LrmVec3{body[3 * a], body[3 * a + 1], body[3 * a + 2]};
            bb = LrmVec3{body[3 * b], body[3 * b + 1], body[3 * b + 2]};
        }
        uint32_t swing_bits = 0u;
        bool clear = live;
        for (size_t l = 0; l < nlegs; l++) {
            const size_t o = l * nedges + e;
            LrmTransitLeg T = lrm_transit_leg_unplanted();
            LrmSwingTerrain N = lrm_swing_terrain_empty();
            if (live && lrm_transit_foot_in_cloud(foot_from[o], (uint32_t)nt) && lrm_transit_foot_in_cloud(foot_to[o], (uint32_t)nt)) {
                const uint32_t ifrom = (uint32_t)foot_from[o], ito = (uint32_t)foot_to[o];
                const float* ta = targets + 3 * (size_t)ifrom;
                const float* tb = targets + 3 * (size_t)ito;
                const LrmVec3 A{ta[0], ta[1], ta[2]}, B{tb[0], tb[1], tb[2]};
                const LrmVec3 D{B.x - A.x, B.y - A.y, B.z - A.z};
                uint64_t mask = 0ull, key = 0ull;
                for (uint32_t s = 0; s < S; s++) {
                    P[s] = lrm_swing_path_point(D, lift, U, s, S);
                    const LrmTransitSample smp = lrm_transit_sample(quats + 4 * a, quats + 4 * b, ba, bb, s, S);
                    const LrmVec3 F = lrm_swing_foot(A, B, P[s], s, S);
                    const LrmVec3 p{F.x - smp.body.x, F.y - smp.body.y, F.z - smp.body.z};
                    float d2 = 0.f;
                    if (lrm_transit_eval(legs[l], smp.q, p, &H, &d2)) {
                        mask |= 1ull << s;
                    } else {
                        const uint64_t k = lrm_transit_key(d2, s);
                        if (k > key) key = k;
                    }
                }
                T = lrm_transit_leg(mask, key, S);
                swing_bits |= 1u << l;
                bool tested = terrain;
                for (uint32_t k = range.k0; tested && k <= range.k1; k++) tested = lrm_swing_point_finite(P[k]);
                if (tested) { // every target: no box is consulted
                    for (uint32_t k = range.k0; k < range.k1; k++) seg[k] = lrm_swing_seg(P[k], P[k + 1]);
                    uint32_t hits = 0u, first_hit = kLrmSwingNoSeg;
                    uint64_t best = kLrmLegClearanceNone;
                    for (size_t t = 0; t < nt; t++) {
                        if (t == ifrom || t == ito) continue; // the two footholds themselves are never tested
                        const LrmVec3 q{targets[3 * t] - A.x, targets[3 * t + 1] - A.y, targets[3 * t + 2] - A.z};
                        float pen = 0.f;
                        uint32_t fh = kLrmSwingNoSeg;
                        const unsigned in = lrm_swing_test(seg, range, foot_radius, reach, q, &pen, &fh);
                        if (in & LRM_SWING_HIT) hits++;
                        if (fh < first_hit) first_hit = fh;
                        if (in & LRM_SWING_NEAR) {
                            const uint64_t k = lrm_leg_clearance_key(pen, (uint32_t)t);
                            if (k < best) best = k;
                        }
                    }
                    N = lrm_swing_terrain(hits, first_hit, best);
                }
                clear = clear && T.first_miss < 0 && N.hits == 0;
            }
            if (mask_out) mask_out[o] = T.mask;
            reached_out[o] = T.reached;
            first_miss_out[o] = T.first_miss;
            if (worst_out) worst_out[o] = T.worst;
            if (worst_d2_out) worst_d2_out[o] = T.worst_d2;
            hits_out[o] = N.hits;
            hit_seg_out[o] = N.hit_seg;
            near_out[o] = N.near;
            if (pen_out) pen_out[o] = N.pen;
        }
        if (swinging_out) swinging_out[e] = (uint8_t)swing_bits;
        if (clear_out) clear_out[e] = clear;
    }
    return LRM_OK;
}

// ---- static foot loads and joint torques per set and lift set (lrm_stance_loads.hip) -----------
namespace {
// every range and scalar check in the documented order, before any early return; fills *P
int stance_loads_args(size_t nposes, size_t nlegs, const int32_t* pose_idx, size_t nsets, const float* com, const float* plane,
                      const uint8_t* lift, size_t nmasks, const float* tau_max, LrmLoadsParams* P) {
    if (nlegs < 1 || nlegs > LRM_MAX_LEGS) return fail(LRM_EINVAL, "stance loads: nlegs must be 1..LRM_MAX_LEGS");
    if (nmasks < 1 || nmasks > LRM_STANCE_MAX_MASKS) return fail(LRM_EINVAL, "stance loads: nmasks must be 1..256");
    if (nposes > (size_t)INT32_MAX || nsets > (size_t)INT32_MAX)
        return fail(LRM_EINVAL, "stance loads: nposes and nsets must not exceed INT32_MAX");
    if ((uint64_t)nmasks * (uint64_t)nlegs * 3ull * (uint64_t)nsets > 0xffffffffull)
        return fail(LRM_EINVAL, "stance loads: more than 2^32 - 1 (lift set, leg, joint, set) answers");
    if (!lift) return fail(LRM_EINVAL, "null argument");
    for (size_t m = 0; m < nmasks; m++)
        if (lift[m] >> nlegs) return fail(LRM_EINVAL, "stance loads: a lift set names a leg at or above nlegs");
    if (!tau_max) return fail(LRM_EINVAL, "null argument");
    for (int k = 0; k < 3; k++)
        if (!(tau_max[k] > 0.f)) return fail(LRM_EINVAL, "stance loads: tau_max must be > 0 (+inf allowed)");
    for (int k = 0; k < 3; k++)
        if (com && !lrm_stance_finite(com[k])) return fail(LRM_EINVAL, "stance loads: com must be finite");
    for (int k = 0; k < 6; k++)
        if (plane && !lrm_stance_finite(plane[k])) return fail(LRM_EINVAL, "stance loads: plane must be finite");
    if (!pose_idx && nsets > nposes) return fail(LRM_EINVAL, "stance loads: without pose_idx, set s takes pose s: nsets <= nposes");
    *P = LrmLoadsParams{};
    for (int k = 0; k < 3; k++) {
        P->S.com[k] = com ? com[k] : 0.f;
        P->S.u[k] = plane ? plane[k] : 0.f;
        P->S.v[k] = plane ? plane[3 + k] : 0.f;
        P->tau_max[k] = tau_max[k];
    }
    P->S.on = plane ? 1u : 0u;
    P->S.nmasks = (uint32_t)nmasks;
    for (size_t m = 0; m < nmasks; m++) P->S.lift[m] = lift[m];
    lrm_loads_up(P->S, P->up);
    return LRM_OK;
}
} // namespace

int lrm_stance_loads_posed_dev(const void* workspace, const void* ik_workspace, const float* quats, size_t nposes, size_t nlegs,
                               const int32_t* pose_idx, size_t nsets, const float* coxa, const float* femur, const float* tibia,
                               const float* com, const float* plane, const uint8_t* lift, size_t nmasks, const float* tau_max,
                               const uint8_t* live_in, uint8_t* status_out, uint8_t* holdable_out, float* peak_out, uint8_t* peak_at_out,
                               float* load_out, float* tau_out, void* stream) {
    LrmLoadsParams P;
    const int rc = stance_loads_args(nposes, nlegs, pose_idx, nsets, com, plane, lift, nmasks, tau_max, &P);
    if (rc != LRM_OK) return rc;
    if (nsets == 0) return LRM_OK;
    if (!workspace || !ik_workspace || !quats || !coxa || !femur || !tibia || !status_out || !holdable_out || !peak_out)
        return fail(LRM_EINVAL, "null argument");
    if (((uintptr_t)workspace | (uintptr_t)ik_workspace) & 15) return fail(LRM_EINVAL, "posed ik: the workspaces must be 16-byte aligned");
    HIP_TRY(lrm_launch_stance_loads_posed(workspace, ik_workspace, quats, nposes, nlegs, pose_idx, nsets, coxa, femur, tibia, P, live_in,
                                          status_out, holdable_out, peak_out, peak_at_out, load_out, tau_out, (hipStream_t)stream),
            "posed stance loads launch");
    return LRM_OK;
}

int lrm_stance_loads_posed_cpu(const float* quats, size_t nposes, const LrmLegDimensions* legs, size_t nlegs, const int32_t* pose_idx,
                               size_t nsets, const float* angles, const float* com, const float* plane, const uint8_t* lift,
                               size_t nmasks, const float* tau_max, const uint8_t* live_in, uint8_t* status_out, uint8_t* holdable_out,
                               float* peak_out, uint8_t* peak_at_out, float* load_out, float* tau_out, double* ms) {
    LrmLoadsParams P;
    const int rc = stance_loads_args(nposes, nlegs, pose_idx, nsets, com, plane, lift, nmasks, tau_max, &P);
    if (rc != LRM_OK) return rc;
    if (nsets == 0) return LRM_OK;
    if (!legs || (nposes && !quats) || !angles || !status_out || !holdable_out || !peak_out) return fail(LRM_EINVAL, "null argument");
    std::vector<LrmPoseRecord> recs(nposes * nlegs);
    std::vector<LrmIkLeg> iks(nposes * nlegs);
    host_pose_records(quats, nullptr, nposes, legs, nlegs, recs.data()); // the body position is not read
    host_pose_ik_records(quats, nposes, legs, nlegs, iks.data());
    const ScopeMs timer{ms};
    for (size_t s = 0; s < nsets; s++) {
        const int64_t p = pose_idx ? (int64_t)pose_idx[s] : (int64_t)s;
        bool live = !(live_in && !live_in[s]) && p >= 0 && (uint64_t)p < nposes;
        LrmStancePt c{0.f, 0.f};
        if (live) c = lrm_stance_com(P.S, quats + 4 * p, &live);
        float xi[8] = {}, eta[8] = {}, g[8][3] = {};
        uint32_t feet = 0u;
        for (size_t l = 0; live && l < nlegs; l++) { // the joints and the lever arms once per (set, leg)
            const size_t o = l * nsets + s;
            LrmLoadsLeg A;
            if (!lrm_loads_leg(P, recs[p * nlegs + l].head, iks[p * nlegs + l], c, angles[3 * o],
                               angles[3 * o + 1], angles[3 * o + 2], &A))
                continue;
            xi[l] = A.xi, eta[l] = A.eta;
            for (int j = 0; j < 3; j++) g[l][j] = A.g[j];
            feet |= 1u << l;
        }
        for (size_t m = 0; m < nmasks; m++) { // every (set, lift set)
            const uint32_t S = lrm_stance_planted(feet, P.S.lift[m]);
            float load[8] = {}, load_o[8], tau_o[8][3];
            const uint8_t st = live ? lrm_loads_solve(xi, eta, S, load) : (uint8_t)LRM_LOADS_DEAD;
            const LrmLoadsPeak Q = lrm_loads_answer(P.tau_max, S, st, load, g, load_o, tau_o);
            const size_t o = m * nsets + s;
            status_out[o] = st;
            holdable_out[o] = Q.holdable;
            peak_out[o] = Q.peak;
            if (peak_at_out) peak_at_out[o] = Q.at;
            for (size_t l = 0; l < nlegs; l++) {
                if (load_out) load_out[(m * nlegs + l) * nsets + s] = load_o[l];
                for (size_t j = 0; tau_out && j < 3; j++) tau_out[((m * nlegs + l) * 3 + j) * nsets + s] = tau_o[l][j];
            }
        }
    }
    return LRM_OK;
}

// ---- pose-graph routes: cost, hops and predecessor per pose (lrm_pose_routes.hip) -----------
namespace {
// the refusals both forms share, in the documented order (rounds and resume are the device form's: the host form passes 1, 0)
int pose_routes_ranges(int direction, size_t rounds, int resume, size_t nposes, size_t nedges, size_t nsources) {
    if (direction < 0 || direction > 2) return fail(LRM_EINVAL, "pose routes: direction must be 0 (both ways), 1 (a to b) or 2 (b to a)");
    if (rounds < 1 || rounds > LRM_ROUTES_MAX_ROUNDS) return fail(LRM_EINVAL, "pose routes: rounds must be 1..4096");
    if (resume < 0 || resume > 1) return fail(LRM_EINVAL, "pose routes: resume must be 0 or 1");
    if (nposes > (size_t)INT32_MAX || nedges > (size_t)INT32_MAX || nsources > (size_t)INT32_MAX)
        return fail(LRM_EINVAL, "pose routes: nposes, nedges and nsources must not exceed INT32_MAX");
    return LRM_OK;
}
int pose_routes_pointers(const int32_t* edge_a, const int32_t* edge_b, size_t nedges, const int32_t* sources, size_t nsources,
                         const int64_t* cost_out, const int32_t* hops_out, const int32_t* pred_edge_out, const int32_t* pred_pose_out) {
    if (nedges && (!edge_a || !edge_b)) return fail(LRM_EINVAL, "null argument");
    if (nsources && !sources) return fail(LRM_EINVAL, "null argument");
    if (!cost_out && !hops_out && !pred_edge_out && !pred_pose_out) return fail(LRM_EINVAL, "pose routes: no output");
    return LRM_OK;
}
} // namespace

size_t lrm_pose_routes_workspace_bytes(size_t nposes, size_t rounds) { return lrm_routes_workspace_bytes(nposes, rounds); }

int lrm_dbg_pose_routes_plan(size_t nedges, uint64_t out[4]) {
    if (!out || nedges > (size_t)INT32_MAX) return fail(LRM_EINVAL, "pose routes plan: null output or nedges > INT32_MAX");
    lrm_routes_plan(nedges, out);
    return LRM_OK;
}

int lrm_pose_routes_dev(size_t nposes, const int32_t* edge_a, const int32_t* edge_b, size_t nedges, const uint8_t* edge_live,
                        const uint8_t* pose_live, const int32_t* edge_cost, const int32_t* sources, size_t nsources, int direction,
                        void* workspace, size_t rounds, int resume, int64_t* cost_out, int32_t* hops_out, int32_t* pred_edge_out,
                        int32_t* pred_pose_out, int32_t* reached_out, int32_t* done_out, void* stream) {
    int rc = pose_routes_ranges(direction, rounds, resume, nposes, nedges, nsources);
    if (rc != LRM_OK) return rc;
    if (nposes == 0) {
        if (reached_out || done_out) HIP_TRY(lrm_launch_pose_routes_empty(reached_out, done_out, (hipStream_t)stream), "pose routes launch");
        return LRM_OK;
    }
    if (!workspace) return fail(LRM_EINVAL, "pose routes: null workspace");
    if ((uintptr_t)workspace & 7) return fail(LRM_EINVAL, "pose routes: the workspace must be 8-byte aligned");
    rc = pose_routes_pointers(edge_a, edge_b, nedges, sources, nsources, cost_out, hops_out, pred_edge_out, pred_pose_out);
    if (rc != LRM_OK) return rc;
    const LrmRoutesArgs A{(uint32_t)nposes, (uint32_t)nedges, (uint32_t)nsources, edge_a, edge_b, edge_cost, sources, edge_live, pose_live,
                          direction, cost_out, hops_out, pred_edge_out, pred_pose_out, reached_out, done_out};
    HIP_TRY(lrm_launch_pose_routes(A, workspace, (uint32_t)rounds, resume, (hipStream_t)stream), "pose routes launch");
    return LRM_OK;
}

// The host loop: a binary-heap Dijkstra on the 64-bit keys over the arcs counting-sorted by their tail, then the predecessor
// by the definition's rule in a loop over the edges.  The fixed point is unique, so this is what the kernels converge to.
int lrm_pose_routes_cpu(size_t nposes, const int32_t* edge_a, const int32_t* edge_b, size_t nedges, const uint8_t* edge_live,
                        const uint8_t* pose_live, const int32_t* edge_cost, const int32_t* sources, size_t nsources, int direction,
                        int64_t* cost_out, int32_t* hops_out, int32_t* pred_edge_out, int32_t* pred_pose_out, int32_t* reached_out,
                        double* ms) {
    int rc = pose_routes_ranges(direction, 1, 0, nposes, nedges, nsources);
    if (rc != LRM_OK) return rc;
    if (nposes == 0) {
        if (reached_out) *reached_out = 0;
        return LRM_OK;
    }
    rc = pose_routes_pointers(edge_a, edge_b, nedges, sources, nsources, cost_out, hops_out, pred_edge_out, pred_pose_out);
    if (rc != LRM_OK) return rc;
    const ScopeMs timer{ms};
    const uint32_t np = (uint32_t)nposes;
    // the arcs of the usable edges, counting-sorted by tail: first[u] .. first[u + 1]
    struct Arc {
        int32_t head;
        uint32_t w;
    };
    std::vector<uint32_t> first(nposes + 1, 0u);
    auto each_arc = [&](auto&& f) {
        for (size_t e = 0; e < nedges; e++) {
            int32_t u, v;
            const uint32_t w = lrm_routes_edge(e, edge_a, edge_b, edge_live, pose_live, edge_cost, np, direction, &u, &v);
            if (w == LRM_ROUTES_DEAD) continue;
            f(e, u, v, w);
            if (direction == 0) f(e, v, u, w);
        }
    };
    each_arc([&](size_t, int32_t u, int32_t, uint32_t) { first[(size_t)u + 1]++; });
    for (size_t p = 0; p < nposes; p++) first[p + 1] += first[p];
    std::vector<Arc> arcs(first[nposes]);
    {
        std::vector<uint32_t> at(first.begin(), first.end() - 1);
        each_arc([&](size_t, int32_t u, int32_t v, uint32_t w) { arcs[at[u]++] = Arc{v, w}; });
    }
    std::vector<uint64_t> key(nposes, LRM_ROUTES_UNREACHED);
    typedef std::pair<uint64_t, int32_t> Item;
    std::vector<Item> heap;
    auto later = [](const Item& x, const Item& y) { return x.first > y.first; };
    for (size_t i = 0; i < nsources; i++) {
        const int32_t s = sources[i];
        if (!lrm_routes_pose(s, np, pose_live) || key[s] == 0ull) continue;
        key[s] = 0ull;
        heap.push_back(Item(0ull, s));
    }
    while (!heap.empty()) { // every key is 0 so far: any order is a heap
        std::pop_heap(heap.begin(), heap.end(), later);
        const Item top = heap.back();
        heap.pop_back();
        if (top.first != key[top.second]) continue; // a lower key was pushed since
        for (uint32_t i = first[top.second]; i < first[(size_t)top.second + 1]; i++) {
            const uint64_t c = lrm_routes_step(top.first, arcs[i].w);
            if (c < key[arcs[i].head]) {
                key[arcs[i].head] = c;
                heap.push_back(Item(c, arcs[i].head));
                std::push_heap(heap.begin(), heap.end(), later);
            }
        }
    }
    int32_t reached = 0;
    for (size_t p = 0; p < nposes; p++) {
        const bool in = key[p] != LRM_ROUTES_UNREACHED;
        reached += in ? 1 : 0;
        if (cost_out) cost_out[p] = in ? (int64_t)(key[p] >> 32) : (int64_t)-1;
        if (hops_out) hops_out[p] = in ? (int32_t)(uint32_t)key[p] : -1;
        if (pred_edge_out) pred_edge_out[p] = -1;
        if (pred_pose_out) pred_pose_out[p] = -1;
    }
    if (reached_out) *reached_out = reached;
    if (pred_edge_out || pred_pose_out) {
        std::vector<uint8_t> has(nposes, 0); // edges in ascending order: the first tight arc into a pose is the smallest edge's
        each_arc([&](size_t e, int32_t u, int32_t v, uint32_t w) {
            if (has[v] || key[v] == LRM_ROUTES_UNREACHED || lrm_routes_step(key[u], w) != key[v]) return;
            has[v] = 1;
            if (pred_edge_out) pred_edge_out[v] = (int32_t)e;
            if (pred_pose_out) pred_pose_out[v] = u;
        });
    }
    return LRM_OK;
}

// ---- pose-graph edges: neighbour poses within a step and a turn, in CSR (lrm_pose_edges.hip) -----------
namespace {
// the refusals all three forms share, in the documented order
int pose_edges_ranges(int form, size_t nposes, float max_step, float min_dot) {
    if (form < 0 || form > 1) return fail(LRM_EINVAL, "pose edges: form must be 0 (q > p) or 1 (q != p)");
    if (nposes > (size_t)INT32_MAX) return fail(LRM_EINVAL, "pose edges: nposes must not exceed INT32_MAX");
    if (!(max_step >= 0.f)) return fail(LRM_EINVAL, "pose edges: max_step must be >= 0 (mm; +inf allowed)");
    if (!(min_dot >= 0.f && min_dot <= 1.f)) return fail(LRM_EINVAL, "pose edges: min_dot must lie in [0, 1]");
    return LRM_OK;
}
int64_t pose_edges_capacity(size_t capacity) { return capacity > (size_t)INT64_MAX ? INT64_MAX : (int64_t)capacity; }
} // namespace

size_t lrm_pose_edges_workspace_bytes(size_t nposes) { return lrm_edges_workspace_bytes(nposes); }

int lrm_dbg_pose_edges_plan(size_t nposes, uint64_t out[4]) {
    if (!out || nposes > (size_t)INT32_MAX) return fail(LRM_EINVAL, "pose edges plan: null output or nposes > INT32_MAX");
    lrm_edges_plan(nposes, out);
    return LRM_OK;
}

int lrm_pose_edge_counts_dev(const float* quats, const float* body, size_t nposes, const uint8_t* pose_live, float max_step, float min_dot,
                             int form, void* workspace, int32_t* count_out, void* stream) {
    const int rc = pose_edges_ranges(form, nposes, max_step, min_dot);
    if (rc != LRM_OK) return rc;
    if (nposes == 0) return LRM_OK;
    if (!quats || !workspace || !count_out) return fail(LRM_EINVAL, "null argument");
    if ((uintptr_t)workspace & 15) return fail(LRM_EINVAL, "pose edges: the workspace must be 16-byte aligned");
    const LrmEdgesArgs A{quats, body, pose_live, (uint32_t)nposes, max_step * max_step, min_dot * min_dot, form};
    HIP_TRY(lrm_launch_pose_edge_counts(A, static_cast<float*>(workspace), count_out, (hipStream_t)stream), "pose edge counts launch");
    return LRM_OK;
}

int lrm_pose_edges_dev(const float* quats, const float* body, size_t nposes, const uint8_t* pose_live, float max_step, float min_dot, int form,
                       void* workspace, const int64_t* offsets, size_t capacity, int32_t* edge_a_out, int32_t* edge_b_out, float* d2_out,
                       float* cos2_out, int32_t* written_out, void* stream) {
    const int rc = pose_edges_ranges(form, nposes, max_step, min_dot);
    if (rc != LRM_OK) return rc;
    if (nposes == 0) return LRM_OK;
    if (!quats || !workspace || !offsets || !edge_a_out || !edge_b_out) return fail(LRM_EINVAL, "null argument");
    if ((uintptr_t)workspace & 15) return fail(LRM_EINVAL, "pose edges: the workspace must be 16-byte aligned");
    if (capacity == 0) { // no row has room: nothing but written_out
        if (written_out) HIP_TRY(hipMemsetAsync(written_out, 0, nposes * sizeof(int32_t), (hipStream_t)stream), "hipMemsetAsync written_out");
        return LRM_OK;
    }
    const LrmEdgesArgs A{quats, body, pose_live, (uint32_t)nposes, max_step * max_step, min_dot * min_dot, form};
    HIP_TRY(lrm_launch_pose_edges(A, static_cast<float*>(workspace), offsets, pose_edges_capacity(capacity), edge_a_out, edge_b_out, d2_out,
                                  cos2_out, written_out, (hipStream_t)stream), "pose edges launch");
    return LRM_OK;
}

// The host loop: every ordered pair (p, q) in ascending q, no culling; the validity and n_p of every pose are computed once,
// by the function the kernels use.
int lrm_pose_edges_cpu(const float* quats, const float* body, size_t nposes, const uint8_t* pose_live, float max_step, float min_dot, int form,
                       int32_t* count_out, const int64_t* offsets, size_t capacity, int32_t* edge_a_out, int32_t* edge_b_out, float* d2_out,
                       float* cos2_out, int32_t* written_out, double* ms) {
    const int rc = pose_edges_ranges(form, nposes, max_step, min_dot);
    if (rc != LRM_OK) return rc;
    if (nposes == 0) return LRM_OK;
    if (!quats || (!offsets && !count_out) || (offsets && (!edge_a_out || !edge_b_out))) return fail(LRM_EINVAL, "null argument");
    if (offsets && capacity == 0) {
        if (written_out) std::memset(written_out, 0, nposes * sizeof(int32_t));
        if (!count_out) {
            if (ms) *ms = 0.0;
            return LRM_OK;
        }
        offsets = nullptr; // the counts are still asked for
    }
    const float step2 = max_step * max_step, dot2 = min_dot * min_dot;
    const int64_t cap = pose_edges_capacity(capacity);
    const ScopeMs timer{ms};
    struct Pose {
        float v[8];
    };
    std::vector<Pose> poses(nposes);
    std::vector<uint8_t> valid(nposes);
    for (size_t p = 0; p < nposes; p++) valid[p] = lrm_edges_pose(quats, body, pose_live, p, poses[p].v);
    for (size_t p = 0; p < nposes; p++) {
        int64_t base = 0, room = 0, n = 0;
        if (offsets) room = lrm_edges_room(offsets, p, cap, &base);
        if (valid[p]) {
            const float* const a = poses[p].v;
            for (size_t q = form ? 0 : p + 1; q < nposes; q++) {
                if (q == p || !valid[q]) continue;
                const float* const b = poses[q].v;
                const float d2 = lrm_edges_d2(a[0], a[1], a[2], b[0], b[1], b[2]);
                if (!(d2 <= step2)) continue;
                const float c = lrm_edges_dot(a + 4, b + 4);
                if (!lrm_edges_turn(c, a[3], b[3], dot2)) continue;
                if (n < room) {
                    edge_a_out[base + n] = (int32_t)p;
                    edge_b_out[base + n] = (int32_t)q;
                    if (d2_out) d2_out[base + n] = d2;
                    if (cos2_out) cos2_out[base + n] = lrm_edges_cos2(c, a[3], b[3]);
                }
                n++;
            }
        }
        if (count_out) count_out[p] = (int32_t)n;
        if (offsets && written_out) written_out[p] = (int32_t)(n < room ? n : room);
    }
    return LRM_OK;
}

// ---- diagnostics: lrm_edge_transit.h's sampled path on arrays (host build / device build) -----------
namespace {
int edge_transit_samples_args(const float* quats, size_t nposes, const int32_t* edge_a, const int32_t* edge_b, size_t nedges,
                              size_t nsamples, const float* out) {
    if (nsamples < 2 || nsamples > LRM_TRANSIT_MAX_SAMPLES) return fail(LRM_EINVAL, "edge transit: nsamples must be 2..64");
    if (nposes > (size_t)INT32_MAX || nedges > (size_t)UINT32_MAX / LRM_TRANSIT_MAX_SAMPLES)
        return fail(LRM_EINVAL, "edge transit samples: too many poses or edges");
    if (nedges && (!quats || !edge_a || !edge_b || !out)) return fail(LRM_EINVAL, "null argument");
    return LRM_OK;
}
} // namespace
int lrm_dbg_edge_transit_samples_host(const float* quats, const float* body, size_t nposes, const int32_t* edge_a, const int32_t* edge_b,
                                      size_t nedges, size_t nsamples, float* out) {
    const int rc = edge_transit_samples_args(quats, nposes, edge_a, edge_b, nedges, nsamples, out);
    if (rc != LRM_OK) return rc;
    for (size_t e = 0; e < nedges; e++) {
        const int64_t a = edge_a[e], b = edge_b[e];
        const bool ok = a >= 0 && b >= 0 && (uint64_t)a < nposes && (uint64_t)b < nposes;
        for (uint32_t s = 0; s < (uint32_t)nsamples; s++) {
            float* o = out + (e * nsamples + s) * 7;
            if (!ok) {
                for (int k = 0; k < 7; k++) o[k] = std::nanf("");
                continue;
            }
            LrmVec3 ba{0.f, 0.f, 0.f}, bb{0.f, 0.f, 0.f};
            if (body) {
                ba = LrmVec3{body[3 * a], body[3 * a + 1], body[3 * a + 2]};
                bb = LrmVec3{body[3 * b], body[3 * b + 1], body[3 * b + 2]};
            }
            const LrmTransitSample smp = lrm_transit_sample(quats + 4 * a, quats + 4 * b, ba, bb, s, (uint32_t)nsamples);
            for (int k = 0; k < 4; k++) o[k] = smp.q[k];
            o[4] = smp.body.x;
            o[5] = smp.body.y;
            o[6] = smp.body.z;
        }
    }
    return LRM_OK;
}
int lrm_dbg_edge_transit_samples_dev(const float* quats, const float* body, size_t nposes, const int32_t* edge_a, const int32_t* edge_b,
                                     size_t nedges, size_t nsamples, float* out, void* stream) {
    const int rc = edge_transit_samples_args(quats, nposes, edge_a, edge_b, nedges, nsamples, out);
    if (rc != LRM_OK) return rc;
    if (nedges == 0) return LRM_OK;
    HIP_TRY(lrm_launch_edge_transit_samples(quats, body, nposes, edge_a, edge_b, nedges, nsamples, out, (hipStream_t)stream),
            "edge transit samples launch");
    return LRM_OK;
}

// ---- diagnostics: lrm_self_clearance.h's pair distance on arrays (host build / device build) -----------
int lrm_dbg_link_pair_dist_host(const float* segs, size_t n, float* out) {
    if (n && (!segs || !out)) return fail(LRM_EINVAL, "null argument");
    for (size_t i = 0; i < n; i++) {
        const float* g = segs + 12 * i;
        out[i] = lrm_self_pair_dist(LrmVec3{g[0], g[1], g[2]}, LrmVec3{g[3], g[4], g[5]}, LrmVec3{g[6], g[7], g[8]}, LrmVec3{g[9], g[10], g[11]});
    }
    return LRM_OK;
}
int lrm_dbg_link_pair_dist_dev(const float* segs, size_t n, float* out, void* stream) {
    if (n && (!segs || !out)) return fail(LRM_EINVAL, "null argument");
    if (n == 0) return LRM_OK;
    HIP_TRY(lrm_launch_link_pair_dist(segs, n, out, (hipStream_t)stream), "link pair distance launch");
    return LRM_OK;
}

namespace {
int any_in_shape_impl(int shape,const float* cx, const float* cy, const float* cz, size_t nc, const float* tx,
                      const float* ty, const float* tz, size_t nt, float radius, float plus_z, float minus_z,
                      bool boxes_ready, uint8_t* out, void* stream) {
    if (!out || (nc && (!cx || !cy || !cz)) || (nt && (!tx || !ty || !tz))) return fail(LRM_EINVAL, "null argument");
    if (nc == 0) return LRM_OK;
    float* boxes = nullptr;
    if (nt >= 4096) {
        const int rc = tile_boxes(nt, &boxes);
        if (rc != LRM_OK) return rc;
    }
    HIP_TRY(lrm_launch_any_in_shape(shape, cx, cy, cz, nc, tx, ty, tz, nt, radius, plus_z, minus_z, boxes, boxes_ready && boxes, out,
                                    (hipStream_t)stream), shape ? "in_cylinder launch" : "in_sphere launch");
    return LRM_OK;
}
} // namespace
int lrm_any_in_sphere_dev(const float* cx, const float* cy, const float* cz, size_t nc, const float* tx,
                          const float* ty, const float* tz, size_t nt, float radius, uint8_t* out, void* stream) {
    return any_in_shape_impl(0, cx, cy, cz, nc, tx, ty, tz, nt, radius, 0.f, 0.f, false, out, stream);
}
int lrm_any_in_cylinder_dev(const float* cx, const float* cy, const float* cz, size_t nc, const float* tx,
                            const float* ty, const float* tz, size_t nt, float radius, float plus_z, float minus_z,
                            uint8_t* out, void* stream) {
    return any_in_shape_impl(1, cx, cy, cz, nc, tx, ty, tz, nt, radius, plus_z, minus_z, false, out, stream);
}

// Morton order of a host cloud (see morton_order above): order_out[k] = index of the k-th point.
int lrm_morton_order(const float* xyz_aos, size_t n, uint64_t* order_out) {
    if (n && (!xyz_aos || !order_out)) return fail(LRM_EINVAL, "null argument");
    std::vector<size_t> idx(n);
    for (size_t i = 0; i < n; i++) idx[i] = i;
    const std::vector<size_t> o = morton_order(xyz_aos, idx);
    for (size_t i = 0; i < n; i++) order_out[i] = (uint64_t)o[i];
    return LRM_OK;
}

// ---- diagnostics: lrm_exact_math.h on arrays (host build / device build) -------------------
int lrm_dbg_exact_math_host(const float* a, const float* b, size_t n, float* at2, float* sn, float* cs) {
    if (n && (!a || !b || !at2 || !sn || !cs)) return fail(LRM_EINVAL, "null argument");
    for (size_t i = 0; i < n; i++) {
        at2[i] = lrm_atan2f(a[i], b[i]);
        lrm_sincosf(a[i], &sn[i], &cs[i]);
    }
    return LRM_OK;
}
int lrm_dbg_exact_math_dev(const float* a, const float* b, size_t n, float* at2, float* sn, float* cs,
                           void* stream) {
    if (n && (!a || !b || !at2 || !sn || !cs)) return fail(LRM_EINVAL, "null argument");
    if (n == 0) return LRM_OK;
    HIP_TRY(lrm_launch_exact_math(a, b, n, at2, sn, cs, (hipStream_t)stream), "exact_math launch");
    return LRM_OK;
}

// ---- diagnostics: block checksums of lrm_atanf / lrm_sincosf over float bit patterns (lrm_dbg_math.h) --------
namespace {
int sums_args_ok(int fn, uint32_t first_block, uint32_t nblocks, const uint64_t* sums_out) {
    if (fn < 0 || fn >= LRM_DBG_MATH_FNS) return fail(LRM_EINVAL, "fn must be 0 (atanf), 1 (sin) or 2 (cos)");
    if (first_block > LRM_DBG_MATH_BLOCKS || nblocks > LRM_DBG_MATH_BLOCKS - first_block)
        return fail(LRM_EINVAL, "first_block + nblocks exceeds the 65536 blocks of the domain");
    if (nblocks && !sums_out) return fail(LRM_EINVAL, "null argument");
    return LRM_OK;
}
void sums_host_blocks(int fn, uint32_t first_block, uint32_t nblocks, int t, int threads, uint64_t* sums_out) {
    for (uint32_t b = (uint32_t)t; b < nblocks; b += (uint32_t)threads)
        sums_out[b] = fn == 0   ? lrm_dbg_math_block_sum<0>(first_block + b)
                      : fn == 1 ? lrm_dbg_math_block_sum<1>(first_block + b)
                                : lrm_dbg_math_block_sum<2>(first_block + b);
}
} // namespace

int lrm_dbg_exact_math_sums_host(int fn, uint32_t first_block, uint32_t nblocks, uint64_t* sums_out) {
    if (int rc = sums_args_ok(fn, first_block, nblocks, sums_out)) return rc;
    // the pool is sized as the table builder's (lrm_toltab.cpp), to 16 threads at the most; blocks are independent
    int threads = (int)std::thread::hardware_concurrency();
    threads = threads < 1 ? 1 : (threads > 16 ? 16 : threads);
    if (const char* e = std::getenv("LRM_DBG_MATH_THREADS")) threads = std::min(16, std::max(1, std::atoi(e)));
    if ((uint32_t)threads > nblocks) threads = nblocks ? (int)nblocks : 1;
    auto work = [&](int t) { sums_host_blocks(fn, first_block, nblocks, t, threads, sums_out); };
    if (threads <= 1) work(0);
    else {
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; t++) pool.emplace_back(work, t);
        for (auto& th : pool) th.join();
    }
    return LRM_OK;
}
int lrm_dbg_exact_math_sums_dev(int fn, uint32_t first_block, uint32_t nblocks, uint64_t* sums_out, void* stream) {
    if (int rc = sums_args_ok(fn, first_block, nblocks, sums_out)) return rc;
    if (nblocks == 0) return LRM_OK;
    HIP_TRY(lrm_launch_exact_math_sums(fn, first_block, nblocks, sums_out, (hipStream_t)stream), "exact_math_sums launch");
    return LRM_OK;
}

int lrm_dbg_sqrt_check_dev(uint64_t* mismatches_out, uint32_t* first_bad_out) {
    if (!mismatches_out || !first_bad_out) return fail(LRM_EINVAL, "null argument");
    unsigned long long* d = nullptr;
    HIP_TRY(hipMalloc(&d, 2 * sizeof(unsigned long long)), "hipMalloc");
    const unsigned long long init[2] = {0ull, ~0ull};
    hipError_t e = hipMemcpy(d, init, sizeof(init), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = lrm_launch_sqrt_check(d, nullptr);
    unsigned long long out[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpy(out, d, sizeof(out), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIP_TRY(e, "sqrt check");
    *mismatches_out = out[0];
    *first_bad_out = out[0] ? (uint32_t)(out[1] - 1) : 0u;
    return LRM_OK;
}

int lrm_dbg_pair_sphere(const LrmLegDimensions* leg, const float* quat, float* out4) {
    if (!leg || !out4) return fail(LRM_EINVAL, "null argument");
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 0, &L);
    for (int k = 0; k < 3; k++) out4[k] = L.pair_center[k];
    out4[3] = L.pair_r2;
    return LRM_OK;
}

int lrm_dbg_fused_reach_host(const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat,
                             uint8_t* mask_out, uint8_t* doubt_out) {
    if (!leg || (n && (!xyz || !mask_out || !doubt_out))) return fail(LRM_EINVAL, "null argument");
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    if (!L.fast_ok) return fail(LRM_EINVAL, "leg not eligible for the filtered evaluation");
    const LrmDistTables T{&L.lists[0][0], &L.dist_tab[0][0], &L.corner_tab[0]};
    for (size_t i = 0; i < n; i++) {
        LrmVec3 p{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        uint32_t unc = 0;
        LrmDistByproduct by;
        lrm_dist_global_fast(L, T, p, unc, &by);
        bool doubt;
        mask_out[i] = lrm_reach_from_dist(L, by, doubt);
        doubt_out[i] = doubt;
    }
    return LRM_OK;
}

// The filtered evaluation (lrm_point_fast.h) on the host, WITHOUT the strict fallback, with its
// `uncertain` flags: tests check that every point not flagged equals the strict result and
// count how many are flagged.  Outputs may be NULL.
int lrm_dbg_fast_host(const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat,
                      uint8_t* mask_out, uint8_t* mask_unc_out, float* dxyz_out, uint8_t* valid_out,
                      uint8_t* dist_unc_out) {
    if (!leg || (n && !xyz)) return fail(LRM_EINVAL, "null argument");
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    if (!L.fast_ok) return fail(LRM_EINVAL, "leg not eligible for the filtered evaluation");
    for (size_t i = 0; i < n; i++) {
        const LrmVec3 p{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        if (mask_out) {
            uint32_t unc = 0;
            mask_out[i] = lrm_reach_global_fast(L, &L.lean[0][0], p, unc);
            if (mask_unc_out) mask_unc_out[i] = (uint8_t)unc;
        }
        if (dxyz_out) {
            uint32_t unc = 0;
            LrmVec3 d = p;
            const bool v = lrm_dist_global_fast(L, LrmDistTables{&L.lists[0][0], &L.dist_tab[0][0], &L.corner_tab[0]}, d, unc);
            dxyz_out[3 * i] = d.x;
            dxyz_out[3 * i + 1] = d.y;
            dxyz_out[3 * i + 2] = d.z;
            if (valid_out) valid_out[i] = v;
            if (dist_unc_out) dist_unc_out[i] = (uint8_t)unc;
        }
    }
    return LRM_OK;
}

// The contract-tolerance evaluation on the host, WITHOUT the re-evaluation of its doubtful points.
int lrm_dbg_tol_host(const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat, uint8_t* mask_out,
                     float* dxyz_out, uint32_t* doubt_out) {
    if (!leg || (n && (!xyz || !mask_out || !dxyz_out || !doubt_out))) return fail(LRM_EINVAL, "null argument");
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    LrmTolLeg TL;
    lrm_compile_tol(L, &TL);
    if (!TL.tol_ok) return fail(LRM_EINVAL, "leg not eligible for the tolerance mode");
    const LrmTolTables T{&TL.circ[0][0], &TL.feat[0]};
    for (size_t i = 0; i < n; i++) {
        LrmVec3 p{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        uint32_t doubt = 0;
        mask_out[i] = lrm_dist_tol(TL, T, p, doubt);
        dxyz_out[3 * i] = p.x;
        dxyz_out[3 * i + 1] = p.y;
        dxyz_out[3 * i + 2] = p.z;
        doubt_out[i] = doubt;
    }
    return LRM_OK;
}
// as lrm_dbg_tol_host with the plane table with deferred decisions (lrm_toltab.cpp) in place of the full plane evaluation;
// doubt bit 0x100 = a cell without an answer.  stats_out[4] (optional): rows, validity rows, refined cells, table bytes
int lrm_dbg_toltab_host(const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat, uint8_t* mask_out,
                        float* dxyz_out, uint32_t* doubt_out, uint32_t* stats_out) {
    if (!leg || (n && (!xyz || !mask_out || !dxyz_out || !doubt_out))) return fail(LRM_EINVAL, "null argument");
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    LrmTolLeg TL;
    lrm_compile_tol(L, &TL);
    if (!TL.tol_ok) return fail(LRM_EINVAL, "leg not eligible for the tolerance mode");
    std::vector<uint8_t> tab;
    if (!lrm_build_tol_tab(TL, &tab)) return fail(LRM_EINVAL, "leg needs more table rows than a cell code can name");
    const LrmTolTabHeader* hd = reinterpret_cast<const LrmTolTabHeader*>(tab.data());
    const LrmTolTabView G = lrm_toltab_view(tab.data(), hd->rows, hd->vrows, lrm_toltab_bound_inner(tab.data()), TL.r_outer);
    if (stats_out) {
        stats_out[0] = hd->n_rows;
        stats_out[1] = hd->n_vrows;
        stats_out[2] = hd->n_fine[0] + hd->n_fine[1];
        stats_out[3] = (uint32_t)tab.size();
    }
    lrm_tab_host_seconds = 0;
    for (size_t i = 0; i < n; i++) {
        LrmVec3 p{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        uint32_t doubt = 0;
        mask_out[i] = lrm_tab_point(TL, G, p, doubt);
        dxyz_out[3 * i] = p.x;
        dxyz_out[3 * i + 1] = p.y;
        dxyz_out[3 * i + 2] = p.z;
        doubt_out[i] = doubt;
    }
    if (stats_out) stats_out[4] = (uint32_t)std::min<unsigned long long>(lrm_tab_host_seconds, 0xffffffffull);
    return LRM_OK;
}
// The bit-exact table-guided evaluation (lrm_point_xtab.h) on the host, WITHOUT the re-evaluation of its doubtful points:
// every point with doubt 0 must equal lrm_dist_cpu / lrm_reach_cpu bit for bit.  stats_out[2] (optional): points whose second
// chain (twin or second candidate) ran, table bytes
int lrm_dbg_xtab_host(const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat, uint8_t* mask_out,
                      float* dxyz_out, uint32_t* doubt_out, uint32_t* stats_out) {
    if (!leg || (n && (!xyz || !mask_out || !dxyz_out || !doubt_out))) return fail(LRM_EINVAL, "null argument");
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    LrmTolLeg TL;
    lrm_compile_tol(L, &TL);
    if (!TL.tol_ok) return fail(LRM_EINVAL, "leg not eligible for the table-guided modes");
    std::vector<uint8_t> tab;
    if (!lrm_build_tol_tab(TL, &tab)) return fail(LRM_EINVAL, "leg needs more table rows than a cell code can name");
    const LrmTolTabHeader* hd = reinterpret_cast<const LrmTolTabHeader*>(tab.data());
    const LrmTolTabView G = lrm_toltab_view(tab.data(), hd->rows, hd->vrows, lrm_toltab_bound_inner(tab.data()), TL.r_outer);
    LrmXtabLeg X;
    lrm_make_xtab_leg(L, TL, &X);
    lrm_xtab_host_seconds = 0;
    for (size_t i = 0; i < n; i++) {
        LrmVec3 p{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        uint32_t doubt = 0;
        mask_out[i] = lrm_xtab_point(X, G, p, doubt);
        dxyz_out[3 * i] = p.x;
        dxyz_out[3 * i + 1] = p.y;
        dxyz_out[3 * i + 2] = p.z;
        doubt_out[i] = doubt;
    }
    if (stats_out) {
        stats_out[0] = (uint32_t)std::min<unsigned long long>(lrm_xtab_host_seconds, 0xffffffffull);
        stats_out[1] = (uint32_t)tab.size();
    }
    return LRM_OK;
}
// LRM_MODE_TOL_REL's two steps on the host: the tolerance evaluation with the plane table (lrm_tab_point<true>: mask, doubt bits and
// the DECISIONS it took), then the strict replay of the winner's value chain from those decisions (lrm_xtab_replay) for every point
// without doubt: dxyz_out must then equal lrm_dist_cpu bit for bit (tests/test_xtab_cpu.py).
int lrm_dbg_replay_host(const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat, uint8_t* mask_out,
                        float* dxyz_out, uint32_t* doubt_out) {
    if (!leg || (n && (!xyz || !mask_out || !dxyz_out || !doubt_out))) return fail(LRM_EINVAL, "null argument");
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    LrmTolLeg TL;
    lrm_compile_tol(L, &TL);
    if (!TL.tol_ok) return fail(LRM_EINVAL, "leg not eligible for the table-guided modes");
    std::vector<uint8_t> tab;
    if (!lrm_build_tol_tab(TL, &tab)) return fail(LRM_EINVAL, "leg needs more table rows than a cell code can name");
    const LrmTolTabHeader* hd = reinterpret_cast<const LrmTolTabHeader*>(tab.data());
    const LrmTolTabView G = lrm_toltab_view(tab.data(), hd->rows, hd->vrows, lrm_toltab_bound_inner(tab.data()), TL.r_outer);
    LrmXtabLeg X;
    lrm_make_xtab_leg(L, TL, &X);
    for (size_t i = 0; i < n; i++) {
        const LrmVec3 p_in{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        LrmVec3 p = p_in;
        uint32_t doubt = 0, info = 0;
        mask_out[i] = lrm_tab_point<true>(TL, G, p, doubt, &info);
        if ((doubt & 0xffffu) == 0u) {
            p = p_in;
            lrm_xtab_replay(X, hd->rows, p, info);
        }
        dxyz_out[3 * i] = p.x;
        dxyz_out[3 * i + 1] = p.y;
        dxyz_out[3 * i + 2] = p.z;
        doubt_out[i] = doubt;
    }
    return LRM_OK;
}
// The plane table of (leg, quat) as the host builder (device = 0) or the device builder (device = 1, on the current device) makes
// it: the table's bytes into out[cap] (when it fits), its size, the build's milliseconds.  LRM_EINVAL when the leg has no table.
int lrm_dbg_toltab_build(const LrmLegDimensions* leg, const float* quat, int device, uint8_t* out, size_t cap, size_t* size_out, float* ms_out) {
    if (!leg || !size_out) return fail(LRM_EINVAL, "null argument");
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    LrmTolLeg TL;
    lrm_compile_tol(L, &TL);
    if (!TL.tol_ok) return fail(LRM_EINVAL, "leg not eligible for the table-guided modes");
    if (!device) {
        std::vector<uint8_t> tab;
        const auto t0 = std::chrono::steady_clock::now();
        if (!lrm_build_tol_tab(TL, &tab)) return fail(LRM_EINVAL, "leg needs more table rows than a cell code can name");
        if (ms_out) *ms_out = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *size_out = tab.size();
        if (out && cap >= tab.size()) std::memcpy(out, tab.data(), tab.size());
        return LRM_OK;
    }
    uint8_t* t = nullptr;
    size_t bytes = 0;
    float ms = 0.f;
    const int rc = lrm_build_tol_tab_dev(TL, nullptr, &t, &bytes, &ms);
    if (rc < 0) return hip_fail((hipError_t)(-rc), "plane table (device build)");
    if (rc == 1) return fail(LRM_EINVAL, "leg needs more table rows than a cell code can name");
    if (rc == 2) return fail(LRM_EINVAL, "the device builder declines this leg (too many unanswered cells) or has no device memory for its scratch");
    *size_out = bytes;
    if (ms_out) *ms_out = ms;
    hipError_t e = hipSuccess;
    if (out && cap >= bytes) e = hipMemcpy(out, t, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(t);
    HIP_TRY(e, "hipMemcpy plane table");
    return LRM_OK;
}
// The table's lower bound of the in-plane distance at plane points (x = abscissa - coxa_length, z) of the INNER grid, next
// to what the full plane evaluation (lrm_tol_plane) finds there: tests/test_tol_cpu.py checks bound <= distance.
int lrm_dbg_toltab_bounds(const float* xz, size_t n, const LrmLegDimensions* leg, const float* quat, float* lb_out,
                          float* dist_out, uint8_t* valid_out, uint32_t* doubt_out) {
    if (!leg || (n && (!xz || !lb_out || !dist_out || !valid_out || !doubt_out))) return fail(LRM_EINVAL, "null argument");
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    LrmTolLeg TL;
    lrm_compile_tol(L, &TL);
    if (!TL.tol_ok) return fail(LRM_EINVAL, "leg not eligible for the tolerance mode");
    std::vector<uint8_t> tab;
    if (!lrm_build_tol_tab(TL, &tab)) return fail(LRM_EINVAL, "leg needs more table rows than a cell code can name");
    const LrmTolTabHeader* hd = reinterpret_cast<const LrmTolTabHeader*>(tab.data());
    const LrmTolTabView G = lrm_toltab_view(tab.data(), hd->rows, hd->vrows, lrm_toltab_bound_inner(tab.data()), TL.r_outer);
    const LrmTolTables T{&TL.circ[0][0], &TL.feat[0]};
    for (size_t i = 0; i < n; i++) {
        const float x = xz[2 * i], z = xz[2 * i + 1];
        const int g = (std::fabs(x) < G.far_limit && std::fabs(z) < G.far_limit) ? 0 : 1;
        uint32_t c0, c1;
        float l0, l1;
        { bool bd; uint32_t s0, s1, fb; if (g) lrm_toltab_lookup2<true>(G, true, 0.f, x, x, z, c0, c1, s0, s1, fb, l0, l1, bd); else lrm_toltab_lookup2<false>(G, false, 0.f, x, x, z, c0, c1, s0, s1, fb, l0, l1, bd); }
        lb_out[i] = l0;
        const float band = TL.band_base + TL.band_slope * (std::fabs(x) + std::fabs(z)), tau = band * LRM_TOL_TIE;
        float du, dz;
        bool valid;
        uint32_t lu = 0;
        lrm_tol_plane(TL, T, x + TL.coxa_length, z, band, tau, du, dz, valid, lu);
        dist_out[i] = std::sqrt(du * du + dz * dz);
        valid_out[i] = valid;
        doubt_out[i] = lu;
    }
    return LRM_OK;
}
// Counting build only (-DLRM_PAIR_COUNT, tools/c3_evidence.py): what reach_any_wave_kernel evaluated since the last call:
// out[0] full (leg, target) evaluations, [1] leg bounding-sphere tests, [2] footholds inside a body's reach sphere, [3] footholds loaded
int lrm_dbg_pair_counts(uint64_t out[4]) {
    if (!out) return fail(LRM_EINVAL, "null argument");
    unsigned long long c[4] = {0, 0, 0, 0};
    const hipError_t e = lrm_pair_counts(c);
    if (e == hipErrorNotSupported) return fail(LRM_EINVAL, "this library was built without -DLRM_PAIR_COUNT");
    HIP_TRY(e, "pair counters");
    for (int i = 0; i < 4; i++) out[i] = c[i];
    return LRM_OK;
}
// After a distance / fused call on device buffers in LRM_MODE_TOL (synchronises that device): how many of its points the
// main kernel queued for the bit-exact fix-up, and how many workgroups overflowed their queue segment (their points are
// all re-evaluated).  Valid until the next tolerance-mode call on a larger cloud regrows the workspace.
int lrm_dbg_tol_queue_counts(uint64_t* n_points, uint64_t* n_queued, uint64_t* n_overflowed) {
    if (!n_points || !n_queued || !n_overflowed) return fail(LRM_EINVAL, "null argument");
    std::lock_guard<std::recursive_mutex> g(g_cache_mu);
    if (!g_tol_last.counts) return fail(LRM_EINVAL, "no tolerance-mode call on device buffers yet");
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur), "hipGetDevice");
    HIP_TRY(hipSetDevice(g_tol_last.dev), "hipSetDevice");
    std::vector<uint32_t> c(g_tol_last.blocks);
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(c.data(), g_tol_last.counts, c.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipSetDevice(cur);
    HIP_TRY(e, "hipMemcpy counts");
    uint64_t q = 0, o = 0;
    for (uint32_t v : c) {
        q += v;
        o += v > g_tol_last.cap;
    }
    *n_points = g_tol_last.n;
    *n_queued = q;
    *n_overflowed = o;
    return LRM_OK;
}
// The grids and queue words of the tolerance-mode and table-guided launches for n points, from the functions the launches use
int lrm_dbg_tol_grid(size_t n, uint64_t out[6]) {
    if (!out) return fail(LRM_EINVAL, "null argument");
    size_t b[3];
    lrm_tol_grid(n, b);
    out[0] = b[0];
    out[1] = b[1];
    out[2] = b[2];
    out[3] = lrm_tol_tab_queue_words(n);
    out[4] = lrm_tol_queue_words(n);
    out[5] = tol_prepare_words(n);
    return LRM_OK;
}
int lrm_dbg_tol_ok(const LrmLegDimensions* leg, const float* quat) {
    if (!leg) return 0;
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    LrmTolLeg TL;
    lrm_compile_tol(L, &TL);
    return TL.tol_ok;
}

namespace {
// The orientation loop of robot_full_struct (several_leg.cu:831-857 -> runPipeline :762-787) on device-resident clouds:
// per orientation rotate both clouds, (optionally) the cylinder culls of eliminateFarAndColliding (:504-525), every
// leg's any-target reachability, and the monotone acceptance (an `active` byte per body).  Everything on the null
// stream; only launches (the per-orientation leg data is a few hundred bytes of kernel arguments).
// b*/t*: the unrotated clouds (SoA), rb*/rt*: scratch for the rotated ones, rot_dev: nquat LrmCompiledLeg slots,
// m1/m2: max(nb, nt) bytes, leg_body: nlegs * nb, all: nb, active (in/out) and accepted (in/out): nb bytes.
int sweep_orientations_dev(const float* bx, const float* by, const float* bz, size_t nb, const float* tx, const float* ty, const float* tz, size_t mt,
                           const LrmLegDimensions* legs, size_t nlegs, const float* quats, size_t nquat, int culls,
                           float* rbx, float* rby, float* rbz, float* rtx, float* rty, float* rtz, LrmCompiledLeg* rot_dev,
                           uint8_t* m1, uint8_t* m2, uint8_t* leg_body, uint8_t* all, uint8_t* active, uint8_t* accepted) {
    {   // every orientation's qtRotate coefficients in one upload: the loop below only launches
        std::vector<LrmCompiledLeg> rots(nquat);
        LrmLegDimensions dummy{};
        for (size_t qi = 0; qi < nquat; qi++) lrm_compile_leg(dummy, quats + 4 * qi, 0, &rots[qi]); // only fwd_rot is used
        if (nquat) HIP_TRY(hipMemcpy(rot_dev, rots.data(), sizeof(LrmCompiledLeg) * nquat, hipMemcpyHostToDevice), "hipMemcpy rotations");
    }
    for (size_t qi = 0; qi < nquat; qi++) {
        const float* q = quats + 4 * qi;
        LrmLegDimensions rl[LRM_MAX_LEGS];
        for (size_t l = 0; l < nlegs; l++) lrm_host_rotate_leg_data(q, legs[l], &rl[l]);
        HIP_TRY(lrm_launch_rotate_soa(bx, by, bz, nb, rot_dev + qi, rbx, rby, rbz, nullptr), "rotate bodies");
        if (mt) HIP_TRY(lrm_launch_rotate_soa(tx, ty, tz, mt, rot_dev + qi, rtx, rty, rtz, nullptr), "rotate targets");
        bool boxes_ready = false; // the kernels of one orientation share the rotated cloud's boxes: only the first builds them
        int rc = LRM_OK;
        if (culls) {
            // eliminateFarAndColliding, several_leg.cu:504-525, with the rotated leg 0
            const LrmLegDimensions& d = rl[0];
            const float s_pitch = sinf(d.coxa_pitch), c_pitch = cosf(d.coxa_pitch);
            const float radius_in = d.body + c_pitch * d.coxa_length + d.femur_length + d.tibia_length;
            const float half_pi = 3.14159265358979323846264338327950288419716939937510582097f / 2;
            const float plus_abs = d.tibia_length * sinf(d.tibia_absolute_pos) +
                                   d.femur_length * sinf(half_pi < d.max_angle_femur ? half_pi : d.max_angle_femur);
            const float plus_z_in = s_pitch * d.coxa_length + plus_abs;
            const float minus_z_in = s_pitch * d.coxa_length - d.femur_length - d.tibia_length;
            rc = any_in_shape_impl(1, rbx, rby, rbz, nb, rtx, rty, rtz, mt, radius_in, plus_z_in, minus_z_in, boxes_ready, m1, nullptr);
            boxes_ready = mt >= 4096;
            if (rc == LRM_OK) rc = any_in_shape_impl(1, rbx, rby, rbz, nb, rtx, rty, rtz, mt, d.body, 250.f, -110.f, boxes_ready, m2, nullptr);
            if (rc != LRM_OK) return rc;
        }
        rc = reach_any_impl(rbx, rby, rbz, nb, rtx, rty, rtz, mt, rl, nlegs, q, active, boxes_ready, leg_body, all, nullptr);
        if (rc != LRM_OK) return rc;
        HIP_TRY(lrm_launch_sweep_update(all, m1, m2, culls ? 1 : 0, nb, active, accepted, nullptr), "sweep update");
    }
    return LRM_OK;
}
} // namespace

// robot_full_struct's pipeline (several_leg.cu:326-877) with masks instead of thrust stream
// compaction, resident on the device from the first upload to the final mask.
// reference_culls != 0 adds the estimator's culls:
//   once      eliminateAlwaysColliding (sphere r = 60, :413-440), eliminateFarBody (r = 400, :442-474),
//             eliminateFarTarget (r = 400 around the surviving bodies, :476-502)
//   per quat  eliminateFarAndColliding (:504-559): keep a body iff some target lies in the big
//             cylinder of (rotated) leg 0 and none in the body cylinder (r = body, z in (-110, 250))
// For each orientation bodies and targets are rotated by the quaternion (rotateData :401-411: a
// kernel with the strict qtRotate arithmetic), the legs' limits are rotated (rotateLegsLimits
// :743-760, host), every leg must find a reachable target (eliminateUnreachable :707-741,
// generalised from 4 to nlegs legs), and a body accepted by one orientation is not tested again
// (flipWorkingSide :396-399: an `active` byte per body instead of partitioning).
int lrm_positionability(const float* bodies, size_t nb, const float* targets, size_t nt,
                        const LrmLegDimensions* legs, size_t nlegs, const float* quats, size_t nquat,
                        int reference_culls, uint8_t* body_mask_out, float* ms) {
    if (!legs || nlegs == 0 || nlegs > LRM_MAX_LEGS) return fail(LRM_EINVAL, "nlegs must be 1..LRM_MAX_LEGS");
    if ((nb && (!bodies || !body_mask_out)) || (nt && !targets) || (nquat && !quats))
        return fail(LRM_EINVAL, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(LRM_ENODEV, "no HIP device");
    if (nb == 0) return LRM_OK;
    Events ev;
    HIP_TRY(hipEventCreate(&ev.a), "hipEventCreate");
    HIP_TRY(hipEventCreate(&ev.b), "hipEventCreate");
    const size_t pb = (nb + 3) & ~(size_t)3, pt = ((nt ? nt : 1) + 3) & ~(size_t)3; // keep component arrays aligned
    DevBuf d_b0, d_t0, d_b, d_t, d_m1, d_m2, d_leg_body, d_all, d_active, d_accepted, d_rot;
    HIP_TRY(d_b0.alloc(3 * pb * sizeof(float)), "hipMalloc bodies");
    HIP_TRY(d_b.alloc(3 * pb * sizeof(float)), "hipMalloc bodies");
    HIP_TRY(d_t0.alloc(3 * pt * sizeof(float)), "hipMalloc targets");
    HIP_TRY(d_t.alloc(3 * pt * sizeof(float)), "hipMalloc targets");
    HIP_TRY(d_m1.alloc(nb > nt ? nb : nt), "hipMalloc mask");
    HIP_TRY(d_m2.alloc(nb > nt ? nb : nt), "hipMalloc mask");
    HIP_TRY(d_leg_body.alloc(nlegs * nb), "hipMalloc leg results");
    HIP_TRY(d_all.alloc(nb), "hipMalloc body results");
    HIP_TRY(d_active.alloc(nb), "hipMalloc active");
    HIP_TRY(d_accepted.alloc(nb), "hipMalloc accepted");
    HIP_TRY(d_rot.alloc(sizeof(LrmCompiledLeg) * (nquat ? nquat : 1)), "hipMalloc rotations");

    // AoS host -> SoA device (component stride `pad`)
    std::vector<float> stage;
    auto upload = [&](const float* aos, const size_t* idx, size_t m, size_t pad, void* dst) -> hipError_t {
        stage.assign(3 * pad, 0.f);
        for (size_t k = 0; k < m; k++) {
            const size_t i = idx ? idx[k] : k;
            stage[k] = aos[3 * i];
            stage[pad + k] = aos[3 * i + 1];
            stage[2 * pad + k] = aos[3 * i + 2];
        }
        return hipMemcpy(dst, stage.data(), 3 * pad * sizeof(float), hipMemcpyHostToDevice);
    };
    // both clouds go to the device in Morton order (body_order maps device slot -> caller index)
    std::vector<size_t> ident_b(nb), ident_t(nt);
    for (size_t i = 0; i < nb; i++) ident_b[i] = i;
    for (size_t i = 0; i < nt; i++) ident_t[i] = i;
    const std::vector<size_t> body_order = morton_order(bodies, ident_b);
    const std::vector<size_t> target_order = morton_order(targets, ident_t);
    HIP_TRY(upload(bodies, body_order.data(), nb, pb, d_b0.p), "hipMemcpy bodies");
    size_t mt = nt; // targets kept after the one-time cull
    if (nt) HIP_TRY(upload(targets, target_order.data(), nt, pt, d_t0.p), "hipMemcpy targets");
    float* B0 = d_b0.as<float>();
    float* T0 = d_t0.as<float>();
    float* B = d_b.as<float>();
    float* T = d_t.as<float>();
    std::vector<uint8_t> active(nb, 1), h1(nb > nt ? nb : nt), h2(nb);
    float total_ms = 0.f;
    HIP_TRY(hipMemset(d_accepted.p, 0, nb), "hipMemset accepted");

    if (reference_culls == 1 && nt) { // 2: the caller has applied the one-time culls (sharded drivers)
        HIP_TRY(hipEventRecord(ev.a, nullptr), "hipEventRecord");
        int rc = lrm_any_in_sphere_dev(B0, B0 + pb, B0 + 2 * pb, nb, T0, T0 + pt, T0 + 2 * pt, nt, 60.f, d_m1.as<uint8_t>(), nullptr);
        if (rc == LRM_OK) rc = lrm_any_in_sphere_dev(B0, B0 + pb, B0 + 2 * pb, nb, T0, T0 + pt, T0 + 2 * pt, nt, 400.f, d_m2.as<uint8_t>(), nullptr);
        if (rc != LRM_OK) return rc;
        HIP_TRY(hipEventRecord(ev.b, nullptr), "hipEventRecord");
        HIP_TRY(hipMemcpy(h1.data(), d_m1.p, nb, hipMemcpyDeviceToHost), "hipMemcpy mask");
        HIP_TRY(hipMemcpy(h2.data(), d_m2.p, nb, hipMemcpyDeviceToHost), "hipMemcpy mask");
        float e = 0.f;
        HIP_TRY(hipEventElapsedTime(&e, ev.a, ev.b), "hipEventElapsedTime");
        total_ms += e;
        std::vector<size_t> alive; // caller indices, in device (Morton) order
        for (size_t i = 0; i < nb; i++) {
            active[i] = (h1[i] == 0 && h2[i] != 0) ? 1 : 0;
            if (active[i]) alive.push_back(body_order[i]);
        }
        // eliminateFarTarget: keep the targets with a surviving body within 400 (compacted once, on the host)
        mt = 0;
        if (!alive.empty()) {
            const size_t na = alive.size(), pa = (na + 3) & ~(size_t)3;
            HIP_TRY(upload(bodies, alive.data(), na, pa, d_b.p), "hipMemcpy bodies");
            HIP_TRY(hipEventRecord(ev.a, nullptr), "hipEventRecord");
            rc = lrm_any_in_sphere_dev(T0, T0 + pt, T0 + 2 * pt, nt, B, B + pa, B + 2 * pa, na, 400.f, d_m1.as<uint8_t>(), nullptr);
            if (rc != LRM_OK) return rc;
            HIP_TRY(hipEventRecord(ev.b, nullptr), "hipEventRecord");
            HIP_TRY(hipMemcpy(h1.data(), d_m1.p, nt, hipMemcpyDeviceToHost), "hipMemcpy mask");
            HIP_TRY(hipEventElapsedTime(&e, ev.a, ev.b), "hipEventElapsedTime");
            total_ms += e;
            std::vector<size_t> kept; // caller indices, still in Morton order
            for (size_t i = 0; i < nt; i++)
                if (h1[i]) kept.push_back(target_order[i]);
            mt = kept.size();
            if (mt) HIP_TRY(upload(targets, kept.data(), mt, pt, d_t0.p), "hipMemcpy targets");
        }
    }
    HIP_TRY(hipMemcpy(d_active.p, active.data(), nb, hipMemcpyHostToDevice), "hipMemcpy active");

    HIP_TRY(hipEventRecord(ev.a, nullptr), "hipEventRecord");
    {
        const int rc = sweep_orientations_dev(B0, B0 + pb, B0 + 2 * pb, nb, T0, T0 + pt, T0 + 2 * pt, mt, legs, nlegs, quats, nquat, reference_culls ? 1 : 0,
                                              B, B + pb, B + 2 * pb, T, T + pt, T + 2 * pt, d_rot.as<LrmCompiledLeg>(), d_m1.as<uint8_t>(), d_m2.as<uint8_t>(),
                                              d_leg_body.as<uint8_t>(), d_all.as<uint8_t>(), d_active.as<uint8_t>(), d_accepted.as<uint8_t>());
        if (rc != LRM_OK) return rc;
    }
    HIP_TRY(hipEventRecord(ev.b, nullptr), "hipEventRecord");
    HIP_TRY(hipMemcpy(h2.data(), d_accepted.p, nb, hipMemcpyDeviceToHost), "hipMemcpy result");
    for (size_t i = 0; i < nb; i++) body_mask_out[body_order[i]] = h2[i];
    float e = 0.f;
    HIP_TRY(hipEventElapsedTime(&e, ev.a, ev.b), "hipEventElapsedTime");
    total_ms += e;
    if (ms) *ms = total_ms;
    return LRM_OK;
}

// lrm_positionability on clouds that already live on the device (SoA float32) with device-resident masks in and out: the
// orientation sweep alone (reference_culls 0: none; 2: the per-orientation cylinder culls -- the caller has applied the
// one-time culls of multi_rot_estimator, several_leg.cu:413-502, as the sharded drivers do).  active_in: NULL = every
// body.  No copies of the clouds, no reordering (feed Morton-ordered clouds: lrm_morton_order); returns after the device
// has finished (null stream).
int lrm_positionability_dev(const float* bx, const float* by, const float* bz, size_t nb, const float* tx, const float* ty,
                            const float* tz, size_t nt, const LrmLegDimensions* legs, size_t nlegs, const float* quats,
                            size_t nquat, int reference_culls, const uint8_t* active_in, uint8_t* accepted_out, float* ms) {
    if (!legs || nlegs == 0 || nlegs > LRM_MAX_LEGS) return fail(LRM_EINVAL, "nlegs must be 1..LRM_MAX_LEGS");
    if ((nb && (!bx || !by || !bz || !accepted_out)) || (nt && (!tx || !ty || !tz)) || (nquat && !quats)) return fail(LRM_EINVAL, "null argument");
    if (reference_culls != 0 && reference_culls != 2) return fail(LRM_EINVAL, "reference_culls must be 0 or 2 here (the one-time culls are the caller's)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(LRM_ENODEV, "no HIP device");
    if (ms) *ms = 0.f;
    if (nb == 0) return LRM_OK;
    Events ev;
    HIP_TRY(hipEventCreate(&ev.a), "hipEventCreate");
    HIP_TRY(hipEventCreate(&ev.b), "hipEventCreate");
    const size_t pb = (nb + 3) & ~(size_t)3, pt = ((nt ? nt : 1) + 3) & ~(size_t)3;
    DevBuf d_b, d_t, d_m1, d_m2, d_leg_body, d_all, d_active, d_rot;
    HIP_TRY(d_b.alloc(3 * pb * sizeof(float)), "hipMalloc bodies");
    HIP_TRY(d_t.alloc(3 * pt * sizeof(float)), "hipMalloc targets");
    HIP_TRY(d_m1.alloc(nb > nt ? nb : nt), "hipMalloc mask");
    HIP_TRY(d_m2.alloc(nb > nt ? nb : nt), "hipMalloc mask");
    HIP_TRY(d_leg_body.alloc(nlegs * nb), "hipMalloc leg results");
    HIP_TRY(d_all.alloc(nb), "hipMalloc body results");
    HIP_TRY(d_active.alloc(nb), "hipMalloc active");
    HIP_TRY(d_rot.alloc(sizeof(LrmCompiledLeg) * (nquat ? nquat : 1)), "hipMalloc rotations");
    if (active_in) HIP_TRY(hipMemcpy(d_active.p, active_in, nb, hipMemcpyDeviceToDevice), "hipMemcpy active");
    else HIP_TRY(hipMemset(d_active.p, 1, nb), "hipMemset active");
    HIP_TRY(hipMemset(accepted_out, 0, nb), "hipMemset accepted");
    float* B = d_b.as<float>();
    float* T = d_t.as<float>();
    HIP_TRY(hipEventRecord(ev.a, nullptr), "hipEventRecord");
    const int rc = sweep_orientations_dev(bx, by, bz, nb, tx, ty, tz, nt, legs, nlegs, quats, nquat, reference_culls ? 1 : 0, B, B + pb, B + 2 * pb,
                                          T, T + pt, T + 2 * pt, d_rot.as<LrmCompiledLeg>(), d_m1.as<uint8_t>(), d_m2.as<uint8_t>(),
                                          d_leg_body.as<uint8_t>(), d_all.as<uint8_t>(), d_active.as<uint8_t>(), accepted_out);
    if (rc != LRM_OK) return rc;
    HIP_TRY(hipEventRecord(ev.b, nullptr), "hipEventRecord");
    HIP_TRY(hipEventSynchronize(ev.b), "hipEventSynchronize");
    float e = 0.f;
    HIP_TRY(hipEventElapsedTime(&e, ev.a, ev.b), "hipEventElapsedTime");
    if (ms) *ms = e;
    return LRM_OK;
}

} // extern "C"

// =====================================================================================================================
// Several GPUs behind the apply_kernel boundary (SURVEY.md section 8(b) "lrm_*_multi", 8(e)): ONE process, ONE host
// thread, ndev devices.  The reference has no such entry (several_leg.cu:800 uses device 0).  The cloud is cut into the
// 64-point-aligned contiguous shards of lrm_shard_bounds -- the same arithmetic as lrm_amd/shard.py, so that a
// torch.distributed run and this call own identical slices -- each device gets one stream, its slice of the input,
// the fused kernels of the current mode, and packs its reach bytes into ballot words; the words are then all-gathered
// over xGMI with RCCL's C API (ncclCommInitAll once per device set, one grouped ncclAllGather per call), so that every
// device ends up with the bit-packed reach mask of the WHOLE cloud (the exchange step of BASELINE config 4), and the
// per-shard bytes / vectors go back to the caller's arrays.  librccl.so is opened on first use with more than one
// device (or when LRM_MULTI_FORCE_RCCL=1 asks for it with one): liblrm.so itself keeps depending on HIP alone.
// =====================================================================================================================
#include <dlfcn.h>

namespace {

__global__ void pack_mask_bits_kernel(const uint8_t* __restrict__ mask, size_t n, uint64_t* __restrict__ words, size_t nwords) {
    // one wave per word: lane i reads byte 64 w + i; words beyond ceil(n / 64) (the shard's padding) become 0
    const size_t w = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (w >= nwords) return;
    const size_t i = w * 64 + (threadIdx.x & 63);
    const uint64_t b = __ballot(i < n && mask[i] != 0);
    if ((threadIdx.x & 63) == 0) words[w] = b;
}

struct Rccl {
    void* handle = nullptr;
    int (*CommInitAll)(void**, int, const int*) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool load(std::string* why) {
        if (handle) return true;
        const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
        for (const char* nm : names)
            if ((handle = dlopen(nm, RTLD_NOW | RTLD_GLOBAL))) break;
        if (!handle) { *why = std::string("dlopen librccl.so: ") + dlerror(); return false; }
        CommInitAll = (decltype(CommInitAll))dlsym(handle, "ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))dlsym(handle, "ncclCommDestroy");
        AllGather = (decltype(AllGather))dlsym(handle, "ncclAllGather");
        GroupStart = (decltype(GroupStart))dlsym(handle, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))dlsym(handle, "ncclGroupEnd");
        GetErrorString = (decltype(GetErrorString))dlsym(handle, "ncclGetErrorString");
        if (!CommInitAll || !CommDestroy || !AllGather || !GroupStart || !GroupEnd || !GetErrorString) {
            *why = "librccl.so lacks an expected symbol";
            dlclose(handle);
            handle = nullptr;
            return false;
        }
        return true;
    }
} g_rccl;
constexpr int kNcclUint64 = 5; // ncclUint64, rccl.h

// communicators of the last device set (ncclCommInitAll costs ~0.1-1 s: kept across calls)
struct MultiComms {
    std::vector<int> devs;
    std::vector<void*> comms;
} g_multi;
void multi_release() {
    if (g_rccl.handle)
        for (void* c : g_multi.comms)
            if (c) (void)g_rccl.CommDestroy(c);
    g_multi.comms.clear();
    g_multi.devs.clear();
}

struct MultiDev {
    int dev = 0;
    size_t lo = 0, hi = 0;
    hipStream_t st = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    void *in = nullptr, *mask = nullptr, *out = nullptr, *words = nullptr, *gathered = nullptr;
};
struct MultiState { // releases everything on every exit path
    std::vector<MultiDev> d;
    int home = 0;
    ~MultiState() {
        for (auto& m : d) {
            if (hipSetDevice(m.dev) != hipSuccess) continue;
            if (m.st) (void)hipStreamSynchronize(m.st);
            if (m.st) tol_workspace_drop(m.dev, (void*)m.st); // the queue workspace keyed by this call's stream goes with the stream
            for (void* p : {m.in, m.mask, m.out, m.words, m.gathered})
                if (p) (void)hipFree(p);
            if (m.a) (void)hipEventDestroy(m.a);
            if (m.b) (void)hipEventDestroy(m.b);
            if (m.st) (void)hipStreamDestroy(m.st);
        }
        (void)hipSetDevice(home);
    }
};

} // namespace

extern "C" {

// LRM_MODE_TOL ahead of time: tables compiled and uploaded, queues of (current device, stream) sized for n_max points
int lrm_tol_prepare(const LrmLegDimensions* leg, const float* quat, size_t n_max, void* stream) {
    if (!leg) return fail(LRM_EINVAL, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(LRM_ENODEV, "no HIP device");
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    if (!L.fast_ok) return LRM_OK; // this leg runs the strict kernels in every mode: nothing to prepare
    std::lock_guard<std::recursive_mutex> g(g_cache_mu);
    TolEntry& E = tol_entry(*leg, quat_or_default(quat), L);
    if (!E.tl.tol_ok) return LRM_OK; // falls back to LRM_MODE_FAST
    const uint8_t* tab = nullptr;
    if (tol_tab_wanted(n_max)) {
        const int rc = tol_tab_device(E, stream, &tab);
        if (rc != LRM_OK) return rc;
    }
    uint32_t* w = nullptr;
    return tol_workspace(tol_prepare_words(n_max), stream, &w);
}

// milliseconds the most recent plane-table build of this process took (host wall clock around the builder; -1: none yet)
int lrm_tol_table_build_ms(float* ms_out) {
    if (!ms_out) return fail(LRM_EINVAL, "null argument");
    std::lock_guard<std::recursive_mutex> g(g_cache_mu);
    *ms_out = g_last_tab_build_ms;
    return LRM_OK;
}

void lrm_release_workspaces(void) {
    std::lock_guard<std::recursive_mutex> g(g_cache_mu);
    int cur = 0;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    for (auto& w : g_tol_ws) {
        if (!w.second.p) continue;
        (void)hipSetDevice(w.first.first);
        (void)hipFree(w.second.p);
    }
    g_tol_ws.clear();
    g_tol_last = TolLast{};
    for (auto& e : g_tol_cache)
        for (auto& d : e.second.tab_dev) {
            (void)hipSetDevice(d.first);
            (void)hipFree(d.second);
        }
    g_tol_cache.clear();
    for (auto& hp : g_host_pipe) {
        (void)hipSetDevice(hp.first);
        host_pipe_free(hp.second);
    }
    g_host_pipe.clear();
    lrm_toltab_dev_release();
    lrm_octree_release();
    for (auto& pp : g_pools) { // the pair kernels' boxes and leg slots: each slot's event first, then the buffers
        DevicePool& P = pp.second;
        (void)hipSetDevice(pp.first);
        for (hipEvent_t& ev : P.slot_done) {
            if (!ev) continue;
            (void)hipEventSynchronize(ev);
            (void)hipEventDestroy(ev);
        }
        if (P.boxes) (void)hipFree(P.boxes);
        if (P.legs) (void)hipFree(P.legs);
    }
    g_pools.clear();
    multi_release();
    if (have) (void)hipSetDevice(cur);
}

// shard r of n items over `world` owners: [lo, hi), boundaries multiples of `align` (64: no ballot word straddles two
// owners); ceil(n / world) rounded up to `align` per owner, the last ones may be short or empty.  = shard.shard_bounds
int lrm_shard_bounds(size_t n, int world, int rank, size_t align, size_t* lo_out, size_t* hi_out) {
    if (world < 1 || rank < 0 || rank >= world || align == 0 || !lo_out || !hi_out) return fail(LRM_EINVAL, "bad shard arguments");
    size_t per = (n + (size_t)world - 1) / (size_t)world;
    per = (per + align - 1) / align * align;
    const size_t lo = std::min(n, (size_t)rank * per);
    *lo_out = lo;
    *hi_out = std::min(n, lo + per);
    return LRM_OK;
}

void lrm_multi_release(void) { multi_release(); }

// apply_kernel (cross_compiled.cu:33-79) for the fused kernel over `ndev` devices.  devices: ordinals, or NULL = 0 .. ndev-1.
// mask_out[n], dxyz_out[3n]: as lrm_reach_dist.  bits_out: NULL, or ceil(n / 64) words = the gathered bit-packed mask as
// device devices[0] holds it after the exchange.  ms_per_dev: NULL or [ndev], each device's kernel milliseconds (HIP events
// on its stream around its launches; 0 for an empty shard).
int lrm_reach_dist_multi(const float* xyz, size_t n, const LrmLegDimensions* leg, const float* quat, int ndev, const int* devices,
                         uint8_t* mask_out, float* dxyz_out, uint64_t* bits_out, float* ms_per_dev) {
    if (!leg || (n && (!xyz || !mask_out || !dxyz_out))) return fail(LRM_EINVAL, "null argument");
    if (ndev < 1 || ndev > 64) return fail(LRM_EINVAL, "ndev must be 1 .. 64");
    int have = 0;
    if (hipGetDeviceCount(&have) != hipSuccess || have == 0) return fail(LRM_ENODEV, "no HIP device");
    std::vector<int> devs(ndev);
    for (int d = 0; d < ndev; d++) {
        devs[d] = devices ? devices[d] : d;
        if (devs[d] < 0 || devs[d] >= have) return fail(LRM_EINVAL, "device ordinal out of range");
        for (int e = 0; e < d; e++)
            if (devs[e] == devs[d]) return fail(LRM_EINVAL, "a device is listed twice");
    }
    const char* force = std::getenv("LRM_MULTI_FORCE_RCCL");
    const bool use_rccl = ndev > 1 || (force && force[0] == '1');
    if (use_rccl) {
        std::string why;
        if (!g_rccl.load(&why)) return fail(LRM_ENODEV, why.c_str());
        if (g_multi.devs != devs) {
            multi_release();
            g_multi.comms.assign(ndev, nullptr);
            const int rc = g_rccl.CommInitAll(g_multi.comms.data(), ndev, devs.data());
            if (rc != 0) {
                g_multi.comms.clear();
                return fail(LRM_ENODEV, (std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(rc)).c_str());
            }
            g_multi.devs = devs;
        }
    }
    LrmCompiledLeg L;
    lrm_compile_leg(*leg, quat_or_default(quat), 1, &L);
    MultiState S;
    (void)hipGetDevice(&S.home);
    S.d.resize(ndev);
    size_t lo0 = 0, per = 0;
    lrm_shard_bounds(n, ndev, 0, 64, &lo0, &per); // shard 0 has the common size (or n, when n is smaller)
    size_t common = (n + (size_t)ndev - 1) / (size_t)ndev;
    common = (common + 63) / 64 * 64;
    const size_t per_words = std::max<size_t>(common / 64, 1);
    // 1. per device: stream, buffers, input slice on its way, kernels, bit words
    for (int d = 0; d < ndev; d++) {
        MultiDev& m = S.d[d];
        m.dev = devs[d];
        lrm_shard_bounds(n, ndev, d, 64, &m.lo, &m.hi);
        const size_t cnt = m.hi - m.lo;
        HIP_TRY(hipSetDevice(m.dev), "hipSetDevice");
        HIP_TRY(hipStreamCreateWithFlags(&m.st, hipStreamNonBlocking), "hipStreamCreate");
        HIP_TRY(hipEventCreate(&m.a), "hipEventCreate");
        HIP_TRY(hipEventCreate(&m.b), "hipEventCreate");
        HIP_TRY(hipMalloc(&m.in, std::max<size_t>(cnt, 1) * 3 * sizeof(float)), "hipMalloc shard input");
        HIP_TRY(hipMalloc(&m.mask, std::max<size_t>(cnt, 1)), "hipMalloc shard mask");
        HIP_TRY(hipMalloc(&m.out, std::max<size_t>(cnt, 1) * 3 * sizeof(float)), "hipMalloc shard output");
        HIP_TRY(hipMalloc(&m.words, per_words * sizeof(uint64_t)), "hipMalloc shard words");
        HIP_TRY(hipMalloc(&m.gathered, per_words * (size_t)ndev * sizeof(uint64_t)), "hipMalloc gathered words");
        if (cnt) HIP_TRY(hipMemcpyAsync(m.in, xyz + 3 * m.lo, cnt * 3 * sizeof(float), hipMemcpyHostToDevice, m.st), "hipMemcpyAsync shard input");
        HIP_TRY(hipEventRecord(m.a, m.st), "hipEventRecord");
        if (cnt) {
            const int rc = launch_dist_aos_mode(2, static_cast<const float*>(m.in), cnt, *leg, quat_or_default(quat), L,
                                                static_cast<uint8_t*>(m.mask), static_cast<float*>(m.out), m.st);
            if (rc != LRM_OK) return rc;
        }
        HIP_TRY(hipEventRecord(m.b, m.st), "hipEventRecord");
        const unsigned pblocks = (unsigned)((per_words * 64 + 255) / 256);
        hipLaunchKernelGGL(pack_mask_bits_kernel, dim3(pblocks), dim3(256), 0, m.st, static_cast<const uint8_t*>(m.mask), cnt,
                           static_cast<uint64_t*>(m.words), per_words);
        HIP_TRY(hipGetLastError(), "pack_mask_bits_kernel");
    }
    // 2. the exchange: every device receives every shard's words (grouped: one collective over all communicators)
    if (use_rccl) {
        int rc = g_rccl.GroupStart();
        hipError_t he = hipSuccess;
        for (int d = 0; d < ndev && rc == 0 && he == hipSuccess; d++) {
            MultiDev& m = S.d[d];
            he = hipSetDevice(m.dev);
            if (he == hipSuccess) rc = g_rccl.AllGather(m.words, m.gathered, per_words, kNcclUint64, g_multi.comms[d], m.st);
        }
        const int rc2 = g_rccl.GroupEnd(); // on every path: a group left open would hang the process's next RCCL call
        HIP_TRY(he, "hipSetDevice");
        if (rc != 0 || rc2 != 0) return fail(LRM_ENODEV, (std::string("ncclAllGather: ") + g_rccl.GetErrorString(rc ? rc : rc2)).c_str());
    } else {
        MultiDev& m = S.d[0];
        HIP_TRY(hipSetDevice(m.dev), "hipSetDevice");
        HIP_TRY(hipMemcpyAsync(m.gathered, m.words, per_words * sizeof(uint64_t), hipMemcpyDeviceToDevice, m.st), "hipMemcpyAsync words");
    }
    // 3. results back: each device's slice of the bytes and vectors, the gathered words from the first device
    for (int d = 0; d < ndev; d++) {
        MultiDev& m = S.d[d];
        const size_t cnt = m.hi - m.lo;
        HIP_TRY(hipSetDevice(m.dev), "hipSetDevice");
        if (cnt) {
            HIP_TRY(hipMemcpyAsync(mask_out + m.lo, m.mask, cnt, hipMemcpyDeviceToHost, m.st), "hipMemcpyAsync shard mask");
            HIP_TRY(hipMemcpyAsync(dxyz_out + 3 * m.lo, m.out, cnt * 3 * sizeof(float), hipMemcpyDeviceToHost, m.st), "hipMemcpyAsync shard output");
        }
        if (d == 0 && bits_out && n)
            HIP_TRY(hipMemcpyAsync(bits_out, m.gathered, (n + 63) / 64 * sizeof(uint64_t), hipMemcpyDeviceToHost, m.st), "hipMemcpyAsync gathered words");
    }
    for (int d = 0; d < ndev; d++) {
        MultiDev& m = S.d[d];
        HIP_TRY(hipSetDevice(m.dev), "hipSetDevice");
        HIP_TRY(hipStreamSynchronize(m.st), "hipStreamSynchronize");
        float e = 0.f;
        HIP_TRY(hipEventElapsedTime(&e, m.a, m.b), "hipEventElapsedTime");
        if (ms_per_dev) ms_per_dev[d] = (m.hi > m.lo) ? e : 0.f;
    }
    (void)per;
    (void)lo0;
    return LRM_OK;
}

} // extern "C"
