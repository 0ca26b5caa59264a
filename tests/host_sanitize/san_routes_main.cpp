// A stand-alone driver for the sanitizer build of the pose routes HOST code (csrc/Makefile, target `sanitize-routes`;
// tests/test_routes_sanitize_cpu.py builds and runs it), in the manner of san_loads_main.cpp: lrm_pose_routes_cpu on a hostile
// corpus -- edge ends and sources of -1, nposes, INT32_MIN and INT32_MAX; costs of INT32_MIN, -1, 0 and INT32_MAX (sums at and
// past the cap); live bytes of 0, 1 and 255; self-loops, duplicates, zero-cost rings; every direction; no edge, no source, one
// pose; every optional pointer NULL; every refusal of the contract in its order.  The host loop is the bit-exact reference of
// the device kernels and shares its arithmetic header.  Every buffer is a heap block of exactly the documented size.  Only
// return codes and a few invariants are checked: outputs are the business of the other tests.  No GPU is touched.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lrm.h"

namespace {

int g_failures = 0;

void expect(int rc, int want, const char* what) {
    if (rc != want) {
        std::fprintf(stderr, "san_routes_main: %.*s returned %d, expected %d (%s)\n", (int)std::strcspn(what, "("), what, rc, want, lrm_last_error());
        ++g_failures;
    }
}
#define OK(call) expect((call), LRM_OK, #call)
#define REFUSED(call) expect((call), LRM_EINVAL, #call)

const int32_t kCosts[] = {0, 1, 2, 7, INT32_MAX, -1, INT32_MIN, 0, 3, INT32_MAX - 1, 0};
constexpr size_t kNCosts = sizeof(kCosts) / sizeof(kCosts[0]);

uint32_t g_state = 12345u;
uint32_t next() { return g_state = g_state * 1664525u + 1013904223u; }

// bit k of `form` keeps optional argument k: edge_live, pose_live, edge_cost, cost, hops, pred_edge, pred_pose, reached, ms
// (with none of the four per-pose outputs the call keeps hops)
void routes(size_t nposes, size_t nedges, size_t nsources, int direction, unsigned form) {
    const int32_t bad[] = {-1, (int32_t)nposes, INT32_MIN, INT32_MAX, -2, (int32_t)nposes + 1};
    auto index = [&](size_t i) { return next() % 16u == 0u || !nposes ? bad[i % 6] : (int32_t)(next() % (uint32_t)nposes); };
    std::vector<int32_t> a(nedges), b(nedges), w(nedges), src(nsources);
    std::vector<uint8_t> el(nedges), pl(nposes);
    for (size_t e = 0; e < nedges; ++e) {
        a[e] = index(e), b[e] = e % 9 == 4 ? a[e] : index(e + 3);
        w[e] = kCosts[next() % kNCosts];
        el[e] = (uint8_t)(e % 7 == 3 ? 0 : (e % 7 == 5 ? 255 : 1));
    }
    for (size_t p = 0; p < nposes; ++p) pl[p] = (uint8_t)(p % 11 == 6 ? 0 : 1);
    for (size_t s = 0; s < nsources; ++s) src[s] = index(s);
    if ((form & 0x78u) == 0u) form |= 0x10u;
    std::vector<int64_t> cost(nposes);
    std::vector<int32_t> hops(nposes), pe(nposes), pp(nposes);
    int32_t reached = -7;
    double ms = 0;
    auto opt = [&](unsigned k, auto* p) { return (form >> k) & 1u ? p : nullptr; };
    OK(lrm_pose_routes_cpu(nposes, a.data(), b.data(), nedges, opt(0, el.data()), opt(1, pl.data()), opt(2, w.data()), src.data(), nsources,
                           direction, opt(3, cost.data()), opt(4, hops.data()), opt(5, pe.data()), opt(6, pp.data()), opt(7, &reached),
                           opt(8, &ms)));
    if ((form >> 7) & 1u) {
        if (reached < 0 || (size_t)reached > nposes) expect(1, 0, "reached within [0, nposes](");
        if ((form >> 4) & 1u) {
            int32_t n = 0;
            for (size_t p = 0; p < nposes; ++p) n += hops[p] >= 0;
            if (n != reached) expect(1, 0, "reached == poses with hops >= 0(");
        }
    }
}

// a chain of `n` maximal costs: the sums pass the cap after two arcs
void cap(int direction) {
    const size_t n = 6;
    std::vector<int32_t> a(n - 1), b(n - 1), w(n - 1, INT32_MAX), src{0, (int32_t)(n - 1)};
    for (size_t e = 0; e + 1 < n; ++e) a[e] = (int32_t)e, b[e] = (int32_t)e + 1;
    std::vector<int64_t> cost(n);
    std::vector<int32_t> hops(n);
    OK(lrm_pose_routes_cpu(n, a.data(), b.data(), n - 1, nullptr, nullptr, w.data(), src.data(), 2, direction, cost.data(), hops.data(), nullptr,
                           nullptr, nullptr, nullptr));
    for (size_t p = 0; p < n; ++p)
        if (cost[p] > 4294967294ll || cost[p] < -1) expect(1, 0, "cost within the cap(");
}

void refusals() {
    std::vector<int32_t> a{0, 1, 2}, b{1, 2, 3}, src{0}, hops(4);
    struct Args {
        size_t nposes = 4, nedges = 3, nsources = 1;
        int direction = 0;
        const int32_t *a, *b, *src;
        int32_t* hops;
    };
    Args base;
    base.a = a.data(), base.b = b.data(), base.src = src.data(), base.hops = hops.data();
    auto call = [&](const Args& x) {
        return lrm_pose_routes_cpu(x.nposes, x.a, x.b, x.nedges, nullptr, nullptr, nullptr, x.src, x.nsources, x.direction, nullptr, x.hops,
                                   nullptr, nullptr, nullptr, nullptr);
    };
    auto with = [&](auto&& edit) {
        Args x = base;
        edit(x);
        return call(x);
    };
    OK(call(base));
    // the range checks, before the no-op
    for (int d : {-1, 3, INT_MAX, INT_MIN}) REFUSED(with([d](Args& x) { x.direction = d, x.nposes = 0; }));
    REFUSED(with([](Args& x) { x.nposes = (size_t)1 << 31; }));
    REFUSED(with([](Args& x) { x.nedges = (size_t)1 << 31, x.nposes = 0; }));
    REFUSED(with([](Args& x) { x.nsources = (size_t)1 << 40, x.nposes = 0; }));
    // nposes == 0 is a no-op, whatever the pointers
    OK(with([](Args& x) { x.nposes = 0, x.a = x.b = x.src = nullptr, x.hops = nullptr; }));
    // the NULL forms
    REFUSED(with([](Args& x) { x.a = nullptr; }));
    REFUSED(with([](Args& x) { x.b = nullptr; }));
    REFUSED(with([](Args& x) { x.src = nullptr; }));
    REFUSED(with([](Args& x) { x.hops = nullptr; }));
    OK(with([](Args& x) { x.a = x.b = nullptr, x.nedges = 0; }));
    OK(with([](Args& x) { x.src = nullptr, x.nsources = 0; }));
    // the device form refuses bad arguments before it touches a device
    REFUSED(lrm_pose_routes_dev(4, a.data(), b.data(), 3, nullptr, nullptr, nullptr, src.data(), 1, 0, nullptr, 4, 0, nullptr, hops.data(), nullptr,
                                nullptr, nullptr, nullptr, nullptr));
    REFUSED(lrm_pose_routes_dev(4, a.data(), b.data(), 3, nullptr, nullptr, nullptr, src.data(), 1, 0, hops.data(), 0, 0, nullptr, hops.data(),
                                nullptr, nullptr, nullptr, nullptr, nullptr));
    REFUSED(lrm_pose_routes_dev(4, a.data(), b.data(), 3, nullptr, nullptr, nullptr, src.data(), 1, 0, hops.data(), 4097, 0, nullptr, hops.data(),
                                nullptr, nullptr, nullptr, nullptr, nullptr));
    REFUSED(lrm_pose_routes_dev(4, a.data(), b.data(), 3, nullptr, nullptr, nullptr, src.data(), 1, 0, hops.data(), 4, 2, nullptr, hops.data(),
                                nullptr, nullptr, nullptr, nullptr, nullptr));
    uint64_t plan[4];
    OK(lrm_dbg_pose_routes_plan(0, plan));
    OK(lrm_dbg_pose_routes_plan(INT32_MAX, plan));
    REFUSED(lrm_dbg_pose_routes_plan((size_t)1 << 31, plan));
    REFUSED(lrm_dbg_pose_routes_plan(1, nullptr));
}

} // namespace

int main() {
    for (int direction = 0; direction < 3; ++direction) {
        for (size_t nposes : {(size_t)1, (size_t)2, (size_t)7, (size_t)64, (size_t)301})
            for (size_t nedges : {(size_t)0, (size_t)1, (size_t)5, (size_t)257, (size_t)2000})
                for (size_t nsources : {(size_t)0, (size_t)1, (size_t)9})
                    for (unsigned form : {0x1ffu, 0u, 0x0aau, 0x155u, 0x0f8u}) routes(nposes, nedges, nsources, direction, form);
        for (unsigned k = 0; k < 9; ++k) routes(97, 700, 3, direction, 0x1ffu & ~(1u << k));  // every optional pointer NULL alone
        for (unsigned k = 3; k < 7; ++k) routes(97, 700, 3, direction, 1u << k);              // every per-pose output alone
        routes(20000, 60000, 4, direction, 0x1ffu);
        cap(direction);
    }
    refusals();
    if (g_failures) {
        std::fprintf(stderr, "san_routes_main: %d call(s) did not return as documented\n", g_failures);
        return 1;
    }
    std::printf("san_routes_main: every call returned as documented\n");
    return 0;
}
