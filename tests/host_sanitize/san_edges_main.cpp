// A stand-alone driver for the sanitizer build of the pose edges HOST code (csrc/Makefile, target `sanitize-edges`;
// tests/test_edges_sanitize_cpu.py builds and runs it), in the manner of san_routes_main.cpp: lrm_pose_edges_cpu on a hostile
// corpus -- NaN, +-inf, FLT_MAX and denormal bodies; NaN, inf, zero, FLT_MAX and denormal quaternions; live bytes of 0, 1 and
// 255; NULL body and NULL pose_live; max_step of 0, +inf and FLT_MAX; min_dot of 0 and 1; capacity 0 and 1; offsets that
// decrease, are negative, overlap, lie past the end or hold INT64_MIN / INT64_MAX; every optional pointer NULL; every refusal
// of the contract in its order, the device forms' included, which come before any device is touched.  The host loop is the
// bit-exact reference of the device kernels and shares its arithmetic header.  Every buffer is a heap block of exactly the
// documented size.  Only return codes and a few invariants are checked: outputs are the business of the other tests.  No GPU
// is touched.
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lrm.h"

namespace {

int g_failures = 0;

void expect(int rc, int want, const char* what) {
    if (rc != want) {
        std::fprintf(stderr, "san_edges_main: %.*s returned %d, expected %d (%s)\n", (int)std::strcspn(what, "("), what, rc, want, lrm_last_error());
        ++g_failures;
    }
}
#define OK(call) expect((call), LRM_OK, #call)
#define REFUSED(call) expect((call), LRM_EINVAL, #call)

uint32_t g_state = 4242u;
uint32_t next() { return g_state = g_state * 1664525u + 1013904223u; }
float unit() { return (float)(next() >> 8) / 16777216.0f; }

const float kBad[] = {NAN, INFINITY, -INFINITY, FLT_MAX, -FLT_MAX, 1e-42f, 0.0f, -0.0f};
constexpr size_t kNBad = sizeof(kBad) / sizeof(kBad[0]);

// kind of offsets: 0 the counts' scan, 1 two per row, 2 decreasing, 3 negative, 4 random with the extremes, 5 past the end
// bit k of `keep` keeps optional argument k: body, pose_live, count, d2, cos2, written, ms
void edges(size_t nposes, int form, float max_step, float min_dot, int kind, size_t capacity_cut, unsigned keep) {
    std::vector<float> quats(4 * nposes), body(3 * nposes);
    std::vector<uint8_t> live(nposes);
    for (size_t p = 0; p < nposes; ++p) {
        for (int k = 0; k < 3; ++k) body[3 * p + k] = 300.0f * unit();
        for (int k = 0; k < 4; ++k) quats[4 * p + k] = 2.0f * unit() - 1.0f;
        if (next() % 8u == 0u) body[3 * p + next() % 3u] = kBad[next() % kNBad];
        if (next() % 8u == 0u) quats[4 * p + next() % 4u] = kBad[next() % kNBad];
        if (next() % 16u == 0u) std::memset(&quats[4 * p], 0, 4 * sizeof(float));
        live[p] = (uint8_t)(p % 11 == 6 ? 0 : (p % 11 == 3 ? 255 : 1));
    }
    auto opt = [&](unsigned k, auto* p) { return (keep >> k) & 1u ? p : nullptr; };
    std::vector<int32_t> count(nposes);
    double ms = 0;
    // the counts alone: no list argument is read
    OK(lrm_pose_edges_cpu(quats.data(), opt(0, body.data()), nposes, opt(1, live.data()), max_step, min_dot, form, count.data(), nullptr, 12345,
                          nullptr, nullptr, nullptr, nullptr, nullptr, opt(6, &ms)));
    std::vector<int64_t> offsets(nposes + 1, 0);
    int64_t total = 0;
    for (size_t p = 0; p < nposes; ++p) {
        if (count[p] < 0 || (size_t)count[p] >= nposes) expect(1, 0, "count within [0, nposes)(");
        offsets[p + 1] = offsets[p] + count[p];
    }
    total = offsets[nposes];
    const int64_t extremes[] = {INT64_MIN, INT64_MAX, -1, total, total + 1, 0};
    for (size_t p = 0; p <= nposes; ++p) {
        if (kind == 1) offsets[p] = 2 * (int64_t)p;
        if (kind == 2) offsets[p] = total - offsets[p];
        if (kind == 3) offsets[p] -= total / 2 + 1;
        if (kind == 4) offsets[p] = next() % 5u == 0u ? extremes[next() % 6u] : (int64_t)(next() % (uint32_t)(total + 2));
        if (kind == 5) offsets[p] += total;
    }
    const size_t capacity = capacity_cut == 0 ? (size_t)total : (capacity_cut == 1 ? 0 : (capacity_cut == 2 ? 1 : (size_t)total / 2));
    int32_t *const ea = new int32_t[capacity], *const eb = new int32_t[capacity]; // blocks of exactly `capacity` entries, never NULL
    float *const d2 = new float[capacity], *const cos2 = new float[capacity];
    std::vector<int32_t> written(nposes, -7);
    OK(lrm_pose_edges_cpu(quats.data(), opt(0, body.data()), nposes, opt(1, live.data()), max_step, min_dot, form, opt(2, count.data()),
                          offsets.data(), capacity, ea, eb, opt(3, d2), opt(4, cos2), opt(5, written.data()), opt(6, &ms)));
    delete[] ea, delete[] eb, delete[] d2, delete[] cos2;
    if ((keep >> 5) & 1u) {
        int64_t sum = 0;
        for (size_t p = 0; p < nposes; ++p) {
            if (written[p] < 0 || written[p] > count[p]) expect(1, 0, "written within [0, count](");
            sum += written[p];
        }
        if (kind == 0 && capacity_cut == 0 && sum != total) expect(1, 0, "every row whole with the counts' offsets(");
    }
}

void refusals() {
    std::vector<float> quats{1, 0, 0, 0, 1, 0, 0, 0}, body{0, 0, 0, 1, 0, 0};
    std::vector<int32_t> count(2), ea(4), eb(4);
    std::vector<int64_t> offsets{0, 1, 2};
    struct Args {
        size_t nposes = 2, capacity = 4;
        float max_step = 5.0f, min_dot = 0.5f;
        int form = 0;
        const float* quats;
        int32_t *count, *ea, *eb;
        const int64_t* offsets;
    };
    Args base;
    base.quats = quats.data(), base.count = count.data(), base.ea = ea.data(), base.eb = eb.data(), base.offsets = offsets.data();
    auto call = [&](const Args& x) {
        return lrm_pose_edges_cpu(x.quats, body.data(), x.nposes, nullptr, x.max_step, x.min_dot, x.form, x.count, x.offsets, x.capacity, x.ea, x.eb,
                                  nullptr, nullptr, nullptr, nullptr);
    };
    auto with = [&](auto&& edit) {
        Args x = base;
        edit(x);
        return call(x);
    };
    OK(call(base));
    // the range checks, before the no-op
    for (int f : {-1, 2, INT_MAX, INT_MIN}) REFUSED(with([f](Args& x) { x.form = f, x.nposes = 0; }));
    REFUSED(with([](Args& x) { x.nposes = (size_t)1 << 31; }));
    for (float s : {NAN, -1.0f, -INFINITY, -1e-42f}) REFUSED(with([s](Args& x) { x.max_step = s, x.nposes = 0; }));
    for (float d : {NAN, -0.5f, 1.5f, INFINITY, -INFINITY}) REFUSED(with([d](Args& x) { x.min_dot = d, x.nposes = 0; }));
    for (float s : {0.0f, -0.0f, INFINITY, FLT_MAX, 1e-42f}) OK(with([s](Args& x) { x.max_step = s; }));
    for (float d : {0.0f, -0.0f, 1.0f, 1e-42f}) OK(with([d](Args& x) { x.min_dot = d; }));
    // nposes == 0 is a no-op, whatever the pointers
    OK(with([](Args& x) { x.nposes = 0, x.quats = nullptr, x.count = x.ea = x.eb = nullptr, x.offsets = nullptr; }));
    // the NULL forms
    REFUSED(with([](Args& x) { x.quats = nullptr; }));
    REFUSED(with([](Args& x) { x.ea = nullptr; }));
    REFUSED(with([](Args& x) { x.eb = nullptr; }));
    REFUSED(with([](Args& x) { x.count = nullptr, x.offsets = nullptr; }));
    OK(with([](Args& x) { x.count = nullptr; }));
    OK(with([](Args& x) { x.offsets = nullptr, x.ea = x.eb = nullptr; }));
    OK(with([](Args& x) { x.capacity = 0; }));
    // the device forms refuse bad arguments before they touch a device
    REFUSED(lrm_pose_edge_counts_dev(quats.data(), nullptr, 2, nullptr, 5.0f, 0.5f, 2, offsets.data(), count.data(), nullptr));
    REFUSED(lrm_pose_edge_counts_dev(quats.data(), nullptr, 2, nullptr, NAN, 0.5f, 0, offsets.data(), count.data(), nullptr));
    REFUSED(lrm_pose_edge_counts_dev(quats.data(), nullptr, 2, nullptr, 5.0f, 2.0f, 0, offsets.data(), count.data(), nullptr));
    REFUSED(lrm_pose_edge_counts_dev(quats.data(), nullptr, 2, nullptr, 5.0f, 0.5f, 0, nullptr, count.data(), nullptr));
    REFUSED(lrm_pose_edge_counts_dev(quats.data(), nullptr, 2, nullptr, 5.0f, 0.5f, 0, offsets.data(), nullptr, nullptr));
    REFUSED(lrm_pose_edges_dev(quats.data(), nullptr, 2, nullptr, 5.0f, 0.5f, -1, offsets.data(), offsets.data(), 4, ea.data(), eb.data(), nullptr,
                               nullptr, nullptr, nullptr));
    REFUSED(lrm_pose_edges_dev(quats.data(), nullptr, (size_t)1 << 31, nullptr, 5.0f, 0.5f, 0, offsets.data(), offsets.data(), 4, ea.data(),
                               eb.data(), nullptr, nullptr, nullptr, nullptr));
    REFUSED(lrm_pose_edges_dev(quats.data(), nullptr, 2, nullptr, 5.0f, 0.5f, 0, offsets.data(), nullptr, 4, ea.data(), eb.data(), nullptr, nullptr,
                               nullptr, nullptr));
    REFUSED(lrm_pose_edges_dev(quats.data(), nullptr, 2, nullptr, 5.0f, 0.5f, 0, offsets.data(), offsets.data(), 4, nullptr, eb.data(), nullptr,
                               nullptr, nullptr, nullptr));
    OK(lrm_pose_edges_dev(nullptr, nullptr, 0, nullptr, 5.0f, 0.5f, 0, nullptr, nullptr, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    OK(lrm_pose_edge_counts_dev(nullptr, nullptr, 0, nullptr, 5.0f, 0.5f, 1, nullptr, nullptr, nullptr));
    uint64_t plan[4];
    OK(lrm_dbg_pose_edges_plan(0, plan));
    OK(lrm_dbg_pose_edges_plan(INT32_MAX, plan));
    REFUSED(lrm_dbg_pose_edges_plan((size_t)1 << 31, plan));
    REFUSED(lrm_dbg_pose_edges_plan(1, nullptr));
    if (lrm_pose_edges_workspace_bytes(0) == 0 || lrm_pose_edges_workspace_bytes(65) != 96) expect(1, 0, "workspace bytes(");
}

} // namespace

int main() {
    const float steps[] = {60.0f, 0.0f, INFINITY, FLT_MAX};
    const float dots[] = {0.0f, 0.9f, 1.0f};
    for (int form = 0; form < 2; ++form) {
        for (size_t nposes : {(size_t)1, (size_t)2, (size_t)7, (size_t)64, (size_t)65, (size_t)301})
            for (float step : steps)
                for (float dot : dots)
                    for (int kind = 0; kind < 6; ++kind)
                        for (size_t cut = 0; cut < 4; ++cut) edges(nposes, form, step, dot, kind, cut, 0x7fu);
        for (unsigned k = 0; k < 7; ++k) edges(97, form, 80.0f, 0.5f, 0, 0, 0x7fu & ~(1u << k));  // every optional pointer NULL alone
        edges(97, form, 80.0f, 0.5f, 4, 3, 0u);
        edges(3000, form, 40.0f, 0.3f, 0, 0, 0x7fu);
    }
    refusals();
    if (g_failures) {
        std::fprintf(stderr, "san_edges_main: %d call(s) did not return as documented\n", g_failures);
        return 1;
    }
    std::printf("san_edges_main: every call returned as documented\n");
    return 0;
}
