// A stand-alone driver for the sanitizer build of the edge transit HOST code (csrc/Makefile, target `sanitize-transit`;
// tests/test_transit_sanitize_cpu.py builds and runs it), in the manner of san_trunk_main.cpp: lrm_edge_transit_posed_cpu and
// lrm_dbg_edge_transit_samples_host on a hostile corpus -- nan, zero, non-unit, antipodal, huge and infinite quaternions; nan,
// infinite and huge bodies and targets; every sample count from 2 to 64; feet of -1, nt, INT32_MIN and INT32_MAX; edge ends out
// of range; every optional pointer NULL; one to eight legs; every refusal of the contract in its order.  The host loop is the
// bit-exact reference of the device kernel and shares its arithmetic header, so this is the out-of-bounds and
// undefined-behaviour check that arithmetic gets.  Every buffer is a heap block of exactly the documented size.  Only return
// codes are checked: outputs are the business of the other tests.  No GPU is touched.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "lrm.h"

namespace {

int g_failures = 0;

void expect(int rc, int want, const char* what) {
    if (rc != want) {
        std::fprintf(stderr, "san_transit_main: %.*s returned %d, expected %d (%s)\n", (int)std::strcspn(what, "("), what, rc, want, lrm_last_error());
        ++g_failures;
    }
}
#define OK(call) expect((call), LRM_OK, #call)
#define REFUSED(call) expect((call), LRM_EINVAL, #call)

constexpr float kInf = std::numeric_limits<float>::infinity();
constexpr float kNan = std::numeric_limits<float>::quiet_NaN();
constexpr float kDen = std::numeric_limits<float>::denorm_min();

// neighbours in this list are the ends of an edge: unit pairs, antipodal pairs (q, -q), orthogonal pairs (dot = 0) and the rest
const float kQuats[][4] = {{1, 0, 0, 0}, {-1, 0, 0, 0}, {0.9238795f, 0, 0.3826834f, 0}, {0.5f, 0.5f, 0.5f, 0.5f}, {-0.5f, -0.5f, -0.5f, -0.5f},
                           {0.8f, -0.2f, 0.1f, 0.5567764f}, {0, 1, 0, 0}, {0, 0, 1, 0}, {kNan, 0, 0, 0}, {1, kNan, kNan, kNan}, {0, 0, 0, 0},
                           {0, 0, 0, 0}, {0.5f, 0.5f, 0.5f, 0.1f}, {3, -2, 1, 4}, {1e30f, 1e30f, -1e30f, 1e30f}, {-1e30f, -1e30f, 1e30f, -1e30f},
                           {kInf, 0, 0, 0}, {1, -kInf, 0, 0}, {kDen, kDen, 0, 0}, {3e38f, 3e38f, 3e38f, 3e38f}, {-3e38f, 3e38f, -3e38f, 3e38f},
                           {1e-19f, 1e-19f, 0, 0}, {1e-10f, 0, 1e-10f, 0}, {1e-30f, 0, 0, 0}};
constexpr size_t kNQuats = sizeof(kQuats) / sizeof(kQuats[0]);
const float kCoords[] = {0.f, 120.f, -250.f, 400.f, -80.f, kNan, kInf, -kInf, 3e38f, -3e38f, 4e6f, kDen, 1e30f, 310.f, -40.f, 95.f};
constexpr size_t kNCoords = sizeof(kCoords) / sizeof(kCoords[0]);
const int32_t kBadIdx[] = {INT32_MIN, INT32_MAX, -1, 0, 1, 2, 3, -2, 1 << 30, INT32_MIN + 1, (int32_t)kNQuats, (int32_t)kNQuats - 1};
constexpr size_t kNBadIdx = sizeof(kBadIdx) / sizeof(kBadIdx[0]);

std::vector<LrmLegDimensions> legs_n(size_t n) {
    std::vector<LrmLegDimensions> legs(n);
    for (size_t l = 0; l < n; ++l) {
        if (l % 2) lrm_get_moonbot_leg(0.7853982f * (float)l, &legs[l]);
        else lrm_get_M2_leg(0.7853982f * (float)l, &legs[l]);
    }
    return legs;
}

struct Scene {
    std::vector<float> quats, body, targets;
    std::vector<int32_t> ea, eb, foot;
    std::vector<uint8_t> live;
};

Scene scene(size_t nlegs, size_t nedges, size_t nt) {
    Scene s;
    s.quats.assign(&kQuats[0][0], &kQuats[0][0] + 4 * kNQuats);
    s.body.resize(3 * kNQuats);
    for (size_t i = 0; i < s.body.size(); ++i) s.body[i] = i < 24 ? 20.f * (float)(i % 7) : kCoords[(i * 5 + i / 3) % kNCoords];
    s.targets.resize(3 * nt);
    for (size_t i = 0; i < s.targets.size(); ++i) s.targets[i] = i < 30 ? 35.f * (float)(i % 11) - 150.f : kCoords[(i * 3 + i / 7) % kNCoords];
    s.ea.resize(nedges);
    s.eb.resize(nedges);
    for (size_t e = 0; e < nedges; ++e) {
        s.ea[e] = e % 5 == 4 ? kBadIdx[e % kNBadIdx] : (int32_t)(e % kNQuats);
        s.eb[e] = e % 7 == 6 ? kBadIdx[(e / 7) % kNBadIdx] : (int32_t)((e + 1 + e / kNQuats) % kNQuats);
    }
    s.foot.resize(nlegs * nedges);
    const int32_t bad[] = {-1, (int32_t)nt, INT32_MIN, INT32_MAX, -2, (int32_t)nt + 1};
    for (size_t i = 0; i < s.foot.size(); ++i) s.foot[i] = i % 4 == 3 ? bad[(i / 4) % 6] : (int32_t)(nt ? (i * 7) % nt : 0);
    s.live.resize(nedges);
    for (size_t e = 0; e < nedges; ++e) s.live[e] = (uint8_t)(e % 4 == 1 ? 0 : (e % 4 == 2 ? 255 : 1));
    return s;
}

// bit k of `form` keeps optional argument k: body, live_in, mask, worst, worst_d2, planted, clear, advance, ms
void transit(size_t nlegs, size_t nedges, size_t nt, size_t S, unsigned form) {
    const auto legs = legs_n(nlegs);
    Scene s = scene(nlegs, nedges, nt);
    const size_t n = nlegs * nedges;
    std::vector<uint64_t> mask(n);
    std::vector<int32_t> reached(n), first(n), worst(n), advance(nedges);
    std::vector<float> d2(n);
    std::vector<uint8_t> planted(nedges), clear(nedges);
    double ms = 0;
    auto opt = [&](unsigned k, auto* p) { return (form >> k) & 1u ? p : nullptr; };
    OK(lrm_edge_transit_posed_cpu(s.targets.data(), nt, s.quats.data(), opt(0, s.body.data()), kNQuats, legs.data(), nlegs, s.ea.data(),
                                  s.eb.data(), nedges, s.foot.data(), S, opt(1, s.live.data()), opt(2, mask.data()), reached.data(),
                                  first.data(), opt(3, worst.data()), opt(4, d2.data()), opt(5, planted.data()), opt(6, clear.data()),
                                  opt(7, advance.data()), opt(8, &ms)));
    std::vector<float> smp(nedges * S * 7);
    OK(lrm_dbg_edge_transit_samples_host(s.quats.data(), opt(0, s.body.data()), kNQuats, s.ea.data(), s.eb.data(), nedges, S, smp.data()));
}

void refusals() {
    const auto legs = legs_n(8);
    Scene s = scene(6, 4, 16);
    std::vector<int32_t> reached(6 * 4), first(6 * 4);
    auto call = [&](size_t nt, size_t nposes, size_t nlegs, size_t nedges, size_t S, const float* tg, const float* q, const LrmLegDimensions* lg,
                    const int32_t* a, const int32_t* b, const int32_t* ft, int32_t* r, int32_t* f) {
        return lrm_edge_transit_posed_cpu(tg, nt, q, nullptr, nposes, lg, nlegs, a, b, nedges, ft, S, nullptr, nullptr, r, f, nullptr, nullptr,
                                          nullptr, nullptr, nullptr, nullptr);
    };
    const float *T = s.targets.data(), *Q = s.quats.data();
    const int32_t *A = s.ea.data(), *B = s.eb.data(), *F = s.foot.data();
    int32_t *R = reached.data(), *M = first.data();
    OK(call(16, kNQuats, 6, 4, 9, T, Q, legs.data(), A, B, F, R, M));
    // the range checks, before the no-op
    REFUSED(call(16, kNQuats, 0, 0, 9, T, Q, legs.data(), A, B, F, R, M));
    REFUSED(call(16, kNQuats, 9, 0, 9, T, Q, legs.data(), A, B, F, R, M));
    for (size_t S : {(size_t)0, (size_t)1, (size_t)65, (size_t)1 << 40}) REFUSED(call(16, kNQuats, 6, 0, S, T, Q, legs.data(), A, B, F, R, M));
    REFUSED(call((size_t)1 << 31, kNQuats, 6, 0, 9, T, Q, legs.data(), A, B, F, R, M));
    REFUSED(call(16, (size_t)1 << 31, 6, 0, 9, T, Q, legs.data(), A, B, F, R, M));
    REFUSED(call(16, kNQuats, 6, ((size_t)UINT32_MAX) / 6 + 1, 9, T, Q, legs.data(), A, B, F, R, M));
    REFUSED(call(16, kNQuats, 1, (size_t)1 << 32, 9, T, Q, legs.data(), A, B, F, R, M));
    // nedges == 0 is a no-op, whatever the pointers
    OK(call((size_t)INT32_MAX, (size_t)INT32_MAX, 8, 0, 64, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    // the NULL forms
    REFUSED(call(16, kNQuats, 6, 4, 9, T, nullptr, legs.data(), A, B, F, R, M));
    REFUSED(call(16, kNQuats, 6, 4, 9, T, Q, nullptr, A, B, F, R, M));
    REFUSED(call(16, kNQuats, 6, 4, 9, T, Q, legs.data(), nullptr, B, F, R, M));
    REFUSED(call(16, kNQuats, 6, 4, 9, T, Q, legs.data(), A, nullptr, F, R, M));
    REFUSED(call(16, kNQuats, 6, 4, 9, T, Q, legs.data(), A, B, nullptr, R, M));
    REFUSED(call(16, kNQuats, 6, 4, 9, T, Q, legs.data(), A, B, F, nullptr, M));
    REFUSED(call(16, kNQuats, 6, 4, 9, T, Q, legs.data(), A, B, F, R, nullptr));
    REFUSED(call(16, kNQuats, 6, 4, 9, nullptr, Q, legs.data(), A, B, F, R, M));
    OK(call(0, kNQuats, 6, 4, 9, nullptr, Q, legs.data(), A, B, F, R, M));  // nt == 0 plants nothing: no cloud is read
    OK(call(16, 0, 6, 4, 9, T, Q, legs.data(), A, B, F, R, M));             // no pose: every edge is dead
    // the samples diagnostic
    std::vector<float> smp(4 * 64 * 7);
    REFUSED(lrm_dbg_edge_transit_samples_host(Q, nullptr, kNQuats, A, B, 4, 1, smp.data()));
    REFUSED(lrm_dbg_edge_transit_samples_host(Q, nullptr, kNQuats, A, B, 4, 65, smp.data()));
    REFUSED(lrm_dbg_edge_transit_samples_host(nullptr, nullptr, kNQuats, A, B, 4, 9, smp.data()));
    REFUSED(lrm_dbg_edge_transit_samples_host(Q, nullptr, kNQuats, A, B, 4, 9, nullptr));
    OK(lrm_dbg_edge_transit_samples_host(nullptr, nullptr, 0, nullptr, nullptr, 0, 9, nullptr));
}

} // namespace

int main() {
    for (size_t S = 2; S <= 64; ++S) transit(1 + S % 8, 29, 47, S, 0x1ffu);           // every sample count
    for (size_t nlegs = 1; nlegs <= 8; ++nlegs)
        for (size_t nedges : {(size_t)1, (size_t)2 * kNQuats + 3})
            for (unsigned form : {0u, 0x1ffu, 0x0aau, 0x155u, 0x003u}) transit(nlegs, nedges, 47, 9, form);
    for (unsigned k = 0; k < 9; ++k) transit(6, 31, 47, 5, 0x1ffu & ~(1u << k));         // every optional pointer NULL alone
    transit(6, 31, 0, 9, 0x1ffu);                                                      // an empty cloud
    transit(6, 31, 1, 64, 0x1ffu);
    refusals();
    if (g_failures) {
        std::fprintf(stderr, "san_transit_main: %d call(s) did not return as documented\n", g_failures);
        return 1;
    }
    std::printf("san_transit_main: every call returned as documented\n");
    return 0;
}
