// A stand-alone driver for the sanitizer build of the swing transit HOST code (csrc/Makefile, target `sanitize-swing`;
// tests/test_swing_sanitize_cpu.py builds and runs it), in the manner of san_transit_main.cpp: lrm_swing_transit_posed_cpu on a
// hostile corpus -- nan, zero, non-unit, antipodal, huge and infinite quaternions; nan, infinite and huge bodies and targets
// (take-off and landing targets among them, so that path points overflow and turn nan); every sample count from 2 to 64 with
// every skip that matters for it; foot_from / foot_to of -1, nt, INT32_MIN and INT32_MAX; edge ends out of range; lifts of
// either sign and of 1e30; foot_radius 0, tiny and huge; every optional pointer NULL; one to eight legs; every refusal of
// the contract in its order.  The host loop is the bit-exact reference of the device kernels and shares its arithmetic header,
// so this is the out-of-bounds and undefined-behaviour check that arithmetic gets.  Every buffer is a heap block of exactly the
// documented size.  Only return codes are checked: outputs are the business of the other tests.  No GPU is touched.
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
        std::fprintf(stderr, "san_swing_main: %.*s returned %d, expected %d (%s)\n", (int)std::strcspn(what, "("), what, rc, want, lrm_last_error());
        ++g_failures;
    }
}
#define OK(call) expect((call), LRM_OK, #call)
#define REFUSED(call) expect((call), LRM_EINVAL, #call)

constexpr float kInf = std::numeric_limits<float>::infinity();
constexpr float kNan = std::numeric_limits<float>::quiet_NaN();
constexpr float kDen = std::numeric_limits<float>::denorm_min();

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
    std::vector<int32_t> ea, eb, from, to;
    std::vector<uint8_t> live;
};

Scene scene(size_t nlegs, size_t nedges, size_t nt) {
    Scene s;
    s.quats.assign(&kQuats[0][0], &kQuats[0][0] + 4 * kNQuats);
    s.body.resize(3 * kNQuats);
    for (size_t i = 0; i < s.body.size(); ++i) s.body[i] = i < 24 ? 20.f * (float)(i % 7) : kCoords[(i * 5 + i / 3) % kNCoords];
    s.targets.resize(3 * nt);
    for (size_t i = 0; i < s.targets.size(); ++i) s.targets[i] = i < 60 ? 35.f * (float)(i % 11) - 150.f : kCoords[(i * 3 + i / 7) % kNCoords];
    s.ea.resize(nedges);
    s.eb.resize(nedges);
    for (size_t e = 0; e < nedges; ++e) {
        s.ea[e] = e % 5 == 4 ? kBadIdx[e % kNBadIdx] : (int32_t)(e % kNQuats);
        s.eb[e] = e % 7 == 6 ? kBadIdx[(e / 7) % kNBadIdx] : (int32_t)((e + 1 + e / kNQuats) % kNQuats);
    }
    s.from.resize(nlegs * nedges);
    s.to.resize(nlegs * nedges);
    const int32_t bad[] = {-1, (int32_t)nt, INT32_MIN, INT32_MAX, -2, (int32_t)nt + 1};
    for (size_t i = 0; i < s.from.size(); ++i) {
        s.from[i] = i % 5 == 3 ? bad[(i / 5) % 6] : (int32_t)(nt ? (i * 7) % nt : 0);
        s.to[i] = i % 7 == 2 ? bad[(i / 7) % 6] : (int32_t)(nt ? (i * 11 + 3) % nt : 0);  // finite and hostile targets, from == to at times
    }
    s.live.resize(nedges);
    for (size_t e = 0; e < nedges; ++e) s.live[e] = (uint8_t)(e % 4 == 1 ? 0 : (e % 4 == 2 ? 255 : 1));
    return s;
}

// bit k of `form` keeps optional argument k: body, live_in, mask, worst, worst_d2, pen, swinging, clear, up, ms
void swing(size_t nlegs, size_t nedges, size_t nt, size_t S, float lift, float radius, float margin, uint32_t skip, unsigned form) {
    const auto legs = legs_n(nlegs);
    Scene s = scene(nlegs, nedges, nt);
    const size_t n = nlegs * nedges;
    std::vector<uint64_t> mask(n);
    std::vector<int32_t> reached(n), first(n), worst(n), hits(n), seg(n), near(n);
    std::vector<float> d2(n), pen(n), up{0.2f, -0.1f, 0.9f};
    std::vector<uint8_t> swinging(nedges), clear(nedges);
    double ms = 0;
    auto opt = [&](unsigned k, auto* p) { return (form >> k) & 1u ? p : nullptr; };
    OK(lrm_swing_transit_posed_cpu(s.targets.data(), nt, s.quats.data(), opt(0, s.body.data()), kNQuats, legs.data(), nlegs, s.ea.data(),
                                   s.eb.data(), nedges, s.from.data(), s.to.data(), S, lift, opt(8, up.data()), radius, margin, skip,
                                   opt(1, s.live.data()), opt(2, mask.data()), reached.data(), first.data(), opt(3, worst.data()),
                                   opt(4, d2.data()), hits.data(), seg.data(), near.data(), opt(5, pen.data()), opt(6, swinging.data()),
                                   opt(7, clear.data()), opt(9, &ms)));
}

void refusals() {
    const auto legs = legs_n(8);
    Scene s = scene(6, 4, 16);
    std::vector<int32_t> r(6 * 4), f(6 * 4), h(6 * 4), g(6 * 4), n(6 * 4);
    const float up[3] = {0, 0, 1};
    struct Args {
        size_t nt = 16, nposes = kNQuats, nlegs = 6, nedges = 4, S = 9;
        float lift = 20.f, radius = 12.f, margin = 5.f;
        uint32_t skip = 1;
        const float *tg, *q, *up;
        const LrmLegDimensions* lg;
        const int32_t *a, *b, *from, *to;
        int32_t *r, *f, *h, *g, *n;
    };
    Args base;
    base.tg = s.targets.data(), base.q = s.quats.data(), base.up = up, base.lg = legs.data();
    base.a = s.ea.data(), base.b = s.eb.data(), base.from = s.from.data(), base.to = s.to.data();
    base.r = r.data(), base.f = f.data(), base.h = h.data(), base.g = g.data(), base.n = n.data();
    auto call = [&](const Args& x) {
        return lrm_swing_transit_posed_cpu(x.tg, x.nt, x.q, nullptr, x.nposes, x.lg, x.nlegs, x.a, x.b, x.nedges, x.from, x.to, x.S, x.lift, x.up,
                                           x.radius, x.margin, x.skip, nullptr, nullptr, x.r, x.f, nullptr, nullptr, x.h, x.g, x.n, nullptr, nullptr,
                                           nullptr, nullptr);
    };
    auto with = [&](auto&& edit) {
        Args x = base;
        edit(x);
        return call(x);
    };
    OK(call(base));
    // the range checks and the scalars, before the no-op
    REFUSED(with([](Args& x) { x.nlegs = 0, x.nedges = 0; }));
    REFUSED(with([](Args& x) { x.nlegs = 9, x.nedges = 0; }));
    for (size_t S : {(size_t)0, (size_t)1, (size_t)65, (size_t)1 << 40}) REFUSED(with([S](Args& x) { x.S = S, x.nedges = 0; }));
    REFUSED(with([](Args& x) { x.nt = (size_t)1 << 31, x.nedges = 0; }));
    REFUSED(with([](Args& x) { x.nposes = (size_t)1 << 31, x.nedges = 0; }));
    REFUSED(with([](Args& x) { x.nedges = ((size_t)UINT32_MAX) / 6 + 1; }));
    for (float v : {kNan, kInf, -kInf}) {
        REFUSED(with([v](Args& x) { x.lift = v, x.nedges = 0; }));
        REFUSED(with([v](Args& x) { x.radius = v, x.nedges = 0; }));
        REFUSED(with([v](Args& x) { x.margin = v, x.nedges = 0; }));
    }
    REFUSED(with([](Args& x) { x.radius = -1.f, x.nedges = 0; }));
    REFUSED(with([](Args& x) { x.margin = -kDen, x.nedges = 0; }));
    REFUSED(with([](Args& x) { x.skip = 64, x.nedges = 0; }));
    REFUSED(with([](Args& x) { x.skip = UINT32_MAX, x.nedges = 0; }));
    for (int k = 0; k < 3; ++k)
        for (float v : {kNan, kInf, -kInf}) {
            float bad[3] = {0, 0, 1};
            bad[k] = v;
            REFUSED(with([&bad](Args& x) { x.up = bad, x.nedges = 0; }));
        }
    // nedges == 0 is a no-op, whatever the pointers
    OK(with([](Args& x) {
        x = Args{};
        x.nt = (size_t)INT32_MAX, x.nposes = (size_t)INT32_MAX, x.nlegs = 8, x.nedges = 0, x.S = 64, x.skip = 63;
        x.tg = x.q = x.up = nullptr, x.lg = nullptr, x.a = x.b = x.from = x.to = nullptr, x.r = x.f = x.h = x.g = x.n = nullptr;
    }));
    // the NULL forms
    REFUSED(with([](Args& x) { x.q = nullptr; }));
    REFUSED(with([](Args& x) { x.lg = nullptr; }));
    REFUSED(with([](Args& x) { x.a = nullptr; }));
    REFUSED(with([](Args& x) { x.b = nullptr; }));
    REFUSED(with([](Args& x) { x.from = nullptr; }));
    REFUSED(with([](Args& x) { x.to = nullptr; }));
    REFUSED(with([](Args& x) { x.r = nullptr; }));
    REFUSED(with([](Args& x) { x.f = nullptr; }));
    REFUSED(with([](Args& x) { x.h = nullptr; }));
    REFUSED(with([](Args& x) { x.g = nullptr; }));
    REFUSED(with([](Args& x) { x.n = nullptr; }));
    REFUSED(with([](Args& x) { x.tg = nullptr; }));
    OK(with([](Args& x) { x.tg = nullptr, x.nt = 0; }));  // nt == 0 lets nothing swing: no cloud is read
    OK(with([](Args& x) { x.nposes = 0; }));              // no pose: every edge is dead
    OK(with([](Args& x) { x.up = nullptr; }));            // up NULL = (0, 0, 1)
    OK(with([](Args& x) { x.radius = 0.f, x.margin = 0.f, x.skip = 63; }));
}

} // namespace

int main() {
    for (size_t S = 2; S <= 64; ++S)  // every sample count, with no skip, the largest skip that leaves a segment, and one more
        for (uint32_t skip : {0u, (uint32_t)((S - 2) / 2), (uint32_t)((S - 2) / 2 + 1), 63u}) swing(1 + S % 8, 29, 67, S, 25.f, 30.f, 10.f, skip, 0x3ffu);
    for (size_t nlegs = 1; nlegs <= 8; ++nlegs)
        for (size_t nedges : {(size_t)1, (size_t)2 * kNQuats + 3})
            for (unsigned form : {0u, 0x3ffu, 0x2aau, 0x155u, 0x003u}) swing(nlegs, nedges, 67, 9, -15.f, 30.f, 10.f, 1, form);
    for (unsigned k = 0; k < 10; ++k) swing(6, 31, 67, 5, 25.f, 30.f, 10.f, 0, 0x3ffu & ~(1u << k));  // every optional pointer NULL alone
    for (float lift : {0.f, 1e30f, -1e30f, 3e38f, kDen})
        for (float radius : {0.f, kDen, 1e-30f, 3e38f}) swing(6, 31, 67, 9, lift, radius, radius, 0, 0x3ffu);
    swing(6, 31, 67, 9, 25.f, 30.f, 3e38f, 0, 0x3ffu);  // radius + margin overflows
    swing(6, 31, 0, 9, 25.f, 30.f, 10.f, 0, 0x3ffu);    // an empty cloud
    swing(6, 31, 1, 64, 25.f, 30.f, 10.f, 0, 0x3ffu);   // from == to everywhere
    swing(6, 31, 2, 64, 25.f, 30.f, 10.f, 0, 0x3ffu);
    refusals();
    if (g_failures) {
        std::fprintf(stderr, "san_swing_main: %d call(s) did not return as documented\n", g_failures);
        return 1;
    }
    std::printf("san_swing_main: every call returned as documented\n");
    return 0;
}
