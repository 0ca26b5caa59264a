// A stand-alone driver for the sanitizer build of the stance loads HOST code (csrc/Makefile, target `sanitize-loads`;
// tests/test_stance_loads_sanitize_cpu.py builds and runs it), in the manner of san_swing_main.cpp: lrm_stance_loads_posed_cpu
// on a hostile corpus -- nan, zero, non-unit, huge and infinite quaternions; nan, infinite and huge joint angles, and angles
// outside the sincos range; pose indices of -1, nposes, INT32_MIN and INT32_MAX; every lift-set count that matters with every
// lift byte; planes that are degenerate, huge or zero; centres of mass up to 3e38; tau_max from the smallest denormal to +inf;
// every optional pointer NULL; one to eight legs; every refusal of the contract in its order.  The host loop is the bit-exact
// reference of the device kernel and shares its arithmetic header, so this is the out-of-bounds and undefined-behaviour check
// that arithmetic gets.  Every buffer is a heap block of exactly the documented size.  Only return codes are checked: outputs
// are the business of the other tests.  No GPU is touched.
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
        std::fprintf(stderr, "san_loads_main: %.*s returned %d, expected %d (%s)\n", (int)std::strcspn(what, "("), what, rc, want, lrm_last_error());
        ++g_failures;
    }
}
#define OK(call) expect((call), LRM_OK, #call)
#define REFUSED(call) expect((call), LRM_EINVAL, #call)

constexpr float kInf = std::numeric_limits<float>::infinity();
constexpr float kNan = std::numeric_limits<float>::quiet_NaN();
constexpr float kDen = std::numeric_limits<float>::denorm_min();

const float kQuats[][4] = {{1, 0, 0, 0}, {-1, 0, 0, 0}, {0.9238795f, 0, 0.3826834f, 0}, {0.5f, 0.5f, 0.5f, 0.5f}, {0.8f, -0.2f, 0.1f, 0.5567764f},
                           {0, 1, 0, 0}, {kNan, 0, 0, 0}, {1, kNan, kNan, kNan}, {0, 0, 0, 0}, {0.5f, 0.5f, 0.5f, 0.1f}, {3, -2, 1, 4},
                           {1e30f, 1e30f, -1e30f, 1e30f}, {kInf, 0, 0, 0}, {1, -kInf, 0, 0}, {kDen, kDen, 0, 0}, {3e38f, 3e38f, 3e38f, 3e38f},
                           {1e-19f, 1e-19f, 0, 0}, {1e-30f, 0, 0, 0}};
constexpr size_t kNQuats = sizeof(kQuats) / sizeof(kQuats[0]);
const float kAngles[] = {0.f, 0.3f, -0.7f, -1.4f, 1.1f, -2.2f, kNan, kInf, -kInf, 119.f, -121.f, 3e38f, kDen, -0.f, 3.1415927f, 1e-20f};
constexpr size_t kNAngles = sizeof(kAngles) / sizeof(kAngles[0]);
const int32_t kBadIdx[] = {INT32_MIN, INT32_MAX, -1, (int32_t)kNQuats, -2, 1 << 30};
const float kPlanes[][6] = {{1, 0, 0, 0, 1, 0}, {1, 0, 0, 0, 0.94f, 0.34f}, {1, 0, 0, 1, 0, 0}, {0, 0, 0, 0, 0, 0}, {3e38f, 3e38f, 3e38f, -3e38f, 3e38f, 3e38f},
                            {kDen, 0, 0, 0, kDen, 0}, {1e20f, 0, 0, 0, 1e20f, 0}};
const float kComs[][3] = {{0, 0, 0}, {60, -40, 10}, {3e38f, 3e38f, -3e38f}, {kDen, 0, 0}, {-0.f, 0, 0}, {1e20f, -1e20f, 1e20f}};
const float kTauMax[][3] = {{kInf, 120, 60}, {kInf, kInf, kInf}, {kDen, kDen, kDen}, {3e38f, 1e-30f, 1}, {1, 1, 1}};

std::vector<LrmLegDimensions> legs_n(size_t n) {
    std::vector<LrmLegDimensions> legs(n);
    for (size_t l = 0; l < n; ++l) {
        if (l % 2) lrm_get_moonbot_leg(0.7853982f * (float)l, &legs[l]);
        else lrm_get_M2_leg(0.7853982f * (float)l, &legs[l]);
    }
    return legs;
}

// bit k of `form` keeps optional argument k: pose_idx, com, plane, live_in, peak_at, load, tau, ms
void loads(size_t nlegs, size_t nsets, size_t nmasks, unsigned form, size_t variant) {
    const auto legs = legs_n(nlegs);
    std::vector<float> quats(&kQuats[0][0], &kQuats[0][0] + 4 * kNQuats), angles(3 * nlegs * nsets);
    for (size_t i = 0; i < angles.size(); ++i)  // mostly plain angles; one in five hostile
        angles[i] = (i + variant) % 5 == 3 ? kAngles[(i / 5 + variant) % kNAngles] : kAngles[(i * 7 + variant) % 6];
    std::vector<int32_t> pose(nsets);
    for (size_t s = 0; s < nsets; ++s) pose[s] = s % 6 == 5 ? kBadIdx[(s / 6) % 6] : (int32_t)((s * 5 + variant) % kNQuats);
    std::vector<uint8_t> live(nsets), lift(nmasks);
    for (size_t s = 0; s < nsets; ++s) live[s] = (uint8_t)(s % 4 == 1 ? 0 : (s % 4 == 2 ? 255 : 1));
    for (size_t m = 0; m < nmasks; ++m) lift[m] = (uint8_t)((m * 37 + variant) & ((1u << nlegs) - 1u));
    std::vector<uint8_t> status(nmasks * nsets), hold(nmasks * nsets), at(nmasks * nsets);
    std::vector<float> peak(nmasks * nsets), load(nmasks * nlegs * nsets), tau(nmasks * nlegs * 3 * nsets);
    double ms = 0;
    auto opt = [&](unsigned k, auto* p) { return (form >> k) & 1u ? p : nullptr; };
    const size_t nsets_ok = (form & 1u) ? nsets : (nsets < kNQuats ? nsets : kNQuats);  // without pose_idx: nsets <= nposes
    OK(lrm_stance_loads_posed_cpu(quats.data(), kNQuats, legs.data(), nlegs, opt(0, pose.data()), nsets_ok, angles.data(),
                                  opt(1, kComs[variant % 6]), opt(2, kPlanes[variant % 7]), lift.data(), nmasks, kTauMax[variant % 5],
                                  opt(3, live.data()), status.data(), hold.data(), peak.data(), opt(4, at.data()), opt(5, load.data()),
                                  opt(6, tau.data()), opt(7, &ms)));
}

void refusals() {
    const auto legs = legs_n(8);
    std::vector<float> quats(&kQuats[0][0], &kQuats[0][0] + 4 * kNQuats), angles(3 * 6 * 4, 0.2f);
    std::vector<uint8_t> st(3 * 4), hd(3 * 4);
    std::vector<float> pk(3 * 4);
    const uint8_t lift[3] = {0, 1, 2};
    const float tau[3] = {kInf, 100, 50};
    struct Args {
        size_t nposes = kNQuats, nlegs = 6, nsets = 4, nmasks = 3;
        const float *q, *ang, *com = nullptr, *plane = nullptr, *tau;
        const LrmLegDimensions* lg;
        const uint8_t* lift;
        uint8_t *st, *hd;
        float* pk;
    };
    Args base;
    base.q = quats.data(), base.ang = angles.data(), base.tau = tau, base.lg = legs.data(), base.lift = lift;
    base.st = st.data(), base.hd = hd.data(), base.pk = pk.data();
    auto call = [&](const Args& x) {
        return lrm_stance_loads_posed_cpu(x.q, x.nposes, x.lg, x.nlegs, nullptr, x.nsets, x.ang, x.com, x.plane, x.lift, x.nmasks, x.tau, nullptr,
                                          x.st, x.hd, x.pk, nullptr, nullptr, nullptr, nullptr);
    };
    auto with = [&](auto&& edit) {
        Args x = base;
        edit(x);
        return call(x);
    };
    OK(call(base));
    // the range checks and the scalars, before the no-op
    REFUSED(with([](Args& x) { x.nlegs = 0, x.nsets = 0; }));
    REFUSED(with([](Args& x) { x.nlegs = 9, x.nsets = 0; }));
    for (size_t nm : {(size_t)0, (size_t)257, (size_t)1 << 40}) REFUSED(with([nm](Args& x) { x.nmasks = nm, x.nsets = 0; }));
    REFUSED(with([](Args& x) { x.nposes = (size_t)1 << 31, x.nsets = 0; }));
    REFUSED(with([](Args& x) { x.nsets = (size_t)1 << 31; }));
    REFUSED(with([](Args& x) { x.nsets = ((size_t)UINT32_MAX) / (3 * 6 * 3) + 1; }));
    REFUSED(with([](Args& x) { x.lift = nullptr, x.nsets = 0; }));
    const uint8_t high[3] = {0, 64, 2};
    REFUSED(with([&](Args& x) { x.lift = high, x.nsets = 0; }));
    REFUSED(with([](Args& x) { x.tau = nullptr, x.nsets = 0; }));
    for (int k = 0; k < 3; ++k)
        for (float v : {kNan, 0.f, -0.f, -1.f, -kInf}) {
            float bad[3] = {1, 1, 1};
            bad[k] = v;
            REFUSED(with([&bad](Args& x) { x.tau = bad, x.nsets = 0; }));
        }
    for (int k = 0; k < 3; ++k)
        for (float v : {kNan, kInf, -kInf}) {
            float bad[3] = {0, 0, 0};
            bad[k] = v;
            REFUSED(with([&bad](Args& x) { x.com = bad, x.nsets = 0; }));
        }
    for (int k = 0; k < 6; ++k)
        for (float v : {kNan, kInf}) {
            float bad[6] = {1, 0, 0, 0, 1, 0};
            bad[k] = v;
            REFUSED(with([&bad](Args& x) { x.plane = bad, x.nsets = 0; }));
        }
    REFUSED(with([](Args& x) { x.nsets = kNQuats + 1; }));  // without pose_idx, set s takes pose s
    // nsets == 0 is a no-op, whatever the pointers
    OK(with([](Args& x) { x.nsets = 0, x.q = x.ang = nullptr, x.lg = nullptr, x.st = x.hd = nullptr, x.pk = nullptr; }));
    // the NULL forms
    REFUSED(with([](Args& x) { x.q = nullptr; }));
    REFUSED(with([](Args& x) { x.lg = nullptr; }));
    REFUSED(with([](Args& x) { x.ang = nullptr; }));
    REFUSED(with([](Args& x) { x.st = nullptr; }));
    REFUSED(with([](Args& x) { x.hd = nullptr; }));
    REFUSED(with([](Args& x) { x.pk = nullptr; }));
}

} // namespace

int main() {
    for (size_t nlegs = 1; nlegs <= 8; ++nlegs)
        for (size_t nsets : {(size_t)1, (size_t)2 * kNQuats + 3})
            for (unsigned form : {0u, 0xffu, 0xaau, 0x55u, 0x03u}) loads(nlegs, nsets, 1 + nlegs, form, nlegs + form);
    for (unsigned k = 0; k < 8; ++k) loads(6, 31, 7, 0xffu & ~(1u << k), k);  // every optional pointer NULL alone
    for (size_t nm : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)256})
        for (size_t variant = 0; variant < 35; ++variant) loads(8, 23, nm, 0xffu, variant);  // every plane x com x tau_max
    for (size_t variant = 0; variant < 35; ++variant) loads(3, 9, 8, 0xffu, variant);
    refusals();
    if (g_failures) {
        std::fprintf(stderr, "san_loads_main: %d call(s) did not return as documented\n", g_failures);
        return 1;
    }
    std::printf("san_loads_main: every call returned as documented\n");
    return 0;
}
