// A stand-alone driver for the sanitizer build of the trunk-leg clearance HOST code (csrc/Makefile, target `sanitize-trunk`;
// tests/test_trunk_sanitize_cpu.py builds and runs it), in the manner of san_main.cpp: lrm_trunk_clearance_posed_cpu and
// lrm_dbg_trunk_link_dist_host on a hostile corpus -- nan, zero, non-unit, huge and infinite quaternions; angles outside the
// sincos range, nan, inf and 1e30; pose indices out of range (INT32_MIN, INT32_MAX, -1, one past the end); every link mask;
// cylinders of radius 0, a denormal thickness and 3e38; every optional pointer NULL; one to eight legs; every refusal of the
// contract; links with every combination of hostile coordinates.  The host loop is the bit-exact reference of the device
// kernel and shares its arithmetic header, so this is the out-of-bounds and undefined-behaviour check that arithmetic gets.
// Every buffer is a heap block of exactly the documented size.  Only return codes are checked: outputs are the business of the
// other tests.  No GPU is touched.
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
        std::fprintf(stderr, "san_trunk_main: %.*s returned %d, expected %d (%s)\n", (int)std::strcspn(what, "("), what, rc, want, lrm_last_error());
        ++g_failures;
    }
}
#define OK(call) expect((call), LRM_OK, #call)
#define REFUSED(call) expect((call), LRM_EINVAL, #call)

constexpr float kInf = std::numeric_limits<float>::infinity();
constexpr float kNan = std::numeric_limits<float>::quiet_NaN();
constexpr float kDen = std::numeric_limits<float>::denorm_min();

const float kQuats[][4] = {{1, 0, 0, 0}, {0.9238795f, 0, 0.3826834f, 0}, {0.5f, 0.5f, 0.5f, 0.5f}, {0.8f, -0.2f, 0.1f, 0.5567764f},
                           {kNan, 0, 0, 0}, {1, kNan, kNan, kNan}, {0, 0, 0, 0}, {0.5f, 0.5f, 0.5f, 0.1f}, {3, -2, 1, 4},
                           {1e30f, 1e30f, -1e30f, 1e30f}, {kInf, 0, 0, 0}, {1, -kInf, 0, 0}, {kDen, kDen, 0, 0}, {3e38f, 3e38f, 3e38f, 3e38f},
                           {1e-19f, 1e-19f, 0, 0}, {1e-10f, 0, 1e-10f, 0}};
constexpr size_t kNQuats = sizeof(kQuats) / sizeof(kQuats[0]);
const float kAngles[] = {0.3f, -0.7f, 200.f, -200.f, 1e30f, -1e30f, kInf, -kInf, kNan, 4e9f, 2147483648.f, kDen, 3e38f, 1e-3f, -2.0f, 1.1f,
                         119.99f, -119.99f, 120.f, -120.f};
constexpr size_t kNAngles = sizeof(kAngles) / sizeof(kAngles[0]);
const int32_t kBadIdx[] = {INT32_MIN, INT32_MAX, -1, 0, 1, 2, 3, -2, 1 << 30, INT32_MIN + 1, (int32_t)kNQuats, (int32_t)kNQuats - 1};
constexpr size_t kNBadIdx = sizeof(kBadIdx) / sizeof(kBadIdx[0]);
const float kTrunks[][3] = {{186.f, 40.f, -80.f}, {0.f, 40.f, -80.f}, {186.f, kDen, 0.f}, {3e38f, 3e38f, -3e38f}, {kDen, 1e-30f, -1e-30f},
                            {1e30f, 1.f, 0.f}};

std::vector<LrmLegDimensions> legs_n(size_t n) {
    std::vector<LrmLegDimensions> legs(n);
    for (size_t l = 0; l < n; ++l) {
        if (l % 2) lrm_get_moonbot_leg(0.7853982f * (float)l, &legs[l]);
        else lrm_get_M2_leg(0.7853982f * (float)l, &legs[l]);
    }
    return legs;
}

// every set count from 0 on, with blocks of exactly the documented size
void posed(size_t nlegs, size_t nsets, bool with_idx, bool with_live, bool with_pen, bool with_free) {
    const auto legs = legs_n(nlegs);
    std::vector<float> quats(&kQuats[0][0], &kQuats[0][0] + 4 * kNQuats);
    const size_t nposes = with_idx ? kNQuats : (nsets > kNQuats ? nsets : kNQuats);
    quats.resize(4 * nposes);
    for (size_t p = kNQuats; p < nposes; ++p) std::memcpy(&quats[4 * p], kQuats[p % kNQuats], 4 * sizeof(float));
    std::vector<float> angles(3 * nlegs * nsets);
    for (size_t i = 0; i < angles.size(); ++i) angles[i] = kAngles[(i * 7 + i / 3) % kNAngles];
    for (size_t i = 0; i + 2 < angles.size(); i += 9) { angles[i] = 0.4f; angles[i + 1] = -0.9f; angles[i + 2] = -1.3f; }  // some valid legs
    std::vector<int32_t> idx(nsets);
    for (size_t s = 0; s < nsets; ++s) idx[s] = s % 3 ? (int32_t)(s % kNQuats) : kBadIdx[s % kNBadIdx];
    std::vector<uint8_t> live(nsets);
    for (size_t s = 0; s < nsets; ++s) live[s] = (uint8_t)(s % 4 == 1 ? 0 : (s % 4 == 2 ? 255 : 1));
    std::vector<uint8_t> hit(nlegs * nsets), worst(nlegs * nsets), fr(nsets);
    std::vector<float> pen(nlegs * nsets);
    const float radius[3] = {28.f, 22.f, 16.f}, thin[3] = {0.f, kDen, 3e38f};
    double ms = 0;
    for (const auto& t : kTrunks)
        for (unsigned links = 0; links < 8; ++links)
            for (const float* r : {radius, thin})
                OK(lrm_trunk_clearance_posed_cpu(quats.data(), nposes, legs.data(), nlegs, with_idx ? idx.data() : nullptr, nsets, angles.data(), r,
                                                 links % 2 ? 0.f : 10.f, links % 3 ? 30.f : 0.f, t[0], t[1], t[2], (uint8_t)links,
                                                 with_live ? live.data() : nullptr, hit.data(), worst.data(), with_pen ? pen.data() : nullptr,
                                                 with_free ? fr.data() : nullptr, links % 2 ? &ms : nullptr));
}

void refusals() {
    const auto legs = legs_n(6);
    const size_t n = 4;
    std::vector<float> quats(&kQuats[0][0], &kQuats[0][0] + 4 * n), angles(3 * 6 * n, 0.1f);
    std::vector<uint8_t> hit(6 * n), worst(6 * n);
    const float radius[3] = {28.f, 22.f, 16.f}, neg[3] = {28.f, -1.f, 16.f}, nanr[3] = {kNan, 1.f, 1.f}, infr[3] = {1.f, 1.f, kInf};
    auto call = [&](size_t nposes, size_t nlegs, size_t nsets, const float* r, float margin, float tip, float R, float pz, float mz, unsigned links,
                    uint8_t* h, uint8_t* w, const float* ang) {
        return lrm_trunk_clearance_posed_cpu(quats.data(), nposes, legs.data(), nlegs, nullptr, nsets, ang, r, margin, tip, R, pz, mz, (uint8_t)links,
                                             nullptr, h, w, nullptr, nullptr, nullptr);
    };
    OK(call(n, 6, n, radius, 0.f, 0.f, 186.f, 40.f, -80.f, 6, hit.data(), worst.data(), angles.data()));
    OK(call(n, 6, 0, radius, 0.f, 0.f, 186.f, 40.f, -80.f, 6, nullptr, nullptr, nullptr));  // nsets == 0 is a no-op
    REFUSED(call(n, 0, n, radius, 0.f, 0.f, 186.f, 40.f, -80.f, 6, hit.data(), worst.data(), angles.data()));
    REFUSED(call(n, 9, n, radius, 0.f, 0.f, 186.f, 40.f, -80.f, 6, hit.data(), worst.data(), angles.data()));
    REFUSED(call(n, 6, (size_t)1 << 31, radius, 0.f, 0.f, 186.f, 40.f, -80.f, 6, hit.data(), worst.data(), angles.data()));
    REFUSED(call((size_t)1 << 31, 6, n, radius, 0.f, 0.f, 186.f, 40.f, -80.f, 6, hit.data(), worst.data(), angles.data()));
    REFUSED(call(n, 6, n + 1, radius, 0.f, 0.f, 186.f, 40.f, -80.f, 6, hit.data(), worst.data(), angles.data()));
    for (const float* r : {(const float*)nullptr, neg, nanr, infr})
        REFUSED(call(n, 6, n, r, 0.f, 0.f, 186.f, 40.f, -80.f, 6, hit.data(), worst.data(), angles.data()));
    for (float bad : {-1.f, kNan, kInf}) {
        REFUSED(call(n, 6, n, radius, bad, 0.f, 186.f, 40.f, -80.f, 6, hit.data(), worst.data(), angles.data()));
        REFUSED(call(n, 6, n, radius, 0.f, bad, 186.f, 40.f, -80.f, 6, hit.data(), worst.data(), angles.data()));
        REFUSED(call(n, 6, n, radius, 0.f, 0.f, bad, 40.f, -80.f, 6, hit.data(), worst.data(), angles.data()));
    }
    for (float bad : {kNan, kInf, -kInf}) {
        REFUSED(call(n, 6, n, radius, 0.f, 0.f, 186.f, bad, -80.f, 6, hit.data(), worst.data(), angles.data()));
        REFUSED(call(n, 6, n, radius, 0.f, 0.f, 186.f, 40.f, bad, 6, hit.data(), worst.data(), angles.data()));
    }
    REFUSED(call(n, 6, n, radius, 0.f, 0.f, 186.f, -80.f, -80.f, 6, hit.data(), worst.data(), angles.data()));
    REFUSED(call(n, 6, n, radius, 0.f, 0.f, 186.f, -80.f, 40.f, 6, hit.data(), worst.data(), angles.data()));
    for (unsigned links : {8u, 14u, 128u, 255u})
        REFUSED(call(n, 6, n, radius, 0.f, 0.f, 186.f, 40.f, -80.f, links, hit.data(), worst.data(), angles.data()));
    REFUSED(call(n, 6, 0, radius, 0.f, 0.f, 186.f, 40.f, -80.f, 8, nullptr, nullptr, nullptr));  // checked before the no-op
    REFUSED(call(n, 6, n, radius, 0.f, 0.f, 186.f, 40.f, -80.f, 6, nullptr, worst.data(), angles.data()));
    REFUSED(call(n, 6, n, radius, 0.f, 0.f, 186.f, 40.f, -80.f, 6, hit.data(), nullptr, angles.data()));
    REFUSED(call(n, 6, n, radius, 0.f, 0.f, 186.f, 40.f, -80.f, 6, hit.data(), worst.data(), nullptr));
    REFUSED(lrm_trunk_clearance_posed_cpu(nullptr, n, legs.data(), 6, nullptr, n, angles.data(), radius, 0.f, 0.f, 186.f, 40.f, -80.f, 6, nullptr,
                                          hit.data(), worst.data(), nullptr, nullptr, nullptr));
    REFUSED(lrm_trunk_clearance_posed_cpu(quats.data(), n, nullptr, 6, nullptr, n, angles.data(), radius, 0.f, 0.f, 186.f, 40.f, -80.f, 6, nullptr,
                                          hit.data(), worst.data(), nullptr, nullptr, nullptr));
}

void link_distance() {
    const float v[] = {0.f, -0.f, kDen, -kDen, 1e30f, -1e30f, 3e38f, -3e38f, kInf, -kInf, kNan, 150.f, -30.f, 40.f, 1e-39f, 600.f};
    std::vector<float> segs;  // A from the cross product of the hostile values, B from a shifted walk through them
    const size_t nv = sizeof(v) / sizeof(v[0]);
    size_t k = 0;
    for (float a : v) for (float b : v) for (float c : v) {
        segs.insert(segs.end(), {a, b, c, v[k % nv], v[(k / 3 + 5) % nv], v[(k / 7 + 11) % nv]});
        ++k;
    }
    std::vector<float> out(segs.size() / 6);
    for (const auto& t : kTrunks) OK(lrm_dbg_trunk_link_dist_host(segs.data(), out.size(), t[0], t[1], t[2], out.data()));
    OK(lrm_dbg_trunk_link_dist_host(segs.data(), out.size(), kNan, kInf, -kInf, out.data()));  // the scalars are not checked here
    OK(lrm_dbg_trunk_link_dist_host(nullptr, 0, 1.f, 1.f, 0.f, nullptr));
    REFUSED(lrm_dbg_trunk_link_dist_host(nullptr, 3, 1.f, 1.f, 0.f, out.data()));
    REFUSED(lrm_dbg_trunk_link_dist_host(segs.data(), 3, 1.f, 1.f, 0.f, nullptr));
}

} // namespace

int main() {
    for (size_t nlegs = 1; nlegs <= 8; ++nlegs)
        for (size_t nsets : {(size_t)0, (size_t)1, (size_t)33})
            for (int form : {0, 5, 10, 15}) posed(nlegs, nsets, form & 1, form & 2, form & 4, form & 8);
    refusals();
    link_distance();
    if (g_failures) {
        std::fprintf(stderr, "san_trunk_main: %d call(s) did not return as documented\n", g_failures);
        return 1;
    }
    std::printf("san_trunk_main: every call returned as documented\n");
    return 0;
}
