// A stand-alone driver for sanitizer builds of the library's HOST code (csrc/Makefile, target `sanitize`;
// tests/test_host_sanitize_cpu.py builds and runs it).  It calls only host functions -- the single-leg entries, the debug
// twins of the table code, every posed *_cpu loop -- on a cloud that fills the leg's bounding cube and on a hostile corpus:
// every combination of +-0, denormals, +-1e30, +-3e38, +-inf, nan, 2^31 and 2^32 in the coordinates; nan, zero, non-unit, huge
// and infinite quaternions; nan, inf and 1e30 bodies; angles outside the sincos range; pose, leg, target, foot and edge
// indices out of range (INT32_MIN, INT32_MAX, -1, one past the end); CSR offsets that decrease, are negative or lie past the
// capacity; every optional pointer NULL in one pass.  Then eight threads build host tables of the same and of different
// (leg, quaternion), run the loops, switch the mode and read the last error.  The host loops are the bit-exact reference of
// the device kernels and share their arithmetic headers, so this is the out-of-bounds and undefined-behaviour check that
// arithmetic gets.  Every buffer is a heap block of exactly the documented size.  Only return codes are checked: outputs
// are the business of the other tests.  No GPU is touched.
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <thread>
#include <vector>

#include "lrm.h"

namespace {

std::atomic<int> g_failures{0};

void expect(int rc, int want, const char* what) {
    if (rc != want) {
        std::fprintf(stderr, "san_main: %.*s returned %d, expected %d (%s)\n", (int)std::strcspn(what, "("), what, rc, want, lrm_last_error());
        ++g_failures;
    }
}
#define OK(call) expect((call), LRM_OK, #call)
#define REFUSED(call) expect((call), LRM_EINVAL, #call)

using F3 = std::vector<float>;
constexpr float kInf = std::numeric_limits<float>::infinity();
constexpr float kNan = std::numeric_limits<float>::quiet_NaN();
constexpr float kDen = std::numeric_limits<float>::denorm_min();

F3 cube_cloud(size_t n, unsigned seed) { // uniform in the leg's bounding cube
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> x(-200.f, 700.f), y(-500.f, 500.f), z(-500.f, 300.f);
    F3 p(3 * n);
    for (size_t i = 0; i < n; ++i) { p[3 * i] = x(rng); p[3 * i + 1] = y(rng); p[3 * i + 2] = z(rng); }
    return p;
}

F3 hostile_cloud() { // the cross product of the hostile values in the three coordinates
    const float v[] = {0.f, -0.f, kDen, -kDen, 1e30f, -1e30f, 3e38f, -3e38f, kInf, -kInf, kNan, 2147483648.f, 4294967296.f, 1e-39f};
    F3 p;
    for (float a : v) for (float b : v) for (float c : v) { p.push_back(a); p.push_back(b); p.push_back(c); }
    return p;
}

const float kQuats[][4] = {{1, 0, 0, 0}, {0.9238795f, 0, 0.3826834f, 0}, {0.5f, 0.5f, 0.5f, 0.5f}, {0.8f, -0.2f, 0.1f, 0.5567764f},
                           {kNan, 0, 0, 0}, {1, kNan, kNan, kNan}, {0, 0, 0, 0}, {0.5f, 0.5f, 0.5f, 0.1f}, {3, -2, 1, 4},
                           {1e30f, 1e30f, -1e30f, 1e30f}, {kInf, 0, 0, 0}, {1, -kInf, 0, 0}, {kDen, kDen, 0, 0}, {3e38f, 3e38f, 3e38f, 3e38f}};
constexpr size_t kNQuats = sizeof(kQuats) / sizeof(kQuats[0]);
const float kBodies[][3] = {{0, 0, 0}, {120, -340, 60}, {-800, 500, -90}, {kNan, 0, 0}, {0, kInf, 0}, {-kInf, -kInf, -kInf}, {1e30f, 0, 0},
                            {0, 0, -1e30f}, {3e38f, 3e38f, 3e38f}, {2147483648.f, 4294967296.f, 0}, {kDen, -kDen, 0}, {4e6f, 4e6f, 0}};
constexpr size_t kNBodies = sizeof(kBodies) / sizeof(kBodies[0]);
const float kAngles[] = {0.3f, -0.7f, 200.f, -200.f, 1e30f, -1e30f, kInf, -kInf, kNan, 4e9f, 2147483648.f, kDen, 3e38f, 1e-3f, -2.0f, 1.1f};
constexpr size_t kNAngles = sizeof(kAngles) / sizeof(kAngles[0]);
const int32_t kBadIdx[] = {INT32_MIN, INT32_MAX, -1, 0, 1, 2, 3, -2, 1 << 30, INT32_MIN + 1};

std::vector<LrmLegDimensions> six_legs() {
    std::vector<LrmLegDimensions> legs(6);
    for (int l = 0; l < 6; ++l) {
        if (l % 2) lrm_get_moonbot_leg(1.0471976f * l, &legs[l]);
        else lrm_get_M2_leg(1.0471976f * l, &legs[l]);
    }
    return legs;
}

// ---- single-leg entries and the debug twins of the table code ----
void single_leg(const F3& pts, const LrmLegDimensions& leg, const float* quat, bool table_twins) {
    const size_t n = pts.size() / 3;
    std::vector<uint8_t> mask(n), valid(n), status(n);
    std::vector<uint32_t> doubt(n);
    F3 d(3 * n), ang(3 * n), tip(3 * n);
    uint32_t stats[5];
    double ms = 0;
    OK(lrm_reach_cpu(pts.data(), n, &leg, quat, mask.data(), &ms));
    OK(lrm_dist_cpu(pts.data(), n, &leg, quat, d.data(), valid.data(), &ms));
    OK(lrm_dist_cpu(pts.data(), n, &leg, quat, d.data(), nullptr, nullptr));
    OK(lrm_ik_cpu(pts.data(), n, &leg, quat, nullptr, ang.data(), status.data(), &ms));
    OK(lrm_ik_cpu(pts.data(), n, &leg, quat, pts.data(), ang.data(), status.data(), nullptr)); // hostile seeds
    OK(lrm_fk_cpu(ang.data(), n, &leg, quat, tip.data(), &ms));
    OK(lrm_fk_cpu(pts.data(), n, &leg, quat, tip.data(), nullptr)); // the cloud read as angles: far outside the sincos range
    if (table_twins) { // a (leg, quaternion) the tolerance mode cannot take is refused, not evaluated
        const int rc = lrm_dbg_toltab_host(pts.data(), n, &leg, quat, mask.data(), d.data(), doubt.data(), stats);
        if (rc != LRM_OK && rc != LRM_EINVAL) expect(rc, LRM_OK, "lrm_dbg_toltab_host");
        expect(lrm_dbg_xtab_host(pts.data(), n, &leg, quat, mask.data(), d.data(), doubt.data(), stats), rc, "lrm_dbg_xtab_host");
        expect(lrm_dbg_replay_host(pts.data(), n, &leg, quat, mask.data(), d.data(), doubt.data()), rc, "lrm_dbg_replay_host");
        if (rc == LRM_OK) {
            OK(lrm_dbg_toltab_host(pts.data(), n, &leg, quat, mask.data(), d.data(), doubt.data(), nullptr));
            OK(lrm_dbg_xtab_host(pts.data(), n, &leg, quat, mask.data(), d.data(), doubt.data(), nullptr));
        }
    }
}

void table_build(const LrmLegDimensions& leg, const float* quat) {
    size_t size = 0;
    float ms = 0;
    const int rc = lrm_dbg_toltab_build(&leg, quat, 0, nullptr, 0, &size, &ms); // the size alone
    if (rc != LRM_OK) { expect(rc, LRM_EINVAL, "lrm_dbg_toltab_build (refusal)"); return; }
    std::vector<uint8_t> buf(size);
    size_t again = 0;
    OK(lrm_dbg_toltab_build(&leg, quat, 0, buf.data(), buf.size(), &again, &ms));
    if (again != size) { std::fprintf(stderr, "san_main: table size %zu then %zu\n", size, again); ++g_failures; }
    if (size > 16) { // a buffer that is too small is left alone
        std::vector<uint8_t> small(size / 2);
        const int rs = lrm_dbg_toltab_build(&leg, quat, 0, small.data(), small.size(), &again, &ms);
        if (rs != LRM_OK && rs != LRM_EINVAL) expect(rs, LRM_OK, "lrm_dbg_toltab_build (small buffer)");
    }
}

// ---- the posed loops ----
struct Scene {
    F3 targets, quats, body, angles;
    std::vector<LrmLegDimensions> legs;
    size_t nt, np, nl;
    bool hostile;
};

Scene make_scene(const F3& targets, bool hostile, size_t np) {
    Scene s;
    s.targets = targets;
    s.nt = targets.size() / 3;
    s.np = np;
    s.hostile = hostile;
    s.legs = six_legs();
    s.nl = s.legs.size();
    for (size_t p = 0; p < np; ++p) {
        const float* q = kQuats[hostile ? p % kNQuats : p % 4];
        const float* b = kBodies[hostile ? (p * 5 + 1) % kNBodies : p % 3];
        s.quats.insert(s.quats.end(), q, q + 4);
        s.body.insert(s.body.end(), b, b + 3);
    }
    for (size_t i = 0; i < 3 * s.nl * np; ++i) s.angles.push_back(hostile ? kAngles[(i * 7 + i / 3) % kNAngles] : kAngles[i % 2] * (1 + i % 3) * 0.4f);
    return s;
}

void posed(const Scene& s, bool null_optionals) {
    const size_t nt = s.nt, np = s.np, nl = s.nl, rows = nl * np;
    static const float no_targets[3] = {0, 0, 0};
    const float* T = s.nt ? s.targets.data() : no_targets;
    const float* Q = s.quats.data();
    const float* B = null_optionals ? nullptr : s.body.data();
    const LrmLegDimensions* L = s.legs.data();
    double ms_store = 0;
    double* ms = null_optionals ? nullptr : &ms_store;
    F3 nominal_store(3 * nl);
    for (size_t l = 0; l < nl; ++l) { nominal_store[3 * l] = 250.f; nominal_store[3 * l + 1] = 30.f * l; nominal_store[3 * l + 2] = l == 3 ? kNan : -120.f; }
    const float* nominal = null_optionals ? nullptr : nominal_store.data();
    const size_t nbad = sizeof(kBadIdx) / sizeof(kBadIdx[0]);
    auto bad = [&](size_t i, size_t past) { return i % 3 == 0 ? kBadIdx[i % nbad] : i % 7 == 0 ? (int32_t)past : (int32_t)(i % (past ? past : 1)); };

    // per-query calls: n queries with their own pose, leg and target index
    const size_t n = nt;
    std::vector<int32_t> pose_idx(n), target_idx(n);
    std::vector<uint8_t> leg_idx(n), mask(n), valid(n), status(n);
    for (size_t i = 0; i < n; ++i) {
        pose_idx[i] = bad(i, np);
        target_idx[i] = bad(i + 1, nt);
        leg_idx[i] = i % 5 == 0 ? (uint8_t)(nl + i % 3) : i % 11 == 0 ? 255 : (uint8_t)(i % nl);
    }
    F3 d(3 * n), ang(3 * n), tip(3 * n);
    const int32_t* PI = null_optionals ? nullptr : pose_idx.data();
    const uint8_t* LI = null_optionals ? nullptr : leg_idx.data();
    OK(lrm_reach_dist_posed_cpu(T, n, PI, LI, Q, B, np, L, nl, mask.data(), valid.data(), d.data(), ms));
    OK(lrm_ik_posed_cpu(T, nt, null_optionals ? nullptr : target_idx.data(), n, PI, LI, Q, B, np, L, nl, null_optionals ? nullptr : T, ang.data(),
                        status.data(), ms));
    OK(lrm_fk_posed_cpu(ang.data(), n, PI, LI, Q, B, np, L, nl, tip.data(), ms));
    OK(lrm_fk_posed_cpu(T, n, PI, LI, Q, B, np, L, nl, tip.data(), ms)); // the cloud read as angles

    // footholds per (pose, leg), their lists, edges, misses and support
    std::vector<int32_t> count(rows), best(rows), written(rows), miss(rows), near(rows);
    F3 best_d2(rows), m2(rows), sx(rows), sy(rows), sz(rows);
    std::vector<uint8_t> all_legs(np);
    OK(lrm_footholds_posed_cpu(T, nt, Q, B, np, L, nl, nominal, count.data(), best.data(), null_optionals ? nullptr : best_d2.data(),
                               null_optionals ? nullptr : all_legs.data(), ms));
    std::vector<int64_t> offsets(rows + 1, 0);
    for (size_t i = 0; i < rows; ++i) offsets[i + 1] = offsets[i] + count[i];
    const size_t cap = (size_t)offsets[rows];
    for (int form = 0; form < 5; ++form) {
        std::vector<int64_t> off = offsets;
        size_t capacity = cap;
        if (form == 1) for (size_t i = 0; i <= rows; ++i) off[i] = offsets[rows - i];                 // decreasing
        if (form == 2) for (size_t i = 0; i <= rows; ++i) off[i] = i % 2 ? -(int64_t)i - 1 : INT64_MIN; // negative
        if (form == 3) for (size_t i = 0; i <= rows; ++i) off[i] = i % 2 ? (int64_t)cap + 1 + i : INT64_MAX - i; // past the capacity
        if (form == 4) capacity = cap / 2;                                                             // the segments' tail has no room
        std::vector<int32_t> idx(capacity ? capacity : 1);
        F3 d2(capacity ? capacity : 1);
        OK(lrm_foothold_lists_posed_cpu(T, nt, Q, B, np, L, nl, nominal, off.data(), capacity, idx.data(), null_optionals ? nullptr : d2.data(),
                                        null_optionals ? nullptr : written.data(), ms));
    }
    const size_t ne = 2 * np + 3;
    std::vector<int32_t> ea(ne), eb(ne), ecount(nl * ne), ebest(nl * ne);
    F3 ed2(nl * ne);
    std::vector<uint8_t> eall(ne);
    for (size_t e = 0; e < ne; ++e) { ea[e] = bad(e, np); eb[e] = bad(e + 2, np); }
    OK(lrm_foothold_edges_posed_cpu(T, nt, Q, B, np, L, nl, nominal, ea.data(), eb.data(), ne, ecount.data(), ebest.data(),
                                    null_optionals ? nullptr : ed2.data(), null_optionals ? nullptr : eall.data(), ms));
    for (float margin : {0.f, 100.f, kInf})
        OK(lrm_foothold_misses_posed_cpu(T, nt, Q, B, np, L, nl, margin, null_optionals ? nullptr : count.data(), miss.data(),
                                         null_optionals ? nullptr : m2.data(), null_optionals ? nullptr : sx.data(), null_optionals ? nullptr : sy.data(),
                                         null_optionals ? nullptr : sz.data(), null_optionals ? nullptr : near.data(), ms));
    std::vector<int32_t> scount(nl * nt), sbest(nl * nt);
    F3 sd2(nl * nt);
    std::vector<uint8_t> smask(nt), live(np);
    for (size_t p = 0; p < np; ++p) live[p] = p % 4 == 1 ? 0 : (uint8_t)(p % 3 ? 1 : 0xA5);
    const uint8_t* LIVE = null_optionals ? nullptr : live.data();
    OK(lrm_foothold_support_posed_cpu(T, nt, Q, B, np, L, nl, nominal, LIVE, scount.data(), sbest.data(), null_optionals ? nullptr : sd2.data(),
                                      null_optionals ? nullptr : smask.data(), ms));

    // body, leg and self clearance, the joints
    std::vector<int32_t> hits(np), top(np), lhits(rows), lworst(rows);
    F3 height(np), pen(rows), joints(12 * rows);
    std::vector<uint8_t> bfree(np), links(rows), with(rows), worst8(rows);
    OK(lrm_body_clearance_posed_cpu(T, nt, Q, B, np, L, nl, 180.f, 60.f, -50.f, -400.f, LIVE, hits.data(), top.data(),
                                    null_optionals ? nullptr : height.data(), null_optionals ? nullptr : bfree.data(), ms));
    const float radius[3] = {28.f, 22.f, 16.f}, thick[3] = {90.f, 0.f, 3e38f};
    const float* A = s.angles.data();
    for (float tip_clear : {0.f, 30.f, 3e38f}) {
        OK(lrm_leg_joints_posed_cpu(A, Q, B, np, L, nl, tip_clear, joints.data(), ms));
        for (const float* r : {radius, thick})
            for (float margin : {0.f, 10.f, 3e38f}) {
                OK(lrm_leg_clearance_posed_cpu(T, nt, Q, B, np, L, nl, A, r, margin, tip_clear, LIVE, lhits.data(), links.data(), lworst.data(),
                                               null_optionals ? nullptr : pen.data(), null_optionals ? nullptr : bfree.data(), ms));
                OK(lrm_self_clearance_posed_cpu(Q, np, L, nl, nullptr, np, A, r, margin, tip_clear, LIVE, lhits.data(), with.data(), links.data(),
                                                worst8.data(), null_optionals ? nullptr : pen.data(), null_optionals ? nullptr : bfree.data(), ms));
            }
    }
    std::vector<int32_t> set_pose(np);
    for (size_t i = 0; i < np; ++i) set_pose[i] = bad(i, np);
    OK(lrm_self_clearance_posed_cpu(Q, np, L, nl, set_pose.data(), np, A, radius, 10.f, 30.f, LIVE, lhits.data(), with.data(), links.data(),
                                    worst8.data(), pen.data(), bfree.data(), ms));

    // stances: one target index per leg, lift sets, a centre of mass and a plane
    const size_t ns = np + 5, nm = 6;
    std::vector<int32_t> foot(nl * ns), spose(ns);
    for (size_t i = 0; i < nl * ns; ++i) foot[i] = bad(i + 1, nt);
    for (size_t i = 0; i < ns; ++i) spose[i] = bad(i, np);
    const uint8_t lift[nm] = {0, 1, 0x2A, 0x15, 0x3F, 0x20}; // a bit at or above nlegs is refused
    const float com[3] = {10.f, s.hostile ? 1e30f : -5.f, 20.f}, nan_com[3] = {kNan, 0.f, 0.f}; // a com that is not finite is refused
    const float plane[6] = {1, 0, 0, 0, s.hostile ? 0.f : 1.f, 0};
    F3 margin_out(nm * ns);
    std::vector<uint8_t> edge(nm * ns), stable(nm * ns), feet(ns), slive(ns, 1);
    slive[1] = 0;
    REFUSED(lrm_stance_stability_cpu(T, nt, Q, B, np, nullptr, foot.data(), np, nl, nan_com, nullptr, lift, nm, 5.f, nullptr, margin_out.data(), nullptr,
                                     stable.data(), nullptr, nullptr));
    OK(lrm_stance_stability_cpu(T, nt, Q, B, np, null_optionals ? nullptr : spose.data(), foot.data(), null_optionals ? np : ns, nl,
                                null_optionals ? nullptr : com, null_optionals ? nullptr : plane, lift, nm, 5.f, null_optionals ? nullptr : slive.data(),
                                margin_out.data(), null_optionals ? nullptr : edge.data(), stable.data(), null_optionals ? nullptr : feet.data(), ms));
}

// block checksums of the exact-math layer: the call's worker threads write disjoint sums, between sentinels
void checksums() {
    const uint64_t guard = 0x5a5a5a5a5a5a5a5aull;
    for (int fn = 0; fn < 3; ++fn) {
        std::vector<uint64_t> sums(5, guard);
        OK(lrm_dbg_exact_math_sums_host(fn, 0x3f7f, 3, sums.data() + 1));
        OK(lrm_dbg_exact_math_sums_host(fn, 65535, 1, sums.data() + 1));
        OK(lrm_dbg_exact_math_sums_host(fn, 7, 0, sums.data() + 1));
        if (sums[0] != guard || sums[4] != guard) { std::fprintf(stderr, "san_main: a checksum outside its range\n"); ++g_failures; }
    }
    OK(lrm_dbg_exact_math_sums_host(0, 0, 0, nullptr));
    REFUSED(lrm_dbg_exact_math_sums_host(3, 0, 1, nullptr));
    REFUSED(lrm_dbg_exact_math_sums_host(0, 65535, 2, nullptr));
    REFUSED(lrm_dbg_exact_math_sums_host(0, 0, 1, nullptr));
}

void pairs_and_bodies(const F3& good, const F3& hostile) {
    // link pairs read from the clouds, four points a pair
    for (const F3* c : {&good, &hostile}) {
        const size_t n = c->size() / 12;
        F3 out(n);
        OK(lrm_dbg_link_pair_dist_host(c->data(), n, out.data()));
    }
    OK(lrm_dbg_link_pair_dist_host(nullptr, 0, nullptr));
    REFUSED(lrm_dbg_link_pair_dist_host(nullptr, 3, nullptr));
    // lrm_footholds_cpu: bodies x targets under one orientation
    const auto legs = six_legs();
    const size_t nl = legs.size();
    for (const F3* bodies : {&good, &hostile}) {
        const size_t nb = 40, nt = 600;
        std::vector<int32_t> count(nl * nb), best(nl * nb);
        F3 d2(nl * nb), nominal(3 * nl, 100.f);
        double ms;
        for (size_t q = 0; q < kNQuats; q += 3) {
            OK(lrm_footholds_cpu(bodies->data(), nb, good.data(), nt, legs.data(), nl, kQuats[q], nominal.data(), count.data(), best.data(), d2.data(), &ms));
            OK(lrm_footholds_cpu(bodies->data(), nb, hostile.data(), nt, legs.data(), nl, kQuats[q], nullptr, count.data(), best.data(), nullptr, nullptr));
        }
        OK(lrm_footholds_cpu(bodies->data(), nb, good.data(), nt, legs.data(), nl, nullptr, nullptr, count.data(), best.data(), nullptr, nullptr));
    }
}

// ---- eight threads ----
void thread_body(int k, const F3* cloud, const Scene* scene) {
    LrmLegDimensions leg;
    lrm_get_M2_leg(k < 4 ? 0.f : 0.4f * k, &leg); // threads 0..3 build the table of one (leg, quaternion), the others their own
    const float* quat = kQuats[k < 4 ? 1 : k % 4];
    for (int round = 0; round < 2; ++round) {
        table_build(leg, quat);
        single_leg(*cloud, leg, quat, true);
        lrm_set_mode(k % 2 ? LRM_MODE_FAST : LRM_MODE_STRICT); // both run the same host code: the loops do not read the mode
        const int mode = lrm_get_mode();
        if (mode != LRM_MODE_FAST && mode != LRM_MODE_STRICT) { std::fprintf(stderr, "san_main: mode %d\n", mode); ++g_failures; }
        REFUSED(lrm_dbg_link_pair_dist_host(nullptr, 1 + k, nullptr));
        if (!lrm_last_error() || !lrm_last_error()[0]) { std::fprintf(stderr, "san_main: no error text after a refusal\n"); ++g_failures; }
        posed(*scene, round == 1);
    }
}

} // namespace

int main(int argc, char** argv) {
    const bool threads_only = argc > 1 && !std::strcmp(argv[1], "--threads-only");
    const F3 good = cube_cloud(6000, 42), hostile = hostile_cloud();
    if (!threads_only) {
        LrmLegDimensions m2, moon;
        lrm_get_M2_leg(0.f, &m2);
        lrm_get_moonbot_leg(-2.4f, &moon);
        for (size_t q = 0; q < kNQuats; ++q) {
            const bool tables = q < 3 || q == 4 || q == 6 || q == 9; // table builds of unit, nan, zero and huge quaternions
            single_leg(q % 2 ? hostile : good, q % 2 ? moon : m2, kQuats[q], tables);
            single_leg(q % 2 ? good : hostile, q % 2 ? m2 : moon, kQuats[q], false);
            if (tables) table_build(m2, kQuats[q]);
        }
        single_leg(hostile, m2, nullptr, true); // quat NULL: the identity
        table_build(moon, nullptr);
        pairs_and_bodies(good, hostile);
        checksums();
        const F3 few(good.begin(), good.begin() + 3 * 900);
        for (int hostile_poses = 0; hostile_poses < 2; ++hostile_poses)
            for (const F3* cloud : {&few, &hostile}) {
                const Scene s = make_scene(*cloud, hostile_poses != 0, hostile_poses ? kNQuats + 3 : 7);
                posed(s, false);
                posed(s, true);
            }
        const Scene none = make_scene(F3(), true, 5); // no targets at all
        posed(none, false);
    }
    {
        const F3 small(good.begin(), good.begin() + 3 * 1500), tiny(good.begin(), good.begin() + 3 * 200);
        const Scene s = make_scene(tiny, true, 9);
        std::vector<std::thread> pool;
        for (int k = 0; k < 8; ++k) pool.emplace_back(thread_body, k, &small, &s);
        for (auto& t : pool) t.join();
        lrm_set_mode(LRM_MODE_FAST);
        checksums(); // its own pool of workers, under the thread sanitizer too
    }
    if (g_failures) { std::fprintf(stderr, "san_main: %d unexpected return codes\n", g_failures.load()); return 1; }
    std::puts("san_main: every call returned as documented");
    return 0;
}
