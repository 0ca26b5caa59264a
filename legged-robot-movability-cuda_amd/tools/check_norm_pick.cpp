// check_norm_pick -- lrm_norm_sums_less(A, B) (csrc/lrm_point.h: the pick of two norms from their sums) against the expression it
// replaces, sqrtf(A) < sqrtf(B), on the host build.  Both rewritten picks go through it: the yaw-limit alternative
// (norm(p) > norm(lim), i.e. the arguments swapped) and the fix-up's pick of the two yaw candidates (norm(a) < norm(b)).
//   check_norm_pick constructed      equal sums, neighbours, neighbours that share a root, the gap's two sides, specials
//   check_norm_pick random N [seed]  N pairs: half of them log-uniform and independent, half a few ulps apart
// Prints one line per class and "MODE: N pairs, M mismatches"; exit status 1 on a mismatch.  Plain g++, no HIP
// (tests/test_norm_pick_cpu.py builds and runs it).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "lrm_point.h"

static unsigned long long g_pairs = 0, g_bad = 0, g_by_sums = 0, g_by_roots = 0, g_shared_root = 0;

static void one(float A, float B) {
    const bool want = sqrtf(A) < sqrtf(B);
    const bool got = lrm_norm_sums_less(A, B);
    // what lrm_norm_sums_less does inside, restated for the class counts
    const bool plain = ((lrm_f2u(A) - 0x0f800000u) < 0x60000000u) && ((lrm_f2u(B) - 0x0f800000u) < 0x60000000u);
    const bool sums = plain && ((A < B * LRM_NORM_GAP) || (A >= B));
    g_pairs++;
    if (sums) g_by_sums++;
    else g_by_roots++;
    if (A != B && sqrtf(A) == sqrtf(B)) g_shared_root++;
    if (want != got) {
        if (g_bad < 10) printf("mismatch: A = %a (0x%08x), B = %a (0x%08x): roots say %d, sums say %d\n", A, lrm_f2u(A), B, lrm_f2u(B), (int)want, (int)got);
        g_bad++;
    }
}
static void both(float A, float B) {
    one(A, B);
    one(B, A);
}

static int finish(const char* mode) {
    printf("decided by the sums: %llu, by the roots: %llu, unequal sums with one root: %llu\n", g_by_sums, g_by_roots, g_shared_root);
    printf("%s: %llu pairs, %llu mismatches\n", mode, g_pairs, g_bad);
    return g_bad ? 1 : 0;
}

static int constructed() {
    std::vector<float> bases;
    // sums across the exponent range: both edges of the interval the sums decide in (2^-96, 2^96), denormals, the largest floats
    for (int e = -149; e <= 127; e += 1)
        for (float m : {1.0f, 1.0000001f, 1.2599210f, 1.4142135f, 1.9999999f}) bases.push_back(ldexpf(m, e));
    for (uint32_t u : {0x0f800000u, 0x0f7fffffu, 0x0f800001u, 0x6f800000u, 0x6f7fffffu, 0x6f800001u, 0x00800000u, 0x007fffffu, 0x00000001u, 0x7f7fffffu})
        bases.push_back(lrm_u2f(u));
    unsigned long long equal = 0, neighbours = 0, shared = 0, gap = 0;
    for (float A : bases) {
        both(A, A);
        equal++;
        const uint32_t ua = lrm_f2u(A);
        for (uint32_t d = 1; d <= 4; d++) { // neighbouring floats on both sides
            if (ua + d < 0x7f800000u) both(A, lrm_u2f(ua + d)), neighbours++;
            if (ua >= d) both(A, lrm_u2f(ua - d)), neighbours++;
        }
        // upward from A: every sum that still has A's root, and the first one whose root differs
        if (A > 0 && ua + 64 < 0x7f800000u) {
            const float ra = sqrtf(A);
            uint32_t u = ua + 1;
            while (sqrtf(lrm_u2f(u)) == ra) both(A, lrm_u2f(u++)), shared++;
            both(A, lrm_u2f(u));
        }
        // the gap: A against the floats around B * (1 - 2^-20) and around B / (1 - 2^-20)
        const float lo = A * LRM_NORM_GAP, hi = A / LRM_NORM_GAP;
        for (float g : {lo, hi}) {
            const uint32_t ug = lrm_f2u(g);
            if (!(g > 0) || ug + 40 >= 0x7f800000u || ug < 40) continue;
            for (int d = -32; d <= 32; d++) both(A, lrm_u2f(ug + (uint32_t)d)), gap++;
        }
    }
    const float inf = INFINITY, nan = NAN;
    const float specials[] = {0.0f, -0.0f, lrm_u2f(1u), lrm_u2f(0x007fffffu), lrm_u2f(0x00800000u), 1.0f, 3.0e38f, inf, -inf, nan, -1.0f, -nan, 1.0e-30f, 1.0e30f};
    unsigned long long special = 0;
    for (float A : specials)
        for (float B : specials) one(A, B), special++;
    printf("equal %llu, neighbours %llu, same root %llu, around the gap %llu, specials %llu\n", equal, neighbours, shared, gap, special);
    if (!equal || !neighbours || !shared || !gap || !special || !g_shared_root || !g_by_sums || !g_by_roots) {
        printf("a class is empty\n");
        return 2;
    }
    return finish("constructed");
}

static int random_pairs(unsigned long long n, unsigned seed) {
    std::mt19937_64 rng(seed);
    for (unsigned long long i = 0; i < n; i++) {
        const uint64_t r = rng();
        // a positive finite pattern, exponents spread over the whole range
        const uint32_t ua = (uint32_t)(r % 0x7f800000u);
        uint32_t ub;
        if (i & 1) ub = (uint32_t)((r >> 32) % 0x7f800000u);
        else { // a few ulps to a few thousand ulps apart: the cases the roots have to decide, and the gap's neighbourhood
            const int32_t d = (int32_t)((r >> 32) & 0x3fff) - 0x2000;
            const int64_t v = (int64_t)ua + ((r >> 50) & 1 ? d : d / 512);
            ub = (uint32_t)(v < 0 ? 0 : (v >= 0x7f800000 ? 0x7f7fffff : v));
        }
        one(lrm_u2f(ua), lrm_u2f(ub));
    }
    return finish("random");
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "constructed")) return constructed();
    if (argc >= 3 && !strcmp(argv[1], "random")) return random_pairs(strtoull(argv[2], nullptr, 10), argc >= 4 ? (unsigned)atoi(argv[3]) : 1u);
    fprintf(stderr, "usage: check_norm_pick constructed | random N [seed]\n");
    return 2;
}
