// Exhaustive / large-sample comparison of csrc/lrm_exact_math.h (host build) with this machine's libm.
//   make -C ../csrc check-exact-math          (g++ -O2 -std=c++17 -mfma -ffp-contract=off -pthread, into csrc/build/)
//   ./check_exact_math sincos [THREADS]          every float with |x| < 120 (2.2e9 values), both results
//   ./check_exact_math atan [THREADS]            every one of the 2^32 floats through atanf
//   ./check_exact_math atanpos [THREADS]         the 2^31 non-negative patterns and every 257th negative one (lrm_atan2f
//                                                only ever passes fabsf(y / x): the negative half is on no product path)
//   ./check_exact_math atan2 [PAIRS [THREADS]]   pseudo-random and structured (y, x) pairs, 6e8 unless PAIRS says otherwise
//   ./check_exact_math pairs FILE [THREADS]      atan2f on the (y, x) float pairs of a binary file (y0 x0 y1 x1 ...)
// THREADS: std::thread workers, default min(16, cores).  The values compared do not depend on it: the work is cut into
// fixed chunks, and a chunk of the random mode seeds its own generator from its number.
// (-mfma: glibc selects its FMA build of sincosf on AVX2 hosts; see the header of lrm_exact_math.h.)
// tests/test_exact_math_cpu.py builds and runs it; the last line of every mode is "MODE: N values, M mismatches".
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>
#include "lrm_exact_math.h"

static bool same(float a, float b) { return lrm_f2u(a) == lrm_f2u(b) || (a != a && b != b); }

static std::mutex g_print;
struct Tally {
    unsigned long n = 0, bad = 0;
};
static std::atomic<unsigned long> g_reported{0};
static bool report_slot() { return g_reported.fetch_add(1) < 5; }

static void check_sincos(float x, Tally& t) {
    if (!(fabsf(x) < 120.f)) return;
    float s0, c0, s1, c1;
    sincosf(x, &s0, &c0);
    lrm_sincosf(x, &s1, &c1);
    t.n++;
    if (!same(s0, s1) || !same(c0, c1)) {
        if (report_slot()) {
            std::lock_guard<std::mutex> lk(g_print);
            printf("sincosf %a (0x%08x): (%a, %a) vs (%a, %a)\n", x, lrm_f2u(x), s0, c0, s1, c1);
        }
        t.bad++;
    }
}
static void check_atan(float x, Tally& t) {
    t.n++;
    const float want = atanf(x), got = lrm_atanf(x);
    if (!same(want, got)) {
        if (report_slot()) {
            std::lock_guard<std::mutex> lk(g_print);
            printf("atanf %a (0x%08x): %a vs %a\n", x, lrm_f2u(x), want, got);
        }
        t.bad++;
    }
}
static void check_atan2(float y, float x, Tally& t) {
    t.n++;
    const float want = atan2f(y, x), got = lrm_atan2f(y, x);
    if (!same(want, got)) {
        if (report_slot()) {
            std::lock_guard<std::mutex> lk(g_print);
            printf("atan2f(%a, %a) (0x%08x, 0x%08x): %a vs %a\n", y, x, lrm_f2u(y), lrm_f2u(x), want, got);
        }
        t.bad++;
    }
}

constexpr uint64_t kChunk = 1ull << 20; // work items per chunk

// the random mode's pairs of chunk c: a xorshift64 stream seeded from the chunk number (splitmix64), four kinds in turn
static void atan2_chunk(uint64_t c, uint64_t lo, uint64_t hi, Tally& t) {
    uint64_t z = 88172645463325252ull + (c + 1) * 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    uint64_t st = (z ^ (z >> 31)) | 1ull;
    for (uint64_t i = lo; i < hi; i++) {
        st ^= st << 13; st ^= st >> 7; st ^= st << 17;
        const uint32_t a = (uint32_t)st, b = (uint32_t)(st >> 32);
        float y, x;
        switch (i % 4) {
        case 0: y = lrm_u2f(a); x = lrm_u2f(b); break;
        case 1: y = (int32_t)a * (1.0f / 4194304.0f); x = (int32_t)b * (1.0f / 4194304.0f); break;
        case 2: y = (int32_t)a * (1.0f / 4194304.0f); x = (b & 1) ? 1.0f : ((b & 2) ? 0.0f : -0.0f); break;
        default:
            y = (a & 7) == 0 ? 0.0f : (int32_t)a * 1e-3f;
            x = (int32_t)b * 1e-3f;
            if ((a & 0xf0) == 0) y = INFINITY;
            if ((b & 0xf00) == 0) x = -INFINITY;
        }
        check_atan2(y, x, t);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* mode = argv[1];
    enum { SINCOS, ATAN, ATANPOS, ATAN2, PAIRS } m;
    if (!strcmp(mode, "sincos")) m = SINCOS;
    else if (!strcmp(mode, "atan")) m = ATAN;
    else if (!strcmp(mode, "atanpos")) m = ATANPOS;
    else if (!strcmp(mode, "atan2")) m = ATAN2;
    else if (!strcmp(mode, "pairs")) m = PAIRS;
    else return 2;
    int arg = 2;
    uint64_t items = 1ull << 32;
    std::vector<float> pairs;
    if (m == ATANPOS) items = (1ull << 31) + ((1ull << 31) + 256) / 257;
    if (m == ATAN2) items = argc > arg ? strtoull(argv[arg++], nullptr, 10) : 600000000ull;
    if (m == PAIRS) {
        if (argc <= arg) return 2;
        FILE* f = fopen(argv[arg++], "rb");
        if (!f) { perror("pairs file"); return 2; }
        float buf[4096];
        size_t got;
        while ((got = fread(buf, sizeof(float), 4096, f)) > 0) pairs.insert(pairs.end(), buf, buf + got);
        fclose(f);
        if (pairs.size() % 2) { fprintf(stderr, "pairs file: odd number of floats\n"); return 2; }
        items = pairs.size() / 2;
    }
    int threads = (int)std::thread::hardware_concurrency();
    threads = threads < 1 ? 1 : (threads > 16 ? 16 : threads);
    if (argc > arg) threads = atoi(argv[arg++]);
    if (threads < 1 || argc > arg) return 2;

    const uint64_t nchunks = (items + kChunk - 1) / kChunk;
    std::atomic<uint64_t> next{0};
    std::vector<Tally> tallies((size_t)threads);
    auto work = [&](int ti) {
        Tally t; // a local tally: no cache line shared between workers
        for (uint64_t c = next.fetch_add(1); c < nchunks; c = next.fetch_add(1)) {
            const uint64_t lo = c * kChunk, hi = lo + kChunk < items ? lo + kChunk : items;
            switch (m) {
            case SINCOS: for (uint64_t u = lo; u < hi; u++) check_sincos(lrm_u2f((uint32_t)u), t); break;
            case ATAN: for (uint64_t u = lo; u < hi; u++) check_atan(lrm_u2f((uint32_t)u), t); break;
            case ATANPOS: // item i < 2^31: pattern i; the others: the negative patterns 0x80000000 + 257 k
                for (uint64_t i = lo; i < hi; i++)
                    check_atan(lrm_u2f((uint32_t)(i < (1ull << 31) ? i : (1ull << 31) + 257 * (i - (1ull << 31)))), t);
                break;
            case ATAN2: atan2_chunk(c, lo, hi, t); break;
            case PAIRS: for (uint64_t i = lo; i < hi; i++) check_atan2(pairs[2 * i], pairs[2 * i + 1], t); break;
            }
        }
        tallies[(size_t)ti] = t;
    };
    if (threads == 1) work(0);
    else {
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; t++) pool.emplace_back(work, t);
        for (auto& th : pool) th.join();
    }
    unsigned long n = 0, bad = 0;
    for (const Tally& t : tallies) { n += t.n; bad += t.bad; }
    printf("%s: %lu values, %lu mismatches\n", mode, n, bad);
    return bad != 0;
}
