// lincomb_selftest.cpp -- host replay of the ciphertext linear combination's scalar chains (hexl-fpga_amd/csrc/f64_arith.hpp lc_term /
// lc_add / lc_finish, called by rns_ops.hip k_ct_lincomb) against unsigned __int128, as pt_mul_selftest.cpp replays the plaintext
// multiply's: IEEE-754 double mul / add / fma / rint round the same way on x86 (-mfma) and on gfx950, so the kernel's own source is checked
// here at operands no GPU test enumerates. The weights are prepared as hexl_ct_lincomb prepares them (centred, and fl(w / q)), and the
// word loop below is the kernel's: a weight of exactly 1 adds the word as it is, the plaintext word and the constant come last.
//   usage: lincomb_selftest <draws> <modulus>...      (tests/test_ct_lincomb_abi.py builds it: g++ -O2 -mfma -ffp-contract=off)
// Per modulus q and for every number of terms 1 ... 8:
//   worst case   every word and every weight of the sum the SAME value, over {q - 1, q/2 - 1, q/2, q/2 + 1, 1} x the same set: all terms of
//                one sign, so every partial sum sits at its bound; with and without the plaintext word and the constant, at their edges
//   weight 1     the path without the multiply, explicit (weight word 1) -- NULL weights are the same code -- on edge and random words
//   random       <draws> sums of pseudo-random words and weights, three in eight with an edge value somewhere
// The intermediates are tracked against the bounds the header documents.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../hexl-fpga_amd/csrc/f64_arith.hpp"

typedef unsigned __int128 u128;
static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures < 20) { std::printf("FAIL line %d: ", __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static double g_term = 0, g_sum = 0, g_acc = 0;     // largest |lc_term| / p, |acc + u| and |acc| / p seen
static long g_cases = 0, g_ones = 0;

// hexl_internal.hpp hx_centre: residue v < q as the centred double in (-q/2, q/2]
static double centre(uint64_t v, uint64_t q) { return v > q / 2 ? (double)v - (double)q : (double)v; }

static double add(double acc, double u, const hxf::Mod m) {
    const double s = acc + u;
    CHECK(__builtin_fabs(u) <= m.p, "addend beyond p: %.0f", u);
    if (__builtin_fabs(s) > g_sum) g_sum = __builtin_fabs(s);
    const double r = hxf::lc_add(acc, u, m);
    CHECK(__builtin_fabs(r) <= m.p / 2 + 2, "partial sum not centred: %.0f", r);
    if (__builtin_fabs(r) / m.p > g_acc) g_acc = __builtin_fabs(r) / m.p;
    return r;
}

// one output word: T terms, pt / cst < 0 = absent
static void one(uint64_t q, const hxf::Mod m, int T, const uint64_t* x, const uint64_t* w, int64_t pt, int64_t cst) {
    u128 want = 0;
    double acc = 0.0;
    for (int t = 0; t < T; ++t) {
        want = (want + (u128)x[t] * w[t]) % q;
        const double wc = centre(w[t], q), wp = wc / (double)q;
        double u = hxf::to_f64(x[t]);
        if (wc == 1.0) ++g_ones;
        else {
            u = hxf::lc_term(u, wc, wp, m);
            if (__builtin_fabs(u) / m.p > g_term) g_term = __builtin_fabs(u) / m.p;
        }
        acc = add(acc, u, m);
    }
    if (pt >= 0) { want = (want + (uint64_t)pt) % q; acc = add(acc, hxf::to_f64((uint64_t)pt), m); }
    if (cst >= 0) { want = (want + (uint64_t)cst) % q; acc = add(acc, centre((uint64_t)cst, q), m); }
    const double r = hxf::lc_finish(acc, m);
    CHECK(r >= 0 && r < m.p && hxf::from_f64(r) == (uint64_t)want, "q=%lu T=%d x0=%lu w0=%lu pt=%ld cst=%ld got %.0f want %lu", q, T, x[0], w[0],
          (long)pt, (long)cst, r, (uint64_t)want);
    ++g_cases;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: lincomb_selftest <draws> <modulus>...\n"); return 2; }
    const long draws = std::atol(argv[1]);
    for (int k = 2; k < argc; ++k) {
        const uint64_t q = std::strtoull(argv[k], nullptr, 10);
        CHECK(q > 2 && q < (1ull << 52), "modulus %lu outside (2, 2^52)", q);
        const hxf::Mod m{(double)q, 1.0 / (double)q};
        const std::vector<uint64_t> edge = {q - 1, q / 2 - 1, q / 2, q / 2 + 1, 1, 0};
        const std::vector<int64_t> addend = {-1, 0, (int64_t)(q - 1), (int64_t)(q / 2), (int64_t)(q / 2 + 1)};
        uint64_t x[8], w[8];
        for (int T = 1; T <= 8; ++T) {
            // worst case: all terms alike -- one sign, the partial sums at their bound
            for (uint64_t xe : edge)
                for (uint64_t we : edge) {
                    for (int t = 0; t < T; ++t) { x[t] = xe; w[t] = we; }
                    for (int64_t pt : addend)
                        for (int64_t cst : addend) one(q, m, T, x, w, pt, cst);
                }
            // the weight-1 path on random words (edge words: above, we = 1)
            for (long it = 0; it < draws / 8; ++it) {
                for (int t = 0; t < T; ++t) { x[t] = rnd() % q; w[t] = 1; }
                one(q, m, T, x, w, it & 1 ? (int64_t)(rnd() % q) : -1, it & 2 ? (int64_t)(rnd() % q) : -1);
            }
            for (long it = 0; it < draws; ++it) {
                const uint64_t r = rnd();
                for (int t = 0; t < T; ++t) { x[t] = rnd() % q; w[t] = rnd() % q; }
                // three draws in eight pin a word, a weight, or all of them to edge values
                if ((r & 7) == 1) x[(r >> 3) % T] = edge[(r >> 8) % edge.size()];
                if ((r & 7) == 2) w[(r >> 3) % T] = edge[(r >> 8) % edge.size()];
                if ((r & 7) == 3)
                    for (int t = 0; t < T; ++t) { x[t] = edge[rnd() % edge.size()]; w[t] = edge[rnd() % edge.size()]; }
                one(q, m, T, x, w, r & 16 ? (int64_t)(rnd() % q) : -1, r & 32 ? (int64_t)(rnd() % q) : -1);
            }
        }
    }
    std::printf("lc_term / lc_add / lc_finish (%d moduli, %ld sums, %ld terms of weight 1): max |term| = %.4f p (bound 1), max |partial sum| = "
                "%.4f p, max |acc + u| = 2^%.3f (limit 2^53)\n", argc - 2, g_cases, g_ones, g_term, g_acc, log2(g_sum));
    CHECK(g_term <= 1.0, "a term beyond p");
    CHECK(g_sum < 9007199254740992.0, "acc + u reaches 2^53");
    CHECK(g_ones > 0, "the weight-1 path never ran");
    std::printf(failures ? "LINCOMB SELFTEST: %d FAILURE(S)\n" : "LINCOMB SELFTEST: ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
