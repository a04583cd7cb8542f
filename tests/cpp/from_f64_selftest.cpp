// from_f64_selftest.cpp -- host replay of the round-and-reduce chain of hexl_rns_from_f64 / hexl_ckks_encode
// (hexl-fpga_amd/csrc/f64_arith.hpp f64_to_residue, called by ckks_encode.hip k_rns_from_f64) against __int128, as pt_mul_selftest.cpp
// replays the plaintext multiply's: IEEE-754 double mul / add / fma / rint round the same way on x86 (-mfma) and on gfx950.
//   usage: from_f64_selftest <draws per binade> <modulus>...    (tests/test_encode_abi.py builds it: g++ -O2 -mfma -ffp-contract=off)
// Per modulus q and for both signs: 0.0, 0.5, 1.5, 2.5 (ties to even), 2^52 - 0.5, 2^53 + 2, 2^62 - 1024, k q and k q +- 1 for k up to
// 2^10, and <draws> pseudo-random doubles in every binade [2^e, 2^(e+1)), e = -2 ... 61. The expected integer is found WITHOUT rint:
// floor and the ties-to-even rule on the exact fraction.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../hexl-fpga_amd/csrc/f64_arith.hpp"

typedef __int128 i128;
static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures < 20) { std::printf("FAIL line %d: ", __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static long g_cases = 0;
static double g_max = 0;      // largest |result| / p

// round to nearest, ties to even, of a finite double below 2^62 in magnitude, as an exact integer
static int64_t round_even(double c) {
    const double f = __builtin_floor(c);          // exact
    const double frac = c - f;                    // exact: both share c's exponent range or f == c
    int64_t r = (int64_t)f;
    if (frac > 0.5 || (frac == 0.5 && (r & 1))) ++r;
    return r;
}

static void one(uint64_t q, const hxf::Mod m, double c) {
    const int64_t r = round_even(c);
    i128 w = (i128)r % (i128)q;
    if (w < 0) w += q;
    const bool ok = hxf::f64_int_in_range(__builtin_rint(c));
    CHECK(ok, "q=%lu c=%a flagged as out of range", q, c);
    const double t = hxf::f64_to_residue(c, m);
    const double l = hxf::lift(t, m);
    CHECK(__builtin_fabs(t) <= m.p / 2 + 2, "q=%lu c=%a: residue %.0f not centred", q, c, t);
    CHECK(l >= 0 && l < m.p && hxf::from_f64(l) == (uint64_t)w, "q=%lu c=%a (integer %ld): got %.0f want %lu", q, c, (long)r, l, (uint64_t)w);
    uint64_t bits;
    std::memcpy(&bits, &l, 8);
    CHECK(bits >> 63 == 0 || l != 0.0, "q=%lu c=%a: the canonical word is -0.0", q, c);
    if (__builtin_fabs(t) / m.p > g_max) g_max = __builtin_fabs(t) / m.p;
    ++g_cases;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: from_f64_selftest <draws per binade> <modulus>...\n"); return 2; }
    const long draws = std::atol(argv[1]);
    const double two52 = 4503599627370496.0, two62 = 4611686018427387904.0;
    CHECK(!hxf::f64_int_in_range(two62) && !hxf::f64_int_in_range(-two62) && !hxf::f64_int_in_range(__builtin_nan("")) &&
          !hxf::f64_int_in_range(__builtin_inf()) && !hxf::f64_int_in_range(9223372036854775808.0), "the range predicate accepts 2^62, NaN or inf");
    for (int k = 2; k < argc; ++k) {
        const uint64_t q = std::strtoull(argv[k], nullptr, 10);
        CHECK(q > 2 && q < (1ull << 52), "modulus %lu outside (2, 2^52)", q);
        const hxf::Mod m{(double)q, 1.0 / (double)q};
        const double fixed[] = {0.0, 0.5, 1.5, 2.5, two52 - 0.5, 2 * two52 + 2, two62 - 1024};
        for (double v : fixed) { one(q, m, v); one(q, m, -v); }
        for (uint64_t kq = 0; kq <= 1024; ++kq)
            for (int d = -1; d <= 1; ++d) {
                const i128 v = (i128)kq * q + d;               // below 2^62; as a double only when it is one exactly
                const double dv = (double)(int64_t)v;
                if ((i128)(int64_t)dv != v) continue;
                one(q, m, dv); one(q, m, -dv);
            }
        for (int e = -2; e < 62; ++e)
            for (long it = 0; it < draws; ++it) {
                const uint64_t bits = ((uint64_t)(1023 + e) << 52) | (rnd() >> 12) | ((rnd() & 1) << 63);
                double c;
                std::memcpy(&c, &bits, 8);
                one(q, m, c);
            }
    }
    std::printf("f64_to_residue (%d moduli, %ld cases): max |residue| = %.4f p (bound 0.5 + 2/p)\n", argc - 2, g_cases, g_max);
    std::printf(failures ? "FROM_F64 SELFTEST: %d FAILURE(S)\n" : "FROM_F64 SELFTEST: ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
