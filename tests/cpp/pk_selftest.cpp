// pk_selftest.cpp -- host build of the public-key encryption chain of hexl-fpga_amd/csrc/sample_core.hpp (pk_operand / pk_product /
// pk_c0 / pk_c1), the source k_pk_encrypt (rlwe.hip) compiles: IEEE-754 double mul / add / fma / rint round the same way on x86 (-mfma)
// and on gfx950, so the kernel's own code is checked here at operands no GPU test enumerates.
//   usage: pk_selftest <draws> <modulus>...      (tests/test_pk_selftest.py builds it: g++ -O2 -mfma -ffp-contract=off)
//   per modulus q: c0 = (pk0 u + e0 + pt) mod q and c1 = (pk1 u + e1) mod q against unsigned __int128, every operand over
//   {0, 1, q/2, q - 2, q - 1} in every position (5^6 cases), then <draws> random ones. The intermediate bounds the header states are
//   asserted on the way: factors and products |.| <= p/2 + 2 after their reduce, the raw product |mul_mod| <= 0.875p, every partial sum
//   in front of a reduce |.| <= 1.5p + 2 and below 2^53, results canonical.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../hexl-fpga_amd/csrc/sample_core.hpp"

typedef unsigned __int128 u128;
static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures < 20) { std::printf("FAIL line %d: ", __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static long g_cases = 0;
static double g_max_product = 0.0, g_max_sum = 0.0;      // relative to p

static bool centred(double x, const hxf::Mod m) { return __builtin_fabs(x) <= m.p / 2 + 2; }

// the chain once more with every intermediate in view: the same functions in the same order as pk_c0 / pk_c1
static void bounds(const hxf::Mod m, double pk0, double pk1, double u, double e0, double e1, double pt) {
    const double ur = hxs::pk_operand(u, m), k0 = hxs::pk_operand(pk0, m), k1 = hxs::pk_operand(pk1, m);
    CHECK(centred(ur, m) && centred(k0, m) && centred(k1, m), "a factor is not centred (p = %.0f)", m.p);
    const double raw[2] = {hxf::mul_mod(k0, ur, m), hxf::mul_mod(k1, ur, m)};
    const double add[2] = {e0, e1};
    for (int k = 0; k < 2; ++k) {
        const double r = __builtin_fabs(raw[k]) / m.p;
        if (r > g_max_product) g_max_product = r;
        CHECK(r <= 0.875, "|mul_mod| = %.3f p", r);
        const double prod = hxs::pk_product(k ? k1 : k0, ur, m);
        CHECK(centred(prod, m), "a product is not centred after its reduce");
        const double s1 = prod + add[k];
        CHECK(__builtin_fabs(s1) <= 1.5 * m.p + 2 && __builtin_fabs(s1) < 9007199254740992.0, "first sum %.0f", s1);
        if (__builtin_fabs(s1) / m.p > g_max_sum) g_max_sum = __builtin_fabs(s1) / m.p;
        const double a1 = hxf::lc_add(prod, add[k], m);
        CHECK(centred(a1, m), "first partial sum not centred");
        if (k == 0) {
            const double s2 = a1 + pt;
            CHECK(__builtin_fabs(s2) <= 1.5 * m.p + 2 && __builtin_fabs(s2) < 9007199254740992.0, "second sum %.0f", s2);
            if (__builtin_fabs(s2) / m.p > g_max_sum) g_max_sum = __builtin_fabs(s2) / m.p;
            CHECK(centred(hxf::lc_add(a1, pt, m), m), "second partial sum not centred");
        }
    }
}

static void one(uint64_t q, const hxf::Mod m, uint64_t pk0, uint64_t pk1, uint64_t u, uint64_t e0, uint64_t e1, uint64_t pt) {
    const uint64_t want0 = (uint64_t)(((u128)pk0 * u + e0 + pt) % q), want1 = (uint64_t)(((u128)pk1 * u + e1) % q);
    const double ur = hxs::pk_operand(hxf::to_f64(u), m);
    const double c0 = hxs::pk_c0(hxs::pk_operand(hxf::to_f64(pk0), m), ur, hxf::to_f64(e0), hxf::to_f64(pt), m);
    const double c1 = hxs::pk_c1(hxs::pk_operand(hxf::to_f64(pk1), m), ur, hxf::to_f64(e1), m);
    CHECK(c0 >= 0 && c0 < m.p && hxf::from_f64(c0) == want0, "pk_c0 q=%lu pk0=%lu u=%lu e0=%lu pt=%lu got %.0f want %lu", q, pk0, u, e0, pt, c0, want0);
    CHECK(c1 >= 0 && c1 < m.p && hxf::from_f64(c1) == want1, "pk_c1 q=%lu pk1=%lu u=%lu e1=%lu got %.0f want %lu", q, pk1, u, e1, c1, want1);
    bounds(m, hxf::to_f64(pk0), hxf::to_f64(pk1), hxf::to_f64(u), hxf::to_f64(e0), hxf::to_f64(e1), hxf::to_f64(pt));
    ++g_cases;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: pk_selftest <draws> <modulus>...\n"); return 2; }
    const long draws = std::atol(argv[1]);
    for (int k = 2; k < argc; ++k) {
        const uint64_t q = std::strtoull(argv[k], nullptr, 10);
        CHECK(q > 4 && q < (1ull << 52), "modulus %lu outside (4, 2^52)", q);
        const hxf::Mod m{(double)q, 1.0 / (double)q};
        const std::vector<uint64_t> edge = {0, 1, q / 2, q - 2, q - 1};
        for (uint64_t pk0 : edge) for (uint64_t pk1 : edge) for (uint64_t u : edge) for (uint64_t e0 : edge) for (uint64_t e1 : edge)
            for (uint64_t pt : edge) one(q, m, pk0, pk1, u, e0, e1, pt);
        // what the call really meets: a ternary mask (-1, 0, 1) and errors of magnitude <= 21 as residues, beside uniform key words
        const uint64_t small[] = {0, 1, 21, q - 21, q - 1};
        for (uint64_t u : {uint64_t(0), uint64_t(1), q - 1}) for (uint64_t e0 : small) for (uint64_t e1 : small)
            one(q, m, rnd() % q, rnd() % q, u, e0, e1, rnd() % q);
        for (long t = 0; t < draws; ++t) one(q, m, rnd() % q, rnd() % q, rnd() % q, rnd() % q, rnd() % q, rnd() % q);
    }
    std::printf("%ld cases, largest |mul_mod| = %.4f p, largest partial sum = %.4f p\n", g_cases, g_max_product, g_max_sum);
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL PASSED\n");
    return 0;
}
