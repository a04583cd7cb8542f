// pt_mul_selftest.cpp -- host replay of the plaintext multiply's scalar chains (hexl-fpga_amd/csrc/f64_arith.hpp pt_mul / pt_mul_acc,
// called by rns_ops.hip k_pt_mul) against unsigned __int128, as f64_selftest.cpp replays the rescale's: IEEE-754 double mul / add / fma /
// rint round the same way on x86 (-mfma) and on gfx950, so the kernel's own source is checked here at operands no GPU test enumerates.
//   usage: pt_mul_selftest <draws> <modulus>...      (tests/test_rns_ops_abi.py builds it: g++ -O2 -mfma -ffp-contract=off)
// Per modulus q: both factors and the previous output word over {0, 1, q - 1, q/2 - 1, q/2, q/2 + 1} (every triple), then <draws>
// pseudo-random triples. The intermediates are recomputed with the same primitives to track the bounds the header documents.
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

static double g_prod = 0, g_sum = 0;      // largest |mul_mod result| / p and largest |product + prev| seen
static long g_cases = 0;

static void one(uint64_t q, const hxf::Mod m, uint64_t c, uint64_t t, uint64_t prev) {
    const double cd = hxf::to_f64(c), td = hxf::to_f64(t), pd = hxf::to_f64(prev);
    const uint64_t want = (uint64_t)((u128)c * t % q), want_acc = (uint64_t)(((u128)c * t + prev) % q);
    const double r = hxf::pt_mul(cd, td, m), ra = hxf::pt_mul_acc(cd, td, pd, m);
    CHECK(r >= 0 && r < m.p && hxf::from_f64(r) == want, "pt_mul q=%lu c=%lu t=%lu got %.0f want %lu", q, c, t, r, want);
    CHECK(ra >= 0 && ra < m.p && hxf::from_f64(ra) == want_acc, "pt_mul_acc q=%lu c=%lu t=%lu prev=%lu got %.0f want %lu", q, c, t, prev, ra, want_acc);
    // the intermediates: operands of mul_mod centred, its result within 0.7p, the sum with prev exact below 2^53
    const double a = hxf::reduce(cd, m), b = hxf::reduce(td, m), u = hxf::mul_mod(a, b, m), s = hxf::pt_mul_centred(cd, td, m) + pd;
    CHECK(__builtin_fabs(a) <= m.p / 2 + 2 && __builtin_fabs(b) <= m.p / 2 + 2, "operands not centred q=%lu c=%lu t=%lu", q, c, t);
    CHECK(__builtin_fabs(u) <= 0.7 * m.p + 2, "mul_mod result beyond 0.7p q=%lu c=%lu t=%lu u=%.0f", q, c, t, u);
    if (__builtin_fabs(u) / m.p > g_prod) g_prod = __builtin_fabs(u) / m.p;
    if (__builtin_fabs(s) > g_sum) g_sum = __builtin_fabs(s);
    ++g_cases;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: pt_mul_selftest <draws> <modulus>...\n"); return 2; }
    const long draws = std::atol(argv[1]);
    for (int k = 2; k < argc; ++k) {
        const uint64_t q = std::strtoull(argv[k], nullptr, 10);
        CHECK(q > 2 && q < (1ull << 52), "modulus %lu outside (2, 2^52)", q);
        const hxf::Mod m{(double)q, 1.0 / (double)q};
        const std::vector<uint64_t> edge = {0, 1, q - 1, q / 2 - 1, q / 2, q / 2 + 1};
        for (uint64_t c : edge)
            for (uint64_t t : edge)
                for (uint64_t prev : edge) one(q, m, c, t, prev);
        for (long it = 0; it < draws; ++it) {
            const uint64_t r = rnd();
            // three draws in eight pin one of the three words to an edge value
            const uint64_t c = (r & 7) == 1 ? edge[(r >> 3) % edge.size()] : rnd() % q;
            const uint64_t t = (r & 7) == 2 ? edge[(r >> 3) % edge.size()] : rnd() % q;
            const uint64_t prev = (r & 7) == 3 ? edge[(r >> 3) % edge.size()] : rnd() % q;
            one(q, m, c, t, prev);
        }
    }
    std::printf("pt_mul / pt_mul_acc (%d moduli, %ld cases): max |mul_mod| = %.4f p (bound 0.7), max |product + prev| = 2^%.3f (limit 2^53)\n",
                argc - 2, g_cases, g_prod, log2(g_sum));
    CHECK(g_sum < 9007199254740992.0, "product + prev reaches 2^53");
    std::printf(failures ? "PT_MUL SELFTEST: %d FAILURE(S)\n" : "PT_MUL SELFTEST: ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
