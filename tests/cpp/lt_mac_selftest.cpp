// lt_mac_selftest.cpp -- host replay of the linear transform's scalar chain (hexl-fpga_amd/csrc/f64_arith.hpp lt_pt / lt_mac / lt_mac_acc,
// called by keyswitch_f64.hip k_ksf_mac_galois's plaintext modes and ckks_ops.hip k_galois_c0_pt) against unsigned __int128, as
// pt_mul_selftest.cpp replays the plaintext multiply's: IEEE-754 double mul / add / fma / rint round the same way on x86 (-mfma) and on gfx950.
//   usage: lt_mac_selftest <draws> <modulus>...      (tests/test_lt_model.py builds it: g++ -O2 -mfma -ffp-contract=off)
// Per modulus q: the plaintext word, the inner sum and the previous accumulator over {0, 1, q - 1, q/2 - 1, q/2, q/2 + 1} (every
// triple), then <draws> pseudo-random triples. The kernels hand the chain CENTRED inner sums and accumulators (outputs of reduce), so
// every residue is tried in both centred forms where two exist (x and x - q for x >= q/2 - 2: reduce may leave either within
// |.| <= q/2 + 2). The intermediates are recomputed with the same primitives to track the bounds the header documents.
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

static double g_prod = 0, g_sum = 0;      // largest |mul_mod result| / p and largest |prev + product| seen
static long g_cases = 0;

// the centred forms of residue x that a reduce output may take: |.| <= q/2 + 2
static int centred_forms(uint64_t x, uint64_t q, double out[2]) {
    int k = 0;
    const double xd = (double)x, qd = (double)q;
    if (xd <= qd / 2 + 2) out[k++] = xd;
    if (qd - xd <= qd / 2 + 2) out[k++] = xd - qd;
    return k;
}

static void one(uint64_t q, const hxf::Mod m, uint64_t t, uint64_t inner, uint64_t prev) {
    const uint64_t want = (uint64_t)((u128)t * inner % q), want_acc = (uint64_t)(((u128)t * inner + prev) % q);
    const double td = hxf::lt_pt(hxf::to_f64(t), m);
    CHECK(__builtin_fabs(td) <= m.p / 2 + 2, "plaintext word not centred q=%lu t=%lu", q, t);
    double in[2], pv[2];
    const int ni = centred_forms(inner, q, in), np = centred_forms(prev, q, pv);
    for (int a = 0; a < ni; ++a) {
        const double first = hxf::lt_mac(in[a], td, m);
        CHECK(__builtin_fabs(first) <= m.p / 2 + 2 && hxf::from_f64(hxf::lift(first, m)) == want,
              "lt_mac q=%lu t=%lu inner=%.0f got %.0f want %lu", q, t, in[a], first, want);
        const double u = hxf::mul_mod(td, in[a], m);
        CHECK(__builtin_fabs(u) <= 0.7 * m.p + 2, "mul_mod result beyond 0.7p q=%lu t=%lu inner=%.0f u=%.0f", q, t, in[a], u);
        if (__builtin_fabs(u) / m.p > g_prod) g_prod = __builtin_fabs(u) / m.p;
        for (int b = 0; b < np; ++b) {
            const double r = hxf::lt_mac_acc(in[a], td, pv[b], m);
            CHECK(__builtin_fabs(r) <= m.p / 2 + 2 && hxf::from_f64(hxf::lift(r, m)) == want_acc,
                  "lt_mac_acc q=%lu t=%lu inner=%.0f prev=%.0f got %.0f want %lu", q, t, in[a], pv[b], r, want_acc);
            const double s = pv[b] + u;
            if (__builtin_fabs(s) > g_sum) g_sum = __builtin_fabs(s);
            ++g_cases;
        }
    }
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: lt_mac_selftest <draws> <modulus>...\n"); return 2; }
    const long draws = std::atol(argv[1]);
    for (int k = 2; k < argc; ++k) {
        const uint64_t q = std::strtoull(argv[k], nullptr, 10);
        CHECK(q > 8 && q < (1ull << 52), "modulus %lu outside (8, 2^52)", q);
        const hxf::Mod m{(double)q, 1.0 / (double)q};
        const std::vector<uint64_t> edge = {0, 1, q - 1, q / 2 - 1, q / 2, q / 2 + 1};
        for (uint64_t t : edge)
            for (uint64_t inner : edge)
                for (uint64_t prev : edge) one(q, m, t, inner, prev);
        for (long it = 0; it < draws; ++it) {
            const uint64_t r = rnd();
            // three draws in eight pin one of the three words to an edge value
            const uint64_t t = (r & 7) == 1 ? edge[(r >> 3) % edge.size()] : rnd() % q;
            const uint64_t inner = (r & 7) == 2 ? edge[(r >> 3) % edge.size()] : rnd() % q;
            const uint64_t prev = (r & 7) == 3 ? edge[(r >> 3) % edge.size()] : rnd() % q;
            one(q, m, t, inner, prev);
        }
    }
    std::printf("lt_mac / lt_mac_acc (%d moduli, %ld cases): max |mul_mod| = %.4f p (bound 0.7), max |prev + product| = 2^%.3f (limit 2^53)\n",
                argc - 2, g_cases, g_prod, log2(g_sum));
    CHECK(g_sum < 9007199254740992.0, "prev + product reaches 2^53");
    std::printf(failures ? "LT_MAC SELFTEST: %d FAILURE(S)\n" : "LT_MAC SELFTEST: ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
