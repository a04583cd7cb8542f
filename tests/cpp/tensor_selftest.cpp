// tensor_selftest.cpp -- host replay of the ciphertext tensor sum's scalar chains (hexl-fpga_amd/csrc/f64_arith.hpp ts_operand / ts_mac /
// ts_finish, called by ct_tensor.hip k_ct_tensor_sum) against unsigned __int128, as lincomb_selftest.cpp replays the linear
// combination's: IEEE-754 double mul / add / fma / rint round the same way on x86 (-mfma) and on gfx950, so the kernel's own source is
// checked here at operands no GPU test enumerates. The word loop below is the kernel's: four operand words per term, three partial sums,
// the cross term as two multiply-accumulates.
//   usage: tensor_selftest <draws> <modulus>...      (tests/test_ct_tensor_abi.py builds it: g++ -O2 -mfma -ffp-contract=off)
// Per modulus q and for every number of terms 1 ... 8:
//   worst case   every term the SAME four words, over {q - 1, q/2 - 1, q/2, q/2 + 1, 1, 0}^4: all products of a sum have one sign, so
//                every partial sum sits at its bound -- with eight terms of (q - 1, q - 1, q - 1, q - 1) and its neighbours beside q/2
//   random       <draws> sums of pseudo-random words, three in eight with an edge value somewhere or everywhere
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

static double g_op = 0, g_prod = 0, g_sum = 0, g_acc = 0;       // largest |operand| / p, |product| / p, |acc + product| and |acc| / p seen
static long g_cases = 0;

static double operand(uint64_t x, const hxf::Mod m) {
    const double r = hxf::ts_operand(hxf::to_f64(x), m);
    CHECK(__builtin_fabs(r) <= m.p / 2 + 2, "operand not centred: %.0f", r);
    if (__builtin_fabs(r) / m.p > g_op) g_op = __builtin_fabs(r) / m.p;
    return r;
}

static double mac(double acc, double a, double b, const hxf::Mod m) {
    const double prod = hxf::mul_mod(a, b, m), s = acc + prod;
    if (__builtin_fabs(prod) / m.p > g_prod) g_prod = __builtin_fabs(prod) / m.p;
    if (__builtin_fabs(s) > g_sum) g_sum = __builtin_fabs(s);
    const double r = hxf::ts_mac(acc, a, b, m);
    CHECK(__builtin_fabs(r) <= m.p / 2 + 2, "partial sum not centred: %.0f", r);
    if (__builtin_fabs(r) / m.p > g_acc) g_acc = __builtin_fabs(r) / m.p;
    return r;
}

// one output word of each component: T terms of (a0, a1, b0, b1) = x[t][0..3]
static void one(uint64_t q, const hxf::Mod m, int T, const uint64_t (*x)[4]) {
    u128 want[3] = {0, 0, 0};
    double d[3] = {0.0, 0.0, 0.0};
    for (int t = 0; t < T; ++t) {
        const uint64_t* w = x[t];
        want[0] = (want[0] + (u128)w[0] * w[2]) % q;
        want[1] = (want[1] + (u128)w[0] * w[3] % q + (u128)w[1] * w[2] % q) % q;
        want[2] = (want[2] + (u128)w[1] * w[3]) % q;
        const double a0 = operand(w[0], m), a1 = operand(w[1], m), b0 = operand(w[2], m), b1 = operand(w[3], m);
        d[0] = mac(d[0], a0, b0, m);
        d[1] = mac(mac(d[1], a0, b1, m), a1, b0, m);
        d[2] = mac(d[2], a1, b1, m);
    }
    for (int k = 0; k < 3; ++k) {
        const double r = hxf::ts_finish(d[k], m);
        CHECK(r >= 0 && r < m.p && hxf::from_f64(r) == (uint64_t)want[k], "q=%lu T=%d component %d words (%lu %lu %lu %lu) got %.0f want %lu", q, T, k,
              x[0][0], x[0][1], x[0][2], x[0][3], r, (uint64_t)want[k]);
    }
    ++g_cases;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: tensor_selftest <draws> <modulus>...\n"); return 2; }
    const long draws = std::atol(argv[1]);
    for (int k = 2; k < argc; ++k) {
        const uint64_t q = std::strtoull(argv[k], nullptr, 10);
        CHECK(q > 2 && q < (1ull << 52), "modulus %lu outside (2, 2^52)", q);
        const hxf::Mod m{(double)q, 1.0 / (double)q};
        const std::vector<uint64_t> edge = {q - 1, q / 2 - 1, q / 2, q / 2 + 1, 1, 0};
        uint64_t x[8][4];
        for (int T = 1; T <= 8; ++T) {
            // worst case: all terms alike -- one sign per component, the partial sums at their bound
            for (uint64_t e0 : edge)
                for (uint64_t e1 : edge)
                    for (uint64_t e2 : edge)
                        for (uint64_t e3 : edge) {
                            for (int t = 0; t < T; ++t) { x[t][0] = e0; x[t][1] = e1; x[t][2] = e2; x[t][3] = e3; }
                            one(q, m, T, x);
                        }
            for (long it = 0; it < draws; ++it) {
                const uint64_t r = rnd();
                for (int t = 0; t < T; ++t)
                    for (int c = 0; c < 4; ++c) x[t][c] = rnd() % q;
                // three draws in eight pin a word, a term, or all of them to edge values
                if ((r & 7) == 1) x[(r >> 3) % T][(r >> 6) & 3] = edge[(r >> 8) % edge.size()];
                if ((r & 7) == 2)
                    for (int c = 0; c < 4; ++c) x[(r >> 3) % T][c] = edge[rnd() % edge.size()];
                if ((r & 7) == 3)
                    for (int t = 0; t < T; ++t)
                        for (int c = 0; c < 4; ++c) x[t][c] = edge[rnd() % edge.size()];
                one(q, m, T, x);
            }
        }
    }
    std::printf("ts_operand / ts_mac / ts_finish (%d moduli, %ld word triples): max |operand| = %.4f p, max |product| = %.4f p (bound 0.875), "
                "max |partial sum| = %.4f p, max |acc + product| = 2^%.3f (limit 2^53)\n", argc - 2, g_cases, g_op, g_prod, g_acc, log2(g_sum));
    CHECK(g_prod <= 0.875, "a product beyond 0.875 p");
    CHECK(g_sum < 9007199254740992.0, "acc + product reaches 2^53");
    std::printf(failures ? "TENSOR SELFTEST: %d FAILURE(S)\n" : "TENSOR SELFTEST: ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
