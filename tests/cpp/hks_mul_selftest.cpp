// hks_mul_selftest.cpp -- host replay of the scalar chains the hybrid multiply adds (hexl-fpga_amd/csrc/f64_arith.hpp hks_acc_pd /
// hks_down_rs, called by keyswitch_hybrid.hip k_hks_down_intt<., true> / k_hks_down<., true>) against unsigned __int128: IEEE-754 double mul / add / fma /
// rint round the same way on x86 (-mfma) and on gfx950, so the kernels' own source is checked here at operands no GPU test enumerates.
// A stand-alone program (tests/test_hks_mul_selftest.py builds it with -fsanitize=address,undefined).
//   usage: hks_mul_selftest <draws> <modulus>...
// acc_pd    acc' = acc + (P mod q) d: acc over the centred range of an hks_mac_term output INCLUDING its edges +-(q/2 + 2), d over the
//           canonical edge words (0, q - 1, beside q/2) and random, P mod q over edge residues and random
// down_rs   out = (acc + (P mod q) d - w) R^-1: the same, w a range-reduced transform output including +-(q/2 + 2), R^-1 any unit
// round     the rescaling source rows: hks_round on an hks_acc_pd output followed exactly (the inverse transform is linear, so the
//           chain is replayed on the value itself) with half = floor(R/2) mod q, also (q - 1) / 2: the value at a source limb, where R = 0
// The intermediates are tracked against the bounds the header documents.
#include <cmath>
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

static uint64_t mulmod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)((u128)a * b % q); }
static double centre(uint64_t v, uint64_t q) { return v > q / 2 ? (double)v - (double)q : (double)v; }
static hxf::Mod mod_of(uint64_t q) { return hxf::Mod{(double)q, 1.0 / (double)q}; }
// the residue in [0, q) of a centred double with |x| <= q/2 + 2
static uint64_t residue(double x, uint64_t q) { return (uint64_t)(((__int128)(long long)x % (__int128)q + q) % q); }

static double g_sum = 0, g_prod = 0, g_diff = 0;                  // largest |acc + product|, |product| / p and |acc' - w| / p seen
static long g_cases = 0;

static std::vector<uint64_t> edges(uint64_t q) { return {q - 1, q - 2, q / 2 - 1, q / 2, q / 2 + 1, q / 2 + 2, 1, 0}; }
// the centred values an hks_mac_term output or a range-reduced transform output can take at its edges: |.| <= q/2 + 2
static std::vector<double> centred_edges(uint64_t q) {
    const double h = std::floor((double)q / 2);
    return {h + 2, -(h + 2), h + 1, -(h + 1), h, -h, h - 1, -(h - 1), 1, -1, 0};
}

static void one(uint64_t q, const hxf::Mod m, double acc, uint64_t d, uint64_t pm, double w, uint64_t rinv, uint64_t half) {
    const double pc = centre(pm, q), pcp = pc / (double)q, rc = centre(rinv, q), rcp = rc / (double)q;
    // acc' = acc + (P mod q) d
    const double prod = hxf::mul_shoup(hxf::to_f64(d), pc, pcp, m);
    const double ap = hxf::hks_acc_pd(acc, hxf::to_f64(d), pc, pcp, m);
    if (std::fabs(acc + prod) > g_sum) g_sum = std::fabs(acc + prod);
    if (std::fabs(prod) / m.p > g_prod) g_prod = std::fabs(prod) / m.p;
    const uint64_t want_ap = (uint64_t)((residue(acc, q) + (u128)pm * d) % q);
    CHECK(std::fabs(ap) <= m.p / 2 + 2, "hks_acc_pd not centred: %.0f (q=%lu)", ap, q);
    CHECK(ap == std::floor(ap) && residue(ap, q) == want_ap, "hks_acc_pd q=%lu acc=%.0f d=%lu pm=%lu: got %.0f want %lu", q, acc, d, pm, ap, want_ap);
    // the rounding of a source row on that value
    const double b = hxf::hks_round(ap, (double)half, m);
    CHECK(b >= 0 && b < m.p && hxf::from_f64(b) == (want_ap + half) % q, "hks_round q=%lu v=%.0f half=%lu: got %.0f", q, ap, half, b);
    // out = (acc' - w) R^-1
    if (std::fabs(ap - w) / m.p > g_diff) g_diff = std::fabs(ap - w) / m.p;
    const double r = hxf::hks_down_rs(hxf::to_f64(d), acc, w, pc, pcp, rc, rcp, m);
    const uint64_t want = mulmod((want_ap + q - residue(w, q)) % q, rinv, q);
    CHECK(r >= 0 && r < m.p && hxf::from_f64(r) == want, "hks_down_rs q=%lu acc=%.0f d=%lu pm=%lu w=%.0f rinv=%lu: got %.0f want %lu", q, acc, d, pm, w, rinv, r, want);
    ++g_cases;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: hks_mul_selftest <draws> <modulus>...\n"); return 2; }
    const long draws = std::atol(argv[1]);
    std::vector<uint64_t> qs;
    for (int k = 2; k < argc; ++k) {
        qs.push_back(std::strtoull(argv[k], nullptr, 10));
        CHECK(qs.back() > 16 && qs.back() < (1ull << 52) && (qs.back() & 1), "modulus %lu outside (16, 2^52) or even", qs.back());
    }
    if (failures) return 1;
    for (uint64_t q : qs) {
        const hxf::Mod m = mod_of(q);
        const std::vector<uint64_t> e = edges(q);
        const std::vector<double> ce = centred_edges(q);
        for (double acc : ce)
            for (uint64_t d : e)
                for (uint64_t pm : e)
                    for (double w : ce) {
                        const uint64_t rinv = e[(d + pm) % e.size()] ? e[(d + pm) % e.size()] : 1;
                        one(q, m, acc, d, pm, w, rinv, (q - 1) / 2);
                        one(q, m, acc, d, pm, w, q - rinv ? q - rinv : 1, e[(uint64_t)(acc + w + 2.0 * (double)q) % e.size()]);
                    }
        for (long it = 0; it < draws; ++it) {
            const double acc = (rnd() & 7) ? centre(rnd() % q, q) : ce[rnd() % ce.size()];
            const double w = (rnd() & 7) ? centre(rnd() % q, q) : ce[rnd() % ce.size()];
            const uint64_t d = (rnd() & 7) ? rnd() % q : e[rnd() % e.size()];
            one(q, m, acc, d, rnd() % q, w, rnd() % (q - 1) + 1, rnd() % q);
        }
    }
    std::printf("hks multiply chains (%d moduli, %ld cases): max |product| = %.4f p, max |acc' - w| = %.4f p, max |acc + product| = 2^%.3f (limit 2^53)\n",
                argc - 2, g_cases, g_prod, g_diff, std::log2(g_sum));
    CHECK(g_prod <= 1.0, "a product beyond p");
    CHECK(g_diff <= 1.5, "acc' - w beyond mul_shoup's 1.5 p");
    CHECK(g_sum < 9007199254740992.0, "acc + product reaches 2^53");
    std::printf(failures ? "HKS MUL SELFTEST: %d FAILURE(S)\n" : "HKS MUL SELFTEST: ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
