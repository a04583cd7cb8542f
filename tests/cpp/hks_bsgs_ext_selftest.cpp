// hks_bsgs_ext_selftest.cpp -- host replay of the scalar chain hexl_hks_linear_transform_bsgs_ext adds (hexl-fpga_amd/csrc/f64_arith.hpp
// hks_ext_acc, called by keyswitch_hybrid.hip k_hks_mac<., HKS_MAC_ACC> and k_hks_ext_add) against unsigned __int128: IEEE-754 double
// mul / add / fma / rint round the same way on x86 (-mfma) and on gfx950, so the kernels' own source is checked here at operands no GPU
// test enumerates. A stand-alone program (tests/test_hks_bsgs_ext_selftest.py builds it with -fsanitize=address,undefined).
//   usage: hks_bsgs_ext_selftest <draws> <modulus>...
// giant     A' = A + W, W built as the kernel builds it: hks_mac_term over dl digits from 0 (u and key at the centred edges
//           +-(q/2 + 2), at the residues of the words 0 and q - 1, and random), then hks_ext_acc onto A at its edges +-(q/2 + 2)
// inner     A' = A + inner, inner an lt_mac / lt_mac_acc output (a plaintext word 0 or q - 1 or random times a stored sum), and the two
//           in sequence as a rotated row issues them: (A + sigma(inner)) + W
// The largest |accumulator + product| inside hks_mac_term and the largest |A + addend| are reported against 2^53.
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

static double centre(uint64_t v, uint64_t q) { return v > q / 2 ? (double)v - (double)q : (double)v; }
static hxf::Mod mod_of(uint64_t q) { return hxf::Mod{(double)q, 1.0 / (double)q}; }
// the residue in [0, q) of a centred double with |x| <= q/2 + 2
static uint64_t residue(double x, uint64_t q) { return (uint64_t)(((__int128)(long long)x % (__int128)q + q) % q); }

static double g_mac = 0, g_add = 0;                               // largest |acc + product| in hks_mac_term, largest |A + addend|
static long g_cases = 0;

// the centred values a reduce output can take at its edges, |.| <= q/2 + 2, with the residues of the canonical words 0 and q - 1
static std::vector<double> centred_edges(uint64_t q) {
    const double h = std::floor((double)q / 2);
    return {h + 2, -(h + 2), h + 1, -(h + 1), h, -h, h - 1, -(h - 1), 1, -1, 0};
}

static double ext_acc(uint64_t q, const hxf::Mod m, double A, double x) {
    if (std::fabs(A + x) > g_add) g_add = std::fabs(A + x);
    const double r = hxf::hks_ext_acc(A, x, m);
    CHECK(r == std::floor(r) && std::fabs(r) <= m.p / 2 + 2, "hks_ext_acc not a centred integer: %.0f (q=%lu)", r, q);
    CHECK(residue(r, q) == (residue(A, q) + residue(x, q)) % q, "hks_ext_acc q=%lu A=%.0f x=%.0f: got %.0f", q, A, x, r);
    ++g_cases;
    return r;
}

// W as k_hks_mac builds it from 0 over the digits, checked term by term
static double giant_sum(uint64_t q, const hxf::Mod m, const std::vector<double>& u, const std::vector<double>& key) {
    double acc = 0.0;
    uint64_t want = 0;
    for (size_t d = 0; d < u.size(); ++d) {
        const double prod = hxf::mul_mod(u[d], key[d], m);
        if (std::fabs(acc + prod) > g_mac) g_mac = std::fabs(acc + prod);
        acc = hxf::hks_mac_term(acc, u[d], key[d], m);
        want = (uint64_t)((want + (u128)residue(u[d], q) * residue(key[d], q)) % q);
        CHECK(std::fabs(acc) <= m.p / 2 + 2 && residue(acc, q) == want, "hks_mac_term q=%lu digit %zu: got %.0f want %lu", q, d, acc, want);
    }
    return acc;
}

// a row's inner word as k_hks_bsgs_sum leaves it: lt_mac of a stored sum, then lt_mac_acc of a second one
static double inner_word(uint64_t q, const hxf::Mod m, double b0, uint64_t t0, double b1, uint64_t t1) {
    const double first = hxf::lt_mac(b0, hxf::lt_pt(hxf::to_f64(t0), m), m);
    const double both = hxf::lt_mac_acc(b1, hxf::lt_pt(hxf::to_f64(t1), m), first, m);
    const uint64_t want = (uint64_t)(((u128)residue(b0, q) * t0 + (u128)residue(b1, q) * t1) % q);
    CHECK(std::fabs(both) <= m.p / 2 + 2 && residue(both, q) == want, "inner q=%lu: got %.0f want %lu", q, both, want);
    return both;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: hks_bsgs_ext_selftest <draws> <modulus>...\n"); return 2; }
    const long draws = std::atol(argv[1]);
    std::vector<uint64_t> qs;
    for (int k = 2; k < argc; ++k) {
        qs.push_back(std::strtoull(argv[k], nullptr, 10));
        CHECK(qs.back() > 16 && qs.back() < (1ull << 52) && (qs.back() & 1), "modulus %lu outside (16, 2^52) or even", qs.back());
    }
    if (failures) return 1;
    for (uint64_t q : qs) {
        const hxf::Mod m = mod_of(q);
        const std::vector<double> ce = centred_edges(q);
        const std::vector<uint64_t> words = {0, q - 1, 1, q / 2, q / 2 + 1};
        // every pairing of an accumulator edge with an addend edge, and the addends built by the kernels' chains from edge operands
        for (double A : ce)
            for (double x : ce) {
                ext_acc(q, m, A, x);
                for (double y : ce) {
                    const double W = giant_sum(q, m, {x, y, -x, y}, {y, x, y, -x});
                    ext_acc(q, m, A, W);
                    for (uint64_t t : words) {
                        const double in = inner_word(q, m, x, t, y, words[(size_t)(t % 3)]);
                        ext_acc(q, m, ext_acc(q, m, A, in), W);                   // a rotated row: sigma(inner), then W
                    }
                }
            }
        for (long it = 0; it < draws; ++it) {
            auto draw = [&]() { return (rnd() & 7) ? centre(rnd() % q, q) : ce[rnd() % ce.size()]; };
            const size_t dl = 1 + rnd() % 8;
            std::vector<double> u(dl), key(dl);
            for (size_t d = 0; d < dl; ++d) { u[d] = draw(); key[d] = draw(); }
            const double W = giant_sum(q, m, u, key);
            const double in = inner_word(q, m, draw(), (rnd() & 3) ? rnd() % q : words[rnd() % words.size()], draw(), rnd() % q);
            ext_acc(q, m, ext_acc(q, m, draw(), in), W);
        }
    }
    std::printf("hks bsgs ext chains (%d moduli, %ld cases): max |acc + product| = 2^%.3f, max |A + addend| = 2^%.3f (limit 2^53)\n",
                argc - 2, g_cases, std::log2(g_mac), std::log2(g_add));
    CHECK(g_mac < 9007199254740992.0, "acc + product reaches 2^53");
    CHECK(g_add < 9007199254740992.0, "A + addend reaches 2^53");
    std::printf(failures ? "HKS BSGS EXT SELFTEST: %d FAILURE(S)\n" : "HKS BSGS EXT SELFTEST: ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
