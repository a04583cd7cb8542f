// sample_selftest.cpp -- host build of hexl-fpga_amd/csrc/sample_core.hpp, the source the kernels of rlwe.hip compile: IEEE-754 double
// mul / add / fma / rint round the same way on x86 (-mfma) and on gfx950, and the block function is 32-bit integer arithmetic, so the
// kernels' own code is checked here at operands no GPU test enumerates.
//   usage: sample_selftest <draws> <modulus>...      (tests/test_sample_selftest.py builds it: g++ -O2 -mfma -ffp-contract=off)
//   block    RFC 8439 section 2.3.2 in this layout: key bytes 00 ... 1f, ctr = 1 | 0x09000000 << 32, stream = 0x4a000000
//   maps     ternary at the thirds of 2^64 and cbd21 at all-ones / all-zeros halves, and both against their definitions on random lanes
//   mod128   per modulus q: (w3 2^96 + w2 2^64 + w1 2^32 + w0) mod q against unsigned __int128 % with every digit over
//            {0, 1, q - 1, q, 2^31, 2^32 - 2, 2^32 - 1} (the low and high digits of q - 1 and q as well), then <draws> random values
//   chains   encrypt_c0 and the Horner step of decrypt against 128-bit integers on edge and random words
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hexl-fpga_amd/csrc/sample_core.hpp"

typedef unsigned __int128 u128;
static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures < 20) { std::printf("FAIL line %d: ", __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static void block_vector() {
    hxs::Seed s;
    for (int k = 0; k < 8; ++k) s.k[k] = (uint32_t)(4 * k) | (uint32_t)(4 * k + 1) << 8 | (uint32_t)(4 * k + 2) << 16 | (uint32_t)(4 * k + 3) << 24;
    const hxs::Block b = hxs::chacha20_block(s, 1ull | (0x09000000ull << 32), 0x4a000000ull);
    static const uint8_t want[64] = {
        0x10, 0xf1, 0xe7, 0xe4, 0xd1, 0x3b, 0x59, 0x15, 0x50, 0x0f, 0xdd, 0x1f, 0xa3, 0x20, 0x71, 0xc4,
        0xc7, 0xd1, 0xf4, 0xc7, 0x33, 0xc0, 0x68, 0x03, 0x04, 0x22, 0xaa, 0x9a, 0xc3, 0xd4, 0x6c, 0x4e,
        0xd2, 0x82, 0x64, 0x46, 0x07, 0x9f, 0xaa, 0x09, 0x14, 0xc2, 0xd7, 0x05, 0xd9, 0x8b, 0x02, 0xa2,
        0xb5, 0x12, 0x9c, 0xd1, 0xde, 0x16, 0x4e, 0xb9, 0xcb, 0xd0, 0x83, 0xe8, 0xa2, 0x50, 0x3c, 0x4e};
    for (int i = 0; i < 16; ++i) {
        const uint32_t w = (uint32_t)want[4 * i] | (uint32_t)want[4 * i + 1] << 8 | (uint32_t)want[4 * i + 2] << 16 | (uint32_t)want[4 * i + 3] << 24;
        CHECK(b.w[i] == w, "RFC 8439 2.3.2 word %d: got %08x want %08x", i, b.w[i], w);
    }
    CHECK(hxs::lane(b, 0) == 0x15593bd1e4e7f110ull && hxs::lane(b, 7) == (0x4e3c50a2ull << 32 | 0xe883d0cbull), "lane extraction");
    CHECK(hxs::counter(3, 5) == ((3ull << 60) | 5) && hxs::uniform_block((1ull << 40) - 1, 15, 15, 32767) < (1ull << 60), "counters");
    CHECK(hxs::uniform_block(3, 2, 10, 517) == (((3ull * 16 + 2) * 1024 + 517) >> 2) && hxs::small_block(3, 10, 517) == ((3ull * 1024 + 517) >> 3),
          "block addressing");
}

static void maps(long draws) {
    const uint64_t t1 = (uint64_t)((((u128)1 << 64) + 2) / 3), t2 = (uint64_t)((((u128)1 << 65) + 2) / 3);
    const struct { uint64_t r; int v; } tern[] = {{0, -1}, {t1 - 1, -1}, {t1, 0}, {t2 - 1, 0}, {t2, 1}, {~0ull, 1}, {1ull << 63, 0}};
    for (auto& c : tern) CHECK(hxs::ternary(c.r) == c.v, "ternary(%016lx) = %d want %d", c.r, hxs::ternary(c.r), c.v);
    const uint64_t ones = 0x1FFFFF;
    const struct { uint64_t r; int v; } cbd[] = {{0, 0}, {ones, 21}, {ones << 21, -21}, {ones | ones << 21, 0}, {~0ull, 0}, {~(ones << 21), 21},
                                                 {1ull << 20, 1}, {1ull << 21, -1}, {1ull << 41, -1}, {1ull << 42, 0}, {0xFFFFFC0000000000ull, 0}};
    for (auto& c : cbd) CHECK(hxs::cbd21(c.r) == c.v, "cbd21(%016lx) = %d want %d", c.r, hxs::cbd21(c.r), c.v);
    for (long k = 0; k < draws; ++k) {
        const uint64_t r = rnd();
        int pc = 0;
        for (int b = 0; b < 21; ++b) pc += (int)((r >> b) & 1) - (int)((r >> (21 + b)) & 1);
        CHECK(hxs::cbd21(r) == pc && hxs::small_value(hxs::KIND_CBD21, r) == pc, "cbd21 on %016lx", r);
        const int tv = r >= t2 ? 1 : r >= t1 ? 0 : -1;
        CHECK(hxs::ternary(r) == tv && hxs::small_value(hxs::KIND_TERNARY, r) == tv, "ternary on %016lx", r);
    }
}

static long g_cases = 0;
static void one_mod(uint64_t q, const hxf::Mod m, double c32, const uint32_t w[4]) {
    const u128 r = ((u128)w[3] << 96) | ((u128)w[2] << 64) | ((u128)w[1] << 32) | w[0];
    const uint64_t want = (uint64_t)(r % q);
    const double got = hxs::mod128(w[0], w[1], w[2], w[3], c32, m);
    CHECK(got >= 0 && got < m.p && hxf::from_f64(got) == want, "q=%lu r=%08x%08x%08x%08x got %.0f want %lu", q, w[3], w[2], w[1], w[0], got, want);
    hxs::Block b{};
    for (int k = 0; k < 4; ++k) b.w[8 + k] = w[k];
    CHECK(hxs::uniform_word(b, 2, c32, m) == got, "uniform_word reads words 4k ... 4k + 3");
    ++g_cases;
}

static void chains(uint64_t q, const hxf::Mod m, uint64_t a, uint64_t s, uint64_t e, uint64_t pt, uint64_t c2) {
    const uint64_t want = (uint64_t)(((u128)pt + e + (u128)q * q - (u128)a * s) % q);
    const double got = hxs::encrypt_c0(hxf::to_f64(a), hxf::to_f64(s), hxf::to_f64(e), hxf::to_f64(pt), m);
    CHECK(got >= 0 && got < m.p && hxf::from_f64(got) == want, "encrypt_c0 q=%lu a=%lu s=%lu e=%lu pt=%lu got %.0f want %lu", q, a, s, e, pt, got, want);
    // decrypt with components (c0, c1, c2) = (e, a, c2): ((c2 s + a) s + e) mod q
    const uint64_t h1 = (uint64_t)(((u128)c2 * s + a) % q), h2 = (uint64_t)(((u128)h1 * s + e) % q);
    const double sr = hxf::reduce(hxf::to_f64(s), m);
    double acc = hxs::horner(hxf::reduce(hxf::to_f64(c2), m), sr, hxf::to_f64(a), m);
    CHECK(__builtin_fabs(acc) <= m.p / 2 + 2 && hxf::from_f64(hxf::lc_finish(acc, m)) == h1, "horner step 1 q=%lu", q);
    acc = hxs::horner(acc, sr, hxf::to_f64(e), m);
    CHECK(__builtin_fabs(acc) <= m.p / 2 + 2 && hxf::from_f64(hxf::lc_finish(acc, m)) == h2, "horner step 2 q=%lu", q);
    ++g_cases;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: sample_selftest <draws> <modulus>...\n"); return 2; }
    const long draws = std::atol(argv[1]);
    block_vector();
    maps(draws);
    for (int k = 2; k < argc; ++k) {
        const uint64_t q = std::strtoull(argv[k], nullptr, 10);
        CHECK(q > 2 && q < (1ull << 52), "modulus %lu outside (2, 2^52)", q);
        const hxf::Mod m{(double)q, 1.0 / (double)q};
        const double c32 = hxs::mod_c32(m);
        CHECK(__builtin_fabs(c32) <= m.p / 2 + 2, "c32 not centred");
        const std::vector<uint32_t> digit = {0u, 1u, (uint32_t)(q - 1), (uint32_t)q, (uint32_t)((q - 1) >> 32), (uint32_t)(q >> 32), 0x80000000u,
                                             0xFFFFFFFEu, 0xFFFFFFFFu};
        for (uint32_t d3 : digit) for (uint32_t d2 : digit) for (uint32_t d1 : digit) for (uint32_t d0 : digit) {
            const uint32_t w[4] = {d0, d1, d2, d3};
            one_mod(q, m, c32, w);
        }
        for (long t = 0; t < draws; ++t) {
            const uint64_t lo = rnd(), hi = rnd();
            const uint32_t w[4] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
            one_mod(q, m, c32, w);
        }
        const std::vector<uint64_t> edge = {0, 1, q / 2 - 1, q / 2, q / 2 + 1, q - 1};
        for (uint64_t a : edge) for (uint64_t s : edge) for (uint64_t e : edge) for (uint64_t pt : edge) chains(q, m, a, s, e, pt, edge[(a + s) % edge.size()]);
        for (long t = 0; t < draws; ++t) chains(q, m, rnd() % q, rnd() % q, rnd() % q, rnd() % q, rnd() % q);
    }
    std::printf("%ld cases\n", g_cases);
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL PASSED\n");
    return 0;
}
