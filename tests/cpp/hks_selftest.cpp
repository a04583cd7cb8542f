// hks_selftest.cpp -- host replay of the hybrid key switch's scalar chains (hexl-fpga_amd/csrc/f64_arith.hpp hks_digit / hks_conv_term /
// hks_conv_finish / hks_mac_term / hks_round / hks_down, called by keyswitch_hybrid.hip) against unsigned __int128: IEEE-754 double
// mul / add / fma / rint round the same way on x86 (-mfma) and on gfx950, so the kernels' own source is checked here at operands no GPU
// test enumerates. A stand-alone program (tests/test_hks_selftest.py builds it with -fsanitize=address,undefined).
//   usage: hks_selftest <draws> <modulus>...
// conversion   every ordered triple (q_a, q_b | q_t) of distinct moduli: the digit {q_a, q_b} converted into q_t, mod-up (fix = 0) and
//              mod-down (fix = q_t - h mod q_t) -- a source limb larger than the target (52 bits beside 27: the quotient inside the
//              range reduction of y has 25 bits) and the reverse; words over edge values and <draws> random pairs
// mac          chains of 1 ... 16 terms, all terms alike (one sign: every partial sum at its bound) and random
// round, down  the special-limb rounding and the subtract-multiply-accumulate epilogue, edge values and random
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
static uint64_t invmod(uint64_t a, uint64_t q) {
    __int128 t = 0, nt = 1, r = q, nr = a % q;
    while (nr != 0) {
        const __int128 k = r / nr;
        __int128 x = t - k * nt; t = nt; nt = x;
        x = r - k * nr; r = nr; nr = x;
    }
    return (uint64_t)(t < 0 ? t + q : t);
}
static double centre(uint64_t v, uint64_t q) { return v > q / 2 ? (double)v - (double)q : (double)v; }
static hxf::Mod mod_of(uint64_t q) { return hxf::Mod{(double)q, 1.0 / (double)q}; }

static double g_sum = 0, g_acc = 0, g_prod = 0;                  // largest |acc + product|, |acc| / p and |product| / p seen
static long g_cases = 0;
static void track(double acc, double prod, double r, const hxf::Mod m) {
    if (std::fabs(acc + prod) > g_sum) g_sum = std::fabs(acc + prod);
    if (std::fabs(prod) / m.p > g_prod) g_prod = std::fabs(prod) / m.p;
    if (std::fabs(r) / m.p > g_acc) g_acc = std::fabs(r) / m.p;
    CHECK(std::fabs(r) <= m.p / 2 + 2, "partial sum not centred: %.0f", r);
}

struct Conv {                                                    // the digit {qa, qb} into qt
    uint64_t qa, qb, qt, hinv_a, hinv_b, wa, wb, fix;
    hxf::Mod ma, mb, mt;
    double ha, hap, hb, hbp, da, dap, db, dbp;
    Conv(uint64_t a, uint64_t b, uint64_t t, uint64_t h) : qa(a), qb(b), qt(t), ma(mod_of(a)), mb(mod_of(b)), mt(mod_of(t)) {
        hinv_a = invmod(qb % qa, qa); hinv_b = invmod(qa % qb, qb);           // (D / q_a)^-1 mod q_a, D = q_a q_b
        wa = qb % qt; wb = qa % qt;                                          // (D / q_a) mod q_t
        fix = qt - h % qt;
        ha = centre(hinv_a, qa); hap = ha / (double)qa; hb = centre(hinv_b, qb); hbp = hb / (double)qb;
        da = centre(wa, qt); dap = da / (double)qt; db = centre(wb, qt); dbp = db / (double)qt;
    }
    void one(uint64_t xa, uint64_t xb) const {
        const uint64_t ya = mulmod(xa, hinv_a, qa), yb = mulmod(xb, hinv_b, qb);
        const double fa = hxf::hks_digit(hxf::to_f64(xa), ha, hap, ma), fb = hxf::hks_digit(hxf::to_f64(xb), hb, hbp, mb);
        CHECK(hxf::from_f64(fa) == ya && hxf::from_f64(fb) == yb, "hks_digit q=(%lu %lu) words (%lu %lu)", qa, qb, xa, xb);
        const uint64_t x = (uint64_t)(((u128)ya * wa + (u128)yb * wb) % qt);
        double acc = 0.0;
        const double ys[2] = {fa, fb}, ws[2] = {da, db}, wps[2] = {dap, dbp};
        for (int i = 0; i < 2; ++i) {
            const double yr = hxf::reduce(ys[i], mt);
            CHECK(std::fabs(yr) <= mt.p / 2 + 2, "y not reduced into the target's range: %.0f", yr);
            const double prod = hxf::mul_shoup(yr, ws[i], wps[i], mt), r = hxf::hks_conv_term(acc, ys[i], ws[i], wps[i], mt);
            track(acc, prod, r, mt);
            acc = r;
        }
        const double up = hxf::hks_conv_finish(acc, 0.0, mt), down = hxf::hks_conv_finish(acc, (double)fix, mt);
        CHECK(up >= 0 && up < mt.p && hxf::from_f64(up) == x, "mod-up (%lu %lu | %lu) words (%lu %lu): got %.0f want %lu", qa, qb, qt, xa, xb, up, x);
        CHECK(down >= 0 && down < mt.p && hxf::from_f64(down) == (x + fix) % qt, "mod-down (%lu %lu | %lu) words (%lu %lu): got %.0f", qa, qb, qt, xa, xb, down);
        ++g_cases;
    }
};

static std::vector<uint64_t> edges(uint64_t q) { return {q - 1, q - 2, q / 2 - 1, q / 2, q / 2 + 1, q / 2 + 2, 1, 0}; }

static void mac_chain(uint64_t q, const hxf::Mod m, int T, const uint64_t* u, const uint64_t* k) {
    u128 want = 0;
    double acc = 0.0;
    for (int t = 0; t < T; ++t) {
        want = (want + (u128)u[t] * k[t]) % q;
        const double ud = hxf::reduce(hxf::to_f64(u[t]), m), kd = centre(k[t], q);
        const double prod = hxf::mul_mod(ud, kd, m), r = hxf::hks_mac_term(acc, ud, kd, m);
        track(acc, prod, r, m);
        acc = r;
    }
    CHECK(hxf::from_f64(hxf::lift(acc, m)) == (uint64_t)want, "hks_mac_term q=%lu T=%d", q, T);
    ++g_cases;
}

static void round_down(uint64_t q, const hxf::Mod m, uint64_t c, uint64_t h, uint64_t old, uint64_t w, uint64_t pinv) {
    const double v = hxf::reduce(hxf::to_f64(c), m);
    const double b = hxf::hks_round(v, (double)(h % q), m);
    CHECK(b >= 0 && b < m.p && hxf::from_f64(b) == (c + h % q) % q, "hks_round q=%lu c=%lu h=%lu: got %.0f", q, c, h, b);
    const double pd = centre(pinv, q);
    const double r = hxf::hks_down(hxf::to_f64(old), v, hxf::reduce(hxf::to_f64(w), m), pd, pd / (double)q, m);
    const uint64_t want = (uint64_t)((old + (u128)((c + q - w) % q) * pinv) % q);
    CHECK(r >= 0 && r < m.p && hxf::from_f64(r) == want, "hks_down q=%lu old=%lu acc=%lu w=%lu pinv=%lu: got %.0f want %lu", q, old, c, w, pinv, r, want);
    ++g_cases;
}

int main(int argc, char** argv) {
    if (argc < 5) { std::printf("usage: hks_selftest <draws> <modulus> <modulus> <modulus>...\n"); return 2; }
    const long draws = std::atol(argv[1]);
    std::vector<uint64_t> qs;
    for (int k = 2; k < argc; ++k) {
        qs.push_back(std::strtoull(argv[k], nullptr, 10));
        CHECK(qs.back() > 16 && qs.back() < (1ull << 52), "modulus %lu outside (16, 2^52)", qs.back());
    }
    if (failures) return 1;
    // the conversion: every ordered triple of distinct moduli
    for (uint64_t qa : qs)
        for (uint64_t qb : qs)
            for (uint64_t qt : qs) {
                if (qa == qb || qa == qt || qb == qt) continue;
                const Conv c(qa, qb, qt, rnd() >> 12);
                for (uint64_t ea : edges(qa))
                    for (uint64_t eb : edges(qb)) c.one(ea, eb);
                for (long it = 0; it < draws / 16 + 1; ++it) c.one(rnd() % qa, rnd() % qb);
            }
    for (uint64_t q : qs) {
        const hxf::Mod m = mod_of(q);
        const std::vector<uint64_t> e = edges(q);
        uint64_t u[16], k[16];
        for (int T = 1; T <= 16; ++T) {
            for (uint64_t eu : e)
                for (uint64_t ek : e) {
                    for (int t = 0; t < T; ++t) { u[t] = eu; k[t] = ek; }
                    mac_chain(q, m, T, u, k);
                }
            for (long it = 0; it < draws / 4 + 1; ++it) {
                for (int t = 0; t < T; ++t) { u[t] = rnd() % q; k[t] = (rnd() & 3) ? rnd() % q : e[rnd() % e.size()]; }
                mac_chain(q, m, T, u, k);
            }
        }
        for (uint64_t c : e)
            for (uint64_t h : e)
                for (uint64_t w : e)
                    for (uint64_t old : {uint64_t(0), q - 1, q / 2}) round_down(q, m, c, h, old, w, e[(c + w) % e.size()] ? e[(c + w) % e.size()] : 1);
        for (long it = 0; it < draws; ++it) round_down(q, m, rnd() % q, rnd() >> 12, rnd() % q, rnd() % q, rnd() % (q - 1) + 1);
    }
    std::printf("hks chains (%d moduli, %ld cases): max |product| = %.4f p, max |partial sum| = %.4f p, max |acc + product| = 2^%.3f (limit 2^53)\n",
                argc - 2, g_cases, g_prod, g_acc, std::log2(g_sum));
    CHECK(g_prod <= 0.875, "a product beyond 0.875 p");
    CHECK(g_sum < 9007199254740992.0, "acc + product reaches 2^53");
    std::printf(failures ? "HKS SELFTEST: %d FAILURE(S)\n" : "HKS SELFTEST: ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
