// key_layout_selftest.cpp -- host build of hexl-fpga_amd/csrc/key_layout.hpp, the source hexl_ks_set_keys (host) and the kernels of
// keygen.hip (device) share. For every (ring, elements-per-thread) geometry a plan can hold keys in, and for the two-halves order of
// n = 32768:
//   * src_of is the permutation hexl_ks_set_keys has always used: Geom::idxB (ntt_core.hpp) restated below from its definition --
//     the coefficient of register r, thread tid is (grpB(r >> KL, tid) << KL) + (r & (2^KL - 1)) -- block by block
//   * src_of is a bijection of [0, n) and pos_of is its inverse, both ways
//   * centre_f64 on a canonical double is centre on the word, at the edges of the range, for odd and even moduli
// Stand-alone: no GPU, no library. Prints "ok <checks>" and exits 0, or names the first failure.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../hexl-fpga_amd/csrc/key_layout.hpp"

static unsigned long long checks = 0;
#define REQUIRE(cond, ...)                                      \
    do {                                                        \
        ++checks;                                               \
        if (!(cond)) { printf("FAIL: " __VA_ARGS__); printf("\n"); exit(1); } \
    } while (0)

// Geom<LOGN, LOGE>::idxB, from the definitions in ntt_core.hpp
static uint32_t geom_idxB(int LOGN, int LOGE, int r, int tid) {
    const int P = (LOGN + LOGE - 1) / LOGE, KL = LOGN - (P - 1) * LOGE, LOGT = LOGN - LOGE, WB = LOGT < 6 ? LOGT : 6;
    const int grp = r >> KL;
    const int grpB = ((tid >> WB) << (LOGE - KL + WB)) + (grp << WB) + (tid & ((1 << WB) - 1));
    return (uint32_t)((grpB << KL) + (r & ((1 << KL) - 1)));
}

static void check_order(uint32_t logn, hxk::Order o, const char* what) {
    const uint32_t n = 1u << logn;
    std::vector<int> seen(n, 0);
    for (uint32_t pos = 0; pos < n; ++pos) {
        const uint32_t j = hxk::src_of(o, pos);
        REQUIRE(j < n, "%s n=%u loge=%u: src_of(%u) = %u out of range", what, n, o.loge, pos, j);
        REQUIRE(!seen[j]++, "%s n=%u loge=%u: word %u stored twice", what, n, o.loge, j);
        REQUIRE(hxk::pos_of(o, j) == pos, "%s n=%u loge=%u: pos_of(src_of(%u)) = %u", what, n, o.loge, pos, hxk::pos_of(o, j));
        if (o.loge) {
            const uint32_t B = 1u << o.blk_logn, T = B >> o.loge, in = pos & (B - 1);
            const uint32_t want = (pos - in) + geom_idxB((int)o.blk_logn, (int)o.loge, (int)(in / T), (int)(in % T));
            REQUIRE(j == want, "%s n=%u loge=%u: src_of(%u) = %u, Geom::idxB says %u", what, n, o.loge, pos, j, want);
        } else {
            REQUIRE(j == pos, "natural order n=%u: src_of(%u) = %u", n, pos, j);
        }
    }
    for (uint32_t j = 0; j < n; ++j)
        REQUIRE(hxk::src_of(o, hxk::pos_of(o, j)) == j, "%s n=%u loge=%u: src_of(pos_of(%u))", what, n, o.loge, j);
}

int main() {
    for (uint32_t logn = 10; logn <= 15; ++logn) {
        for (uint32_t loge = 4; loge <= 5; ++loge) check_order(logn, {logn, loge}, "B order");
        check_order(logn, {logn, 0}, "natural order");
    }
    check_order(15, {14, 4}, "two halves");
    check_order(15, {14, 5}, "two halves");
    const uint64_t qs[] = {65537, 65536, (1ull << 27) - 39, (1ull << 40) + 2, (1ull << 52) - 1, (1ull << 52) - 2};
    for (uint64_t q : qs)
        for (uint64_t v : std::vector<uint64_t>{0, 1, q / 2 - 1, q / 2, q / 2 + 1, q / 2 + 2, q - 2, q - 1})
            REQUIRE(hxk::centre_f64((double)v, (double)q) == hxk::centre(v, q), "centre_f64(%llu, %llu)", (unsigned long long)v, (unsigned long long)q);
    printf("ok %llu\n", checks);
    return 0;
}
