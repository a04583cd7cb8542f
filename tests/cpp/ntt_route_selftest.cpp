// ntt_route_selftest.cpp -- the route of a standalone _NTT / _INTT launch (hexl-fpga_amd/csrc/ntt_route.hpp) against expectations
// written out as literals from the rules of DESIGN.md 4.2: family, geometry, tier, persistence, grids, prepare / redo launches and the
// hint clearing, for every ring dimension and direction, at the modulus thresholds, around the persistence threshold of the batch, and
// with each knob off its default. Host only (tests/test_ntt_route_selftest.py builds it with -fsanitize=address,undefined).
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "../../hexl-fpga_amd/csrc/ntt_route.hpp"

static int failures = 0, checks = 0;

// the fields of a route in the order of the literals below
struct Want {
    NttFamily family; int loge, lazy; bool semi, persistent, prepare, clear_hint, redo; unsigned grid, redo_grid;
};
struct Call {
    bool inverse; int logn; uint64_t q; size_t batch;
    int num_cu = 256; bool hinted = false; bool scale_in_range = true; NttKnobs knobs = {};
};

static void expect(const char* what, const Call& c, const Want& w) {
    const NttRoute r = ntt_route(c.inverse, c.logn, c.q, c.scale_in_range, c.batch, c.num_cu, c.hinted, c.knobs);
    ++checks;
    const bool ok = r.family == w.family && r.loge == w.loge && r.lazy == w.lazy && r.semi == w.semi && r.persistent == w.persistent &&
                    r.prepare == w.prepare && r.clear_hint == w.clear_hint && r.redo == w.redo && r.grid == w.grid && r.redo_grid == w.redo_grid &&
                    (r.logn == c.logn || w.family == NTT_NOTHING || w.family == NTT_BADARG);
    if (ok) return;
    ++failures;
    printf("FAIL %s: %s logn %d q %llu batch %zu cus %d hinted %d\n  got  family %d loge %d lazy %d semi %d persistent %d prepare %d clear %d redo %d grid %u redo_grid %u\n"
           "  want family %d loge %d lazy %d semi %d persistent %d prepare %d clear %d redo %d grid %u redo_grid %u\n",
           what, c.inverse ? "inv" : "fwd", c.logn, (unsigned long long)c.q, c.batch, c.num_cu, (int)c.hinted,
           (int)r.family, r.loge, r.lazy, (int)r.semi, (int)r.persistent, (int)r.prepare, (int)r.clear_hint, (int)r.redo, r.grid, r.redo_grid,
           (int)w.family, w.loge, w.lazy, (int)w.semi, (int)w.persistent, (int)w.prepare, (int)w.clear_hint, (int)w.redo, w.grid, w.redo_grid);
}

constexpr bool FWD = false, INV = true;
constexpr uint64_t P16 = 65536ull, P49 = 562949953421312ull, P50 = 1125899906842624ull, P52 = 4503599627370496ull;
constexpr uint64_t LAZY_MAX = 2269391999729664ull;        // 2^51 (1 + 2^-7)
constexpr uint64_t SEMI_MAX = 4503603922337792ull;        // 2^52 (1 + 2^-20)
constexpr uint64_t STRICT_MAX = 5066549580791808ull;      // 2^52 * 1.125: the first modulus of the integer kernels
constexpr uint64_t Q51 = 2251799813685247ull;             // lazy tier, period 3
constexpr uint64_t Q59 = 576460752303415297ull;           // 59 bits

int main() {
    // the LDS bytes and resident workgroups per CU the grids rest on (ntt.hip ties ntt_lds_used to Geom)
    static_assert(ntt_lds_used(10) == 8960 && ntt_lds_used(11) == 17920 && ntt_lds_used(12) == 35840 && ntt_lds_used(13) == 71680 &&
                  ntt_lds_used(14) == 143360 && ntt_lds_used(15) == 143360, "LDS bytes per ring dimension");
    static_assert(ntt_slots(10, 1) == 18 && ntt_slots(11, 1) == 9 && ntt_slots(12, 1) == 4 && ntt_slots(13, 1) == 2 && ntt_slots(14, 1) == 1 &&
                  ntt_slots(15, 1) == 1, "workgroups per CU");
    static_assert(!ntt_half_only(14) && ntt_half_only(15), "only N = 32768 exchanges in half-size rounds");

    // ---- every ring dimension, both directions, lazy tier, around the persistence threshold, on 256 and on 4 CUs ----
    const int fwd_loge[6] = {4, 4, 5, 4, 4, 0}, inv_loge[6] = {4, 4, 5, 5, 4, 0};          // FP64 family, default E16 masks (N = 32768: below)
    const unsigned slots256[5] = {4608, 2304, 1024, 512, 256}, slots4[5] = {72, 36, 16, 8, 4};
    for (int dir = 0; dir < 2; ++dir)
        for (int logn = 10; logn <= 14; ++logn)
            for (int small = 0; small < 2; ++small) {
                const bool inv = dir != 0;
                const int cus = small ? 4 : 256, loge = (inv ? inv_loge : fwd_loge)[logn - 10];
                const unsigned s = (small ? slots4 : slots256)[logn - 10];
                expect("batch 1", {inv, logn, Q51, 1, cus}, {NTT_F64, loge, 3, false, false, true, false, false, 1, 0});
                expect("batch = slots", {inv, logn, Q51, s, cus}, {NTT_F64, loge, 3, false, false, true, false, false, s, 0});
                expect("batch = slots + 1", {inv, logn, Q51, s + 1, cus}, {NTT_F64, loge, 3, false, true, true, false, false, s, 0});
                expect("batch 0", {inv, logn, Q51, 0, cus}, {NTT_NOTHING, 0, 0, false, false, false, false, false, 0, 0});
            }
    // N = 32768: the halves family, min(batch, CUs) workgroups and a redo launch on min(that, 32), never `persistent`
    for (int dir = 0; dir < 2; ++dir) {
        const bool inv = dir != 0;
        expect("halves batch 1", {inv, 15, Q51, 1}, {NTT_HALVES, 4, 3, false, false, true, false, true, 1, 1});
        expect("halves batch 33", {inv, 15, Q51, 33}, {NTT_HALVES, 4, 3, false, false, true, false, true, 33, 32});
        expect("halves batch = CUs", {inv, 15, Q51, 256}, {NTT_HALVES, 4, 3, false, false, true, false, true, 256, 32});
        expect("halves batch = CUs + 1", {inv, 15, Q51, 257}, {NTT_HALVES, 4, 3, false, false, true, false, true, 256, 32});
        expect("halves 4 CUs batch 4", {inv, 15, Q51, 4, 4}, {NTT_HALVES, 4, 3, false, false, true, false, true, 4, 4});
        expect("halves 4 CUs batch 5", {inv, 15, Q51, 5, 4}, {NTT_HALVES, 4, 3, false, false, true, false, true, 4, 4});
        expect("halves batch 0", {inv, 15, Q51, 0}, {NTT_NOTHING, 0, 0, false, false, false, false, false, 0, 0});
        expect("halves strict", {inv, 15, P52, 8}, {NTT_HALVES, 4, 0, !inv, false, true, false, true, 8, 8});
        expect("halves strict above semi", {inv, 15, SEMI_MAX + 1, 8}, {NTT_HALVES, 4, 0, false, false, true, false, true, 8, 8});
        expect("halves small modulus", {inv, 15, P16, 8}, {NTT_HALVES, 4, 3, false, false, true, false, true, 8, 8});
    }
    // ring dimensions without kernels
    for (int logn : {-1, 0, 9, 16, 20}) {
        expect("bad ring", {FWD, logn, Q51, 8}, {NTT_BADARG, 0, 0, false, false, false, false, false, 0, 0});
        expect("bad ring", {INV, logn, Q59, 8}, {NTT_BADARG, 0, 0, false, false, false, false, false, 0, 0});
        expect("bad ring, empty batch", {INV, logn, Q51, 0}, {NTT_NOTHING, 0, 0, false, false, false, false, false, 0, 0});
    }

    // ---- the modulus thresholds, N = 16384 (every forward tier has a kernel) and N = 4096 (periods 6 and 12 run the period-3 kernels) ----
    expect("below 2^16", {FWD, 14, P16 - 1, 8}, {NTT_INT, 4, 0, false, false, false, false, false, 8, 0});
    expect("below 2^16", {INV, 14, P16 - 1, 8}, {NTT_INT, 4, 0, false, false, false, false, false, 8, 0});
    expect("below 2^16, hint ignored", {FWD, 14, P16 - 1, 8, 256, true}, {NTT_INT, 4, 0, false, false, false, false, false, 8, 0});
    expect("2^16", {FWD, 14, P16, 8}, {NTT_F64, 4, 12, false, false, true, false, false, 8, 0});
    expect("2^16", {INV, 14, P16, 8}, {NTT_F64, 4, 3, false, false, true, false, false, 8, 0});
    expect("2^49", {FWD, 14, P49, 8}, {NTT_F64, 4, 12, false, false, true, false, false, 8, 0});
    expect("2^49 + 1", {FWD, 14, P49 + 1, 8}, {NTT_F64, 4, 6, false, false, true, false, false, 8, 0});
    expect("2^50", {FWD, 14, P50, 8}, {NTT_F64, 4, 6, false, false, true, false, false, 8, 0});
    expect("2^50 + 1", {FWD, 14, P50 + 1, 8}, {NTT_F64, 4, 3, false, false, true, false, false, 8, 0});
    expect("lazy bound", {FWD, 14, LAZY_MAX, 8}, {NTT_F64, 4, 3, false, false, true, false, false, 8, 0});
    expect("lazy bound + 1", {FWD, 14, LAZY_MAX + 1, 8}, {NTT_F64, 4, 0, true, false, true, false, false, 8, 0});
    expect("2^52 - 1", {FWD, 14, P52 - 1, 8}, {NTT_F64, 4, 0, true, false, true, false, false, 8, 0});
    expect("2^52", {FWD, 14, P52, 8}, {NTT_F64, 4, 0, true, false, true, false, false, 8, 0});
    expect("semi bound", {FWD, 14, SEMI_MAX, 8}, {NTT_F64, 4, 0, true, false, true, false, false, 8, 0});
    expect("semi bound + 1", {FWD, 14, SEMI_MAX + 1, 8}, {NTT_F64, 4, 0, false, false, true, false, false, 8, 0});
    expect("strict bound - 1", {FWD, 14, STRICT_MAX - 1, 8}, {NTT_F64, 4, 0, false, false, true, false, false, 8, 0});
    expect("strict bound", {FWD, 14, STRICT_MAX, 8}, {NTT_INT, 4, 0, false, false, false, false, false, 8, 0});
    expect("59 bits", {FWD, 14, Q59, 8}, {NTT_INT, 4, 0, false, false, false, false, false, 8, 0});
    for (uint64_t q : {P16, P49, P49 + 1, P50, P50 + 1, LAZY_MAX}) {
        expect("lazy tiers at N = 4096", {FWD, 12, q, 8}, {NTT_F64, 5, 3, false, false, true, false, false, 8, 0});
        expect("inverse: one lazy tier", {INV, 14, q, 8}, {NTT_F64, 4, 3, false, false, true, false, false, 8, 0});
    }
    expect("strict at N = 4096", {FWD, 12, LAZY_MAX + 1, 8}, {NTT_F64, 5, 0, true, false, true, false, false, 8, 0});
    expect("strict at N = 4096 above semi", {FWD, 12, SEMI_MAX + 1, 8}, {NTT_F64, 5, 0, false, false, true, false, false, 8, 0});
    for (uint64_t q : {LAZY_MAX + 1, P52 - 1, P52, SEMI_MAX, SEMI_MAX + 1, STRICT_MAX - 1})
        expect("inverse strict: never semi", {INV, 14, q, 8}, {NTT_F64, 4, 0, false, false, true, false, false, 8, 0});
    expect("inverse strict bound", {INV, 14, STRICT_MAX, 8}, {NTT_INT, 4, 0, false, false, false, false, false, 8, 0});
    expect("inverse 59 bits", {INV, 14, Q59, 8}, {NTT_INT, 4, 0, false, false, false, false, false, 8, 0});
    // the six-and-twelve tiers keep their kernels when persistent
    expect("2^49 persistent", {FWD, 14, P49, 1024}, {NTT_F64, 4, 12, false, true, true, false, false, 256, 0});
    expect("2^50 persistent", {FWD, 14, P50, 1024}, {NTT_F64, 4, 6, false, true, true, false, false, 256, 0});

    // ---- the strict inverse at N = 16384: persistent runs are followed by a redo launch on min(slots, 32) workgroups ----
    expect("strict inverse, batch = slots", {INV, 14, P52, 256}, {NTT_F64, 4, 0, false, false, true, false, false, 256, 0});
    expect("strict inverse, persistent", {INV, 14, P52, 257}, {NTT_F64, 4, 0, false, true, true, false, true, 256, 32});
    expect("strict inverse, persistent, 4 CUs", {INV, 14, P52, 5, 4}, {NTT_F64, 4, 0, false, true, true, false, true, 4, 4});
    expect("strict inverse, 4 CUs, batch = slots", {INV, 14, P52, 4, 4}, {NTT_F64, 4, 0, false, false, true, false, false, 4, 0});
    expect("lazy inverse, persistent: no redo", {INV, 14, Q51, 257}, {NTT_F64, 4, 3, false, true, true, false, false, 256, 0});
    expect("strict forward, persistent: no redo", {FWD, 14, P52, 257}, {NTT_F64, 4, 0, true, true, true, false, false, 256, 0});
    expect("strict inverse at N = 8192, persistent: no redo", {INV, 13, P52, 513}, {NTT_F64, 5, 0, false, true, true, false, false, 512, 0});

    // ---- the integer family: LOGE 4, 5, 5, 5, 4, 5, one workgroup per polynomial, but the persistent inverse at N = 16384 ----
    const int int_loge[6] = {4, 5, 5, 5, 4, 5};
    for (int logn = 10; logn <= 15; ++logn)
        for (int dir = 0; dir < 2; ++dir) {
            const bool inv = dir != 0, ip = inv && logn == 14;
            const int e = int_loge[logn - 10];
            const unsigned s = logn == 15 ? 256 : slots256[logn - 10];
            expect("59 bits", {inv, logn, Q59, s}, {NTT_INT, e, 0, false, false, false, false, false, s, 0});
            expect("59 bits, batch > slots", {inv, logn, Q59, s + 1}, {NTT_INT, e, 0, false, ip, false, false, false, ip ? s : s + 1, 0});
            expect("59 bits, hint ignored", {inv, logn, Q59, 3, 256, true}, {NTT_INT, e, 0, false, false, false, false, false, 3, 0});
            // hinted: still prepared, and the integer kernel clears the hint when the tables verify
            expect("hinted", {inv, logn, Q51, s, 256, true}, {NTT_INT, e, 0, false, false, true, true, false, s, 0});
            expect("hinted, batch > slots", {inv, logn, Q51, s + 1, 256, true}, {NTT_INT, e, 0, false, ip, true, true, false, ip ? s : s + 1, 0});
            expect("hinted strict", {inv, logn, P52, 2, 4, true}, {NTT_INT, e, 0, false, false, true, true, false, 2, 0});
            Call c{inv, logn, Q51, 3};
            c.knobs.integer = 1;
            expect("HEXL_NTT_INT=1", c, {NTT_INT, e, 0, false, false, false, false, false, 3, 0});
            c.hinted = true;
            expect("HEXL_NTT_INT=1, hint ignored", c, {NTT_INT, e, 0, false, false, false, false, false, 3, 0});
        }
    expect("persistent integer inverse, 4 CUs", {INV, 14, Q59, 5, 4}, {NTT_INT, 4, 0, false, true, false, false, false, 4, 0});
    expect("integer inverse, 4 CUs, batch = slots", {INV, 14, Q59, 4, 4}, {NTT_INT, 4, 0, false, false, false, false, false, 4, 0});
    // inverse whose scale factors are not residues: integer kernels, nothing prepared (the forward transform has no such argument)
    {
        Call c{INV, 14, Q51, 257};
        c.scale_in_range = false;
        expect("inverse a >= q", c, {NTT_INT, 4, 0, false, true, false, false, false, 256, 0});
        c.hinted = true;
        expect("inverse a >= q, hint ignored", c, {NTT_INT, 4, 0, false, true, false, false, false, 256, 0});
        c.logn = 12;
        expect("inverse a >= q, N = 4096", c, {NTT_INT, 5, 0, false, false, false, false, false, 257, 0});
    }

    // ---- each knob off its default, one at a time ----
    for (int dir = 0; dir < 2; ++dir) {
        const bool inv = dir != 0;
        // HEXL_NTT_PERSIST=0: one workgroup per polynomial everywhere, and no redo launch behind the strict inverse
        for (int logn = 10; logn <= 14; ++logn) {
            Call c{inv, logn, Q51, slots256[logn - 10] + 1};
            c.knobs.persist = 0;
            expect("HEXL_NTT_PERSIST=0", c, {NTT_F64, (inv ? inv_loge : fwd_loge)[logn - 10], 3, false, false, true, false, false, slots256[logn - 10] + 1, 0});
        }
        {
            Call c{inv, 14, P52, 1024};
            c.knobs.persist = 0;
            expect("HEXL_NTT_PERSIST=0, strict", c, {NTT_F64, 4, 0, !inv, false, true, false, false, 1024, 0});
            c.q = Q59;
            expect("HEXL_NTT_PERSIST=0, integer", c, {NTT_INT, 4, 0, false, false, false, false, false, 1024, 0});
            c.q = Q51;
            c.logn = 15;
            expect("HEXL_NTT_PERSIST=0 leaves the halves family alone", c, {NTT_HALVES, 4, 3, false, false, true, false, true, 256, 32});
        }
        // HEXL_NTT_HALVES=0: N = 32768 on the one-per-workgroup kernels at LOGE 5, never persistent, no redo; other rings unchanged
        {
            Call c{inv, 15, Q51, 257};
            c.knobs.halves = 0;
            expect("HEXL_NTT_HALVES=0", c, {NTT_F64, 5, 3, false, false, true, false, false, 257, 0});
            c.q = P52;
            expect("HEXL_NTT_HALVES=0, strict", c, {NTT_F64, 5, 0, !inv, false, true, false, false, 257, 0});
            c.q = P49;
            expect("HEXL_NTT_HALVES=0, small modulus", c, {NTT_F64, 5, 3, false, false, true, false, false, 257, 0});
            c.hinted = true;
            expect("HEXL_NTT_HALVES=0, hinted", c, {NTT_INT, 5, 0, false, false, true, true, false, 257, 0});
            c.hinted = false;
            c.logn = 14;
            c.q = Q51;
            expect("HEXL_NTT_HALVES=0, N = 16384", c, {NTT_F64, 4, 3, false, true, true, false, false, 256, 0});
        }
        // HEXL_NTT_E16: the mask replaces both directions' defaults at N = 2048 .. 8192 and nothing else
        for (int mask : {0, 7, 2}) {
            for (int logn = 10; logn <= 15; ++logn) {
                Call c{inv, logn, Q51, 2};
                c.knobs.e16 = mask;
                const int loge = logn >= 11 && logn <= 13 ? (((mask >> (logn - 11)) & 1) ? 4 : 5) : 4;
                if (logn == 15) expect("HEXL_NTT_E16, N = 32768", c, {NTT_HALVES, 4, 3, false, false, true, false, true, 2, 2});
                else expect("HEXL_NTT_E16", c, {NTT_F64, loge, 3, false, false, true, false, false, 2, 0});
                c.hinted = true;                     // the integer family has no 16-coefficient variants at N = 2048 .. 8192
                expect("HEXL_NTT_E16, hinted", c, {NTT_INT, int_loge[logn - 10], 0, false, false, true, true, false, 2, 0});
            }
        }
    }
    {
        Call c{FWD, 11, LAZY_MAX + 1, 2305};
        c.knobs.e16 = 0;
        expect("HEXL_NTT_E16=0, strict, persistent", c, {NTT_F64, 5, 0, true, true, true, false, false, 2304, 0});
        c.knobs.e16 = 7;
        c.logn = 12;
        c.batch = 1025;
        expect("HEXL_NTT_E16=7, strict, persistent", c, {NTT_F64, 4, 0, true, true, true, false, false, 1024, 0});
    }

    printf("%d checks, %d failures\n", checks, failures);
    if (failures) return 1;
    printf("ALL PASSED\n");
    return 0;
}
