// ntt_route.hpp -- the route of a standalone _NTT / _INTT launch: which kernel family runs, at which geometry and tier, persistent or
// not, on which grids, with or without k_ntt_prepare in front and a k_ntt_redo_* launch behind. One pure host function of the call's
// arguments, the device's CU count, the host hint and the four HEXL_NTT_* knobs: no HIP, no kernel header. ntt.hip executes a route
// (and ties the constants restated here to Geom with static_asserts); tests/cpp/ntt_route_selftest.cpp checks the decisions on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "f64_arith.hpp"

// the four process-wide knobs as hx_knob reads them
struct NttKnobs {
    long integer = 0;    // HEXL_NTT_INT=1: integer butterflies only
    long persist = 1;    // HEXL_NTT_PERSIST=0: one workgroup per polynomial instead of persistent workgroups with input prefetch
    long halves = 1;     // HEXL_NTT_HALVES=0: N = 32768 back on the monolithic half-size-exchange kernels (A/B)
    int e16 = -1;        // HEXL_NTT_E16 >= 0: bit mask over logn - 11, 16 coefficients per thread, forced for both directions
};

enum NttFamily {
    NTT_NOTHING,         // empty batch: status 0, nothing launched
    NTT_BADARG,          // no kernel for this ring dimension: HEXL_E_BADARG, nothing reserved
    NTT_INT,             // k_ntt_fwd / k_ntt_inv (persistent: k_ntt_inv_ip), the op-for-op replay of the reference's Harvey butterflies
    NTT_F64,             // k_ntt_*_x, one workgroup per polynomial (persistent: k_ntt_*_p)
    NTT_HALVES           // k_ntt_*_h: N = 32768 as two 16384-point sub-transforms on Geom<14, 4>, k_ntt_redo_*<15, 5> behind
};

struct NttRoute {
    NttFamily family = NTT_NOTHING;
    int logn = 0, loge = 0;              // ring dimension; Geom<., loge> of the transform kernel
    int lazy = 0;                        // FP64 tier: 0 strict, else the reduction period the kernel is built for (3 / 6 / 12)
    bool semi = false;                   // strict forward tier on the semi-strict butterflies
    bool persistent = false;             // `grid` workgroups walk the batch (the _p / _ip kernels) instead of one workgroup per polynomial
    bool prepare = false;                // fast-path eligible: takes a slot of the violation-counter ring, k_ntt_prepare runs first
    bool clear_hint = false;             // the integer kernel is given that counter and the hint word, and clears the hint when the tables verified
    bool redo = false;                   // d_ntt_redo (batch + 1 words) is reserved before k_ntt_prepare, a k_ntt_redo_* launch follows the transform
    unsigned grid = 0, redo_grid = 0;
};

// Geom<logn, .>::LDS_USED (ntt_core.hpp; it does not depend on LOGE): the padded polynomial, or half of it where the whole does not fit
// the CU's 160 KiB (HALF_ONLY: N = 32768 in one workgroup)
constexpr size_t ntt_lds_whole(int logn) { return (((size_t)1 << logn) + ((size_t)1 << (logn - 4)) + (((size_t)1 << (logn - 9)) << 4)) * 8; }
constexpr bool ntt_half_only(int logn) { return ntt_lds_whole(logn) > 160 * 1024; }
constexpr size_t ntt_lds_used(int logn) { return ntt_half_only(logn) ? ntt_lds_whole(logn - 1) : ntt_lds_whole(logn); }
// workgroups the device holds at once: 18, 9, 4, 2, 1, 1 per CU for N = 1024 ... 32768
constexpr size_t ntt_slots(int logn, int num_cu) {
    return (size_t)num_cu * (ntt_lds_used(logn) > 80 * 1024 ? 1 : (160 * 1024) / ntt_lds_used(logn));
}
// coefficients per thread (as an exponent) of the integer kernels, and of the FP64 ones where HEXL_NTT_E16 has no say.
// N = 16384: 16 coefficients per thread x 1024 threads (4 waves/SIMD) measured ~10 % faster than 32 x 512
constexpr int ntt_loge(int logn) { return (logn == 14 || logn <= 10) ? 4 : 5; }
// the persistent FP64 kernels whose fallback is a k_ntt_redo_* launch of its own: the strict inverse at N = 16384 (ntt.hip ntt_inv_redo)
constexpr bool ntt_f64_redo(bool inverse, int logn, int lazy) { return inverse && logn == 14 && lazy == 0; }
// the launch behind the fast kernel is nearly always EMPTY: 32 workgroups (an empty dispatch of one 141 KiB workgroup per CU measured 4.7 us,
// 5 % of a 512-polynomial launch); a batch under tables that are not Shoup tables runs there once, then the host hint sends it to the
// dedicated integer kernels
constexpr unsigned ntt_redo_grid(unsigned fast_grid) { return fast_grid < 32u ? fast_grid : 32u; }

// scale_in_range: the inverse's n^-1 and n^-1 W are below q (the forward transform passes true); hinted: an earlier launch on this
// context found exactly these tables not to be Shoup tables (ntt.hip NttHint)
inline NttRoute ntt_route(bool inverse, int logn, uint64_t q, bool scale_in_range, size_t batch, int num_cu, bool hinted, const NttKnobs& k) {
    NttRoute r;
    if (!batch) return r;
    if (logn < 10 || logn > 15) { r.family = NTT_BADARG; return r; }
    r.logn = logn;
    const size_t slots = ntt_slots(logn, num_cu);
    // The exact FP64 fast path serves the moduli its strict tier holds, and an inverse whose scale factors are residues. Every eligible
    // call has its tables verified by k_ntt_prepare -- a hinted one too: it runs the integer kernels, which clear the hint once the
    // tables are genuine.
    r.prepare = k.integer != 1 && q >= (1ull << 16) && q < hxf::STRICT_NTT_MAX_Q && scale_in_range;
    r.clear_hint = r.prepare && hinted;
    if (!r.prepare || hinted) {
        r.family = NTT_INT;
        r.loge = ntt_loge(logn);
        // Persistent integer inverse for N = 16384 only (8.3 M against 7.6 M inverse NTT/s). A persistent forward integer kernel measured
        // no faster in rounds 2 and 4 (8.1 M against 8.6 M; N = 1024: 165 M against 195 M) -- the integer butterflies are bound by their
        // instruction count, the prefetch registers cost what the hidden load latency gains -- and is gone.
        r.persistent = inverse && logn == 14 && k.persist != 0 && batch > slots;
        r.grid = (unsigned)(r.persistent ? slots : batch);
        return r;
    }
    // tier: fewer range reductions for smaller moduli. The forward transform has kernels for the periods 6 and 12 at N = 16384 only (a
    // shorter period is always valid), and in the strict tier the semi-strict butterflies (f64_arith.hpp ct_bfly_semi, 11 instead of 14
    // instructions) in the wave-uniform passes up to 2^52 (1 + 2^-20) -- q = 2^52 + 393217 included. The inverse has one lazy tier.
    const double pd = (double)q;
    if (inverse) {
        r.lazy = pd <= hxf::LAZY_MAX_MODULUS ? 3 : 0;
    } else {
        const int period = hxf::lazy_period_for(pd);
        r.lazy = logn == 14 && (period == 12 || period == 6) ? period : period ? 3 : 0;
        r.semi = period == 0 && pd <= hxf::SEMI_MAX_MODULUS;
    }
    // N = 32768 is beyond the reference's envelope: two sub-transforms per polynomial, one workgroup per CU walking the batch, every
    // fallback in the redo launch
    if (logn == 15 && k.halves != 0) {
        r.family = NTT_HALVES;
        r.loge = 4;
        r.grid = (unsigned)(batch < (size_t)num_cu ? batch : (size_t)num_cu);
        r.redo = true;
        r.redo_grid = ntt_redo_grid(r.grid);
        return r;
    }
    r.family = NTT_F64;
    // N = 2048 .. 8192: 16 coefficients per thread where that measured faster than 32 (twice the waves per CU, but a different run length
    // per lane in the B-order access): forward N = 2048 (+17 %) and 8192 (+16 %), inverse N = 2048 (+12 %); N = 4096 lost 16 % both
    // ways, the inverse at 8192 11 % (tools/ntt_n_sweep.py)
    const int e16 = k.e16 >= 0 ? k.e16 : (inverse ? 0b001 : 0b101);
    r.loge = logn >= 11 && logn <= 13 ? (((e16 >> (logn - 11)) & 1) ? 4 : 5) : ntt_loge(logn);
    // persistent workgroups with input prefetch wherever 2 E more registers fit (not N = 32768 in one workgroup: 64 data registers at
    // 1024 threads) and the batch fills the chip more than once
    r.persistent = k.persist != 0 && !ntt_half_only(logn) && batch > slots;
    r.grid = (unsigned)(r.persistent ? slots : batch);
    r.redo = r.persistent && ntt_f64_redo(inverse, logn, r.lazy);
    r.redo_grid = r.redo ? ntt_redo_grid(r.grid) : 0;
    return r;
}
