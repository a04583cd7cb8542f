// key_layout.hpp -- where a switching-key word lives in each copy a keyswitch plan holds, one source for the host
// (capi.hip hexl_ks_set_keys), the kernels (keygen.hip) and a host replay (tests/cpp/key_layout_selftest.cpp), like f64_arith.hpp.
//
// A plan keeps its keys as [L][L + 1][2][n] limbs -- key d, slot (limb slot < L, or the special prime at slot L), component k -- in up
// to three copies, each with its own ORDER of the n words of a limb and its own word FORMAT:
//   natural order   word j at position j                                                    (the lone-keyswitch path)
//   B order         every block of 2^blk_logn words in the register order a forward transform of Geom<blk_logn, loge> leaves:
//                   position r * T + tid of the block holds coefficient idxB(r, tid), T = 2^(blk_logn - loge). blk_logn = log2(n) except
//                   for the slot-major copy at n = 32768, whose transforms are two 16384-point halves (blk_logn = 14)
// A position is computed, never looked up: idxB is a fixed shuffle of the index bits, so its inverse is one too.
#pragma once
#include <stdint.h>

#include "f64_arith.hpp"

namespace hxk {

// loge == 0: natural order
struct Order { uint32_t blk_logn, loge; };

// the bit fields of the B order of Geom<logn, loge> (ntt_core.hpp): a coefficient index is, from the low end,
//   [KL bits: r low] [WB bits: tid low] [loge - KL bits: r high] [logn - loge - WB bits: tid high]
struct Fields { uint32_t KL, WB, logt; };
HX_HD Fields fields(uint32_t logn, uint32_t loge) {
    const uint32_t P = (logn + loge - 1) / loge, logt = logn - loge;
    return {logn - (P - 1) * loge, logt < 6 ? logt : 6, logt};
}
// coefficient held in register r of thread tid (mirrors Geom::idxB)
HX_HD uint32_t idxB(uint32_t logn, uint32_t loge, uint32_t r, uint32_t tid) {
    const Fields f = fields(logn, loge);
    const uint32_t grp = ((tid >> f.WB) << (loge - f.KL + f.WB)) + ((r >> f.KL) << f.WB) + (tid & ((1u << f.WB) - 1));
    return (grp << f.KL) + (r & ((1u << f.KL) - 1));
}
// ... and the position r * T + tid that holds coefficient j
HX_HD uint32_t posB(uint32_t logn, uint32_t loge, uint32_t j) {
    const Fields f = fields(logn, loge);
    const uint32_t r_lo = j & ((1u << f.KL) - 1), t_lo = (j >> f.KL) & ((1u << f.WB) - 1);
    const uint32_t r_hi = (j >> (f.KL + f.WB)) & ((1u << (loge - f.KL)) - 1), t_hi = j >> (loge + f.WB);
    return (((r_hi << f.KL) + r_lo) << f.logt) + (t_hi << f.WB) + t_lo;
}

// the caller's word index stored at position pos of a limb ...
HX_HD uint32_t src_of(const Order o, uint32_t pos) {
    if (!o.loge) return pos;
    const uint32_t in = pos & ((1u << o.blk_logn) - 1), logt = o.blk_logn - o.loge;
    return (pos - in) + idxB(o.blk_logn, o.loge, in >> logt, in & ((1u << logt) - 1));
}
// ... and the position the caller's word j goes to: src_of(o, pos_of(o, j)) == j
HX_HD uint32_t pos_of(const Order o, uint32_t j) {
    if (!o.loge) return j;
    const uint32_t in = j & ((1u << o.blk_logn) - 1);
    return (j - in) + posB(o.blk_logn, o.loge, in);
}

// word formats. CENTRED: residue v < q as the double in (-q/2, q/2] the FP64 kernels work on
HX_HD double centre(uint64_t v, uint64_t q) { return v > q / 2 ? (double)v - (double)q : (double)v; }
// the same for a canonical word held as a double (p = q < 2^52 odd: p / 2 is exact, and v > p / 2 is v > floor(q / 2))
HX_HD double centre_f64(double v, double p) { return v > 0.5 * p ? v - p : v; }

}  // namespace hxk
