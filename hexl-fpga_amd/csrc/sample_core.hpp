// sample_core.hpp -- the random streams of hexl_sample / hexl_rlwe_encrypt / hexl_pk_encrypt, one source for
// the kernels (rlwe.hip) and for the host (tests/cpp/sample_selftest.cpp and pk_selftest.cpp replay it against RFC 8439's vector and
// unsigned __int128), like f64_arith.hpp.
//
// ChaCha20 in counter mode, the 20-round block function of RFC 8439 on this 16-word state:
//   words 0-3    0x61707865 0x3320646e 0x79622d32 0x6b206574
//   words 4-11   seed[0..7], the caller's 32 bytes as eight little-endian u32
//   words 12-13  low and high half of ctr = (kind << 60) | block
//   words 14-15  low and high half of the caller's 64-bit stream
// Output words w[0..15] = rounds + input state; u64 lane t < 8 is w[2t] | w[2t+1] << 32. Every output word of a sampler is a function
// of (seed, stream, kind, ABSOLUTE polynomial index c, limb i, coefficient j) alone, so neither chunking nor the grid changes a result:
//   UNIFORM (1)  word j of polynomial (c, limb i): block = ((c 16 + i) n + j) >> 2, r = lane[2 (j & 3)] + 2^64 lane[2 (j & 3) + 1],
//                word = r mod q_i (bias below 2^-76, no rejection)
//   TERNARY (2)  coefficient j of polynomial c: block = (c n + j) >> 3, r = lane[j & 7], v = ((r 3) >> 64) - 1
//   CBD21   (3)  the same addressing, v = popcount(r & 0x1FFFFF) - popcount((r >> 21) & 0x1FFFFF)
// The block function is 32-bit add / xor / rotate, the small maps plain integer arithmetic. r mod q for the 128-bit r runs on the
// FP64 chains of f64_arith.hpp (moduli < 2^52), which is where this library has its exact modular arithmetic: a 64 x 64-bit integer
// product costs four to five multiply instructions on gfx950, an FP64 fma one. No inline assembly.
#pragma once
#include "f64_arith.hpp"

namespace hxs {

constexpr int KIND_UNIFORM = 1, KIND_TERNARY = 2, KIND_CBD21 = 3;
constexpr uint64_t MAX_INDEX = 1ull << 40;      // first + count <= 2^40 keeps every block index below 2^60

struct Seed { uint32_t k[8]; };
struct Block { uint32_t w[16]; };

HX_HD uint32_t rotl(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }
HX_HD void quarter(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
    a += b; d ^= a; d = rotl(d, 16);
    c += d; b ^= c; b = rotl(b, 12);
    a += b; d ^= a; d = rotl(d, 8);
    c += d; b ^= c; b = rotl(b, 7);
}

HX_HD uint64_t counter(int kind, uint64_t block) { return ((uint64_t)kind << 60) | block; }

HX_HD Block chacha20_block(const Seed& s, uint64_t ctr, uint64_t stream) {
    const uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, s.k[0], s.k[1], s.k[2], s.k[3],
                             s.k[4], s.k[5], s.k[6], s.k[7], (uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)stream, (uint32_t)(stream >> 32)};
    Block x;
#pragma unroll
    for (int i = 0; i < 16; ++i) x.w[i] = in[i];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        quarter(x.w[0], x.w[4], x.w[8], x.w[12]);
        quarter(x.w[1], x.w[5], x.w[9], x.w[13]);
        quarter(x.w[2], x.w[6], x.w[10], x.w[14]);
        quarter(x.w[3], x.w[7], x.w[11], x.w[15]);
        quarter(x.w[0], x.w[5], x.w[10], x.w[15]);
        quarter(x.w[1], x.w[6], x.w[11], x.w[12]);
        quarter(x.w[2], x.w[7], x.w[8], x.w[13]);
        quarter(x.w[3], x.w[4], x.w[9], x.w[14]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) x.w[i] += in[i];
    return x;
}

HX_HD uint64_t lane(const Block& b, int t) { return (uint64_t)b.w[2 * t] | ((uint64_t)b.w[2 * t + 1] << 32); }

// block indices; c is the absolute polynomial index, n = 2^logn
HX_HD uint64_t uniform_block(uint64_t c, uint32_t i, uint32_t logn, uint32_t j) { return ((((c << 4) + i) << logn) + j) >> 2; }
HX_HD uint64_t small_block(uint64_t c, uint32_t logn, uint32_t j) { return ((c << logn) + j) >> 3; }

// (w3 2^96 + w2 2^64 + w1 2^32 + w0) mod p as the canonical double, p < 2^52: Horner in base 2^32 on centred residues. Every 32-bit
// digit is exact as a double and enters through reduce (|.| <= p/2 + 2: a digit may be far above a 27-bit p); c32 = reduce(2^32) is the
// centred 2^32 mod p. A step is f64_to_residue's: mul_mod on two reduce outputs (|product| <= 0.7p) plus a reduce output,
// |sum| <= 1.2p + 2 < 2^53 -- exact and inside reduce's domain.
HX_HD double mod_c32(const hxf::Mod m) { return hxf::reduce(4294967296.0, m); }
HX_HD double mod128(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, double c32, const hxf::Mod m) {
    double acc = hxf::reduce((double)w3, m);
    acc = hxf::reduce(hxf::mul_mod(acc, c32, m) + hxf::reduce((double)w2, m), m);
    acc = hxf::reduce(hxf::mul_mod(acc, c32, m) + hxf::reduce((double)w1, m), m);
    acc = hxf::reduce(hxf::mul_mod(acc, c32, m) + hxf::reduce((double)w0, m), m);
    return hxf::lift(acc, m);
}
// UNIFORM word j & 3 = k of a block: lanes 2k (low half of r) and 2k + 1 (high half) are words 4k ... 4k + 3
HX_HD double uniform_word(const Block& b, int k, double c32, const hxf::Mod m) {
    return mod128(b.w[4 * k], b.w[4 * k + 1], b.w[4 * k + 2], b.w[4 * k + 3], c32, m);
}

// the four UNIFORM words j0 ... j0 + 3 (j0 a multiple of 4: one block, none of it wasted) of polynomial (c, limb i), canonical, as
// doubles -- what every kernel that draws a mask runs (rlwe.hip k_sample_uniform / k_rlwe_encrypt, keygen.hip k_ks_gen)
HX_HD void uniform4(double a[4], const Seed& seed, uint64_t stream, uint64_t c, uint32_t i, uint32_t logn, uint32_t j0, const hxf::Mod m) {
    const Block blk = chacha20_block(seed, counter(KIND_UNIFORM, uniform_block(c, i, logn, j0)), stream);
    const double c32 = mod_c32(m);
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = uniform_word(blk, k, c32, m);
}

// the two small maps, r one u64 lane
HX_HD int ternary(uint64_t r) { return (int)(uint64_t)(((unsigned __int128)r * 3u) >> 64) - 1; }
HX_HD int cbd21(uint64_t r) {
    return __builtin_popcount((uint32_t)r & 0x1FFFFFu) - __builtin_popcount((uint32_t)(r >> 21) & 0x1FFFFFu);
}
HX_HD int small_value(int kind, uint64_t r) { return kind == KIND_TERNARY ? ternary(r) : cbd21(r); }

// ---- the scalar chains of k_rlwe_encrypt / k_rlwe_decrypt, all operands canonical words as doubles (0 <= . < p) ----
// c0 = (pt + e - a s) mod p: pt_mul_centred leaves |a s| <= p/2 + 2, and each lc_add takes a centred sum and a word of [0, p)
HX_HD double encrypt_c0(double a, double s, double e, double pt, const hxf::Mod m) {
    return hxf::lc_finish(hxf::lc_add(hxf::lc_add(-hxf::pt_mul_centred(a, s, m), e, m), pt, m), m);
}
// Horner step: (acc s + c) mod p centred, acc centred (|.| <= p/2 + 2, mul_mod's operand range), sr = reduce(s), c canonical:
// |product| <= 0.7p, reduced, then lc_add's |acc + u| <= 1.5p + 2
HX_HD double horner(double acc, double sr, double c, const hxf::Mod m) {
    return hxf::lc_add(hxf::reduce(hxf::mul_mod(acc, sr, m), m), c, m);
}

// ---- the scalar chain of k_pk_encrypt (hexl_pk_encrypt), all operands canonical words as doubles (0 <= . < p);
// tests/cpp/pk_selftest.cpp replays it against 128-bit integers and asserts every bound named here ----
// a factor as both products take it: canonical -> centred, |.| <= p/2 + 2, mul_mod's operand range. u is converted ONCE per word and
// meets pk0 and pk1.
HX_HD double pk_operand(double x, const hxf::Mod m) { return hxf::reduce(x, m); }
// (key u) mod p, centred: keyr and ur outputs of pk_operand, so |mul_mod| <= 0.7p (f64_arith.hpp; 0.875p by the coarser count of
// ts_mac's note), which the reduce brings back to |.| <= p/2 + 2 -- the partial sum lc_add is bounded for
HX_HD double pk_product(double keyr, double ur, const hxf::Mod m) { return hxf::reduce(hxf::mul_mod(keyr, ur, m), m); }
// c0 = (pk0 u + e0 + pt) mod p, canonical: each lc_add takes a centred sum (|.| <= p/2 + 2) and a canonical word of [0, p),
// |sum| <= 1.5p + 2 < 2^53, exact and inside reduce's domain, and leaves |.| <= p/2 + 2 again, which is what lc_finish lifts. pt = 0.0
// for an encryption of zero: the same chain.
HX_HD double pk_c0(double pk0r, double ur, double e0, double pt, const hxf::Mod m) {
    return hxf::lc_finish(hxf::lc_add(hxf::lc_add(pk_product(pk0r, ur, m), e0, m), pt, m), m);
}
// c1 = (pk1 u + e1) mod p, canonical: one lc_add on the same bounds
HX_HD double pk_c1(double pk1r, double ur, double e1, const hxf::Mod m) {
    return hxf::lc_finish(hxf::lc_add(pk_product(pk1r, ur, m), e1, m), m);
}

}  // namespace hxs
