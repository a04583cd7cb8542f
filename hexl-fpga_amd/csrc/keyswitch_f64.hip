// keyswitch_f64.hip -- K4 on the FP64 pipe: the production keyswitch path when every modulus is < 2^52
// (the reference's own limit, host/src/keyswitch.cpp:32). Dataflow of SURVEY 2.1-K4 steps 1-7 as four kernels per
// chunk of instances -- k_ksf_up (steps 1-2), k_ksf_mac (3), k_ksf_intt_sp (4), k_ksf_moddown (5-7); small batches
// split steps 1-2 into k_ksf_intt + k_ksf_ntt_up. Arithmetic from f64_arith.hpp (exact integers in doubles), so
// results are bit-identical to the integer path (keyswitch.hip) and to the reference's canonical pipeline.
//
// HBM-resident intermediates are doubles: c (canonical, natural order; small batches only), u and prod in the
// forward transform's register order ("B order": stored as [register][thread], fully coalesced, and consumed the
// same way), s' (canonical, natural order); keys in B order too, twiddles centred. Only t_target (read) and result
// (read-modify-write) are converted from/to uint64.
#include <stdlib.h>

#include "hexl_internal.hpp"
#ifndef KSF_BIG_PRIO
#define KSF_BIG_PRIO 1222  // ... in k_ksf_ntt_up / k_ksf_moddown at N = 32768 (32 coefficients per thread, half-size re-deals)
#endif
#ifndef KSF_UP_PRIO
#define KSF_UP_PRIO 1222   // wave priority by pass in k_ksf_up (0 = off)
#endif
#include "ntt_core_f64.hpp"

using namespace hx;

// the kernels whose workgroup runs ONE forward transform: wave priorities at N = 32768 only
template <int LOGN> struct KsfOneTransformOpt : NttOpt { static constexpr int FPRIO = LOGN >= 15 ? KSF_BIG_PRIO : 0; };
// k_ksf_up: transform after transform in one workgroup
struct KsfUpOpt : NttOpt { static constexpr int FPRIO = KSF_UP_PRIO; };

struct KsArgsF {
    const KsModF64* mods;    // [K]
    const double* tables;    // [K][4][n]: w, w/p, inverse w (first entry at index 1), inverse w/p
    const double* keys;      // [L][L+1][2][n] centred, B order
    double* c;               // [chunk][L][n]          canonical, natural order
    double* u;               // [chunk][L+1][L][n]     |u| <= 2.14p (no final range reduction), B order
    double* prod;            // [chunk][2][L+1][n]     centred, B order
    double* s;               // [chunk][2][n]          canonical, natural order
    const u64* t_target;     // [chunk][L][n]
    u64* result;             // [chunk][2][L][n]
    u32 L, K, nb;
    u32* range_flag;         // set to 1 when a t_target / result word is not below its modulus (hexl_ks_range_check)
    u32 overwrite;           // 1: `result` is written, not accumulated into (the host-pointer path: the HOST adds, fpga.cpp:441-475)
    u32 skip;                // latency path: moduli of one size (hexl_ks_plan::x_skip) -> s' enters the mod-down transform un-reduced
    unsigned long long tiermap;   // kernels built with LAZY = -1 (plans of mixed tiers): nibble i = reduction period of limb i
};

__device__ __forceinline__ u32 xcd_item_f(u32 bid, u32 total) {   // see keyswitch.hip: XCD-contiguous work ranges
    const u32 q = total >> 3, r = total & 7, xcd = bid & 7, j = bid >> 3;
    return xcd * q + (xcd < r ? xcd : r) + j;
}

// ---- small batches: one transform per workgroup, so that even a single keyswitch spreads over L*L + ... CUs ----
// step 1: c_d = INTT_{q_d}(t_target[d]) as canonical doubles
// mixed-tier kernels (LAZY = -1): four schedules per forward transform at N = 16384 (two -- lazy period 3 / strict -- measured no faster)
// CT (hexl_rotate_hoisted only, here and in k_ksf_up): t_target is component 1 of a ciphertext batch [b][2][L][n] read in place -- row d of
// instance b lies at row 2 b L + d, not b L + d
template <int LOGN, int LOGE, int LAZY, bool CT = false>
__global__ __launch_bounds__(1 << (LOGN - LOGE)) void k_ksf_intt(KsArgsF a) {
    using G = Geom<LOGN, LOGE>;
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const int tid = threadIdx.x;
    const u32 item = blockIdx.x;                                  // b*L + d
    const u32 d = __builtin_amdgcn_readfirstlane(item % a.L);
    const KsModF64 md = a.mods[d];
    const double* tb = a.tables + size_t(d) * 4 * G::N;
    const u64* src = a.t_target + size_t(CT ? 2 * item - d : item) * G::N;
    double v[G::E];
    hxf::RangeMask bad = 0;
#pragma unroll
    for (int r = 0; r < G::E; ++r) v[r] = hxf::reduce(hxf::to_f64_checked(src[G::idxB(r, tid)], md.m, bad), md.m);
    hxf::report_range(bad, a.range_flag);
    // step 2 for slot == d needs no transform: NTT_{q_d}(INTT_{q_d}(t_d) mod q_d) = t_d (the reference recomputes
    // it; same value for in-range data). The registers already hold t_d in B order.
    {
        const u32 b = item / a.L;
        double* ud = a.u + ((size_t(b) * (a.L + 1) + d) * a.L + d) * G::N;
#pragma unroll
        for (int r = 0; r < G::E; ++r) ud[r * G::T + tid] = v[r];
    }
    with_tier<LAZY, false>(a.tiermap, d, [&](auto T) {             // (an inverse transform has two forms: strict and lazy)
        WgNttF64<LOGN, LOGE, decltype(T)::value>::template inverse<true>(v, ldsd, tid, tb + 2 * G::N, tb + 3 * G::N, md.m, md.sc);
    });
    double* dst = a.c + size_t(item) * G::N;
#pragma unroll
    for (int r = 0; r < G::E; ++r) dst[G::idxA(r, tid)] = hxf::lift(v[r], md.m);
}

// step 2: u[b][slot][d] = NTT_{q_i}(c_d mod q_i) for slot != d (slot == d is written by k_ksf_intt), one
// transform per workgroup, kept in the forward transform's register order ("B order", fully coalesced).
// (Capping this kernel at 96 VGPRs so that a k_ksf_mac workgroup of the other lane could be co-resident was
// measured: +12 % instructions, no throughput gain -- not done.)
template <int LOGN, int LOGE, int LAZY>
__global__ __launch_bounds__(1 << (LOGN - LOGE)) void k_ksf_ntt_up(KsArgsF a) {
    using G = Geom<LOGN, LOGE>;
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const int tid = threadIdx.x;
    const u32 L = a.L;
    // (b*L + d)*L + s, XCD-contiguous: the L transforms that read the same c_d run back to back on one XCD, so c_d
    // comes from HBM once and from that XCD's L2 afterwards
    const u32 item = __builtin_amdgcn_readfirstlane(xcd_item_f(blockIdx.x, gridDim.x));
    const u32 bd = item / L, sidx = item - bd * L;
    const u32 b = bd / L, d = bd - b * L;
    const u32 slot = sidx + (sidx >= d ? 1u : 0u);                // 0..L without d; slot L is the special prime
    const u32 i = slot < L ? slot : a.K - 1;
    const KsModF64 md = a.mods[i];
    const Mod m = md.m;
    double* dst = a.u + ((size_t(b) * (L + 1) + slot) * L + d) * G::N;
    double v[G::E];
    const double* cd = a.c + (size_t(b) * L + d) * G::N;
#pragma unroll
    for (int r = 0; r < G::E; ++r) v[r] = hxf::reduce(cd[G::idxA(r, tid)], m);          // c_d mod q_i (intt1_redu.hpp:36-42)
    const double* tb = a.tables + size_t(i) * 4 * G::N;
    // no final range reduction (LAZY): |u| <= 2.14p, which mul_mod in k_ksf_mac accepts (|u.key| < 2^102,
    // |result| < p); tests/cpp/f64_selftest.cpp replays exactly this chain against 128-bit integers
    with_tier<LAZY, LOGN == 14>(a.tiermap, i, [&](auto T) {
        using W = WgNttF64<LOGN, LOGE, decltype(T)::value, KsfOneTransformOpt<LOGN>>;   // N = 32768: +7 % (batch 32 at N = 16384: -5 %)
        W::template forward<true, false>(v, ldsd, tid, tb, tb + G::N, m);
    });
#pragma unroll
    for (int r = 0; r < G::E; ++r) dst[r * G::T + tid] = v[r];
}

// ---- large batches: one workgroup per polynomial of the INPUT, all its transforms back to back ----
// steps 1-2 in one kernel: c_d = INTT_{q_d}(t_target[d]) (canonical), then u[b][slot][d] = NTT_{q_i}(c_d mod q_i)
// for every slot. One workgroup per (b, d) keeps c_d in registers (A order is both the inverse transform's output
// and the forward transform's input order) and runs the L forward transforms back to back: c never travels to
// memory, and only the first of the L+1 transforms waits for an input -- a lone workgroup per CU otherwise idles
// ~5 us per transform on that wait (tools/load_probe.hip, tools/ntt_timeline.hip). The waves of the workgroup only
// meet at each transform's cross-wave re-deal, so early waves start the next slot while late ones still store.
// u is kept in the forward transform's register order ("B order", fully coalesced).
template <int LOGN, int LOGE, int LAZY, bool CT = false>
__global__ __launch_bounds__(1 << (LOGN - LOGE)) void k_ksf_up(KsArgsF a) {
    static_assert(LAZY >= 0, "one schedule for all L + 1 transforms of the workgroup: plans of mixed tiers run k_ksf_intt + k_ksf_ntt_up");
    using G = Geom<LOGN, LOGE>;
    // FPRIO 1222: this workgroup runs L transforms back to back -- the pass in front of the cross-wave barrier at the lower wave
    // priority (ntt_core_f64.hpp hx_fwd_prio): N = 32768, L = 3, batch 2048: 143.5 k -> 163.5 k keyswitch/s (+14 %)
    using W = WgNttF64<LOGN, LOGE, LAZY, KsfUpOpt>;
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const u32 L = a.L;
    const u32 item = blockIdx.x;                                  // b*L + d
    const u32 b = __builtin_amdgcn_readfirstlane(item / L), d = item - b * L;
    double c[G::E];
    {
        const int tid = threadIdx.x;
        const KsModF64 md = a.mods[d];
        const double* tb = a.tables + size_t(d) * 4 * G::N;
        const u64* src = a.t_target + size_t(CT ? 2 * item - d : item) * G::N;
        // uniform row pointer + unsigned 32-bit thread offset: SGPR-base addressing, no 64-bit VALU address math
        const u32 tB = u32(G::idxB(0, tid));
        hxf::RangeMask bad = 0;
#pragma unroll
        for (int r = 0; r < G::E; ++r) c[r] = hxf::reduce(hxf::to_f64_checked((src + G::idxB(r, 0))[tB], md.m, bad), md.m);
        hxf::report_range(bad, a.range_flag);
        // step 2 for slot == d needs no transform: NTT_{q_d}(INTT_{q_d}(t_d) mod q_d) = t_d (the reference
        // recomputes it; same value for in-range data). The registers already hold t_d in B order.
        double* ud = a.u + ((size_t(b) * (L + 1) + d) * L + d) * G::N;
#pragma unroll
        for (int r = 0; r < G::E; ++r) __builtin_nontemporal_store(c[r], &(ud + r * G::T)[u32(tid)]);   // streamed to k_ksf_mac
        W::template inverse<true>(c, ldsd, tid, tb + 2 * G::N, tb + 3 * G::N, md.m, md.sc);
#pragma unroll
        for (int r = 0; r < G::E; ++r) c[r] = hxf::lift(c[r], md.m);                    // canonical c_d, A order
    }
#pragma unroll 1
    for (u32 s = 0; s < L; ++s) {
        const u32 slot = s + (s >= d ? 1u : 0u);                  // 0..L without d; slot L is the special prime
        const u32 i = slot < L ? slot : a.K - 1;
        const Mod m = a.mods[i].m;
        int tid = threadIdx.x;                                    // laundered per slot: otherwise every LDS / global
        asm volatile("" : "+v"(tid));                             // address is hoisted out of the loop and spilled
        u32 toff = i * 4 * G::N;                                  // laundered offset, not pointer: a laundered pointer
        asm volatile("" : "+s"(toff));                            // loses its address space and turns the loads into FLAT
        const double* tb = a.tables + toff;
        double v[G::E];
#pragma unroll
        for (int r = 0; r < G::E; ++r) v[r] = hxf::reduce(c[r], m);                     // c_d mod q_i (intt1_redu.hpp:36-42)
        // not FRESH: other waves may still be reading their LDS block of the previous transform. No final range
        // reduction (LAZY): |u| <= 2.14p, which mul_mod in k_ksf_mac accepts (tests/cpp/f64_selftest.cpp)
        W::template forward<false, false>(v, ldsd, tid, tb, tb + G::N, m);
        double* dst = a.u + ((size_t(b) * (L + 1) + slot) * L + d) * G::N;
#pragma unroll
        for (int r = 0; r < G::E; ++r) __builtin_nontemporal_store(v[r], &(dst + r * G::T)[u32(tid)]);
    }
}

// the inner chain of step 3: one accumulator takes one coefficient of one digit times its key word
__device__ __forceinline__ double ksf_mac_term(double acc, double u, double key, Mod m) {
    return hxf::reduce(acc + hxf::mul_mod(u, key, m), m);
}

// step 3: prod[b][k][slot] = sum_d u[b][slot][d] . key[d][k][slot]  (dyadmult.hpp:128-140). Pure streaming:
// a thread owns two adjacent coefficients of one slot, keeps their 2*L*2 key words in registers and walks the
// batch, so keys are read once per launch and u / prod exactly once.
template <int MAXL>
__global__ __launch_bounds__(256) void k_ksf_mac(KsArgsF a, u32 n) {
    const u32 L = a.L;
    const u32 pairs = n >> 1;
    const u32 gid = blockIdx.x * blockDim.x + threadIdx.x;        // (slot, pair)
    const u32 slot = gid / pairs;
    if (slot > L) return;
    const u32 j = (gid - slot * pairs) * 2;
    const u32 i = slot < L ? slot : a.K - 1;
    const Mod m = a.mods[i].m;
    typedef double d2 __attribute__((ext_vector_type(2)));
    d2 key[MAXL][2];
#pragma unroll
    for (int d = 0; d < MAXL; ++d)
        if (d < (int)L) {
            key[d][0] = *reinterpret_cast<const d2*>(a.keys + ((size_t(d) * (L + 1) + slot) * 2 + 0) * n + j);
            key[d][1] = *reinterpret_cast<const d2*>(a.keys + ((size_t(d) * (L + 1) + slot) * 2 + 1) * n + j);
        }
    for (u32 b = blockIdx.y; b < a.nb; b += gridDim.y) {
        const double* ub = a.u + ((size_t(b) * (L + 1) + slot) * L) * n + j;
        d2 acc0 = {0.0, 0.0}, acc1 = {0.0, 0.0};
#pragma unroll
        for (int d = 0; d < MAXL; ++d)
            if (d < (int)L) {
                const d2 u = __builtin_nontemporal_load(reinterpret_cast<const d2*>(ub + size_t(d) * n));   // read exactly once
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    acc0[e] = ksf_mac_term(acc0[e], u[e], key[d][0][e], m);
                    acc1[e] = ksf_mac_term(acc1[e], u[e], key[d][1][e], m);
                }
            }
        __builtin_nontemporal_store(acc0, reinterpret_cast<d2*>(a.prod + ((size_t(b) * 2 + 0) * (L + 1) + slot) * n + j));
        __builtin_nontemporal_store(acc1, reinterpret_cast<d2*>(a.prod + ((size_t(b) * 2 + 1) * (L + 1) + slot) * n + j));
    }
}

// step 3 with the Galois automorphism inside it, for the callers that share one mod-up among many rotations:
//     sum[b][k][slot] = sum_d sigma_g(u[b][slot][d]) . key[d][k][slot]
// In NTT-output index space sigma_g is out[j] = in[galois_src(j)]; u, the keys and prod are stored in B order, so a thread takes ONE
// output index j (gid = slot*n + j), reads the keys and writes prod at position posB(j), and gathers u from posB(galois_src(j)):
// src = idxB^-1 . pi_g . idxB without a table.
// The gather reads global memory directly, 8 bytes per lane. pi_g maps every aligned block of 2^k indices onto an aligned block of
// 2^k indices (the low k bits of j are the high k bits of brv(j), and (2 brv(j) + 1) g only carries upwards), and B order keeps an
// aligned block of 64 indices as 2^KL rows of 64 >> KL adjacent words: a wave's 64 sources fill exactly as many cache lines as its 64
// outputs, merely in another order, and a workgroup's (256 indices; 512 at N = 32768, where KL = 5) are whole 128-byte lines. No LDS, no
// barrier; the price against k_ksf_mac is 8-byte instead of 16-byte accesses. The keys stay in registers while the thread walks the batch.
// u is not range-reduced (|u| <= 2.14p, KsArgsF) and a permutation moves words without changing them, so the bound holds for every
// word gathered and the inner chain is k_ksf_mac's (ksf_mac_term). g = 1 is served too (galois_src(j) = j).
// What becomes of the reduced sum is the kernel's mode:
//   KSF_MAC_STORE    hexl_rotate_hoisted, and the baby steps of hexl_linear_transform_bsgs: prod = sum, streamed to the kernels of steps 4-7
//                    (or to k_lt_bsgs_sum)
//   KSF_MAC_PT_FIRST hexl_linear_transform, a chunk's first rotation: prod = pt[slot] . sum (hxf::lt_mac), prod is not read
//   KSF_MAC_PT_ACC   ... its later rotations: prod = prod + pt[slot] . sum (hxf::lt_mac_acc), the old word requested in front of the gather
// pt is [L + 1][n] u64 in plain NTT-output order, row L modulo the special prime: the thread's word is pt[slot][j], coalesced in j,
// converted once and the same for every instance the thread walks. The plaintext modes store plainly -- the next rotation reads the
// words -- and prod never leaves the extended basis between rotations, so steps 4-7 run once for all of them.
struct HoistGeom { u32 logn, loge, kl, wb, g; };                 // Geom<LOGN, LOGE>: N, E, KL, WB as exponents; the Galois element
enum KsfMacMode : int { KSF_MAC_STORE, KSF_MAC_PT_FIRST, KSF_MAC_PT_ACC };

__device__ __forceinline__ u32 posB(u32 j, const HoistGeom& h) {  // inverse of Geom::idxB: position r*T + tid that holds NTT-output index j
    const u32 r = (j & ((1u << h.kl) - 1)) | (((j >> (h.kl + h.wb)) & ((1u << (h.loge - h.kl)) - 1)) << h.kl);
    const u32 tid = ((j >> h.kl) & ((1u << h.wb) - 1)) | ((j >> (h.loge + h.wb)) << h.wb);
    return (r << (h.logn - h.loge)) | tid;
}

// a thread of the kernels that own ONE NTT-output index j of one slot: gid = slot * n + j; false for the threads past slot L. The caller
// reads and writes B-ordered rows at posB(j)
__device__ __forceinline__ bool hoist_item(const KsArgsF& a, const HoistGeom& h, u32& gid, u32& slot, u32& j) {
    gid = blockIdx.x * blockDim.x + threadIdx.x;
    slot = gid >> h.logn;
    if (slot > a.L) return false;
    j = gid & ((1u << h.logn) - 1);
    return true;
}

// PT: `const u64*` in the plaintext modes, nothing in KSF_MAC_STORE -- the hidden kernel arguments follow the declared ones, so an
// argument nobody reads would still move the offsets the kernel loads them from
template <int MAXL, KsfMacMode MODE, class... PT>
__global__ __launch_bounds__(512) void k_ksf_mac_galois(KsArgsF a, HoistGeom h, PT... pt) {
    static_assert(sizeof...(PT) == (MODE != KSF_MAC_STORE), "one plaintext, in the plaintext modes only");
    const u32 L = a.L, n = 1u << h.logn;
    u32 gid, slot, j;
    if (!hoist_item(a, h, gid, slot, j)) return;
    const u32 pos = posB(j, h), src = posB(galois_src(j, h.logn, h.g), h);
    const u32 i = slot < L ? slot : a.K - 1;
    const Mod m = a.mods[i].m;
    double w = 0.0;
    if constexpr (MODE != KSF_MAC_STORE) w = hxf::lt_pt(hxf::to_f64((pt, ...)[gid]), m);   // (pt, ...): the one pointer of the pack
    double key[MAXL][2];
#pragma unroll
    for (int d = 0; d < MAXL; ++d)
        if (d < (int)L) {
            key[d][0] = a.keys[((size_t(d) * (L + 1) + slot) * 2 + 0) * n + pos];
            key[d][1] = a.keys[((size_t(d) * (L + 1) + slot) * 2 + 1) * n + pos];
        }
    for (u32 b = blockIdx.y; b < a.nb; b += gridDim.y) {
        const double* ub = a.u + ((size_t(b) * (L + 1) + slot) * L) * n + src;
        double* p0 = a.prod + ((size_t(b) * 2 + 0) * (L + 1) + slot) * n + pos;
        double* p1 = a.prod + ((size_t(b) * 2 + 1) * (L + 1) + slot) * n + pos;
        double prev0 = 0.0, prev1 = 0.0;
        if constexpr (MODE == KSF_MAC_PT_ACC) { prev0 = *p0; prev1 = *p1; }   // requested in front of the gather
        double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
        for (int d = 0; d < MAXL; ++d)
            if (d < (int)L) {
                const double u = ub[size_t(d) * n];               // plain load: the rest of the line is another lane's, or the next wave's
                acc0 = ksf_mac_term(acc0, u, key[d][0], m);
                acc1 = ksf_mac_term(acc1, u, key[d][1], m);
            }
        if constexpr (MODE == KSF_MAC_STORE) {
            __builtin_nontemporal_store(acc0, p0);
            __builtin_nontemporal_store(acc1, p1);
        } else if constexpr (MODE == KSF_MAC_PT_FIRST) {
            *p0 = hxf::lt_mac(acc0, w, m); *p1 = hxf::lt_mac(acc1, w, m);
        } else {
            *p0 = hxf::lt_mac_acc(acc0, w, prev0, m); *p1 = hxf::lt_mac_acc(acc1, w, prev1, m);
        }
    }
}

// step 3 of one giant step of a baby-step/giant-step linear transform (hexl_linear_transform_bsgs):
//     prod[b][k][slot] = sum_i pt_{j,i}[slot] . B_i[b][k][slot]
// B_i is what k_ksf_mac_galois<., KSF_MAC_STORE> (k_ksf_mac for g = 1) stored for baby step i, the inner sum of the plaintext modes,
// computed once per chunk instead of once per giant step. No keys, no gather: a thread owns NTT-output index j of one slot as
// k_ksf_mac_galois does (hoist_item), reads its plaintext word pt[slot][j] (plain order, coalesced in j) and the two stored words at
// posB(j) per term of the per-call table, keeps both accumulators in registers across the terms and writes prod once -- no
// read-modify-write of prod per rotation. The plaintext words come from L2 from the second instance on.
// The scalar chain is that of k_ksf_mac_galois's plaintext modes unchanged -- lt_pt, lt_mac for the first term, lt_mac_acc after it --
// and its inner operand is, as there, an output of reduce (the last operation of the stored multiply-accumulate): the bound chain of
// f64_arith.hpp and its host replay (tests/cpp/lt_mac_selftest.cpp) cover this kernel as they stand.
struct HxBsgsTerm { const u64* pt; const double* B; };           // pt: [L + 1][n]; B: baby step's slice [nb][2][L + 1][n], B order

__global__ __launch_bounds__(256) void k_lt_bsgs_sum(KsArgsF a, HoistGeom h, const HxBsgsTerm* terms, u32 n_terms) {
    const u32 L = a.L, n = 1u << h.logn;
    u32 gid, slot, j;
    if (!hoist_item(a, h, gid, slot, j)) return;
    const u32 pos = posB(j, h);
    const u32 i = slot < L ? slot : a.K - 1;
    const Mod m = a.mods[i].m;
    for (u32 b = blockIdx.y; b < a.nb; b += gridDim.y) {
        const size_t o0 = ((size_t(b) * 2 + 0) * (L + 1) + slot) * n + pos, o1 = ((size_t(b) * 2 + 1) * (L + 1) + slot) * n + pos;
        const HxBsgsTerm first = terms[0];                        // uniform: scalar loads
        const double t0 = hxf::lt_pt(hxf::to_f64(first.pt[gid]), m);
        double acc0 = hxf::lt_mac(first.B[o0], t0, m), acc1 = hxf::lt_mac(first.B[o1], t0, m);
        for (u32 r = 1; r < n_terms; ++r) {
            const HxBsgsTerm term = terms[r];
            const double w = hxf::lt_pt(hxf::to_f64(term.pt[gid]), m);
            acc0 = hxf::lt_mac_acc(term.B[o0], w, acc0, m);
            acc1 = hxf::lt_mac_acc(term.B[o1], w, acc1, m);
        }
        __builtin_nontemporal_store(acc0, a.prod + o0);           // streamed to k_ksf_intt_sp / k_ksf_moddown, as k_ksf_mac_galois stores
        __builtin_nontemporal_store(acc1, a.prod + o1);
    }
}

// step 4: s'_k = INTT_{q_sp}(prod[k][special]) + floor(q_sp/2)  (mod q_sp), canonical
template <int LOGN, int LOGE, int LAZY>
__global__ __launch_bounds__(1 << (LOGN - LOGE)) void k_ksf_intt_sp(KsArgsF a) {
    using G = Geom<LOGN, LOGE>;
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const int tid = threadIdx.x;
    const u32 L = a.L;
    const u32 item = blockIdx.x;                                  // b*2 + k
    const u32 i = a.K - 1;
    const KsModF64 md = a.mods[i];
    const Mod m = md.m;
    const double* tb = a.tables + size_t(i) * 4 * G::N;
    const double* src = a.prod + (size_t(item) * (L + 1) + L) * G::N;
    double v[G::E];
#pragma unroll
    for (int r = 0; r < G::E; ++r) v[r] = __builtin_nontemporal_load(&src[r * G::T + tid]);
    with_tier<LAZY, false>(a.tiermap, i, [&](auto T) {
        WgNttF64<LOGN, LOGE, decltype(T)::value>::template inverse<true>(v, ldsd, tid, tb + 2 * G::N, tb + 3 * G::N, m, md.sc);
    });
    double* dst = a.s + size_t(item) * G::N;
#pragma unroll
    for (int r = 0; r < G::E; ++r)                                // intt2_redu.hpp:25,43
        dst[G::idxA(r, tid)] = hxf::lift(hxf::reduce(hxf::lift(v[r], m) + md.half, m), m);
}

// steps 5-7: w = NTT((s' + fix_i) mod q_i); result += (prod - w) * msf_i
template <int LOGN, int LOGE, int LAZY>
__global__ __launch_bounds__(1 << (LOGN - LOGE)) void k_ksf_moddown(KsArgsF a) {
    using G = Geom<LOGN, LOGE>;
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const int tid = threadIdx.x;
    const u32 L = a.L;
    // (b*2 + k)*L + i, XCD-contiguous: the L transforms that read the same s'_k run back to back on one XCD
    const u32 item = __builtin_amdgcn_readfirstlane(xcd_item_f(blockIdx.x, gridDim.x));
    const u32 bk = item / L, i = item - bk * L;
    const u32 b = bk >> 1, k = bk & 1;
    const KsModF64 md = a.mods[i];
    const Mod m = md.m;
    const double* tb = a.tables + size_t(i) * 4 * G::N;

    const double* sk = a.s + (size_t(b) * 2 + k) * G::N;
    double v[G::E];
#pragma unroll
    for (int r = 0; r < G::E; ++r) v[r] = hxf::reduce(sk[G::idxA(r, tid)] + md.fix, m);   // intt2_redu.hpp:49-51
    const double* pk = a.prod + ((size_t(b) * 2 + k) * (L + 1) + i) * G::N;
    u64* res = a.result + ((size_t(b) * 2 + k) * L + i) * G::N;
    // prod is requested right after the cross-wave re-deal and lands during the remaining passes; result is
    // requested first thing in the epilogue and lands during the (prod - w) * msf multiplications
    double pv[G::E];
    with_tier<LAZY, LOGN == 14>(a.tiermap, i, [&](auto T) {
        using W = WgNttF64<LOGN, LOGE, decltype(T)::value, KsfOneTransformOpt<LOGN>>;   // N = 32768: +7 % (N = 16384: +-0)
        if constexpr (G::HALF_ONLY) {                              // N = 32768: no registers to hold prod during the transform
            W::template forward<true, false>(v, ldsd, tid, tb, tb + G::N, m);
#pragma unroll
            for (int r = 0; r < G::E; ++r) pv[r] = (pk + r * G::T)[u32(tid)];
        } else {
            W::template forward<true, false>(v, ldsd, tid, tb, tb + G::N, m, 0u, [&] {    // |w| <= 2.14p: |prod - w| <= 2.64p below
#pragma unroll
                for (int r = 0; r < G::E; ++r) pv[r] = (pk + r * G::T)[u32(tid)];
            });
        }
    });
    const u32 tB = u32(G::idxB(0, tid));
    if (!G::HALF_ONLY && a.overwrite) {                           // host-pointer path: the output itself, canonical; the HOST adds
#pragma unroll
        for (int r = 0; r < G::E; ++r)
            (res + G::idxB(r, 0))[tB] = hxf::from_f64(hxf::lift(hxf::reduce(hxf::mul_shoup(pv[r] - v[r], md.msf, md.msf_p, m), m), m));
        return;
    }
    u64 old[G::E];
#pragma unroll
    for (int r = 0; r < G::E; ++r) old[r] = (res + G::idxB(r, 0))[tB];
#pragma unroll
    for (int r = 0; r < G::E; ++r) v[r] = hxf::mul_shoup(pv[r] - v[r], md.msf, md.msf_p, m);    // ms.hpp:70-82
    hxf::RangeMask bad = 0;
#pragma unroll
    for (int r = 0; r < G::E; ++r) {
        const double rr = hxf::reduce(hxf::to_f64_checked(old[r], m, bad) + v[r], m);            // fpga.cpp:453-457
        (res + G::idxB(r, 0))[tB] = hxf::from_f64(hxf::lift(rr, m));
    }
    hxf::report_range(bad, a.range_flag);
}

// ---- latency path (round 4): a LONE keyswitch -- the SEAL bridge's only call shape (experimental/bridge-seal/tests/
// fpga_context.h:13-16: set_worksize_KeySwitch(1)) -- in THREE dependent kernels instead of five. The dataflow is four transforms
// deep whatever the kernel count (INTT -> NTT -> INTT_sp -> NTT); what can go is kernel boundaries and memory round trips:
//   k_ksl_intt (b, d)        c_d = INTT(t_d) -> scratch; zeroes its share of the (integer) accumulator `prod`            step 1
//   k_ksl_up   (b, slot, d)  NTT_{q_slot}(c_d mod q_slot) (slot == d: t_d itself, no transform), times key[d][slot][k], canonical,
//                            ADDED into prod[k][slot] by 64-bit integer atomics: the sum over d of L <= 15 residues below 2^52
//                            stays below 2^56, is exact in any order, and costs no extra kernel                       steps 2-3
//   k_ksl_down (b, k, i)     every workgroup sums-down its own copy of the special limb: INTT_sp(prod[k][special]) stays in
//                            registers (the inverse's output order is the forward's input order), then NTT_{q_i}, then the
//                            mod-switch epilogue with prod[k][i] requested behind the cross-wave re-deal               steps 4-7
// L + L(L+1) + 2L workgroups of one transform each (54 + ... at L = 6): the chip is mostly idle, latency is all that counts.
// prod[.] mod q: the atomically accumulated word is below L q; four conditional subtractions bring it below q.
template <int MAXBITS = 4>
__device__ __forceinline__ u64 fold_below_q(u64 x, u64 q) {
#pragma unroll
    for (int s = MAXBITS - 1; s >= 0; --s) { const u64 m = q << s; x = x >= m ? x - m : x; }
    return x;
}

template <int LOGN, int LOGE, int LAZY>
__global__ __launch_bounds__(1 << (LOGN - LOGE)) void k_ksl_intt(KsArgsF a) {
    using G = Geom<LOGN, LOGE>;
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const int tid = threadIdx.x;
    const u32 item = blockIdx.x;                                  // b*L + d
    const u32 L = a.L;
    const u32 b = item / L, d = __builtin_amdgcn_readfirstlane(item - b * L);
    // this workgroup's rows of the accumulator (2 (L+1) rows per instance, dealt round robin over its L workgroups)
    u64* acc = reinterpret_cast<u64*>(a.prod) + size_t(b) * 2 * (L + 1) * G::N;
    for (u32 row = d; row < 2 * (L + 1); row += L)
#pragma unroll
        for (int r = 0; r < G::E; ++r) (acc + size_t(row) * G::N + G::idxA(r, 0))[u32(tid)] = 0;
    const KsModF64 md = a.mods[d];
    const double* tb = a.tables + size_t(d) * 4 * G::N;
    const u64* src = a.t_target + size_t(item) * G::N;
    const u64 qd = (u64)md.m.p;
    double v[G::E];
    hxf::RangeMask bad = 0;
    const u32 tB = u32(G::idxB(0, tid));
#pragma unroll
    for (int r = 0; r < G::E; ++r) v[r] = hxf::to_f64_lt52_checked((src + G::idxB(r, 0))[tB], qd, bad);   // canonical words as they are
    hxf::report_range(bad, a.range_flag);
    with_tier<LAZY, false>(a.tiermap, d, [&](auto T) {
        WgNttF64<LOGN, LOGE, decltype(T)::value, InvNoWpOpt<>>::template inverse<true>(v, ldsd, tid, tb + 2 * G::N, tb + 3 * G::N, md.m, md.sc);
    });
    double* dst = a.c + size_t(item) * G::N;
#pragma unroll
    for (int r = 0; r < G::E; ++r) (dst + G::idxA(r, 0))[u32(tid)] = hxf::lift(v[r], md.m);
}

template <int LOGN, int LOGE, int LAZY>
__global__ __launch_bounds__(1 << (LOGN - LOGE)) void k_ksl_up(KsArgsF a) {
    using G = Geom<LOGN, LOGE>;
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const int tid = threadIdx.x;
    const u32 L = a.L;
    const u32 item = blockIdx.x;                                  // (b*(L+1) + slot)*L + d
    const u32 bs = item / L, d = item - bs * L;
    const u32 b = bs / (L + 1), slot = __builtin_amdgcn_readfirstlane(bs - b * (L + 1));
    const u32 i = slot < L ? slot : a.K - 1;
    const KsModF64 md = a.mods[i];
    const Mod m = md.m;
    const double* k0 = a.keys + (size_t(d) * (L + 1) + slot) * 2 * G::N;        // key[d][slot][0], [1] follows; B order
    double v[G::E], ka[G::E], kb[G::E];
    auto request_keys = [&] {
#pragma unroll
        for (int r = 0; r < G::E; ++r) { ka[r] = (k0 + r * G::T)[u32(tid)]; kb[r] = (k0 + G::N + r * G::T)[u32(tid)]; }
    };
    if (slot == d) {                                              // NTT(INTT(t_d) mod q_d) = t_d: no transform
        const u64* src = a.t_target + (size_t(b) * L + d) * G::N;
        const u32 tB = u32(G::idxB(0, tid));
        u64 raw[G::E];
#pragma unroll
        for (int r = 0; r < G::E; ++r) raw[r] = (src + G::idxB(r, 0))[tB];
        request_keys();
#pragma unroll
        for (int r = 0; r < G::E; ++r) v[r] = hxf::reduce(hxf::to_f64(raw[r]), m);
    } else {
        const double* cd = a.c + (size_t(b) * L + d) * G::N;
#pragma unroll
        for (int r = 0; r < G::E; ++r) v[r] = hxf::reduce((cd + G::idxA(r, 0))[u32(tid)], m);   // c_d mod q_i (intt1_redu.hpp:36-42)
        const double* tb = a.tables + size_t(i) * 4 * G::N;
        with_tier<LAZY, LOGN == 14>(a.tiermap, i, [&](auto T) {                                // |u| <= 2.14p; keys behind the cross-wave re-deal
            WgNttF64<LOGN, LOGE, decltype(T)::value>::template forward<true, false>(v, ldsd, tid, tb, tb + G::N, m, 0u, request_keys);
        });
    }
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(a.prod) + size_t(b) * 2 * (L + 1) * G::N;
    unsigned long long* p0 = acc + size_t(0 * (L + 1) + slot) * G::N;
    unsigned long long* p1 = acc + size_t(1 * (L + 1) + slot) * G::N;
#pragma unroll
    for (int r = 0; r < G::E; ++r) {
        const u64 t0 = hxf::from_f64(hxf::lift(hxf::reduce(hxf::mul_mod(v[r], ka[r], m), m), m));
        const u64 t1 = hxf::from_f64(hxf::lift(hxf::reduce(hxf::mul_mod(v[r], kb[r], m), m), m));
        // relaxed, device scope, no return value: the order of the L additions does not matter for an integer sum
        __hip_atomic_fetch_add(p0 + r * G::T + tid, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(p1 + r * G::T + tid, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <int LOGN, int LOGE, int LAZY>
__global__ __launch_bounds__(1 << (LOGN - LOGE)) void k_ksl_down(KsArgsF a) {
    using G = Geom<LOGN, LOGE>;
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const int tid = threadIdx.x;
    const u32 L = a.L;
    const u32 item = blockIdx.x;                                  // (b*2 + k)*L + i
    const u32 bk = item / L, i = __builtin_amdgcn_readfirstlane(item - bk * L);
    const u32 b = bk >> 1, k = bk & 1;
    const KsModF64 msp = a.mods[a.K - 1], md = a.mods[i];
    const Mod m = md.m;
    const u64* acc = reinterpret_cast<const u64*>(a.prod) + size_t(b) * 2 * (L + 1) * G::N;
    const u64* psp = acc + size_t(k * (L + 1) + L) * G::N;        // accumulated special limb, B order
    const u64* pi = acc + size_t(k * (L + 1) + i) * G::N;
    double v[G::E];
    {
        const u64 qsp = (u64)msp.m.p;
#pragma unroll
        for (int r = 0; r < G::E; ++r) v[r] = hxf::to_f64_lt52(fold_below_q<4>((psp + r * G::T)[u32(tid)], qsp));
        const double* ts = a.tables + size_t(a.K - 1) * 4 * G::N;
        with_tier<LAZY, false>(a.tiermap, a.K - 1, [&](auto T) {
            WgNttF64<LOGN, LOGE, decltype(T)::value, InvNoWpOpt<>>::template inverse<true>(v, ldsd, tid, ts + 2 * G::N, ts + 3 * G::N, msp.m, msp.sc);
        });
        // y = s' - floor(q_sp/2), the exact centred remainder (keyswitch_x.hip ksx_special_down; intt2_redu.hpp:25-51), A order
#pragma unroll
        for (int r = 0; r < G::E; ++r) {
            const double c = hxf::lift(v[r], msp.m);
            v[r] = c > msp.half ? c - msp.m.p : c;
        }
    }
    if (!a.skip) {
#pragma unroll
        for (int r = 0; r < G::E; ++r) v[r] = hxf::reduce(v[r], m);
    }
    const double* tb = a.tables + size_t(i) * 4 * G::N;
    u64 praw[G::E];
    with_tier<LAZY, LOGN == 14>(a.tiermap, i, [&](auto T) {
        WgNttF64<LOGN, LOGE, decltype(T)::value>::template forward<false, false>(v, ldsd, tid, tb, tb + G::N, m, 0u, [&] {     // |w| <= 2.14p
#pragma unroll
            for (int r = 0; r < G::E; ++r) praw[r] = (pi + r * G::T)[u32(tid)];
        });
    });
    const u64 qi = (u64)m.p;
    u64* res = a.result + ((size_t(b) * 2 + k) * L + i) * G::N;
    const u32 tB = u32(G::idxB(0, tid));
    if (a.overwrite) {                                            // host-pointer path: the output itself, canonical; the HOST adds
#pragma unroll
        for (int r = 0; r < G::E; ++r) {
            const double pv = hxf::reduce(hxf::to_f64_lt52(fold_below_q<4>(praw[r], qi)), m);
            (res + G::idxB(r, 0))[tB] = hxf::from_f64(hxf::lift(hxf::reduce(hxf::mul_shoup(pv - v[r], md.msf, md.msf_p, m), m), m));
        }
        return;
    }
    u64 old[G::E];
#pragma unroll
    for (int r = 0; r < G::E; ++r) old[r] = (res + G::idxB(r, 0))[tB];
    hxf::RangeMask bad = 0;
#pragma unroll
    for (int r = 0; r < G::E; ++r) {
        const double pv = hxf::reduce(hxf::to_f64_lt52(fold_below_q<4>(praw[r], qi)), m);
        const double out = hxf::mul_shoup(pv - v[r], md.msf, md.msf_p, m);                          // ms.hpp:70-82
        const double rr = hxf::reduce(hxf::to_f64_lt52_checked(old[r], qi, bad) + out, m);          // fpga.cpp:453-457
        (res + G::idxB(r, 0))[tB] = hxf::from_f64(hxf::lift(rr, m));
    }
    hxf::report_range(bad, a.range_flag);
}

// ---- the stages of a chunk, each launched from ONE place: the keyswitch (run_chunk_f64) and the hoisted callers (HoistRun) share them.
// A stage opts its kernels in to their dynamic LDS before it launches them and returns the launch error. ----
static u32 ksf_batch_lanes(u32 nb) { return nb < 8 ? nb : 8; }    // step 3's grid.y: 8 batch lanes keep >= 2048 workgroups in flight
template <class F>
static void ksf_with_maxl(u32 L, F f) {                           // step 3's key registers: room for 8 or 16 digits
    if (L <= 8) f(hx_int<8>{});
    else        f(hx_int<16>{});
}

// steps 1-2 (inverse + mod-up transforms). CT: t_target is component 1 of a ciphertext batch, read in place
template <int LOGN, int LOGE, int LAZY, bool CT>
static int ksf_stage_up(hexl_ctx* c, hipStream_t st, const KsArgsF& a) {
    using G = Geom<LOGN, LOGE>;
    const u32 L = a.L, nb = a.nb;
    // one workgroup per input polynomial (all its transforms back to back) once that alone fills the chip twice;
    // below that one workgroup per transform, so that small batches still spread over the CUs (N = 32768: 64 VGPRs of data already)
    const bool fused_up = LAZY >= 0 && (hx_knob_ks_fuse() & 1) && nb * L >= 2 * (u32)c->num_cu && !G::HALF_ONLY;
    if constexpr (LAZY >= 0)
        if (fused_up) {
            if (int rc = hx_lds_optin<k_ksf_up<LOGN, LOGE, LAZY, CT>>(c->device, G::LDS_USED)) return rc;
            hipLaunchKernelGGL((k_ksf_up<LOGN, LOGE, LAZY, CT>), dim3(nb * L), dim3(G::T), G::LDS_USED, st, a);
            return (int)hipGetLastError();
        }
    if (int rc = hx_lds_optin<k_ksf_intt<LOGN, LOGE, LAZY, CT>, k_ksf_ntt_up<LOGN, LOGE, LAZY>>(c->device, G::LDS_USED)) return rc;
    hipLaunchKernelGGL((k_ksf_intt<LOGN, LOGE, LAZY, CT>), dim3(nb * L), dim3(G::T), G::LDS_USED, st, a);
    hipLaunchKernelGGL((k_ksf_ntt_up<LOGN, LOGE, LAZY>), dim3(nb * L * L), dim3(G::T), G::LDS_USED, st, a);
    return (int)hipGetLastError();
}

// step 3 into a.prod
template <int LOGN, int LOGE>
static int ksf_stage_mac(hipStream_t st, const KsArgsF& a) {
    using G = Geom<LOGN, LOGE>;
    const dim3 grid((a.L + 1) * (G::N / 2) / 256, ksf_batch_lanes(a.nb));
    ksf_with_maxl(a.L, [&](auto M) { hipLaunchKernelGGL((k_ksf_mac<decltype(M)::value>), grid, dim3(256), 0, st, a, (u32)G::N); });
    return (int)hipGetLastError();
}

// step 3 with sigma_g inside the multiply-accumulate; d_pt: the rotation's plaintext (the plaintext modes). The identity that only
// stores is the keyswitch's own step 3
template <int LOGN, int LOGE>
static int ksf_stage_mac_galois(hipStream_t st, const KsArgsF& a, u32 g, KsfMacMode mode, const u64* d_pt) {
    using G = Geom<LOGN, LOGE>;
    if (g == 1 && mode == KSF_MAC_STORE) return ksf_stage_mac<LOGN, LOGE>(st, a);
    const HoistGeom h{LOGN, LOGE, G::KL, G::WB, g};
    const u32 wg = G::KL + 4 > 8 ? 1u << (G::KL + 4) : 256u;       // 2^KL rows of >= 16 adjacent words: whole 128-byte lines per workgroup
    static_assert(G::KL + 4 <= 9, "k_ksf_mac_galois is bounded at 512 threads");
    const dim3 grid((a.L + 1) * G::N / wg, ksf_batch_lanes(a.nb)), block(wg);
    ksf_with_maxl(a.L, [&](auto M) {
        constexpr int MAXL = decltype(M)::value;
        if (mode == KSF_MAC_STORE)         hipLaunchKernelGGL((k_ksf_mac_galois<MAXL, KSF_MAC_STORE>), grid, block, 0, st, a, h);
        else if (mode == KSF_MAC_PT_FIRST) hipLaunchKernelGGL((k_ksf_mac_galois<MAXL, KSF_MAC_PT_FIRST>), grid, block, 0, st, a, h, d_pt);
        else                               hipLaunchKernelGGL((k_ksf_mac_galois<MAXL, KSF_MAC_PT_ACC>), grid, block, 0, st, a, h, d_pt);
    });
    return (int)hipGetLastError();
}

// step 3 of a giant step: the weighted sum of the stored baby products into a.prod, no keys
template <int LOGN, int LOGE>
static int ksf_stage_bsgs_sum(hipStream_t st, const KsArgsF& a, const HxBsgsTerm* d_terms, u32 n_terms) {
    using G = Geom<LOGN, LOGE>;
    const HoistGeom h{LOGN, LOGE, G::KL, G::WB, 1};
    hipLaunchKernelGGL(k_lt_bsgs_sum, dim3((a.L + 1) * G::N / 256, ksf_batch_lanes(a.nb)), dim3(256), 0, st, a, h, d_terms, n_terms);
    return (int)hipGetLastError();
}

// step 4 (steps & 1) and steps 5-7 (steps & 2) on a.prod, into a.result
// (the fusion of steps 1-2 applied here -- s' in registers, L mod-down transforms per workgroup -- measured 8 % slower
// than the two kernels: its epilogue loads cannot be requested early, tools/experiments/fused_down.patch)
template <int LOGN, int LOGE, int LAZY>
static int ksf_stage_down(hexl_ctx* c, hipStream_t st, const KsArgsF& a, int steps = 3) {
    using G = Geom<LOGN, LOGE>;
    if (int rc = hx_lds_optin<k_ksf_intt_sp<LOGN, LOGE, LAZY>, k_ksf_moddown<LOGN, LOGE, LAZY>>(c->device, G::LDS_USED)) return rc;
    if (steps & 1) hipLaunchKernelGGL((k_ksf_intt_sp<LOGN, LOGE, LAZY>), dim3(a.nb * 2), dim3(G::T), G::LDS_USED, st, a);
    if (steps & 2) hipLaunchKernelGGL((k_ksf_moddown<LOGN, LOGE, LAZY>), dim3(a.nb * a.L * 2), dim3(G::T), G::LDS_USED, st, a);
    return (int)hipGetLastError();
}

template <int LOGN, int LOGE, int LAZY>
static int run_chunk_f64(hexl_ks_plan* p, const KsArgsF& a, int stage_mask, hipEvent_t* ev) {
    using G = Geom<LOGN, LOGE>;
    hexl_ctx* c = p->ctx;
    hipStream_t st = p->cur;
    const u32 L = a.L, nb = a.nb;
    // latency path (three kernels, above): a LONE keyswitch. Measured (tools/batch_sweep.py, N = 16384, device-resident): 70.3 us
    // against 72.5 us for the five kernels at L = 6, 72.2 against 73.2 at L = 7 -- the four dependent transforms, ~14 us each for a
    // lone workgroup (9-10 us of FP64 issue on ONE CU + a cold 128 KiB load + a kernel boundary), are what bounds it, not the
    // kernel count; from two keyswitches up the five kernels win (their per-(slot, d) workgroups skip the redundant special-limb
    // inverse: 73.5 against 78.3 us at two, 78.4 against 96.9 at four). HEXL_KS_LAT=0 turns it off, 1 forces it for every batch
    // that takes this pipeline (tests).
    // Not for N = 32768 (no registers for the key rows beside 64 data registers); timing runs (ev) keep the five-kernel path,
    // whose stages the events bracket.
    const int lat = hx_knob_ks_lat();
    if constexpr (!G::HALF_ONLY)
    if (!ev && stage_mask == 7 && L <= 15 && (lat == 1 || (lat != 0 && nb == 1))) {
        if (int rc = hx_lds_optin<k_ksl_intt<LOGN, LOGE, LAZY>, k_ksl_up<LOGN, LOGE, LAZY>, k_ksl_down<LOGN, LOGE, LAZY>>(c->device, G::LDS_USED))
            return rc;
        hipLaunchKernelGGL((k_ksl_intt<LOGN, LOGE, LAZY>), dim3(nb * L), dim3(G::T), G::LDS_USED, st, a);
        hipLaunchKernelGGL((k_ksl_up<LOGN, LOGE, LAZY>), dim3(nb * (L + 1) * L), dim3(G::T), G::LDS_USED, st, a);
        hipLaunchKernelGGL((k_ksl_down<LOGN, LOGE, LAZY>), dim3(nb * 2 * L), dim3(G::T), G::LDS_USED, st, a);
        return (int)hipGetLastError();
    }
    // timing stages: 1 = steps 1-2 (inverse + mod-up transforms), 2 = steps 3-4, 4 = steps 5-7
    if (ev) HX_CHECK(hipEventRecord(ev[0], st));
    if (stage_mask & 1)
        if (int rc = ksf_stage_up<LOGN, LOGE, LAZY, false>(c, st, a)) return rc;
    if (ev) HX_CHECK(hipEventRecord(ev[1], st));
    if (stage_mask & 2) {
        if (int rc = ksf_stage_mac<LOGN, LOGE>(st, a)) return rc;
        if (int rc = ksf_stage_down<LOGN, LOGE, LAZY>(c, st, a, 1)) return rc;
    }
    if (ev) HX_CHECK(hipEventRecord(ev[2], st));
    if (stage_mask & 4)
        if (int rc = ksf_stage_down<LOGN, LOGE, LAZY>(c, st, a, 2)) return rc;
    if (ev) HX_CHECK(hipEventRecord(ev[3], st));
    return 0;
}

size_t hx_ks_f64_scratch_words(size_t L) { return L + (L + 1) * L + 2 * (L + 1) + 2; }   // per instance, in units of n

// constants, tables and keys of `p`; scratch (the chunk `mem->cur_scratch` points at) and range flag of `mem` -- the same plan, except for
// the hoisted callers, where every rotation's plan works in plans[0]'s scratch
static KsArgsF ksf_args(const hexl_ks_plan* p, const hexl_ks_plan* mem, u64* d_result, const u64* d_t_target, size_t nb) {
    const size_t n = p->n, L = p->L;
    KsArgsF a;
    a.mods = p->d_mods_f64; a.tables = p->d_tables_f64; a.keys = p->d_keys_f64;
    a.c = (double*)mem->cur_scratch;
    a.u = a.c + mem->cap * L * n;
    a.prod = a.u + mem->cap * (L + 1) * L * n;
    a.s = a.prod + mem->cap * 2 * (L + 1) * n;
    a.t_target = d_t_target; a.result = d_result;
    a.L = (u32)L; a.K = p->K; a.nb = (u32)nb;
    a.range_flag = mem->d_flag;
    a.overwrite = p->overwrite_result ? 1u : 0u;
    a.skip = p->x_skip ? 1u : 0u;
    a.tiermap = hx_tiermap(p);
    return a;
}
// the tier of the kernels a plan's chunks run on: see hx_launch_keyswitch_f64
static int ksf_lazy(const hexl_ks_plan* p) {
    static const bool lookup = hx_knob_ks_per_limb() == 2;
    return p->mixed && lookup ? -1 : p->f64_lazy;
}

int hx_launch_keyswitch_f64(hexl_ks_plan* p, u64* d_result, const u64* d_t_target, size_t nb, int stage_mask,
                            hipEvent_t* ev) {
    const KsArgsF a = ksf_args(p, p, d_result, d_t_target, nb);
    // Limbs of different tiers: the kernels built with LAZY = -1 look the schedule up per transform (with_tier). They are NOT the default
    // here: this pipeline serves the batches that do not fill the chip, where latency binds, not FP64 issue, and a kernel that carries
    // two to four copies of its transforms spills (k_ksf_moddown 80 registers, k_ksl_up 116) -- bridge-seal's chain at 2 ... 48 instances runs
    // 1-12 % FASTER on the plan-wide tier (round 5, tools/seal_chain_rate.py; 4 instances: 44.3 k against 38.9 k keyswitch/s). The slot-major
    // pipeline (one launch per tier group, +14 %) and the lone-keyswitch kernels keep their per-limb tiers. HEXL_KS_PER_LIMB=2 selects the
    // per-transform lookup here as well (tests).
    // LAZY template argument = forward reduction period (f64_arith.hpp): 3 when every modulus <= 2^51(1+2^-7), 6 / 12
    // for moduli <= 2^50 / 2^49 (N = 16384 only; the smaller transforms keep 3), 0 = strict
    return hx_with_f64_geom(p->logn, ksf_lazy(p), [&](auto N, auto E, auto Z) { return run_chunk_f64<N, E, Z>(p, a, stage_mask, ev); });
}

// ---- the hoisted callers: many rotations of one ciphertext batch share the keyswitch's steps 1-2 (hexl_rotate_hoisted,
// hexl_linear_transform, hexl_linear_transform_bsgs). One run works in p0's keyswitch scratch, chunk after chunk, everything on the
// context's stream: one lane, so nothing has to be joined and the next mod-up overwrites u behind the last multiply-accumulate that read
// it. The stage methods take the plan whose keys (mac) or whose constants and tier (down) the kernels use; u, prod, s' and the range flag
// are always p0's. ----
struct HoistRun {
    hexl_ks_plan* p0;
    hexl_ctx* c;
    size_t chunk, per;                                             // instances per chunk; words of one ciphertext, 2 L n

    HoistRun(hexl_ks_plan* p, size_t chunk_) : p0(p), c(p->ctx), chunk(chunk_), per(2 * size_t(p->L) * p->n) {}
    // p0's keyswitch scratch, grown as hx_launch_keyswitch grows it
    int reserve() {
        if (int rc = hx_ks_reserve_scratch(p0, chunk)) return rc;
        p0->cur = c->stream;
        p0->cur_scratch = p0->d_scratch;
        return 0;
    }
    // steps 1-2 on d_c1 = component 1 of nb ciphertexts [nb][2][L][n], read in place, into u
    int up(const u64* d_c1, size_t nb) const {
        const KsArgsF a = ksf_args(p0, p0, nullptr, d_c1, nb);
        return hx_with_f64_geom(p0->logn, ksf_lazy(p0), [&](auto N, auto E, auto Z) { return ksf_stage_up<N, E, Z, true>(c, c->stream, a); });
    }
    // step 3 of one rotation with the keys of `keys`: sigma_g(u) . key into prod (`mode`, d_pt: KsfMacMode), or into `prod` when given.
    // (No transform, so no tier: only the geometry is dispatched on, here and in sum)
    int mac(const hexl_ks_plan* keys, u32 g, KsfMacMode mode, const u64* d_pt, double* prod, size_t nb) const {
        KsArgsF a = ksf_args(keys, p0, nullptr, nullptr, nb);
        if (prod) a.prod = prod;
        return hx_with_f64_geom(p0->logn, 0, [&](auto N, auto E, auto) { return ksf_stage_mac_galois<N, E>(c->stream, a, g, mode, d_pt); });
    }
    // step 3 of a giant step: the weighted sum of stored products into prod
    int sum(const HxBsgsTerm* d_terms, size_t n_terms, size_t nb) const {
        const KsArgsF a = ksf_args(p0, p0, nullptr, nullptr, nb);
        return hx_with_f64_geom(p0->logn, 0, [&](auto N, auto E, auto) { return ksf_stage_bsgs_sum<N, E>(c->stream, a, d_terms, (u32)n_terms); });
    }
    // steps 4-7 on prod with the constants and on the tier of `tier`, ADDED into d_out (whatever the plan's overwrite_result says)
    int down(const hexl_ks_plan* tier, u64* d_out, size_t nb) const {
        KsArgsF a = ksf_args(tier, p0, d_out, nullptr, nb);
        a.overwrite = 0;
        return hx_with_f64_geom(p0->logn, ksf_lazy(tier), [&](auto N, auto E, auto Z) { return ksf_stage_down<N, E, Z>(c, c->stream, a); });
    }
};

// Arguments checked by hexl_rotate_hoisted (ckks_ops.hip). Per chunk: the mod-up of c1 on plans[0]'s tier, then per rotation
// (sigma_g(c0), 0) into its output, its multiply-accumulate and steps 4-7 on ITS plan's tier, accumulated into the output.
int hx_launch_rotate_hoisted(hexl_ks_plan* const* plans, const u64* galois_elts, size_t n_rot, u64* const* d_outs, const u64* d_ct,
                             size_t batch) {
    hexl_ks_plan* p0 = plans[0];
    HoistRun run(p0, hx_ks_chunk_of(p0, batch));
    if (int rc = run.reserve()) return rc;
    const size_t half = run.per / 2;
    return hx_for_chunks(batch, run.chunk, [&](size_t b0, size_t nb) {
        const u64* ct = d_ct + b0 * run.per;
        if (int rc = run.up(ct + half, nb)) return rc;
        for (size_t r = 0; r < n_rot; ++r) {
            const u32 g = (u32)galois_elts[r];
            u64* out = d_outs[r] + b0 * run.per;
            if (int rc = hx_launch_galois_c0(run.c, out, ct, nb, p0->L, p0->logn, g)) return rc;
            if (int rc = run.mac(plans[r], g, KSF_MAC_STORE, nullptr, nullptr, nb)) return rc;
            if (int rc = run.down(plans[r], out, nb)) return rc;
        }
        return 0;
    });
}

// Arguments checked by hexl_linear_transform (ckks_ops.hip). Per chunk, all on plans[0]'s tier: the shared mod-up, the plaintext-weighted
// c0 / identity terms into d_out (hx_launch_galois_c0_pt), one multiply-accumulate launch per rotation into plans[0]'s prod (plan r's
// keys), then the special-prime inverse and the mod-down ONCE, added into d_out.
int hx_launch_linear_transform(hexl_ks_plan* const* plans, const u64* galois_elts, const u64* const* d_pts, size_t n_rot,
                               const u64* d_pt_identity, u64* d_out, const u64* d_ct, size_t batch) {
    hexl_ks_plan* p0 = plans[0];
    HoistRun run(p0, hx_ks_chunk_of(p0, batch));
    if (int rc = run.reserve()) return rc;
    hexl_ctx* c = run.c;
    // the per-call table of the c0 kernel. The source is pageable host memory: the copy has left it when hipMemcpyAsync returns, and
    // the stream orders it behind the previous call's kernels that read the table
    std::vector<HxLtRot> table(n_rot);
    for (size_t r = 0; r < n_rot; ++r) table[r] = HxLtRot{d_pts[r], galois_elts[r]};
    if (int rc = c->d_shared.reserve(n_rot * sizeof(HxLtRot))) return rc;
    HX_CHECK(hipMemcpyAsync(c->d_shared, table.data(), n_rot * sizeof(HxLtRot), hipMemcpyHostToDevice, c->stream));
    const size_t half = run.per / 2;
    return hx_for_chunks(batch, run.chunk, [&](size_t b0, size_t nb) {
        const u64* ct = d_ct + b0 * run.per;
        u64* out = d_out + b0 * run.per;
        if (int rc = run.up(ct + half, nb)) return rc;
        if (int rc = hx_launch_galois_c0_pt(p0, out, ct, (const HxLtRot*)c->d_shared.get(), n_rot, d_pt_identity, nb, p0->L, p0->d_flag)) return rc;
        for (size_t r = 0; r < n_rot; ++r)
            if (int rc = run.mac(plans[r], (u32)galois_elts[r], r ? KSF_MAC_PT_ACC : KSF_MAC_PT_FIRST, d_pts[r], nullptr, nb)) return rc;
        return run.down(p0, out, nb);
    });
}

// ---- baby-step/giant-step linear transform (hexl_linear_transform_bsgs): out = sum_j Rot_{G_j}( sum_i pt_{j,i} . Rot_{g_i}(ct) ) ----
static size_t bsgs_slice_bytes(const hexl_ks_plan* p) { return 2 * (size_t(p->L) + 1) * p->n * sizeof(double); }   // one baby step, one instance
size_t hx_lt_bsgs_chunk(const hexl_ks_plan* p, size_t n_baby, size_t batch) {
    const size_t chunk = hx_ks_chunk_of(p, batch);
    if (hx_ks_chunk_forced() || !n_baby || !chunk) return chunk;   // a forced chunk stays
    const size_t fit = HX_LT_BSGS_STORE_BYTES / bsgs_slice_bytes(p) / n_baby;
    return fit >= chunk ? chunk : fit ? fit : 1;
}
size_t hexl_lt_bsgs_scratch_bytes(const hexl_ks_plan* p, size_t n_baby, size_t batch) {
    if (!p) return 0;
    const size_t chunk = hx_lt_bsgs_chunk(p, n_baby, batch);
    const size_t fixed = 2 * size_t(p->L) * p->n * sizeof(u64) + hexl_ks_scratch_bytes(p, 1);   // t_j and the keyswitch scratch, per instance
    if (chunk && n_baby > (SIZE_MAX / chunk - fixed) / bsgs_slice_bytes(p)) return SIZE_MAX;
    return chunk * (n_baby * bsgs_slice_bytes(p) + fixed);
}

// Arguments checked by hexl_linear_transform_bsgs (ckks_ops.hip). Per chunk:
//   the mod-up of c1 once; one multiply-accumulate per baby step that some row uses, its prod pointed at that step's slice of the baby store
//   (u is free after the last of them);
//   per giant step j: the key-free part of row j into t_j (hx_launch_galois_c0_pt), the weighted sum of the stored products into prod
//   (k_lt_bsgs_sum) and the mod-down ONCE, added into t_j -- hexl_linear_transform's words for row j; then t_j rotated by G_j as
//   hexl_rotate_hoisted rotates it (mod-up of t_j's component 1 into the same u, giant_plans[j]'s keys and tier) with the key-free part
//   sigma_{G_j}(t_j[0]) WRITTEN to d_out by the first giant step and ADDED by the later ones, and the mod-down accumulating on top.
//   G_j = 1: t_j itself is written (the first giant step computes it in place in d_out) or added.
// Everything but a rotated giant step's steps 4-7 runs on p0's tier. Every word that reaches d_out is canonical and every addition is
// modulo q_i, so d_out holds the sum of the per-row results of the two parent entry points, word for word.
int hx_launch_linear_transform_bsgs(hexl_ks_plan* p0, hexl_ks_plan* const* baby_plans, const u64* baby_elts, size_t n_baby,
                                    hexl_ks_plan* const* giant_plans, const u64* giant_elts, size_t n_giant, const u64* const* d_pts,
                                    const u64* const* d_pt_identity, u64* d_out, const u64* d_ct, size_t batch) {
    HoistRun run(p0, hx_lt_bsgs_chunk(p0, n_baby, batch));
    if (int rc = run.reserve()) return rc;
    hexl_ctx* c = run.c;
    const size_t chunk = run.chunk, half = run.per / 2, slice = 2 * (size_t(p0->L) + 1) * p0->n;
    if (n_baby)
        if (int rc = p0->d_bsgs_b.reserve(n_baby * chunk * slice)) return rc;
    if (int rc = p0->d_bsgs_t.reserve(chunk * run.per)) return rc;
    // the per-call tables, row after row: what the c0 kernel walks (plaintext, Galois element) and what the sum kernel walks (plaintext,
    // baby slice). Pageable sources, stream-ordered behind the previous call's readers, as hx_launch_linear_transform's table
    std::vector<HxLtRot> rots;
    std::vector<HxBsgsTerm> terms;
    std::vector<size_t> off(n_giant + 1);
    std::vector<char> used(n_baby, 0);
    for (size_t j = 0; j < n_giant; ++j) {
        off[j] = rots.size();
        for (size_t i = 0; i < n_baby; ++i)
            if (const u64* pt = d_pts[j * n_baby + i]) {
                rots.push_back(HxLtRot{pt, baby_elts[i]});
                terms.push_back(HxBsgsTerm{pt, p0->d_bsgs_b + i * chunk * slice});
                used[i] = 1;
            }
    }
    const size_t total = off[n_giant] = rots.size();
    static_assert(sizeof(HxLtRot) == 16 && sizeof(HxBsgsTerm) == 16, "the two tables share one 16-byte-aligned reservation");
    if (total) {
        if (int rc = c->d_shared.reserve(total * (sizeof(HxLtRot) + sizeof(HxBsgsTerm)))) return rc;
        HX_CHECK(hipMemcpyAsync(c->d_shared, rots.data(), total * sizeof(HxLtRot), hipMemcpyHostToDevice, c->stream));
        HX_CHECK(hipMemcpyAsync((HxLtRot*)c->d_shared.get() + total, terms.data(), total * sizeof(HxBsgsTerm), hipMemcpyHostToDevice, c->stream));
    }
    const HxLtRot* d_rots = (const HxLtRot*)c->d_shared.get();
    const HxBsgsTerm* d_terms = (const HxBsgsTerm*)(d_rots + total);
    return hx_for_chunks(batch, run.chunk, [&](size_t b0, size_t nb) {
        const u64* ct = d_ct + b0 * run.per;
        u64* out = d_out + b0 * run.per;
        if (total) {
            if (int rc = run.up(ct + half, nb)) return rc;
            for (size_t i = 0; i < n_baby; ++i)
                if (used[i])
                    if (int rc = run.mac(baby_plans[i], (u32)baby_elts[i], KSF_MAC_STORE, nullptr, p0->d_bsgs_b + i * chunk * slice, nb)) return rc;
        }
        for (size_t j = 0; j < n_giant; ++j) {
            const size_t cnt = off[j + 1] - off[j];
            const u32 g = (u32)giant_elts[j];
            u64* t = (j == 0 && g == 1) ? out : p0->d_bsgs_t;
            if (int rc = hx_launch_galois_c0_pt(p0, t, ct, d_rots + off[j], cnt, d_pt_identity ? d_pt_identity[j] : nullptr, nb, p0->L, p0->d_flag)) return rc;
            if (cnt) {
                if (int rc = run.sum(d_terms + off[j], cnt, nb)) return rc;
                if (int rc = run.down(p0, t, nb)) return rc;        // accumulated into what the c0 kernel wrote
            }
            if (g == 1) {
                if (j)
                    if (int rc = hx_launch_galois_add(p0, out, t, nb, 1, 2, p0->L)) return rc;
                continue;
            }
            if (int rc = run.up(t + half, nb)) return rc;           // the babies are stored: u is free
            if (int rc = j ? hx_launch_galois_add(p0, out, t, nb, g, 1, p0->L) : hx_launch_galois_c0(c, out, t, nb, p0->L, p0->logn, g)) return rc;
            if (int rc = run.mac(giant_plans[j], g, KSF_MAC_STORE, nullptr, nullptr, nb)) return rc;
            if (int rc = run.down(giant_plans[j], out, nb)) return rc;
        }
        return 0;
    });
}
