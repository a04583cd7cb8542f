// keyswitch_hybrid.hip -- the hybrid key switch: alpha data limbs per digit, n_p = K - L special primes, ONE installed
// key for every level. A pipeline of its own beside the per-limb gadget of keyswitch_f64.hip / keyswitch_x.hip, attached to an FP64 plan
// (hexl_hks borrows the plan's context, stream, moduli, constants and tables, and owns its keys, conversion constants and scratch).
// Per chunk of instances at level l (T_l = {0 .. l-1} + S, S = {L .. K-1}, dl = ceil(l / alpha) digits), every line modulo its limb:
//   1   a_i = INTT_i(t[i]), canonical words; ext_d[i] = t[i] for the digit d that holds i                              k_hks_intt
//   2a  y_i = a_i (D/q_i)^-1;  x_d[j] = sum_{i in G_d} y_i (D/q_i mod q_j)  for every j in T_l outside the digit       k_hks_conv<UP>
//   2b  ext_d[j] = NTT_j(x_d[j]), in place                                                                             k_hks_fwd
//   3   acc[k][j] = sum_d ext_d[j] key[d][k][j]                                                                        k_hks_mac
//   4a  b_s = (INTT_s(acc[k][s]) + floor(P/2)) mod q_s for s in S, in place                                            k_hks_down_intt<false>
//   4b  w_i = sum_s b_s (P/q_s)^-1 (P/q_s mod q_i) + fix_i  for i < l                                                  k_hks_conv<DOWN>
//   4c  result[k][i] += (acc[k][i] - NTT_i(w_i)) P^-1                                                                   k_hks_down<false>
// The hybrid multiply (hexl_hks_relinearize_rescale, hexl_hks_multiply_sum_rescale) replaces step 4 by ONE mod-down that
// divides X_k = P d_k + KSacc_k by R = P q_(l-1), from the source basis B = S + {l - 1} into the limbs i < l - 1 -- the same three kernels
// with RS set, on the rows of the constants that belong to R:
//   4a' b_s = (INTT_s(acc'[k][s]) + floor(R/2)) mod q_s for s in B, in place; acc'[k][l-1] = acc[k][l-1] + (P mod q) d_k[l-1]    k_hks_down_intt<true>
//   4b' w_i = sum_{s in B} b_s (R/q_s)^-1 (R/q_s mod q_i) + fix_i  for i < l - 1                                        k_hks_conv<RS>
//   4c' out[k][i] = (acc[k][i] + (P mod q_i) d_k[i] - NTT_i(w_i)) R^-1, WRITTEN, [2][l - 1][n]                            k_hks_down<true>
// The hoisted callers (hexl_hks_rotate_hoisted, hexl_hks_linear_transform) run steps 1-2 ONCE per chunk on c1 of the
// ciphertexts, read in place, and step 3 per rotation with sigma_g applied to ext on the way in and the keys of that rotation's object:
//   3g  acc[k][j] = sum_d sigma_g(ext_d[j]) key_r[d][k][j]   (stored, or weighted by a plaintext and summed over the rotations)   k_hks_mac, a mode with HksRot
// The double-hoisted BSGS (hexl_hks_linear_transform_bsgs_ext) keeps the giant steps in the extended basis as well: per
// rotated row ONE half mod-down (steps 4a-4c on component 1 alone: the C1 forms of the three kernels), a second mod-up, and
//   3G  A[k][j] += sum_d sigma_G(ext'_d[j]) key_G[d][k][j]                                                              k_hks_mac, HKS_MAC_ACC
//   3s  A[0][j] += sigma_G(inner[0][j]) on every row of T_l, the special rows included                                 k_hks_ext_add
// and ONE mod-down of A per call, by P or -- with the rescale folded in -- by R with d_k = F_k, the key-free sums.
// The transforms are one workgroup per polynomial on WgNttF64, limb-major, as k_rns_fwd / k_rns_inv (rns_ops.hip) and k_rs_intt /
// k_rs_down (ckks_ops.hip); every intermediate lies at its LOGICAL index (coefficients in natural order, NTT form in the transforms'
// output order), so the word-wise kernels between them need no index map and the keys keep the caller's order. The scalar chains
// are f64_arith.hpp's hks_* functions (tests/cpp/hks_selftest.cpp replays them against __int128).
#include "hexl_internal.hpp"
#include "ntt_core_f64.hpp"
#include "number_theory.hpp"

using namespace hx;

constexpr u32 HKS_MAX_LIMBS = 16;                                 // hexl_ks_plan::tier has 16 limbs
// The base conversions of every level, one CONVERSION ROW of the source and weight tables each:
//   row l - 1        the mod-up of level l (sources: the limbs of a digit; targets: T_l outside the digit)
//   row 16           the mod-down by P, the same at every level (sources S; targets the data limbs)
//   row 16 + (l - 1) the rescaling mod-down of level l >= 2 (sources S and the limb l - 1; targets i < l - 1)
// and one DIVISOR ROW of the third table per divisor of a mod-down: row 0 for P, row l - 1 for R = P q_(l-1).
enum HksConv : int { HKS_CONV_UP, HKS_CONV_DOWN, HKS_CONV_RS, HKS_CONV_DOWN1 };   // DOWN1: the mod-down by P of component 1 alone
constexpr u32 HKS_CONV_ROWS = 2 * HKS_MAX_LIMBS;
struct HksSrc { double hinv, hinv_p; };                           // (D / q_i)^-1 mod q_i centred, and fl(. / q_i)
struct HksWt { double w, wp; };                                   // (D / q_i) mod q_j centred, and fl(. / q_j)
struct HksDiv {                                                   // per (divisor Q = P or R, plan limb)
    double inv, inv_p;       // a target limb i: Q^-1 mod q_i centred, fl(. / q_i)
    double fix;              // a target limb i: q_i - (floor(Q/2) mod q_i), in [1, q_i]
    double half;             // a source limb s: floor(Q/2) mod q_s
    double pm, pm_p;         // Q = R, i < l: P mod q_i centred, fl(. / q_i)
};
static size_t hks_conv_row(HksConv mode, u32 l) { return mode == HKS_CONV_UP ? l - 1 : mode == HKS_CONV_RS ? HKS_MAX_LIMBS + (l - 1) : HKS_MAX_LIMBS; }
static size_t hks_div_row(HksConv mode, u32 l) { return mode == HKS_CONV_RS ? l - 1 : 0; }

struct hexl_hks {
    hexl_ks_plan* plan = nullptr;
    u32 alpha = 0, dnum = 0, np = 0;
    bool have_keys = false;
    HxDevBuf<double> d_keys;          // [dnum][2][K][n] centred, the caller's order
    double p_mod[HKS_MAX_LIMBS] = {}; // [K]: P mod q_i canonical (host; hexl_hks_keygen's plaintext weight, keygen.hip)
    HxDevBuf<HksSrc> d_src;           // [32][16]: (conversion row, source limb)
    HxDevBuf<HksWt> d_wt;             // [32][16][16]: (conversion row, source limb, target limb)
    HxDevBuf<HksDiv> d_div;           // [16][16]: (divisor row, plan limb)
    // scratch of one chunk, grow-only (the stream drain rule of the context: everything runs on its stream)
    HxDevBuf<u64> d_coef;             // [chunk][L][n]        a_i, canonical, natural order; after step 3: w of component 0 (doubles)
    HxDevBuf<double> d_ext;           // [chunk][dnum][K][n]  x_d, then ext_d; after step 3 its first l rows per instance: w of component 1
                                      //                      (the hoisted callers keep ext for the next rotation: d_w1)
    HxDevBuf<double> d_acc;           // [chunk][2][K][n]     acc; rows of S: b_s after step 4a
    HxDevBuf<u64> d_slice;            // rotate / relinearize: the key switch's input of one slice, [slice][L][n]
    HxDevBuf<double> d_w1;            // the hoisted callers: w of component 1, [chunk][L][n] (grow-only, allocated at their first call)
    // hexl_hks_linear_transform_bsgs, both grow-only and allocated at its first call
    HxDevBuf<double> d_bsgs_b;        // baby store: [n_baby][chunk][2][K][n], slice i = the stored sums of baby step i, [nb][2][T][n] of it used
    HxDevBuf<u64> d_bsgs_t;           // one giant step's inner sum t_j: [chunk][2][L][n] canonical words ([nb][2][l][n] of it used)
    HxDevBuf<u64> d_d01;              // hexl_hks_multiply_sum_rescale: (d0, d1) of one chunk's tensor sums, [chunk][2][L][n] (grow-only,
                                      // [nb][2][l][n] of it used; allocated at its first call)
                                      // hexl_hks_linear_transform_bsgs_ext with rescale = 1: F, the key-free sums of one chunk, the same shape
    HxDevBuf<double> d_ext_a;         // hexl_hks_linear_transform_bsgs_ext: A, the giant steps' sum in the extended basis, [chunk][2][K][n]
                                      // ([nb][2][T][n] of it used; grow-only, allocated at its first call)
    explicit hexl_hks(hexl_ks_plan* p)
        : plan(p), d_keys(p->ctx), d_src(p->ctx), d_wt(p->ctx), d_div(p->ctx), d_coef(p->ctx), d_ext(p->ctx), d_acc(p->ctx), d_slice(p->ctx),
          d_w1(p->ctx), d_bsgs_b(p->ctx), d_bsgs_t(p->ctx), d_d01(p->ctx), d_ext_a(p->ctx) {}
};

struct HksArgs {
    const KsModF64* mods;       // [K]
    const double* tables;       // [K][4][n] (keyswitch_f64.hip KsArgsF)
    const HksSrc* src;          // [16]: the conversion row of the launch (hks_point_rows: the level's mod-up, or the stage's mod-down)
    const HksWt* wt;            // [16][16]: the same row
    const void* reserved;       // never set or read (see the assertion behind the struct)
    const HksDiv* div;          // [16]: the divisor row of the launch
    const double* keys;        // [dnum][2][K][n]
    const u64* t;               // [nb][tstride][n], rows 0 ... l - 1 of an instance are read (tstride = l, or 2 l for c1 of a ciphertext in place)
    u64* result;                // [nb][2][l][n] (the rescaling mod-down: [nb][2][l - 1][n])
    const u64* d01;             // the rescaling mod-down: word of (d_k, instance b, limb i) at d01 + b d01_stride + (k l + i) n
    unsigned long long d01_stride;
    u64* coef;                  // [nb][l][n]
    double* ext;                // [nb][dl][T][n]
    double* acc;                // [nb][2][T][n]
    double* w1;                 // [nb][l][n]: w of component 1 (the hoisted callers); nullptr: the first rows of the instance's ext block
    u32 L, K, l, T, dl, alpha, nb, logn, tstride;
    unsigned long long limbmap; // nibble jT = plan limb of row jT of T_l (T_l is not a prefix of the plan's limbs when l < L)
    unsigned long long tiermap; // LAZY = -1: nibble i = reduction period of limb i (keyswitch_f64.hip)
};
// the kernels of steps 1-3 do not read the divisor constants and keep the instruction streams they had while every field they load keeps
// its kernel-argument offset: `reserved` stands where the second of the two former constants pointers stood
static_assert(offsetof(HksArgs, div) == 40 && offsetof(HksArgs, keys) == 48 && sizeof(HksArgs) == 176, "HksArgs: kernel-argument offsets");
__device__ __forceinline__ u32 hks_limb(const HksArgs& a, u32 jT) { return u32(a.limbmap >> (4 * jT)) & 15u; }
// w of (instance b, component k, limb i): component 0 in the coefficient buffer, component 1 in the first rows of the instance's ext block
// (both are dead once step 3 has run, and dl * T >= l) -- or in a buffer of its own where ext has to survive step 4 (uniform)
__device__ __forceinline__ double* hks_w(const HksArgs& a, u32 b, u32 k, u32 i, size_t n) {
    if (k == 0) return reinterpret_cast<double*>(a.coef) + (size_t(b) * a.l + i) * n;
    return a.w1 ? a.w1 + (size_t(b) * a.l + i) * n : a.ext + (size_t(b) * a.dl * a.T + i) * n;
}

struct HksFwdOpt : NttOpt { static constexpr int XSD = 0; };      // centred inputs, FINAL's range reduction behind the tail (rns_ops.hip RnsFwdOpt)

// step 1, one workgroup per (limb i < l, instance): k_rns_inv with the digit's own row of ext written on the way in
template <int LOGN, int LOGE, int LAZY>
__global__ __launch_bounds__(1 << (LOGN - LOGE)) void k_hks_intt(HksArgs a) {
    using G = Geom<LOGN, LOGE>;
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const int tid = threadIdx.x;
    const u32 i = blockIdx.x / a.nb, b = blockIdx.x - i * a.nb;
    const KsModF64 md = a.mods[i];
    const Mod m = md.m;
    const double* tb = a.tables + size_t(i) * 4 * G::N;
    const u64* src = a.t + (size_t(b) * a.tstride + i) * G::N;
    const u32 tB = u32(G::idxB(0, tid));
    double v[G::E];
#pragma unroll
    for (int r = 0; r < G::E; ++r) v[r] = hxf::reduce(hxf::to_f64((src + G::idxB(r, 0))[tB]), m);
    // ext_d[i] = t[i] for the digit that holds i: NTT_i(x_d mod q_i) = t[i], no transform
    double* own = a.ext + ((size_t(b) * a.dl + i / a.alpha) * a.T + i) * G::N;
#pragma unroll
    for (int r = 0; r < G::E; ++r) (own + G::idxB(r, 0))[tB] = v[r];
    with_tier<LAZY, LOGN == 14>(a.tiermap, i, [&](auto T) {
        WgNttF64<LOGN, LOGE, decltype(T)::value, InvNoWpOpt<true>>::template inverse<true>(
            v, ldsd, tid, tb + 2 * G::N, tb + 3 * G::N, m, md.sc);
    });
    u64* dst = a.coef + (size_t(b) * a.l + i) * G::N;
#pragma unroll
    for (int r = 0; r < G::E; ++r) (dst + G::idxA(r, 0))[u32(tid)] = hxf::from_f64(hxf::lift(v[r], m));
}

// step 2b, one workgroup per (row jT of T_l, digit d, instance), in place: a workgroup holds its whole polynomial before it stores
// (the re-deals' barriers lie between the last load and the first store). Rows inside their own digit were written by k_hks_intt.
template <int LOGN, int LOGE, int LAZY>
__global__ __launch_bounds__(1 << (LOGN - LOGE)) void k_hks_fwd(HksArgs a) {
    using G = Geom<LOGN, LOGE>;
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const int tid = threadIdx.x;
    const u32 per = a.dl * a.nb;
    const u32 jT = blockIdx.x / per, rem = blockIdx.x - jT * per;
    const u32 d = rem / a.nb, b = rem - d * a.nb;
    if (jT < a.l && jT / a.alpha == d) return;                   // (uniform)
    const u32 j = hks_limb(a, jT);
    const Mod m = a.mods[j].m;
    const double* tb = a.tables + size_t(j) * 4 * G::N;
    double* row = a.ext + ((size_t(b) * a.dl + d) * a.T + jT) * G::N;
    double v[G::E];
#pragma unroll
    for (int r = 0; r < G::E; ++r) v[r] = hxf::reduce((row + G::idxA(r, 0))[u32(tid)], m);
    with_tier<LAZY, LOGN == 14>(a.tiermap, j, [&](auto T) {
        WgNttF64<LOGN, LOGE, decltype(T)::value, HksFwdOpt>::template forward<true, true>(v, ldsd, tid, tb, tb + G::N, m);
    });
    const u32 tB = u32(G::idxB(0, tid));
#pragma unroll
    for (int r = 0; r < G::E; ++r) (row + G::idxB(r, 0))[tB] = v[r];
}

// Steps 4a and 4c, and 4a' and 4c' of the rescaling calls (RS): the mod-down by the divisor Q whose row a.div is, Q = P or R = P q_(l-1).
// step 4a, one workgroup per (source row, instance, component), in place: b_s = (INTT_s(acc[k][s]) + floor(Q/2)) mod q_s, canonical.
// The sources are the rows of S; RS: one more per (instance, component), the data limb l - 1, which takes (P mod q) d_k on the way in
// (step 3'). That row of acc is dead for everything else: the rescaled output has no limb l - 1.
// C1 (with the divisor P only): component 1 alone, one workgroup per (source row, instance) -- the half mod-down that forms u_j of a
// rotated row of hexl_hks_linear_transform_bsgs_ext; component 0 of acc is neither read nor written.
template <int LOGN, int LOGE, int LAZY, bool RS, bool C1 = false>
__global__ __launch_bounds__(1 << (LOGN - LOGE)) void k_hks_down_intt(HksArgs a) {
    static_assert(!(RS && C1), "the half mod-down divides by P");
    using G = Geom<LOGN, LOGE>;
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const int tid = threadIdx.x;
    const u32 np = a.K - a.L;
    const u32 si = blockIdx.x / (C1 ? a.nb : 2 * a.nb), bk = C1 ? 2 * (blockIdx.x - si * a.nb) + 1 : blockIdx.x - si * 2 * a.nb;
    const bool data = RS && si == np;                            // (uniform)
    const u32 s = data ? a.l - 1 : a.L + si, jT = data ? a.l - 1 : a.l + si;
    const KsModF64 md = a.mods[s];
    const Mod m = md.m;
    const HksDiv dv = a.div[s];
    const double* tb = a.tables + size_t(s) * 4 * G::N;
    double* row = a.acc + (RS ? size_t(bk) * a.T + jT : size_t(bk) * a.T + a.l + si) * G::N;   // one row; each mode's own sum order
    const u32 tB = u32(G::idxB(0, tid));
    double v[G::E];
#pragma unroll
    for (int r = 0; r < G::E; ++r) v[r] = (row + G::idxB(r, 0))[tB];               // an hks_mac_term output: |v| <= q_s/2 + 2
    if (data) {
        const u64* dk = a.d01 + size_t(bk >> 1) * a.d01_stride + (size_t(bk & 1) * a.l + s) * G::N;
#pragma unroll
        for (int r = 0; r < G::E; ++r) v[r] = hxf::hks_acc_pd(v[r], hxf::to_f64((dk + G::idxB(r, 0))[tB]), dv.pm, dv.pm_p, m);
    }
    with_tier<LAZY, LOGN == 14>(a.tiermap, s, [&](auto T) {
        WgNttF64<LOGN, LOGE, decltype(T)::value, InvNoWpOpt<true>>::template inverse<true>(
            v, ldsd, tid, tb + 2 * G::N, tb + 3 * G::N, m, md.sc);
    });
#pragma unroll
    for (int r = 0; r < G::E; ++r) (row + G::idxA(r, 0))[u32(tid)] = hxf::hks_round(v[r], dv.half, m);
}

// step 4c, one workgroup per (target limb i, instance, component): k_rs_down's shape -- the transform of w, then the epilogue on acc and
// a second word, both requested behind the transform (k_rs_down's LAZY < 0 form). The second word is the one `result` holds, and the
// output is accumulated onto it, [2][l][n]; RS: it is d_k, which enters as (P mod q_i) d_k, and the output is WRITTEN, [2][l - 1][n].
// C1: component 1 alone, one workgroup per (target limb, instance); component 0 of `result` keeps its words.
template <int LOGN, int LOGE, int LAZY, bool RS, bool C1 = false>
__global__ __launch_bounds__(1 << (LOGN - LOGE)) void k_hks_down(HksArgs a) {
    static_assert(!(RS && C1), "the half mod-down divides by P");
    using G = Geom<LOGN, LOGE>;
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const int tid = threadIdx.x;
    const u32 i = blockIdx.x / (C1 ? a.nb : 2 * a.nb), bk = C1 ? 2 * (blockIdx.x - i * a.nb) + 1 : blockIdx.x - i * 2 * a.nb;
    const u32 b = bk >> 1, k = bk & 1;
    const Mod m = a.mods[i].m;
    const HksDiv dv = a.div[i];
    const double* tb = a.tables + size_t(i) * 4 * G::N;
    const double* w = hks_w(a, b, k, i, G::N);
    double v[G::E];
#pragma unroll
    for (int r = 0; r < G::E; ++r) v[r] = hxf::reduce((w + G::idxA(r, 0))[u32(tid)], m);
    with_tier<LAZY, LOGN == 14>(a.tiermap, i, [&](auto T) {
        WgNttF64<LOGN, LOGE, decltype(T)::value, HksFwdOpt>::template forward<true, true>(v, ldsd, tid, tb, tb + G::N, m);
    });
    const double* pk = a.acc + (size_t(bk) * a.T + i) * G::N;
    const u64* dk = RS ? a.d01 + size_t(b) * a.d01_stride + (size_t(k) * a.l + i) * G::N : nullptr;
    u64* res = a.result + (size_t(bk) * (RS ? a.l - 1 : a.l) + i) * G::N;
    const u64* second = RS ? dk : res;
    const u32 tB = u32(G::idxB(0, tid));
    // in groups of eight registers: beside the 2^LOGE words of w, all of acc and the second words do not fit the registers of N = 32768
    constexpr int GRP = G::E < 8 ? G::E : 8;
#pragma unroll
    for (int r0 = 0; r0 < G::E; r0 += GRP) {
        double pv[GRP];
        u64 sv[GRP];
#pragma unroll
        for (int r = 0; r < GRP; ++r) { pv[r] = (pk + G::idxB(r0 + r, 0))[tB]; sv[r] = (second + G::idxB(r0 + r, 0))[tB]; }
#pragma unroll
        for (int r = 0; r < GRP; ++r) {
            const double x = hxf::to_f64(sv[r]);
            (res + G::idxB(r0 + r, 0))[tB] = hxf::from_f64(RS ? hxf::hks_down_rs(x, pv[r], v[r0 + r], dv.pm, dv.pm_p, dv.inv, dv.inv_p, m)
                                                              : hxf::hks_down(x, pv[r], v[r0 + r], dv.inv, dv.inv_p, m));
        }
    }
}

// ---- the word-wise kernels: 256 lanes, a lane owns two adjacent indices (16-byte accesses), a workgroup 512 of them ----
constexpr u32 HKS_THREADS = 256, HKS_LOG_PIECE = 9;
static_assert(HKS_THREADS * 2 == 1u << HKS_LOG_PIECE, "a workgroup covers its piece exactly");
static_assert(HKS_THREADS == HX_WW_THREADS, "hx_ww_grid(., ., ., HKS_LOG_PIECE) counts these workgroups");

// steps 2a and 4b: the fast base conversion, no correction term. One workgroup per (instance, group, piece): group = digit d < dl
// (mod-up: sources the words a_i of G_d, targets every row of T_l outside the digit) or component k (DOWN: sources b_s, s in S, targets
// the data limbs i < l, fix_i added). Per coefficient the <= MAXS source words are loaded and y formed ONCE; every target limb reduces y
// into its own range before the products (hks_conv_term). Moduli and weights of a target are wave-uniform: scalar loads.
// HKS_CONV_RS is the mod-down of the rescaling calls: one more source per component, the row l - 1 of acc (limb l - 1, not contiguous
// with the special rows), one target fewer. a.src / a.wt / a.div are the rows of the launch's conversion and divisor (hks_point_rows).
// HKS_CONV_DOWN1 is HKS_CONV_DOWN on component 1 alone: one group per instance, w into d_w1 (hks_w with k = 1), coef untouched.
template <HksConv MODE, int MAXS>
__global__ __launch_bounds__(HKS_THREADS) void k_hks_conv(HksArgs a) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    typedef unsigned long long u2 __attribute__((ext_vector_type(2)));
    constexpr bool DOWN = MODE != HKS_CONV_UP, RS = MODE == HKS_CONV_RS;
    const u32 lp = a.logn - HKS_LOG_PIECE;
    const u32 grp = blockIdx.x >> lp, piece = blockIdx.x - (grp << lp);
    constexpr bool ONE = MODE == HKS_CONV_DOWN1;
    const u32 ng = ONE ? 1u : DOWN ? 2u : a.dl;
    const u32 b = grp / ng, g = ONE ? 1u : grp - b * ng;
    const size_t n = size_t(1) << a.logn, c = (size_t(piece) << HKS_LOG_PIECE) + 2 * threadIdx.x;
    const u32 s0 = DOWN ? a.L : g * a.alpha;                      // first source limb (plan index)
    const u32 ns = RS ? a.K - a.L + 1 : DOWN ? a.K - a.L : (a.l - s0 < a.alpha ? a.l - s0 : a.alpha);
    // source si: its plan limb, and (the mod-downs) its row of T_l in acc -- RS: the last source is the data limb l - 1
    auto src_limb = [&](u32 si) { return RS && si + 1 == ns ? a.l - 1 : s0 + si; };
    auto src_row = [&](u32 si) { return RS && si + 1 == ns ? a.l - 1 : a.l + si; };
    double y[MAXS][2];
#pragma unroll
    for (int si = 0; si < MAXS; ++si)
        if (si < (int)ns) {
            const u32 i = src_limb(si);
            const Mod m = a.mods[i].m;
            const HksSrc hs = a.src[i];
            double v[2];
            if constexpr (DOWN) {
                const d2 t = *reinterpret_cast<const d2*>(a.acc + ((size_t(b) * 2 + g) * a.T + src_row(si)) * n + c);
                v[0] = t.x; v[1] = t.y;
            } else {
                const u2 t = *reinterpret_cast<const u2*>(a.coef + (size_t(b) * a.l + i) * n + c);
                v[0] = hxf::to_f64(t.x); v[1] = hxf::to_f64(t.y);
            }
            y[si][0] = hxf::hks_digit(v[0], hs.hinv, hs.hinv_p, m);
            y[si][1] = hxf::hks_digit(v[1], hs.hinv, hs.hinv_p, m);
        }
    const u32 nt = RS ? a.l - 1 : DOWN ? a.l : a.T;
    for (u32 jT = 0; jT < nt; ++jT) {
        const u32 j = hks_limb(a, jT);
        if (!DOWN && j >= s0 && j < s0 + ns) continue;            // inside the digit: k_hks_intt wrote the row
        const Mod m = a.mods[j].m;
        double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
        for (int si = 0; si < MAXS; ++si)
            if (si < (int)ns) {
                const HksWt wt = a.wt[src_limb(si) * HKS_MAX_LIMBS + j];
                acc0 = hxf::hks_conv_term(acc0, y[si][0], wt.w, wt.wp, m);
                acc1 = hxf::hks_conv_term(acc1, y[si][1], wt.w, wt.wp, m);
            }
        const double fix = DOWN ? a.div[j].fix : 0.0;
        const d2 o = {hxf::hks_conv_finish(acc0, fix, m), hxf::hks_conv_finish(acc1, fix, m)};
        double* dst = DOWN ? hks_w(a, b, g, jT, n) : a.ext + ((size_t(b) * a.dl + g) * a.T + jT) * n;
        *reinterpret_cast<d2*>(dst + c) = o;
    }
}

// step 3: acc[b][k][jT] = sum_d ext[b][d][jT] . key[d][k][limb of jT], k_ksf_mac's structure with dl terms: a lane keeps the 2 dl key
// vectors of its two indices in registers and walks the batch, so the keys are read once per launch and ext / acc exactly once.
// step 3 of the hoisted callers, one rotation: sum[b][k][jT] = sum_d sigma_g(ext[b][d][jT]) . key_r[d][k][limb of jT] -- the same with ext
// gathered. ext lies at its logical index, so word j of sigma_g(ext) is word galois_src(j) of ext, no position map. pi_g maps every
// aligned block of 2^k indices onto an aligned block of 2^k (keyswitch_f64.hip k_ksf_mac_galois); with k = 1: the sources of a lane's two
// adjacent indices c, c + 1 are the two words of ONE aligned pair, s and s ^ 1 -- (2 brv(c + 1) + 1) g = (2 brv(c) + 1) g + n g, and
// n g = n (mod 2n) for an odd g, which flips the top bit of (e - 1) / 2 and so the lowest bit of the source. The gather is therefore one
// 16-byte load at s & ~1 and a swap when s is odd: keys, plaintext, acc AND ext stay 16-byte accesses, and a wave's 64 sources are the
// 1 KiB of one aligned block of 128 indices, whole cache lines in another order. g = 1 is served too (s = c, no swap).
// Where ext is read and what becomes of the reduced sum (an hks_mac_term output, i.e. a reduce output: what lt_mac / lt_mac_acc take
// as `inner`) is MODE:
//   HKS_MAC_PLAIN     the key switch: no galois_src, no swap, keys from a.keys, acc = sum
//   HKS_MAC_STORE     hexl_hks_rotate_hoisted: acc = sum
//   HKS_MAC_PT_FIRST  hexl_hks_linear_transform, a chunk's first rotation: acc = pt[limb of jT] . sum (hxf::lt_mac), acc is not read
//   HKS_MAC_PT_ACC    ... its later rotations: acc = acc + pt . sum (hxf::lt_mac_acc), the old words requested in front of the gather
// pt is [K][n] canonical words in the transforms' output order: the lane's pair is converted once (hxf::lt_pt) and serves every instance
// it walks. acc never leaves the extended basis between rotations, so step 4 runs once for all of them.
//   HKS_MAC_ACC       hexl_hks_linear_transform_bsgs_ext, a rotated giant step: acc = acc + sum (hxf::hks_ext_acc), no plaintext --
//                     PT_ACC's read-modify-write without the weight; a.acc points at A
struct HksRot { const double* keys; const u64* pt; u32 g; };      // the rotation's object's keys [dnum][2][K][n]; pt: the plaintext modes
enum HksMacMode : int { HKS_MAC_PLAIN, HKS_MAC_STORE, HKS_MAC_PT_FIRST, HKS_MAC_PT_ACC, HKS_MAC_ACC };

// ONE kernel template for both: ROT is empty for HKS_MAC_PLAIN -- the kernel's arguments are (HksArgs) alone, as the key switch's always
// were -- and {HksRot} for the other modes, (HksArgs, HksRot). `(rot, ...)` is that one HksRot; it is named only where MODE has one.
template <int MAXD, HksMacMode MODE, class... ROT>
__global__ __launch_bounds__(HKS_THREADS) void k_hks_mac(HksArgs a, ROT... rot) {
    static_assert(sizeof...(ROT) == (MODE == HKS_MAC_PLAIN ? 0 : 1), "HksRot goes with every mode but the plain one");
    typedef double d2 __attribute__((ext_vector_type(2)));
    typedef unsigned long long u2 __attribute__((ext_vector_type(2)));
    constexpr bool PT = MODE == HKS_MAC_PT_FIRST || MODE == HKS_MAC_PT_ACC;
    const u32 n = 1u << a.logn, pairs = n >> 1;
    const u32 gid = blockIdx.x * blockDim.x + threadIdx.x;        // (row of T_l, pair)
    const u32 jT = gid / pairs;
    if (jT >= a.T) return;
    const u32 c = (gid - jT * pairs) * 2;
    u32 sp = c;                                                   // the aligned pair that holds the sources of c and c + 1
    bool swap = false;
    if constexpr (MODE != HKS_MAC_PLAIN) {
        const u32 s = galois_src(c, a.logn, (rot, ...).g);        // the source of c; that of c + 1 is s ^ 1
        sp = s & ~1u;
        swap = s & 1u;
    }
    const u32 j = hks_limb(a, jT);
    const Mod m = a.mods[j].m;
    d2 w = {0.0, 0.0};
    if constexpr (PT) {
        const u2 t = *reinterpret_cast<const u2*>((rot, ...).pt + size_t(j) * n + c);
        w.x = hxf::lt_pt(hxf::to_f64(t.x), m); w.y = hxf::lt_pt(hxf::to_f64(t.y), m);
    }
    d2 key[MAXD][2];
#pragma unroll
    for (int d = 0; d < MAXD; ++d)
        if (d < (int)a.dl) {
            const double* keys;
            if constexpr (MODE == HKS_MAC_PLAIN) keys = a.keys; else keys = (rot, ...).keys;
            key[d][0] = *reinterpret_cast<const d2*>(keys + ((size_t(d) * 2 + 0) * a.K + j) * n + c);
            key[d][1] = *reinterpret_cast<const d2*>(keys + ((size_t(d) * 2 + 1) * a.K + j) * n + c);
        }
    for (u32 b = blockIdx.y; b < a.nb; b += gridDim.y) {
        const double* ub = a.ext + (size_t(b) * a.dl * a.T + jT) * n + sp;
        // acc of component k. The plain mode forms each address at its store, the others both in front of the gather, where the
        // PT_ACC loads need them: the order each mode's instruction stream has always had
        d2* p0 = MODE == HKS_MAC_PLAIN ? nullptr : reinterpret_cast<d2*>(a.acc + ((size_t(b) * 2 + 0) * a.T + jT) * n + c);
        d2* p1 = MODE == HKS_MAC_PLAIN ? nullptr : reinterpret_cast<d2*>(a.acc + ((size_t(b) * 2 + 1) * a.T + jT) * n + c);
        d2 prev0 = {0.0, 0.0}, prev1 = {0.0, 0.0};
        if constexpr (MODE == HKS_MAC_PT_ACC || MODE == HKS_MAC_ACC) { prev0 = *p0; prev1 = *p1; }
        d2 acc0 = {0.0, 0.0}, acc1 = {0.0, 0.0};
#pragma unroll
        for (int d = 0; d < MAXD; ++d)
            if (d < (int)a.dl) {
                const d2 v = *reinterpret_cast<const d2*>(ub + size_t(d) * a.T * n);
                const d2 u = {swap ? v.y : v.x, swap ? v.x : v.y};
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    acc0[e] = hxf::hks_mac_term(acc0[e], u[e], key[d][0][e], m);
                    acc1[e] = hxf::hks_mac_term(acc1[e], u[e], key[d][1][e], m);
                }
            }
        if constexpr (PT) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                acc0[e] = MODE == HKS_MAC_PT_FIRST ? hxf::lt_mac(acc0[e], w[e], m) : hxf::lt_mac_acc(acc0[e], w[e], prev0[e], m);
                acc1[e] = MODE == HKS_MAC_PT_FIRST ? hxf::lt_mac(acc1[e], w[e], m) : hxf::lt_mac_acc(acc1[e], w[e], prev1[e], m);
            }
        }
        if constexpr (MODE == HKS_MAC_ACC) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                acc0[e] = hxf::hks_ext_acc(prev0[e], acc0[e], m);
                acc1[e] = hxf::hks_ext_acc(prev1[e], acc1[e], m);
            }
        }
        if constexpr (MODE == HKS_MAC_PLAIN) p0 = reinterpret_cast<d2*>(a.acc + ((size_t(b) * 2 + 0) * a.T + jT) * n + c);
        *p0 = acc0;
        if constexpr (MODE == HKS_MAC_PLAIN) p1 = reinterpret_cast<d2*>(a.acc + ((size_t(b) * 2 + 1) * a.T + jT) * n + c);
        *p1 = acc1;
    }
}

// step 3 of one giant step of hexl_hks_linear_transform_bsgs, k_lt_bsgs_sum (keyswitch_f64.hip) on this layout:
//     acc[b][k][jT] = sum_r pt_r[limb of jT] . B_r[b][k][jT]
// B_r is what k_hks_mac<., HKS_MAC_STORE> stored for the baby step of term r: the inner sum of the plaintext modes, computed once
// per chunk instead of once per giant step. No keys, no gather, no position map: a stored vector lies at its logical index like every
// hybrid intermediate, so a lane owns two adjacent indices of one row of T_l as in k_hks_mac and every access is 16 bytes. It walks the
// row's terms of the per-call table (wave-uniform: scalar loads), keeps both accumulators in registers across them and writes acc ONCE --
// where k_hks_mac<., HKS_MAC_PT_ACC> reads and writes acc per term. The plaintext is indexed by the PHYSICAL limb (pt is [K][n]),
// the stored vectors and acc by the row jT of T_l. The scalar chain is that of the plaintext modes unchanged and in the same order --
// lt_pt, lt_mac for the first term, lt_mac_acc after it -- on the same inner operand (an hks_mac_term output, stored exactly), so acc
// holds the very doubles hexl_hks_linear_transform's multiply-accumulates leave for that row.
struct HksBsgsTerm { const u64* pt; const double* B; };           // pt: [K][n]; B: the baby step's slice [nb][2][T][n]

__global__ __launch_bounds__(HKS_THREADS) void k_hks_bsgs_sum(HksArgs a, const HksBsgsTerm* terms, u32 n_terms) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    typedef unsigned long long u2 __attribute__((ext_vector_type(2)));
    const u32 n = 1u << a.logn, pairs = n >> 1;
    const u32 gid = blockIdx.x * blockDim.x + threadIdx.x;        // (row of T_l, pair)
    const u32 jT = gid / pairs;
    if (jT >= a.T) return;
    const u32 c = (gid - jT * pairs) * 2;
    const u32 j = hks_limb(a, jT);
    const Mod m = a.mods[j].m;
    const size_t po = size_t(j) * n + c;
    for (u32 b = blockIdx.y; b < a.nb; b += gridDim.y) {
        const size_t o0 = ((size_t(b) * 2 + 0) * a.T + jT) * n + c, o1 = ((size_t(b) * 2 + 1) * a.T + jT) * n + c;
        const HksBsgsTerm first = terms[0];                       // uniform: scalar loads
        const u2 t = *reinterpret_cast<const u2*>(first.pt + po);
        const d2 f0 = *reinterpret_cast<const d2*>(first.B + o0), f1 = *reinterpret_cast<const d2*>(first.B + o1);
        d2 acc0, acc1;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const double w = hxf::lt_pt(hxf::to_f64(t[e]), m);
            acc0[e] = hxf::lt_mac(f0[e], w, m);
            acc1[e] = hxf::lt_mac(f1[e], w, m);
        }
        for (u32 r = 1; r < n_terms; ++r) {
            const HksBsgsTerm term = terms[r];
            const u2 tr = *reinterpret_cast<const u2*>(term.pt + po);
            const d2 v0 = *reinterpret_cast<const d2*>(term.B + o0), v1 = *reinterpret_cast<const d2*>(term.B + o1);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const double w = hxf::lt_pt(hxf::to_f64(tr[e]), m);
                acc0[e] = hxf::lt_mac_acc(v0[e], w, acc0[e], m);
                acc1[e] = hxf::lt_mac_acc(v1[e], w, acc1[e], m);
            }
        }
        *reinterpret_cast<d2*>(a.acc + o0) = acc0;
        *reinterpret_cast<d2*>(a.acc + o1) = acc1;
    }
}

// step 3s of hexl_hks_linear_transform_bsgs_ext: A[b][k][jT] += sigma_g(src[b][k][jT]) for k < n_comp, on EVERY row
// of T_l -- the special rows are permuted like the data rows: sigma_g acts on the polynomial, whatever modulus it is reduced by. src is
// a row's inner sum as k_hks_bsgs_sum left it in acc, A what a.acc points at here; both [nb][2][T][n] doubles, reduce outputs, at the
// logical index. k_hks_mac's lane layout and gather: the written side is 16-byte accesses at c, the read side ONE 16-byte load at the
// aligned pair that holds the sources of c and c + 1, swapped when the source of c is odd. A rotated row adds component 0 alone
// (n_comp = 1: its component 1 went through the half mod-down and the giant key), a row with G = 1 both with g = 1 (no permutation).
__global__ __launch_bounds__(HKS_THREADS) void k_hks_ext_add(HksArgs a, const double* src, u32 g, u32 n_comp) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    const u32 n = 1u << a.logn, pairs = n >> 1;
    const u32 gid = blockIdx.x * blockDim.x + threadIdx.x;        // (row of T_l, pair)
    const u32 jT = gid / pairs;
    if (jT >= a.T) return;
    const u32 c = (gid - jT * pairs) * 2;
    const u32 s = galois_src(c, a.logn, g);                       // the source of c; that of c + 1 is s ^ 1
    const u32 sp = s & ~1u;
    const bool swap = s & 1u;
    const Mod m = a.mods[hks_limb(a, jT)].m;
    for (u32 b = blockIdx.y; b < a.nb; b += gridDim.y)
        for (u32 k = 0; k < n_comp; ++k) {
            const size_t row = ((size_t(b) * 2 + k) * a.T + jT) * n;
            d2* p = reinterpret_cast<d2*>(a.acc + row + c);
            const d2 prev = *p;
            const d2 v = *reinterpret_cast<const d2*>(src + row + sp);
            const d2 o = {hxf::hks_ext_acc(prev.x, swap ? v.y : v.x, m), hxf::hks_ext_acc(prev.y, swap ? v.x : v.y, m)};
            *p = o;
        }
}

// the key install: the caller's [dnum][2][K][n] canonical words as centred doubles at the same place, one workgroup per (row, piece)
struct HksInstallArgs { const KsModF64* mods; const u64* in; double* out; u32 K, logn; };
__global__ __launch_bounds__(HKS_THREADS) void k_hks_install(HksInstallArgs a) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    typedef unsigned long long u2 __attribute__((ext_vector_type(2)));
    const u32 lp = a.logn - HKS_LOG_PIECE;
    const u32 row = blockIdx.x >> lp, piece = blockIdx.x - (row << lp);       // row = (d 2 + k) K + i
    const u64 q = (u64)a.mods[row % a.K].m.p;
    const size_t at = (size_t(row) << a.logn) + (size_t(piece) << HKS_LOG_PIECE) + 2 * threadIdx.x;
    const u2 v = *reinterpret_cast<const u2*>(a.in + at);
    const d2 o = {hxk::centre(v.x % q, q), hxk::centre(v.y % q, q)};
    *reinterpret_cast<d2*>(a.out + at) = o;
}

// the key export, the install's inverse: the centred doubles as canonical words at the same place of the caller's [dnum][2][K][n]
struct HksExportArgs { const KsModF64* mods; const double* in; u64* out; u32 K, logn; };
__global__ __launch_bounds__(HKS_THREADS) void k_hks_export(HksExportArgs a) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    typedef unsigned long long u2 __attribute__((ext_vector_type(2)));
    const u32 lp = a.logn - HKS_LOG_PIECE;
    const u32 row = blockIdx.x >> lp, piece = blockIdx.x - (row << lp);       // row = (d 2 + k) K + i
    const double q = a.mods[row % a.K].m.p;
    const size_t at = (size_t(row) << a.logn) + (size_t(piece) << HKS_LOG_PIECE) + 2 * threadIdx.x;
    const d2 v = *reinterpret_cast<const d2*>(a.in + at);
    const u2 o = {hxf::from_f64(v.x < 0.0 ? v.x + q : v.x), hxf::from_f64(v.y < 0.0 ? v.y + q : v.y)};
    *reinterpret_cast<u2*>(a.out + at) = o;
}

// relinearize: ct3[nb][3][l][n] -> out[nb][2][l][n] (components 0-1) and t[nb][l][n] (component 2); words are moved, never interpreted
struct HksMoveArgs { const u64* in; u64* out; u64* t; u32 l, logn; };
__global__ __launch_bounds__(HKS_THREADS) void k_hks_split3(HksMoveArgs a) {
    typedef unsigned long long u2 __attribute__((ext_vector_type(2)));
    const u32 lp = a.logn - HKS_LOG_PIECE;
    const u32 br = blockIdx.x >> lp, piece = blockIdx.x - (br << lp);
    const u32 b = br / (3 * a.l), r = br - b * 3 * a.l;           // r = k l + i
    const size_t n = size_t(1) << a.logn, c = (size_t(piece) << HKS_LOG_PIECE) + 2 * threadIdx.x;
    u64* row = r < 2 * a.l ? a.out + (size_t(b) * 2 * a.l + r) * n : a.t + (size_t(b) * a.l + (r - 2 * a.l)) * n;
    *reinterpret_cast<u2*>(row + c) = *reinterpret_cast<const u2*>(a.in + (size_t(b) * 3 * a.l + r) * n + c);
}
// rotate, behind hx_launch_galois(out <- ct): component 1 of out[nb][2][l][n] moves to t[nb][l][n] and is zeroed
__global__ __launch_bounds__(HKS_THREADS) void k_hks_take_c1(HksMoveArgs a) {
    typedef unsigned long long u2 __attribute__((ext_vector_type(2)));
    const u32 lp = a.logn - HKS_LOG_PIECE;
    const u32 bi = blockIdx.x >> lp, piece = blockIdx.x - (bi << lp);
    const u32 b = bi / a.l, i = bi - b * a.l;
    const size_t n = size_t(1) << a.logn, c = (size_t(piece) << HKS_LOG_PIECE) + 2 * threadIdx.x;
    u64* c1 = a.out + ((size_t(b) * 2 + 1) * a.l + i) * n + c;
    *reinterpret_cast<u2*>(a.t + (size_t(b) * a.l + i) * n + c) = *reinterpret_cast<const u2*>(c1);
    const u2 zero = {0, 0};
    *reinterpret_cast<u2*>(c1) = zero;
}

// ---- host side ----
// the forward reduction period every limb of T_l shares, else -1 (hx_level_tier for a basis that is not a prefix)
static int hks_level_tier(const hexl_ks_plan* p, u32 l) {
    for (u32 i = 1; i < l; ++i)
        if (p->tier[i] != p->tier[0]) return -1;
    for (u32 s = p->L; s < p->K; ++s)
        if (p->tier[s] != p->tier[0]) return -1;
    return p->tier[0];
}

template <class F>
static void hks_with_max(u32 count, F f) {                        // register room for 1, 2, 4, 8 or 16 sources / digits
    if (count <= 1) f(hx_int<1>{});
    else if (count <= 2) f(hx_int<2>{});
    else if (count <= 4) f(hx_int<4>{});
    else if (count <= 8) f(hx_int<8>{});
    else f(hx_int<16>{});
}
static u32 hks_piece_grid(const hexl_ks_plan* p, size_t rows) { return (u32)(rows << (p->logn - HKS_LOG_PIECE)); }

// A chunk's launches in three stages, all on the context's stream: steps 1-2 (up), step 3 (mac) and step 4 (down). The key switch runs
// them back to back; the hoisted callers run `up` once per chunk and the other two per rotation, or `down` once (hks_hoist_*).
template <int LOGN, int LOGE, int LAZY>
static int hks_optin(hexl_hks* h) {
    return hx_lds_optin<k_hks_intt<LOGN, LOGE, LAZY>, k_hks_fwd<LOGN, LOGE, LAZY>, k_hks_down_intt<LOGN, LOGE, LAZY, false>,
                        k_hks_down<LOGN, LOGE, LAZY, false>, k_hks_down_intt<LOGN, LOGE, LAZY, true>, k_hks_down<LOGN, LOGE, LAZY, true>,
                        k_hks_down_intt<LOGN, LOGE, LAZY, false, true>, k_hks_down<LOGN, LOGE, LAZY, false, true>>(
        h->plan->ctx->device, Geom<LOGN, LOGE>::LDS_USED);
}
// the rows of the constants a launch reads: the conversion `mode` at level l, and the divisor of that mod-down
static void hks_point_rows(const hexl_hks* h, HksConv mode, u32 l, HksArgs& a) {
    a.src = h->d_src + hks_conv_row(mode, l) * HKS_MAX_LIMBS;
    a.wt = h->d_wt + hks_conv_row(mode, l) * HKS_MAX_LIMBS * HKS_MAX_LIMBS;
    a.div = h->d_div + hks_div_row(mode, l) * HKS_MAX_LIMBS;
}

template <int LOGN, int LOGE, int LAZY>
static int hks_stage_up(hexl_hks* h, const HksArgs& a) {
    using G = Geom<LOGN, LOGE>;
    hexl_ks_plan* p = h->plan;
    if (int rc = hks_optin<LOGN, LOGE, LAZY>(h)) return rc;
    hipStream_t st = p->ctx->stream;
    const dim3 wg(G::T), ww(HKS_THREADS);
    const u32 nb = a.nb;
    hipLaunchKernelGGL((k_hks_intt<LOGN, LOGE, LAZY>), dim3(a.l * nb), wg, G::LDS_USED, st, a);
    hks_with_max(a.alpha < a.l ? a.alpha : a.l, [&](auto M) {
        hipLaunchKernelGGL((k_hks_conv<HKS_CONV_UP, decltype(M)::value>), dim3(hks_piece_grid(p, size_t(nb) * a.dl)), ww, 0, st, a);
    });
    hipLaunchKernelGGL((k_hks_fwd<LOGN, LOGE, LAZY>), dim3(a.T * a.dl * nb), wg, G::LDS_USED, st, a);
    return (int)hipGetLastError();
}

// one workgroup column per 512 indices of a row of T_l, up to 8 rows of workgroups share the batch (no transform: no geometry, no tier)
static dim3 hks_mac_grid(const HksArgs& a) { return dim3(a.T * ((1u << a.logn) / 2) / HKS_THREADS, a.nb < 8 ? a.nb : 8); }
static int hks_stage_mac(hexl_hks* h, const HksArgs& a) {
    hks_with_max(a.dl, [&](auto M) {
        hipLaunchKernelGGL((k_hks_mac<decltype(M)::value, HKS_MAC_PLAIN>), hks_mac_grid(a), dim3(HKS_THREADS), 0, h->plan->ctx->stream, a);
    });
    return (int)hipGetLastError();
}
static int hks_stage_mac_galois(hexl_hks* h, const HksArgs& a, const HksRot& rot, HksMacMode mode) {
    hipStream_t st = h->plan->ctx->stream;
    const dim3 grid = hks_mac_grid(a), ww(HKS_THREADS);
    hks_with_max(a.dl, [&](auto M) {
        constexpr int D = decltype(M)::value;
        if (mode == HKS_MAC_STORE)         hipLaunchKernelGGL((k_hks_mac<D, HKS_MAC_STORE, HksRot>), grid, ww, 0, st, a, rot);
        else if (mode == HKS_MAC_ACC)      hipLaunchKernelGGL((k_hks_mac<D, HKS_MAC_ACC, HksRot>), grid, ww, 0, st, a, rot);
        else if (mode == HKS_MAC_PT_FIRST) hipLaunchKernelGGL((k_hks_mac<D, HKS_MAC_PT_FIRST, HksRot>), grid, ww, 0, st, a, rot);
        else                               hipLaunchKernelGGL((k_hks_mac<D, HKS_MAC_PT_ACC, HksRot>), grid, ww, 0, st, a, rot);
    });
    return (int)hipGetLastError();
}

static int hks_stage_bsgs_sum(hexl_hks* h, const HksArgs& a, const HksBsgsTerm* d_terms, u32 n_terms) {
    hipLaunchKernelGGL(k_hks_bsgs_sum, hks_mac_grid(a), dim3(HKS_THREADS), 0, h->plan->ctx->stream, a, d_terms, n_terms);
    return (int)hipGetLastError();
}

// step 4, or step 4' of the rescaling calls (RS: a.d01 and a.result set by the caller; l >= 2): sources S, and the limb l - 1 with RS;
// targets the data limbs, all but the limb l - 1 with RS
template <int LOGN, int LOGE, int LAZY, bool RS>
static int hks_stage_down(hexl_hks* h, const HksArgs& a) {
    using G = Geom<LOGN, LOGE>;
    constexpr HksConv MODE = RS ? HKS_CONV_RS : HKS_CONV_DOWN;
    hexl_ks_plan* p = h->plan;
    if (int rc = hks_optin<LOGN, LOGE, LAZY>(h)) return rc;
    hipStream_t st = p->ctx->stream;
    const dim3 wg(G::T), ww(HKS_THREADS);
    const u32 nb = a.nb, nsrc = a.K - a.L + RS, ntgt = a.l - RS;
    HksArgs dn = a;
    hks_point_rows(h, MODE, a.l, dn);
    hipLaunchKernelGGL((k_hks_down_intt<LOGN, LOGE, LAZY, RS>), dim3(nsrc * 2 * nb), wg, G::LDS_USED, st, dn);
    hks_with_max(nsrc, [&](auto M) {
        hipLaunchKernelGGL((k_hks_conv<MODE, decltype(M)::value>), dim3(hks_piece_grid(p, size_t(nb) * 2)), ww, 0, st, dn);
    });
    hipLaunchKernelGGL((k_hks_down<LOGN, LOGE, LAZY, RS>), dim3(ntgt * 2 * nb), wg, G::LDS_USED, st, dn);
    return (int)hipGetLastError();
}

// step 4 on component 1 alone (a.w1 set): half the workgroups of each of the three launches, nothing of component 0 read or written
template <int LOGN, int LOGE, int LAZY>
static int hks_stage_down_c1(hexl_hks* h, const HksArgs& a) {
    using G = Geom<LOGN, LOGE>;
    hexl_ks_plan* p = h->plan;
    if (int rc = hks_optin<LOGN, LOGE, LAZY>(h)) return rc;
    hipStream_t st = p->ctx->stream;
    const dim3 wg(G::T), ww(HKS_THREADS);
    const u32 nb = a.nb, nsrc = a.K - a.L;
    HksArgs dn = a;
    hks_point_rows(h, HKS_CONV_DOWN1, a.l, dn);
    hipLaunchKernelGGL((k_hks_down_intt<LOGN, LOGE, LAZY, false, true>), dim3(nsrc * nb), wg, G::LDS_USED, st, dn);
    hks_with_max(nsrc, [&](auto M) {
        hipLaunchKernelGGL((k_hks_conv<HKS_CONV_DOWN1, decltype(M)::value>), dim3(hks_piece_grid(p, nb)), ww, 0, st, dn);
    });
    hipLaunchKernelGGL((k_hks_down<LOGN, LOGE, LAZY, false, true>), dim3(a.l * nb), wg, G::LDS_USED, st, dn);
    return (int)hipGetLastError();
}

static int hks_stage_ext_add(hexl_hks* h, const HksArgs& a, const double* src, u32 g, u32 n_comp) {
    hipLaunchKernelGGL(k_hks_ext_add, hks_mac_grid(a), dim3(HKS_THREADS), 0, h->plan->ctx->stream, a, src, g, n_comp);
    return (int)hipGetLastError();
}

template <int LOGN, int LOGE, int LAZY>
static int hks_run_chunk(hexl_hks* h, const HksArgs& a) {
    if (int rc = hks_stage_up<LOGN, LOGE, LAZY>(h, a)) return rc;
    if (int rc = hks_stage_mac(h, a)) return rc;
    return a.d01 ? hks_stage_down<LOGN, LOGE, LAZY, true>(h, a) : hks_stage_down<LOGN, LOGE, LAZY, false>(h, a);
}

static size_t hks_chunk_of(const hexl_hks* h, size_t batch) { return hx_ks_chunk_of(h->plan, batch); }
// THE scratch account: rows of n 64-bit words per instance of a chunk, at the full level, buffer by buffer. Every reserve and every
// hexl_hks_*_scratch_bytes reads it.
struct HksRows {
    size_t coef, ext, acc;            // the key switch: L, dnum K, 2 K
    size_t w1;                        // the hoisted callers: + L
    size_t t;                         // hexl_hks_linear_transform_bsgs: + 2 L beside w1
    size_t slice, d01;                // the slice of rotate / relinearize / the tensor calls: L; the rescaling tensor call: + 2 L beside it
    size_t ext_a;                     // hexl_hks_linear_transform_bsgs_ext: + 2 K beside the BSGS call's, and d01 with rescale = 1
    size_t ks() const { return coef + ext + acc; }
};
static HksRows hks_rows(const hexl_hks* h) {
    const size_t L = h->plan->L, K = h->plan->K;
    return HksRows{L, size_t(h->dnum) * K, 2 * K, L, 2 * L, L, 2 * L, 2 * K};
}
static size_t hks_row_bytes(const hexl_hks* h) { return h->plan->n * sizeof(u64); }

// the scratch of chunks of `chunk` instances and a chunk's kernel arguments at level l, all but the per-chunk pointers and nb
static int hks_reserve(hexl_hks* h, size_t chunk) {
    const size_t n = h->plan->n;
    const HksRows r = hks_rows(h);
    if (int rc = h->d_coef.reserve(chunk * r.coef * n)) return rc;
    if (int rc = h->d_ext.reserve(chunk * r.ext * n)) return rc;
    return h->d_acc.reserve(chunk * r.acc * n);
}
static HksArgs hks_args(const hexl_hks* h, u32 l) {
    const hexl_ks_plan* p = h->plan;
    HksArgs a{};
    a.mods = p->d_mods_f64; a.tables = p->d_tables_f64;
    hks_point_rows(h, HKS_CONV_UP, l, a);
    a.keys = h->d_keys;
    a.coef = h->d_coef; a.ext = h->d_ext; a.acc = h->d_acc;
    a.L = p->L; a.K = p->K; a.l = l; a.T = l + h->np;
    a.dl = (l + h->alpha - 1) / h->alpha;
    a.alpha = h->alpha; a.logn = p->logn; a.tstride = l;
    for (u32 jT = 0; jT < a.T; ++jT) a.limbmap |= (unsigned long long)(jT < l ? jT : p->L + (jT - l)) << (4 * jT);
    a.tiermap = hx_tiermap(p);
    return a;
}

// The key switch of `batch` instances at level l, chunk by chunk on the context's stream. feed(b0, nb, a) points the chunk's arguments:
// a.t / a.tstride at its input and a.result at its output -- [nb][2][l][n], ADDED into -- and, for the rescaling mod-down, a.d01 /
// a.d01_stride at its (d0, d1), with a.result [nb][2][l - 1][n] WRITTEN; it launches what fills them.
template <class F>
static int hks_launch(hexl_hks* h, size_t batch, u32 l, F feed) {
    hexl_ks_plan* p = h->plan;
    const size_t chunk = hks_chunk_of(h, batch);
    if (int rc = hks_reserve(h, chunk)) return rc;
    HksArgs a = hks_args(h, l);
    const int lazy = hks_level_tier(p, l);
    return hx_for_chunks(batch, chunk, [&](size_t b0, size_t nb) {
        a.nb = (u32)nb;
        if (int rc = feed(b0, nb, a)) return rc;
        return hx_with_f64_geom(p->logn, lazy, [&](auto N, auto E, auto Z) { return hks_run_chunk<N, E, Z>(h, a); });
    });
}
// d_result[batch][2][l][n] += KS(d_t[batch][l][n]), the caller's arrays
static int hks_keyswitch(hexl_hks* h, u64* d_result, const u64* d_t, size_t batch, u32 l) {
    const size_t n = h->plan->n;
    return hks_launch(h, batch, l, [&](size_t b0, size_t, HksArgs& a) {
        a.t = d_t + b0 * l * n;
        a.result = d_result + b0 * 2 * l * n;
        return 0;
    });
}

// conversion constants for every level, exact integer work: per (conversion row, source limb, target limb) the two weights, and per
// (divisor row, limb) the mod-down's
static int hks_constants(hexl_hks* h) {
    const hexl_ks_plan* p = h->plan;
    const u32 L = p->L, K = p->K, alpha = h->alpha;
    const std::vector<u64>& q = p->moduli;
    std::vector<HksSrc> src(size_t(HKS_CONV_ROWS) * HKS_MAX_LIMBS, HksSrc{0.0, 0.0});
    std::vector<HksWt> wt(size_t(HKS_CONV_ROWS) * HKS_MAX_LIMBS * HKS_MAX_LIMBS, HksWt{0.0, 0.0});
    // the limbs of `sources` convert into the targets of `targets` (a target that is a source is skipped): (D / q_i)^-1 mod q_i and
    // (D / q_i) mod q_j, D the sources' product
    auto fill = [&](std::vector<HksSrc>& src, std::vector<HksWt>& wt, u32 row, const std::vector<u32>& sources, const std::vector<u32>& targets) {
        auto is_source = [&](u32 j) {
            for (u32 o : sources)
                if (o == j) return true;
            return false;
        };
        for (u32 i : sources) {
            auto hat_mod = [&](u64 m) {
                u64 r = 1 % m;
                for (u32 o : sources)
                    if (o != i) r = hxnt::mulmod(r, q[o] % m, m);
                return r;
            };
            const double hinv = hx_centre(hxnt::invmod(hat_mod(q[i]), q[i]), q[i]);
            src[size_t(row) * HKS_MAX_LIMBS + i] = HksSrc{hinv, hinv / (double)q[i]};
            for (u32 j : targets) {
                if (is_source(j)) continue;
                const double w = hx_centre(hat_mod(q[j]), q[j]);
                wt[(size_t(row) * HKS_MAX_LIMBS + i) * HKS_MAX_LIMBS + j] = HksWt{w, w / (double)q[j]};
            }
        }
    };
    auto limbs = [](u32 lo, u32 hi) {
        std::vector<u32> v;
        for (u32 i = lo; i < hi; ++i) v.push_back(i);
        return v;
    };
    fill(src, wt, hks_conv_row(HKS_CONV_DOWN, 0), limbs(L, K), limbs(0, L));
    for (u32 l = 1; l <= L; ++l) {
        std::vector<u32> basis = limbs(0, l), B = limbs(L, K);
        basis.insert(basis.end(), B.begin(), B.end());
        for (u32 lo = 0; lo < l; lo += alpha) fill(src, wt, hks_conv_row(HKS_CONV_UP, l), limbs(lo, lo + alpha < l ? lo + alpha : l), basis);
        if (l < 2) continue;
        B.push_back(l - 1);                                       // the rescaling mod-down: sources S + {l - 1}, targets i < l - 1
        fill(src, wt, hks_conv_row(HKS_CONV_RS, l), B, limbs(0, l - 1));
    }
    // Per limb P mod q_i once, and from it every divisor row: row 0 is Q = P (sources S, targets every data limb), row l - 1 is
    // Q = R = P q_(l-1) of level l >= 2 (sources S and the limb l - 1, targets i < l - 1; the limbs l ... L - 1 are not in its basis).
    std::vector<HksDiv> div(size_t(HKS_MAX_LIMBS) * HKS_MAX_LIMBS, HksDiv{0.0, 0.0, 0.0, 0.0, 0.0, 0.0});
    for (u32 i = 0; i < K; ++i) {
        const u64 qi = q[i];
        u64 P = 1 % qi;
        for (u32 s = L; s < K; ++s) P = hxnt::mulmod(P, q[s] % qi, qi);
        h->p_mod[i] = (double)P;
        for (u32 l = 1; l <= L; ++l) {
            const bool rs = l >= 2;
            if (rs && i >= l && i < L) continue;
            const u64 Q = rs ? hxnt::mulmod(P, q[l - 1] % qi, qi) : P;
            // floor(Q / 2) = (Q - 1) / 2 for the odd Q: ((Q mod q) - 1) (q + 1) / 2 mod q (Q = 0 modulo a source limb)
            const u64 half = hxnt::mulmod((Q + qi - 1) % qi, (qi + 1) / 2, qi);
            HksDiv& c = div[hks_div_row(rs ? HKS_CONV_RS : HKS_CONV_DOWN, l) * HKS_MAX_LIMBS + i];
            if (i >= L || (rs && i == l - 1)) {
                c.half = (double)half;
            } else {
                c.inv = hx_centre(hxnt::invmod(Q, qi), qi);
                c.inv_p = c.inv / (double)qi;
                c.fix = (double)(qi - half);
            }
            if (rs && i < l) {
                c.pm = hx_centre(P, qi);
                c.pm_p = c.pm / (double)qi;
            }
        }
    }
    if (int rc = h->d_src.upload_once(src.data(), src.size())) return rc;
    if (int rc = h->d_wt.upload_once(wt.data(), wt.size())) return rc;
    return h->d_div.upload_once(div.data(), div.size());
}

// ---- entry points of include/hexl_mi355x.h ----
static bool hks_galois_elt_ok(u64 g, u64 n) { return (g & 1) && g < 2 * n; }
// the checks the three launching entry points share: handle, plan, level; *bytes = the size of [batch][comps][n_limbs][n] words
static bool hks_call_ok(const hexl_hks* h, size_t batch, u64 n_limbs, u64 comps, size_t* bytes) {
    if (!h || !hx_f64_plan_ok(h->plan, n_limbs, 1, h->plan->L)) return false;
    const hexl_ks_plan* p = h->plan;
    if (!hx_words_bytes(batch, comps, n_limbs, p->n, bytes)) return false;
    const size_t chunk = hks_chunk_of(h, batch);
    size_t scratch;
    if (!hx_words_bytes(chunk, 1, hks_rows(h).ks(), p->n, &scratch)) return false;
    // the largest grids of a chunk: one workgroup per (row of T_l, digit, instance), one per (instance, 3 l rows, piece)
    return hx_wg_grid_ok(chunk, u64(p->K) * h->dnum) && chunk <= HX_MAX_GRID / (size_t(3 * p->L) << (p->logn - HKS_LOG_PIECE));
}

extern "C" int hexl_hks_create(hexl_ks_plan* p, uint64_t digit_limbs, hexl_hks** out) {
    if (!out) return HEXL_E_BADARG;
    *out = nullptr;
    if (!hx_f64_plan_ok(p) || p->K <= p->L || p->K > HKS_MAX_LIMBS || !hx_in_range(digit_limbs, 1, p->L)) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    hexl_hks* h = new hexl_hks(p);
    h->alpha = (u32)digit_limbs;
    h->dnum = (p->L + h->alpha - 1) / h->alpha;
    h->np = p->K - p->L;
    int rc = hks_constants(h);
    if (!rc) rc = h->d_keys.reserve(size_t(h->dnum) * 2 * p->K * p->n);
    if (rc) { delete h; return rc; }
    *out = h;
    return 0;
}

extern "C" int hexl_hks_destroy(hexl_hks* h) {
    if (!h) return HEXL_E_BADARG;
    (void)hipSetDevice(h->plan->ctx->device);
    (void)hipStreamSynchronize(h->plan->ctx->stream);             // the buffers go with the object: nothing may still use them
    delete h;
    return 0;
}

extern "C" int hexl_hks_set_keys_device(hexl_hks* h, const uint64_t* d_keys) {
    if (!h || !d_keys) return HEXL_E_BADARG;
    const hexl_ks_plan* p = h->plan;
    HX_CHECK(hipSetDevice(p->ctx->device));
    const HksInstallArgs a{p->d_mods_f64, d_keys, h->d_keys, p->K, p->logn};
    hipLaunchKernelGGL(k_hks_install, dim3(hks_piece_grid(p, size_t(h->dnum) * 2 * p->K)), dim3(HKS_THREADS), 0, p->ctx->stream, a);
    if (int rc = (int)hipGetLastError()) return rc;
    h->have_keys = true;
    return 0;
}

HxHksKeys hx_hks_keys(hexl_hks* h) { return HxHksKeys{h->plan, h->d_keys, h->p_mod, h->alpha, h->dnum}; }
void hx_hks_set_keyed(hexl_hks* h) { h->have_keys = true; }

extern "C" int hexl_hks_export_keys(const hexl_hks* h, uint64_t* d_out) {
    if (!h || !d_out) return HEXL_E_BADARG;
    if (!h->have_keys) return HEXL_E_NOKEYS;
    const hexl_ks_plan* p = h->plan;
    HX_CHECK(hipSetDevice(p->ctx->device));
    const HksExportArgs a{p->d_mods_f64, h->d_keys, d_out, p->K, p->logn};
    hipLaunchKernelGGL(k_hks_export, dim3(hks_piece_grid(p, size_t(h->dnum) * 2 * p->K)), dim3(HKS_THREADS), 0, p->ctx->stream, a);
    return (int)hipGetLastError();
}

extern "C" int hexl_hks_keyswitch(hexl_hks* h, uint64_t* d_result, const uint64_t* d_t_target, size_t batch, uint64_t n_limbs) {
    size_t t_bytes;
    if (!d_result || !d_t_target || !hks_call_ok(h, batch, n_limbs, 1, &t_bytes)) return HEXL_E_BADARG;
    if (hx_ranges_overlap(d_result, 2 * t_bytes, d_t_target, t_bytes)) return HEXL_E_BADARG;
    if (!h->have_keys) return HEXL_E_NOKEYS;
    if (!batch) return 0;
    HX_CHECK(hipSetDevice(h->plan->ctx->device));
    return hks_keyswitch(h, d_result, d_t_target, batch, (u32)n_limbs);
}

// The slice loop of hexl_rotate / hexl_relinearize: fill(b0, nb, out, t) writes what the key switch adds into to `out` and its input to
// the slice buffer; everything runs on the context's stream, so the next slice's fill is behind this slice's key switch.
template <class F>
static int hks_slices(hexl_hks* h, u64* d_out, size_t batch, u32 l, F fill) {
    const size_t n = h->plan->n;
    const size_t slice = hks_chunk_of(h, batch);
    if (int rc = h->d_slice.reserve(slice * hks_rows(h).slice * n)) return rc;
    return hx_for_chunks(batch, slice, [&](size_t b0, size_t nb) {
        u64* out = d_out + b0 * 2 * l * n;
        if (int rc = fill(b0, nb, out, (u64*)h->d_slice)) return rc;
        return hks_keyswitch(h, out, h->d_slice, nb, l);
    });
}

extern "C" int hexl_hks_relinearize(hexl_hks* h, uint64_t* d_out, const uint64_t* d_ct3, size_t batch, uint64_t n_limbs) {
    size_t in_bytes;
    if (!d_out || !d_ct3 || !hks_call_ok(h, batch, n_limbs, 3, &in_bytes)) return HEXL_E_BADARG;
    if (hx_ranges_overlap(d_out, in_bytes / 3 * 2, d_ct3, in_bytes)) return HEXL_E_BADARG;
    if (!h->have_keys) return HEXL_E_NOKEYS;
    if (!batch) return 0;
    hexl_ks_plan* p = h->plan;
    HX_CHECK(hipSetDevice(p->ctx->device));
    const size_t n = p->n, l = n_limbs;
    return hks_slices(h, d_out, batch, (u32)l, [&](size_t b0, size_t nb, u64* out, u64* t) {
        const HksMoveArgs a{d_ct3 + b0 * 3 * l * n, out, t, (u32)l, p->logn};
        hipLaunchKernelGGL(k_hks_split3, dim3(hks_piece_grid(p, nb * 3 * l)), dim3(HKS_THREADS), 0, p->ctx->stream, a);
        return (int)hipGetLastError();
    });
}

extern "C" int hexl_hks_rotate(hexl_hks* h, uint64_t* d_out, const uint64_t* d_ct, size_t batch, uint64_t n_limbs, uint64_t galois_elt) {
    size_t bytes;
    if (!d_out || !d_ct || !hks_call_ok(h, batch, n_limbs, 2, &bytes) || !hks_galois_elt_ok(galois_elt, h->plan->n)) return HEXL_E_BADARG;
    if (hx_ranges_overlap(d_out, bytes, d_ct, bytes)) return HEXL_E_BADARG;      // a permutation cannot run in place
    if (!h->have_keys) return HEXL_E_NOKEYS;
    if (!batch) return 0;
    hexl_ks_plan* p = h->plan;
    HX_CHECK(hipSetDevice(p->ctx->device));
    const size_t n = p->n, l = n_limbs;
    return hks_slices(h, d_out, batch, (u32)l, [&](size_t b0, size_t nb, u64* out, u64* t) {
        // out = (sigma_g(c0), sigma_g(c1)), then component 1 moves to the slice buffer and is zeroed
        if (int rc = hx_launch_galois(p->ctx, out, d_ct + b0 * 2 * l * n, nb * 2 * l, p->logn, (u32)galois_elt)) return rc;
        const HksMoveArgs a{nullptr, out, t, (u32)l, p->logn};
        hipLaunchKernelGGL(k_hks_take_c1, dim3(hks_piece_grid(p, nb * l)), dim3(HKS_THREADS), 0, p->ctx->stream, a);
        return (int)hipGetLastError();
    });
}

extern "C" size_t hexl_hks_scratch_bytes(const hexl_hks* h, size_t batch) {
    if (!h) return 0;
    return hks_chunk_of(h, batch) * hks_rows(h).ks() * hks_row_bytes(h);
}

// ---- the hybrid multiply: the tensor sum, the key switch of its component 2 and -- the rescaling calls -- ONE mod-down
// by R = P q_(l-1) instead of the key switch's by P and hexl_rescale's by q_(l-1). The tensor kernel is ct_tensor.hip's, launched through
// hx_launch_tensor with its two output descriptors pointed at this object's buffers. ----
// What the two tensor-fed entry points check alike, everything HEXL_E_BADARG: arrays, term count, handle and level (lo ... L), operand
// entries and their overlap with d_out[batch][2][out_limbs][n], sizes and grids. `s` comes back with the operands laid in.
static bool hks_mul_ok(const hexl_hks* h, const u64* d_out, const u64* const* d_as, const u64* const* d_bs, const u64* in_limbs, size_t n_terms,
                       size_t batch, u64 n_limbs, u64 lo, u64 out_limbs, TsArgs& s) {
    if (!h || !d_out || !d_as || !d_bs || !hx_in_range(n_terms, 1, TS_MAX_TERMS) || n_limbs < lo) return false;
    size_t bytes, out_bytes, buffers;
    if (!hks_call_ok(h, batch, n_limbs, 2, &bytes)) return false;
    const hexl_ks_plan* p = h->plan;
    // the largest operand has K limbs: if that size fits, every other one does; the slice and d01 buffers; the tensor kernel's grid
    if (!hx_words_bytes(batch, 2, p->K, p->n, &bytes) || !hx_words_bytes(batch, 2, out_limbs, p->n, &out_bytes) ||
        !hx_words_bytes(hks_chunk_of(h, batch), 1, hks_rows(h).slice + hks_rows(h).d01, p->n, &buffers) || !hx_ww_grid_ok(p, hks_chunk_of(h, batch), n_limbs) ||
        !hx_wg_grid_ok(hks_chunk_of(h, batch), 2 * u64(p->K)))
        return false;
    return hx_tensor_operands(p, d_as, d_bs, in_limbs, n_terms, batch, n_limbs, d_out, out_bytes, s) == 0;
}
// the tensor sums of instances b0 ... b0 + nb - 1: components 0-1 to out01 ([nb][2][l][n]), component 2 to out2 ([nb][l][n])
static int hks_mul_tensor(hexl_ks_plan* p, const TsArgs& s, size_t b0, size_t nb, u64* out01, u64* out2) {
    const size_t n = p->n;
    TsArgs c = s;
    for (u32 k = 0; k < s.n_terms; ++k) {
        c.a[k] += b0 * 2 * c.la[k] * n;
        c.b[k] += b0 * 2 * c.lb[k] * n;
    }
    c.out01 = out01;
    c.out2 = out2;
    c.stride01 = 2ull * s.L * n;
    c.stride2 = 1ull * s.L * n;
    return hx_launch_tensor(p, c, nb);
}

extern "C" int hexl_hks_multiply_sum_relinearize(hexl_hks* h, uint64_t* d_out, const uint64_t* const* d_as, const uint64_t* const* d_bs,
                                                 const uint64_t* in_limbs, size_t n_terms, size_t batch, uint64_t n_limbs) {
    TsArgs s{};
    if (!hks_mul_ok(h, d_out, d_as, d_bs, in_limbs, n_terms, batch, n_limbs, 1, n_limbs, s)) return HEXL_E_BADARG;
    if (!h->have_keys) return HEXL_E_NOKEYS;
    if (!batch) return 0;
    hexl_ks_plan* p = h->plan;
    HX_CHECK(hipSetDevice(p->ctx->device));
    return hks_slices(h, d_out, batch, (u32)n_limbs, [&](size_t b0, size_t nb, u64* out, u64* t) { return hks_mul_tensor(p, s, b0, nb, out, t); });
}

extern "C" int hexl_hks_relinearize_rescale(hexl_hks* h, uint64_t* d_out, const uint64_t* d_ct3, size_t batch, uint64_t n_limbs) {
    size_t in_bytes;
    if (!d_out || !d_ct3 || n_limbs < 2 || !hks_call_ok(h, batch, n_limbs, 3, &in_bytes)) return HEXL_E_BADARG;
    if (hx_ranges_overlap(d_out, in_bytes / (3 * n_limbs) * 2 * (n_limbs - 1), d_ct3, in_bytes)) return HEXL_E_BADARG;
    if (!hx_wg_grid_ok(hks_chunk_of(h, batch), 2 * u64(h->plan->K))) return HEXL_E_BADARG;
    if (!h->have_keys) return HEXL_E_NOKEYS;
    if (!batch) return 0;
    HX_CHECK(hipSetDevice(h->plan->ctx->device));
    const size_t n = h->plan->n, l = n_limbs;
    // d2 and (d0, d1) are read where they lie: no split copy
    return hks_launch(h, batch, (u32)l, [&](size_t b0, size_t, HksArgs& a) {
        a.result = d_out + b0 * 2 * (l - 1) * n;
        a.d01 = d_ct3 + b0 * 3 * l * n;
        a.d01_stride = 3ull * l * n;
        a.t = a.d01 + 2 * l * n;
        a.tstride = 3 * (u32)l;
        return 0;
    });
}

extern "C" int hexl_hks_multiply_sum_rescale(hexl_hks* h, uint64_t* d_out, const uint64_t* const* d_as, const uint64_t* const* d_bs,
                                             const uint64_t* in_limbs, size_t n_terms, size_t batch, uint64_t n_limbs) {
    TsArgs s{};
    if (!hks_mul_ok(h, d_out, d_as, d_bs, in_limbs, n_terms, batch, n_limbs, 2, n_limbs - 1, s)) return HEXL_E_BADARG;
    if (!h->have_keys) return HEXL_E_NOKEYS;
    if (!batch) return 0;
    hexl_ks_plan* p = h->plan;
    HX_CHECK(hipSetDevice(p->ctx->device));
    const size_t n = p->n, l = n_limbs, chunk = hks_chunk_of(h, batch);
    if (int rc = h->d_slice.reserve(chunk * hks_rows(h).slice * n)) return rc;
    if (int rc = h->d_d01.reserve(chunk * hks_rows(h).d01 * n)) return rc;
    // one lane: the next chunk's tensor kernel overwrites the two buffers behind this chunk's last kernel that reads them
    return hks_launch(h, batch, (u32)l, [&](size_t b0, size_t nb, HksArgs& a) {
        a.result = d_out + b0 * 2 * (l - 1) * n;
        a.d01 = h->d_d01;
        a.d01_stride = 2ull * l * n;
        a.t = h->d_slice;
        a.tstride = (u32)l;
        return hks_mul_tensor(p, s, b0, nb, h->d_d01, h->d_slice);
    });
}

extern "C" size_t hexl_hks_mul_scratch_bytes(const hexl_hks* h, size_t batch) {
    if (!h) return 0;
    const HksRows r = hks_rows(h);
    return hks_chunk_of(h, batch) * (r.ks() + r.slice + r.d01) * hks_row_bytes(h);
}

// ---- the hoisted callers: many rotations of one ciphertext batch share steps 1-2 (hexl_hks_rotate_hoisted), and step 4 as well
// (hexl_hks_linear_transform). One run works in hks[0]'s scratch, chunk after chunk, everything on the context's stream: one lane, so
// the next chunk's mod-up overwrites ext behind the last multiply-accumulate that read it. The other objects lend their keys only. ----
struct HksHoist {
    hexl_hks* h0;
    hexl_ks_plan* p;
    size_t chunk, per;                                            // instances per chunk; words of one ciphertext, 2 l n
    HksArgs a;
    int lazy;
    HksHoist(hexl_hks* h, size_t batch, u32 l)
        : h0(h), p(h->plan), chunk(hks_chunk_of(h, batch)), per(2 * size_t(l) * h->plan->n), a(hks_args(h, l)), lazy(hks_level_tier(h->plan, l)) {}
    // hks[0]'s key switch scratch and w of component 1 in a buffer of its own: ext has to survive step 4 for the next rotation
    int reserve() {
        if (int rc = hks_reserve(h0, chunk)) return rc;
        if (int rc = h0->d_w1.reserve(chunk * hks_rows(h0).w1 * p->n)) return rc;
        a.coef = h0->d_coef; a.ext = h0->d_ext; a.acc = h0->d_acc; a.w1 = h0->d_w1;
        a.tstride = 2 * a.l;
        return 0;
    }
    // steps 1-2 on component 1 of nb ciphertexts [nb][2][l][n], read in place, into ext
    int up(const u64* d_ct, size_t nb) {
        a.t = d_ct + per / 2;
        a.nb = (u32)nb;
        return hx_with_f64_geom(p->logn, lazy, [&](auto N, auto E, auto Z) { return hks_stage_up<N, E, Z>(h0, a); });
    }
    // `store` (HKS_MAC_STORE): the sums go there, [nb][2][T][n], instead of acc
    int mac(const hexl_hks* keys, u32 g, HksMacMode mode, const u64* d_pt, double* store = nullptr) const {
        HksArgs m = a;
        if (store) m.acc = store;
        return hks_stage_mac_galois(h0, m, HksRot{keys->d_keys, d_pt, g}, mode);
    }
    // step 3 of a giant step: the weighted sum of stored baby products into acc
    int sum(const HksBsgsTerm* d_terms, size_t n_terms) const { return hks_stage_bsgs_sum(h0, a, d_terms, (u32)n_terms); }
    // step 4 on acc, ADDED into d_out
    int down(u64* d_out) {
        a.result = d_out;
        return hx_with_f64_geom(p->logn, lazy, [&](auto N, auto E, auto Z) { return hks_stage_down<N, E, Z, false>(h0, a); });
    }
    // ---- hexl_hks_linear_transform_bsgs_ext: A is the sum of the giant steps in the extended basis, [nb][2][T][n] ----
    // step 4 on component 1 of acc alone, ADDED into component 1 of d_t[nb][2][l][n]; w in d_w1, coef and component 0 untouched
    int down_c1(u64* d_t) {
        a.result = d_t;
        return hx_with_f64_geom(p->logn, lazy, [&](auto N, auto E, auto Z) { return hks_stage_down_c1<N, E, Z>(h0, a); });
    }
    // A += sigma_g of the first n_comp components of acc, every row of T_l
    int ext_add(double* A, u32 g, u32 n_comp) const {
        HksArgs m = a;
        m.acc = A;
        return hks_stage_ext_add(h0, m, a.acc, g, n_comp);
    }
    // the one mod-down of A: by P, ADDED into d_out[nb][2][l][n] (F == nullptr: the key-free sums lie there), or by R = P q_(l-1) with
    // d_k = F_k ([nb][2][l][n]), WRITTEN to d_out[nb][2][l - 1][n]
    int down_ext(double* A, u64* d_out, const u64* F) const {
        HksArgs m = a;
        m.acc = A;
        m.result = d_out;
        m.d01 = F;
        m.d01_stride = per;
        return hx_with_f64_geom(p->logn, lazy, [&](auto N, auto E, auto Z) {
            return F ? hks_stage_down<N, E, Z, true>(h0, m) : hks_stage_down<N, E, Z, false>(h0, m);
        });
    }
};

// What the three hoisted entry points check alike (everything here decides HEXL_E_BADARG). hks_hoist_ok: plan, level, sizes and grids of
// a run in h0's scratch. s: bytes of a batch of ciphertexts, of one plaintext [K][n], of the rows of an identity plaintext that are read.
// hks_hoist_list_ok: the objects of one list share h0's plan and alpha, and the list's Galois elements. A NULL object passes: the BSGS
// call allows one where it is unused, the other two have refused it before they come here. The BSGS call did not run hks_hoist_ok's
// overflow check of the key switch's rows + w1 at the key switch's chunk before it shared this function; it is a new
// refusal there, reachable only with scratch sizes near 2^64 bytes, and gives the HEXL_E_BADARG that call's own size check gives.
struct HksHoistBytes { size_t ct, pt, id; };
static bool hks_hoist_ok(const hexl_hks* h0, size_t batch, u64 n_limbs, HksHoistBytes* s) {
    if (!hks_call_ok(h0, batch, n_limbs, 2, &s->ct)) return false;
    const hexl_ks_plan* p = h0->plan;
    const HksRows r = hks_rows(h0);
    size_t scratch;                                               // with w of component 1
    if (!hx_words_bytes(hks_chunk_of(h0, batch), 1, r.ks() + r.w1, p->n, &scratch)) return false;
    s->pt = size_t(p->K) * p->n * sizeof(u64);
    s->id = size_t(n_limbs) * p->n * sizeof(u64);
    return true;
}
static bool hks_hoist_list_ok(const hexl_hks* h0, hexl_hks* const* hks, const u64* galois_elts, size_t count) {
    for (size_t r = 0; r < count; ++r) {
        if (hks[r] && (hks[r]->plan != h0->plan || hks[r]->alpha != h0->alpha)) return false;
        if (!hks_galois_elt_ok(galois_elts[r], h0->plan->n)) return false;
    }
    return true;
}

extern "C" int hexl_hks_rotate_hoisted(hexl_hks* const* hks, const uint64_t* galois_elts, size_t n_rot, uint64_t* const* d_outs,
                                       const uint64_t* d_ct, size_t batch, uint64_t n_limbs) {
    if (!hks || !galois_elts || !d_outs || !d_ct) return HEXL_E_BADARG;
    if (!n_rot) return 0;
    for (size_t r = 0; r < n_rot; ++r)
        if (!hks[r] || !d_outs[r]) return HEXL_E_BADARG;
    HksHoistBytes s;
    if (!hks_hoist_ok(hks[0], batch, n_limbs, &s) || !hks_hoist_list_ok(hks[0], hks, galois_elts, n_rot)) return HEXL_E_BADARG;
    for (size_t r = 0; r < n_rot; ++r) {
        if (hx_ranges_overlap(d_outs[r], s.ct, d_ct, s.ct)) return HEXL_E_BADARG;
        for (size_t q = 0; q < r; ++q)
            if (hx_ranges_overlap(d_outs[r], s.ct, d_outs[q], s.ct)) return HEXL_E_BADARG;
    }
    for (size_t r = 0; r < n_rot; ++r)
        if (!hks[r]->have_keys) return HEXL_E_NOKEYS;
    if (!batch) return 0;
    hexl_ks_plan* p = hks[0]->plan;
    HX_CHECK(hipSetDevice(p->ctx->device));
    HksHoist run(hks[0], batch, (u32)n_limbs);
    if (int rc = run.reserve()) return rc;
    // per chunk: the mod-up of c1, then per rotation (sigma_g(c0), 0) into its output, its multiply-accumulate and step 4 added into it
    return hx_for_chunks(batch, run.chunk, [&](size_t b0, size_t nb) {
        const u64* ct = d_ct + b0 * run.per;
        if (int rc = run.up(ct, nb)) return rc;
        for (size_t r = 0; r < n_rot; ++r) {
            const u32 g = (u32)galois_elts[r];
            u64* out = d_outs[r] + b0 * run.per;
            if (int rc = hx_launch_galois_c0(p->ctx, out, ct, nb, (u32)n_limbs, p->logn, g)) return rc;
            if (int rc = run.mac(hks[r], g, HKS_MAC_STORE, nullptr)) return rc;
            if (int rc = run.down(out)) return rc;
        }
        return 0;
    });
}

extern "C" int hexl_hks_linear_transform(hexl_hks* const* hks, const uint64_t* galois_elts, const uint64_t* const* d_pts, size_t n_rot,
                                         const uint64_t* d_pt_identity, uint64_t* d_out, const uint64_t* d_ct, size_t batch,
                                         uint64_t n_limbs) {
    if (!hks || !galois_elts || !d_pts || !d_out || !d_ct || !n_rot) return HEXL_E_BADARG;
    if (n_rot > SIZE_MAX / sizeof(HxLtRot)) return HEXL_E_BADARG;
    for (size_t r = 0; r < n_rot; ++r)
        if (!hks[r] || !d_pts[r]) return HEXL_E_BADARG;
    HksHoistBytes s;
    if (!hks_hoist_ok(hks[0], batch, n_limbs, &s) || !hks_hoist_list_ok(hks[0], hks, galois_elts, n_rot)) return HEXL_E_BADARG;
    if (hx_ranges_overlap(d_out, s.ct, d_ct, s.ct)) return HEXL_E_BADARG;
    if (d_pt_identity && hx_ranges_overlap(d_out, s.ct, d_pt_identity, s.id)) return HEXL_E_BADARG;
    for (size_t r = 0; r < n_rot; ++r)
        if (hx_ranges_overlap(d_out, s.ct, d_pts[r], s.pt)) return HEXL_E_BADARG;
    for (size_t r = 0; r < n_rot; ++r)
        if (!hks[r]->have_keys) return HEXL_E_NOKEYS;
    if (!batch) return 0;
    hexl_ks_plan* p = hks[0]->plan;
    hexl_ctx* c = p->ctx;
    HX_CHECK(hipSetDevice(c->device));
    HksHoist run(hks[0], batch, (u32)n_limbs);
    if (int rc = run.reserve()) return rc;
    // the per-call table of the key-free kernel, as hx_launch_linear_transform builds it (keyswitch_f64.hip): pageable source, so the copy
    // has left it when hipMemcpyAsync returns, and the stream orders it behind the previous call's kernels that read the table
    std::vector<HxLtRot> table(n_rot);
    for (size_t r = 0; r < n_rot; ++r) table[r] = HxLtRot{d_pts[r], galois_elts[r]};
    if (int rc = c->d_shared.reserve(n_rot * sizeof(HxLtRot))) return rc;
    HX_CHECK(hipMemcpyAsync(c->d_shared, table.data(), n_rot * sizeof(HxLtRot), hipMemcpyHostToDevice, c->stream));
    // per chunk: the mod-up of c1, the key-free terms into d_out, one multiply-accumulate per rotation into acc, step 4 ONCE added into d_out
    return hx_for_chunks(batch, run.chunk, [&](size_t b0, size_t nb) {
        const u64* ct = d_ct + b0 * run.per;
        u64* out = d_out + b0 * run.per;
        if (int rc = run.up(ct, nb)) return rc;
        if (int rc = hx_launch_galois_c0_pt(p, out, ct, (const HxLtRot*)c->d_shared.get(), n_rot, d_pt_identity, nb, (u32)n_limbs, nullptr)) return rc;
        for (size_t r = 0; r < n_rot; ++r)
            if (int rc = run.mac(hks[r], (u32)galois_elts[r], r ? HKS_MAC_PT_ACC : HKS_MAC_PT_FIRST, d_pts[r])) return rc;
        return run.down(out);
    });
}

extern "C" size_t hexl_hks_hoisted_scratch_bytes(const hexl_hks* h, size_t batch) {
    if (!h) return 0;
    const HksRows r = hks_rows(h);
    return hks_chunk_of(h, batch) * (r.ks() + r.w1) * hks_row_bytes(h);
}

// ---- baby-step/giant-step linear transform on the hybrid gadget (hexl_hks_linear_transform_bsgs):
//      out = sum_j Rot_{G_j}( sum_i pt_{j,i} . Rot_{g_i}(ct) + pt_id_j . ct ),  hx_launch_linear_transform_bsgs (keyswitch_f64.hip) stage by
// stage on the hybrid stages. Per chunk, in h0's scratch (h0: the first non-NULL object, baby objects first):
//   the mod-up of c1 once; one k_hks_mac<., STORE> per baby step that some row uses, its sums pointed at that step's slice of the
//   baby store (coef and ext are free after the last of them);
//   per giant step j: the key-free part of row j into t_j (hx_launch_galois_c0_pt), the weighted sum of the stored products into acc
//   (k_hks_bsgs_sum) and the mod-down ONCE, added into t_j -- hexl_hks_linear_transform's words for row j; then t_j rotated by G_j as
//   hexl_hks_rotate_hoisted rotates it (mod-up of t_j's component 1 into the same coef / ext, giant_hks[j]'s keys) with the key-free part
//   sigma_{G_j}(t_j[0]) WRITTEN to d_out by the first giant step and ADDED by the later ones, and the mod-down accumulating on top.
//   G_j = 1: t_j itself is written (the first giant step computes it in place in d_out) or added.
// Where w of component 1 lives (the scratch pitfall of 4.6.11): in BOTH mod-downs -- the row's and the giant rotation's -- in d_w1, the
// hoisted callers' buffer, never on ext; w of component 0 in coef, which is dead once the mod-up's conversion has run and is rewritten
// by the next mod-up only behind the mod-down that read it (one stream). So no consumer of ext can meet a w.
// Every word that reaches d_out is canonical and every addition is modulo q_i, so d_out holds the sum of the per-row results of the two
// parent entry points, word for word. ----
static size_t hks_bsgs_slice_bytes(const hexl_hks* h) { return 2 * size_t(h->plan->K) * h->plan->n * sizeof(double); }   // one baby step, one instance
static size_t hks_bsgs_chunk(const hexl_hks* h, size_t n_baby, size_t batch) {
    const size_t chunk = hks_chunk_of(h, batch);
    if (hx_ks_chunk_forced() || !n_baby || !chunk) return chunk;  // a forced chunk stays
    const size_t fit = HX_LT_BSGS_STORE_BYTES / hks_bsgs_slice_bytes(h) / n_baby;
    return fit >= chunk ? chunk : fit ? fit : 1;
}

// ext: hexl_hks_linear_transform_bsgs_ext, which holds A as well, and F with rescale = 1
static size_t hks_bsgs_scratch(const hexl_hks* h, size_t n_baby, size_t batch, bool ext, int rescale) {
    const size_t chunk = hks_bsgs_chunk(h, n_baby, batch);
    // per instance: the hoisted callers' scratch and t_j
    const HksRows r = hks_rows(h);
    const size_t fixed = (r.ks() + r.w1 + r.t + (ext ? r.ext_a : 0) + (ext && rescale ? r.d01 : 0)) * hks_row_bytes(h);
    if (chunk && (fixed > SIZE_MAX / chunk || n_baby > (SIZE_MAX / chunk - fixed) / hks_bsgs_slice_bytes(h))) return SIZE_MAX;
    return chunk * (n_baby * hks_bsgs_slice_bytes(h) + fixed);
}
extern "C" size_t hexl_hks_bsgs_scratch_bytes(const hexl_hks* h, size_t n_baby, size_t batch) {
    return h ? hks_bsgs_scratch(h, n_baby, batch, false, 0) : 0;
}
extern "C" size_t hexl_hks_bsgs_ext_scratch_bytes(const hexl_hks* h, size_t n_baby, size_t batch, int rescale) {
    return h ? hks_bsgs_scratch(h, n_baby, batch, true, rescale) : 0;
}

// What the two BSGS entry points check alike and in this order: HEXL_E_BADARG, then HEXL_E_NOKEYS for an object that is USED. out_limbs:
// the limbs of d_out[batch][2][out_limbs][n] (n_limbs, or n_limbs - 1 behind the folded rescale). *h0_out: the scratch owner.
static int hks_bsgs_check(hexl_hks* const* baby_hks, const uint64_t* baby_elts, size_t n_baby, hexl_hks* const* giant_hks,
                          const uint64_t* giant_elts, size_t n_giant, const uint64_t* const* d_pts, const uint64_t* const* d_pt_identity,
                          const uint64_t* d_out, const uint64_t* d_ct, size_t batch, uint64_t n_limbs, uint64_t out_limbs, bool ext,
                          int rescale, hexl_hks** h0_out) {
    if (!baby_hks || !baby_elts || !giant_hks || !giant_elts || !d_pts || !d_out || !d_ct || !n_giant) return HEXL_E_BADARG;
    if (n_giant > SIZE_MAX / sizeof(HxLtRot) / 2 || (n_baby && n_giant > SIZE_MAX / sizeof(HxLtRot) / 2 / n_baby)) return HEXL_E_BADARG;
    // the object that lends its scratch and buffers: baby_hks[0] whenever there is one
    hexl_hks* h0 = nullptr;
    for (size_t i = 0; i < n_baby && !h0; ++i) h0 = baby_hks[i];
    for (size_t j = 0; j < n_giant && !h0; ++j) h0 = giant_hks[j];
    if (!h0) return HEXL_E_BADARG;
    // the rows and the objects a term needs, then what the hoisted callers check too (at the key switch's chunk, which this call's never
    // exceeds), then the overlaps and the sizes of the baby store
    for (size_t j = 0; j < n_giant; ++j) {
        bool any = d_pt_identity && d_pt_identity[j];
        for (size_t i = 0; i < n_baby && !any; ++i) any = d_pts[j * n_baby + i] != nullptr;
        if (!any) return HEXL_E_BADARG;                             // a giant row with no term at all
    }
    for (size_t j = 0; j < n_giant; ++j)
        for (size_t i = 0; i < n_baby; ++i)
            if (d_pts[j * n_baby + i] && !baby_hks[i]) return HEXL_E_BADARG;
    for (size_t j = 0; j < n_giant; ++j)
        if (!giant_hks[j] && giant_elts[j] != 1) return HEXL_E_BADARG;
    HksHoistBytes s;
    if (!hks_hoist_ok(h0, batch, n_limbs, &s) || !hks_hoist_list_ok(h0, baby_hks, baby_elts, n_baby) ||
        !hks_hoist_list_ok(h0, giant_hks, giant_elts, n_giant))
        return HEXL_E_BADARG;
    // the output's real size: the overlap checks of hexl_hks_linear_transform_bsgs_ext with rescale = 1 see [batch][2][n_limbs - 1][n]
    const size_t out_bytes = s.ct / n_limbs * out_limbs;
    if (hx_ranges_overlap(d_out, out_bytes, d_ct, s.ct)) return HEXL_E_BADARG;
    for (size_t j = 0; j < n_giant; ++j) {
        const u64* pt_id = d_pt_identity ? d_pt_identity[j] : nullptr;
        if (pt_id && hx_ranges_overlap(d_out, out_bytes, pt_id, s.id)) return HEXL_E_BADARG;
        for (size_t i = 0; i < n_baby; ++i)
            if (const u64* pt = d_pts[j * n_baby + i])
                if (hx_ranges_overlap(d_out, out_bytes, pt, s.pt)) return HEXL_E_BADARG;
    }
    if (n_baby > HX_LT_BSGS_STORE_BYTES / hks_bsgs_slice_bytes(h0)) return HEXL_E_BADARG;   // not one instance would fit the baby store
    if (hks_bsgs_scratch(h0, n_baby, batch, ext, rescale) == SIZE_MAX) return HEXL_E_BADARG;
    for (size_t j = 0; j < n_giant; ++j) {
        if (giant_elts[j] != 1 && !giant_hks[j]->have_keys) return HEXL_E_NOKEYS;
        for (size_t i = 0; i < n_baby; ++i)
            if (d_pts[j * n_baby + i] && !baby_hks[i]->have_keys) return HEXL_E_NOKEYS;
    }
    *h0_out = h0;
    return 0;
}

// What the two BSGS entry points run alike in h0's scratch: the hoisted callers' buffers at the BSGS chunk, the baby store, t_j, and the
// per-call tables, row after row: what the c0 kernel walks (plaintext, Galois element) and what the sum kernel walks (plaintext, baby
// slice). Pageable sources, stream-ordered behind the previous call's readers, as hexl_hks_linear_transform's table
struct HksBsgsRun {
    HksHoist run;
    size_t slice = 0, total = 0;                                  // doubles of one baby step's slice; terms of all rows
    std::vector<size_t> off;                                      // row j's terms: off[j] ... off[j + 1] - 1
    std::vector<char> used;                                       // baby step i is used by some row
    const HxLtRot* d_rots = nullptr;
    const HksBsgsTerm* d_terms = nullptr;
    HksBsgsRun(hexl_hks* h0, size_t n_baby, size_t n_giant, size_t batch, u32 l) : run(h0, batch, l), off(n_giant + 1), used(n_baby, 0) {
        run.chunk = hks_bsgs_chunk(h0, n_baby, batch);
    }
    int prepare(const uint64_t* baby_elts, const uint64_t* const* d_pts) {
        hexl_hks* h0 = run.h0;
        hexl_ctx* c = run.p->ctx;
        const size_t n_baby = used.size(), n_giant = off.size() - 1, n = run.p->n;
        if (int rc = run.reserve()) return rc;
        slice = run.chunk * 2 * run.p->K * n;
        if (n_baby)
            if (int rc = h0->d_bsgs_b.reserve(n_baby * slice)) return rc;
        if (int rc = h0->d_bsgs_t.reserve(run.chunk * hks_rows(h0).t * n)) return rc;
        std::vector<HxLtRot> rots;
        std::vector<HksBsgsTerm> terms;
        for (size_t j = 0; j < n_giant; ++j) {
            off[j] = rots.size();
            for (size_t i = 0; i < n_baby; ++i)
                if (const u64* pt = d_pts[j * n_baby + i]) {
                    rots.push_back(HxLtRot{pt, baby_elts[i]});
                    terms.push_back(HksBsgsTerm{pt, h0->d_bsgs_b + i * slice});
                    used[i] = 1;
                }
        }
        total = off[n_giant] = rots.size();
        static_assert(sizeof(HxLtRot) == 16 && sizeof(HksBsgsTerm) == 16, "the two tables share one 16-byte-aligned reservation");
        if (total) {
            if (int rc = c->d_shared.reserve(total * (sizeof(HxLtRot) + sizeof(HksBsgsTerm)))) return rc;
            HX_CHECK(hipMemcpyAsync(c->d_shared, rots.data(), total * sizeof(HxLtRot), hipMemcpyHostToDevice, c->stream));
            HX_CHECK(hipMemcpyAsync((HxLtRot*)c->d_shared.get() + total, terms.data(), total * sizeof(HksBsgsTerm), hipMemcpyHostToDevice, c->stream));
        }
        d_rots = (const HxLtRot*)c->d_shared.get();
        d_terms = (const HksBsgsTerm*)(d_rots + total);
        return 0;
    }
    // the mod-up of c1 and one stored multiply-accumulate per baby step that some row uses (coef and ext are free after the last of them)
    int babies(hexl_hks* const* baby_hks, const uint64_t* baby_elts, const u64* ct, size_t nb) {
        if (!total) return 0;
        if (int rc = run.up(ct, nb)) return rc;
        for (size_t i = 0; i < used.size(); ++i)
            if (used[i])
                if (int rc = run.mac(baby_hks[i], (u32)baby_elts[i], HKS_MAC_STORE, nullptr, run.h0->d_bsgs_b + i * slice)) return rc;
        return 0;
    }
};

extern "C" int hexl_hks_linear_transform_bsgs(hexl_hks* const* baby_hks, const uint64_t* baby_elts, size_t n_baby,
                                              hexl_hks* const* giant_hks, const uint64_t* giant_elts, size_t n_giant,
                                              const uint64_t* const* d_pts, const uint64_t* const* d_pt_identity, uint64_t* d_out,
                                              const uint64_t* d_ct, size_t batch, uint64_t n_limbs) {
    hexl_hks* h0 = nullptr;
    if (int rc = hks_bsgs_check(baby_hks, baby_elts, n_baby, giant_hks, giant_elts, n_giant, d_pts, d_pt_identity, d_out, d_ct, batch, n_limbs,
                                n_limbs, false, 0, &h0))
        return rc;
    if (!batch) return 0;
    hexl_ks_plan* p = h0->plan;
    hexl_ctx* c = p->ctx;
    HX_CHECK(hipSetDevice(c->device));
    const u32 l = (u32)n_limbs;
    HksBsgsRun br(h0, n_baby, n_giant, batch, l);
    if (int rc = br.prepare(baby_elts, d_pts)) return rc;
    HksHoist& run = br.run;
    const std::vector<size_t>& off = br.off;
    const HxLtRot* d_rots = br.d_rots;
    const HksBsgsTerm* d_terms = br.d_terms;
    return hx_for_chunks(batch, run.chunk, [&](size_t b0, size_t nb) {
        const u64* ct = d_ct + b0 * run.per;
        u64* out = d_out + b0 * run.per;
        run.a.nb = (u32)nb;
        if (int rc = br.babies(baby_hks, baby_elts, ct, nb)) return rc;
        for (size_t j = 0; j < n_giant; ++j) {
            const size_t cnt = off[j + 1] - off[j];
            const u32 g = (u32)giant_elts[j];
            u64* t = (j == 0 && g == 1) ? out : h0->d_bsgs_t.get();
            if (int rc = hx_launch_galois_c0_pt(p, t, ct, d_rots + off[j], cnt, d_pt_identity ? d_pt_identity[j] : nullptr, nb, l, nullptr)) return rc;
            if (cnt) {
                if (int rc = run.sum(d_terms + off[j], cnt)) return rc;
                if (int rc = run.down(t)) return rc;                // accumulated into what the c0 kernel wrote; w1 in d_w1
            }
            if (g == 1) {
                if (j)
                    if (int rc = hx_launch_galois_add(p, out, t, nb, 1, 2, l)) return rc;
                continue;
            }
            if (int rc = run.up(t, nb)) return rc;                  // the babies are stored: coef and ext are free
            if (int rc = j ? hx_launch_galois_add(p, out, t, nb, g, 1, l) : hx_launch_galois_c0(c, out, t, nb, l, p->logn, g)) return rc;
            if (int rc = run.mac(giant_hks[j], g, HKS_MAC_STORE, nullptr)) return rc;
            if (int rc = run.down(out)) return rc;                  // w1 in d_w1 again
        }
        return 0;
    });
}

// ---- the double-hoisted BSGS (hexl_hks_linear_transform_bsgs_ext): the giant steps are summed in the extended basis
// and divided ONCE. Per chunk, in h0's scratch: the babies as above; A (d_ext_a) and F -- d_out itself, or d_d01 with the rescale folded
// in -- zeroed; per row j the key-free part kf_j into t_j and the weighted sum of the stored products into acc (an identity-only row
// that rotates: zeros), then
//   G_j = 1:  F += kf_j, A += inner_j (both components, no permutation);
//   G_j != 1: the HALF mod-down of acc's component 1 added into t_j's component 1 (u_j; w in d_w1, coef and component 0 untouched),
//             A[0] += sigma_G(inner_j[0]) on every row of T_l, the mod-up of u_j into coef / ext (the babies are stored: both are free),
//             F[0] += sigma_G(kf_j[0]), A += the giant key's multiply-accumulate of sigma_G(ext');
// and the mod-down of A: by P added into F, or by R = P q_(l-1) with d_k = F_k. One lane: every reader of t_j, acc, coef and ext is in
// front of the next row's writer on the stream. ----
extern "C" int hexl_hks_linear_transform_bsgs_ext(hexl_hks* const* baby_hks, const uint64_t* baby_elts, size_t n_baby,
                                                  hexl_hks* const* giant_hks, const uint64_t* giant_elts, size_t n_giant,
                                                  const uint64_t* const* d_pts, const uint64_t* const* d_pt_identity, uint64_t* d_out,
                                                  const uint64_t* d_ct, size_t batch, uint64_t n_limbs, int rescale) {
    if ((rescale != 0 && rescale != 1) || (rescale && n_limbs < 2)) return HEXL_E_BADARG;
    hexl_hks* h0 = nullptr;
    if (int rc = hks_bsgs_check(baby_hks, baby_elts, n_baby, giant_hks, giant_elts, n_giant, d_pts, d_pt_identity, d_out, d_ct, batch, n_limbs,
                                n_limbs - rescale, true, rescale, &h0))
        return rc;
    if (!batch) return 0;
    hexl_ks_plan* p = h0->plan;
    hexl_ctx* c = p->ctx;
    HX_CHECK(hipSetDevice(c->device));
    const u32 l = (u32)n_limbs;
    HksBsgsRun br(h0, n_baby, n_giant, batch, l);
    if (int rc = br.prepare(baby_elts, d_pts)) return rc;
    HksHoist& run = br.run;
    const size_t n = p->n;
    if (int rc = h0->d_ext_a.reserve(run.chunk * hks_rows(h0).ext_a * n)) return rc;
    if (rescale)
        if (int rc = h0->d_d01.reserve(run.chunk * hks_rows(h0).d01 * n)) return rc;
    double* A = h0->d_ext_a;
    return hx_for_chunks(batch, run.chunk, [&](size_t b0, size_t nb) {
        const u64* ct = d_ct + b0 * run.per;
        u64* out = d_out + b0 * 2 * (l - rescale) * n;
        u64* F = rescale ? h0->d_d01.get() : out;
        u64* t = h0->d_bsgs_t.get();
        run.a.nb = (u32)nb;
        const size_t row_words = size_t(run.a.T) * n, acc_bytes = nb * 2 * row_words * sizeof(double);   // one component of one instance; A
        if (int rc = br.babies(baby_hks, baby_elts, ct, nb)) return rc;
        HX_CHECK(hipMemsetAsync(A, 0, acc_bytes, c->stream));
        HX_CHECK(hipMemsetAsync(F, 0, nb * run.per * sizeof(u64), c->stream));
        for (size_t j = 0; j < n_giant; ++j) {
            const size_t cnt = br.off[j + 1] - br.off[j];
            const u32 g = (u32)giant_elts[j];
            if (int rc = hx_launch_galois_c0_pt(p, t, ct, br.d_rots + br.off[j], cnt, d_pt_identity ? d_pt_identity[j] : nullptr, nb, l, nullptr)) return rc;
            if (cnt)
                if (int rc = run.sum(br.d_terms + br.off[j], cnt)) return rc;
            if (g == 1) {
                if (int rc = hx_launch_galois_add(p, F, t, nb, 1, 2, l)) return rc;
                if (cnt)
                    if (int rc = run.ext_add(A, 1, 2)) return rc;
                continue;
            }
            // inner_j = 0: u_j = kf_j[1] + down_P(0), the overshoot alone. Component 1 of every instance is cleared (one strided fill);
            // component 0 is neither read nor written for such a row
            if (!cnt) HX_CHECK(hipMemset2DAsync(run.a.acc + row_words, 2 * row_words * sizeof(double), 0, row_words * sizeof(double), nb, c->stream));
            if (int rc = run.down_c1(t)) return rc;
            if (cnt)
                if (int rc = run.ext_add(A, g, 1)) return rc;
            if (int rc = run.up(t, nb)) return rc;
            if (int rc = hx_launch_galois_add(p, F, t, nb, g, 1, l)) return rc;
            if (int rc = run.mac(giant_hks[j], g, HKS_MAC_ACC, nullptr, A)) return rc;
        }
        return run.down_ext(A, out, rescale ? F : nullptr);
    });
}
