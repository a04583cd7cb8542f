// ckks_encode.hip -- the canonical embedding on the device: the one step of a CKKS flow that was host-only (DESIGN.md 4.6.4 "Encode and
// decode"). zeta = exp(i pi / n); slot k < n/2 belongs to the evaluation point zeta^(5^k mod 2n) (SEAL's convention, and the example's).
//   rns_from_f64   out[c][i] = NTT_i(rint(coeff_j) mod q_i)                                k_rns_from_f64 (k_rns_fwd with another load)
//   rns_to_f64     INTT_i per limb (rns_ops.hip k_rns_inv into plan scratch), then the centred CRT value of every coefficient
//                  as a double through Garner's mixed-radix digits                          k_crt_to_f64
//   ckks_encode    coeff_j = scale (2/n) Re(sum_k z_k zeta^(-j 5^k)), then rns_from_f64     k_embed_inv (+ k_embed_inv_top at n = 32768)
//   ckks_decode    rns_to_f64, then z_k = m(zeta^(5^k)) / scale                             k_embed_fwd (+ k_embed_fwd_top)
// The embedding as ONE plain FFT of n/2 complex points. With u_j = m_j + i m_(j + n/2) (zeta^(n/2 . 5^k) = i for every k) and 5^k = 4 s + 1:
//   z_k = sum_(j < n/2) (u_j zeta^j) exp(2 pi i j s / (n/2)):  a twist by zeta^j, a DFT of n/2 points, and the permutation s -> k.
// Decode runs it decimation-in-frequency (natural order in, bit-reversed out, then the scatter to slot k); encode runs the conjugate
// decimation-in-time (the gather from slot k, bit-reversed in, natural out, then the conjugate twist with scale / (n/2) folded in). Both
// use one table of positions, and the real coefficients live in a plan scratch as n doubles per instance: Re at j, Im at j + n/2 --
// which IS the coefficient vector. FP64 plans only. Twiddles are the plan's table of the 2n-th roots, computed on the host in long
// double and rounded once: no device sincos.
#include <math.h>

#include "hexl_internal.hpp"
#include "ntt_core_f64.hpp"
#include "number_theory.hpp"

using namespace hx;

// ---- the embedding FFT ----
struct cplx { double re, im; };
__device__ __forceinline__ cplx cadd(cplx a, cplx b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cplx csub(cplx a, cplx b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
// zeta^t (t < 2n), conjugated for the encode direction
template <bool CONJ>
__device__ __forceinline__ cplx root(const double2* roots, u32 t) {
    const double2 w = roots[t];
    return {w.x, CONJ ? -w.y : w.y};
}

constexpr u32 EMB_MAX_LOGB = 13;            // complex points one workgroup holds in LDS: 8192 x 16 bytes = 128 KiB of the CU's 160
constexpr u32 EMB_MAX_THREADS = 1024;
constexpr u32 EMB_TOP_THREADS = 256;

struct EmbArgs {
    const double2* roots;       // [2n]
    const u32* perm;            // [n/2]
    double* coeffs;             // [nb][n] plan scratch: Re of point j at j, Im at j + n/2
    const double* slots_in;     // encode: [nb][n/2][2]
    double* slots_out;          // decode: [nb][n/2][2]
    double factor;              // encode: scale / (n/2); decode: 1 / scale
    u32 logn, logb;             // a workgroup holds block blockIdx.x % 2^(logn - 1 - logb) of 2^logb points of instance blockIdx.x >> (logn - 1 - logb)
};

// One radix-2 stage per barrier on 2^logb points in LDS, Re and Im in two arrays of doubles: a half-wave's 32 eight-byte accesses are one
// 256-byte bank row for every stride >= 32 points and two rows below that (the five innermost stages).
// Decode, decimation in frequency: strides 2^(logb-1) ... 1 of a block that starts from natural order. With logb = logn - 1 the block is the
// whole transform and the load applies the twist; otherwise k_embed_fwd_top has run the twist and the one stage that spans the blocks.
__global__ __launch_bounds__(EMB_MAX_THREADS) void k_embed_fwd(EmbArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const u32 logh = a.logn - 1, B = 1u << a.logb, T = blockDim.x, tid = threadIdx.x;
    const u32 inst = blockIdx.x >> (logh - a.logb), part = blockIdx.x - (inst << (logh - a.logb));
    double *re = lds, *im = lds + B;
    const double* c = a.coeffs + (size_t(inst) << a.logn) + (size_t(part) << a.logb);
    const bool whole = a.logb == logh;
    for (u32 p = tid; p < B; p += T) {
        cplx u{c[p], c[p + (size_t(1) << logh)]};
        if (whole) u = cmul(u, root<false>(a.roots, p));
        re[p] = u.re; im[p] = u.im;
    }
    __syncthreads();
    for (int s = int(a.logb) - 1; s >= 0; --s) {
        const u32 h = 1u << s;
        for (u32 bt = tid; bt < B / 2; bt += T) {
            const u32 j = bt & (h - 1), i = ((bt >> s) << (s + 1)) + j;
            const cplx x{re[i], im[i]}, y{re[i + h], im[i + h]};
            const cplx sum = cadd(x, y), d = cmul(csub(x, y), root<false>(a.roots, j << (a.logn - s)));
            re[i] = sum.re; im[i] = sum.im;
            re[i + h] = d.re; im[i + h] = d.im;
        }
        __syncthreads();
    }
    double2* z = reinterpret_cast<double2*>(a.slots_out) + (size_t(inst) << logh);
    const u32* perm = a.perm + (size_t(part) << a.logb);
    for (u32 p = tid; p < B; p += T) z[perm[p]] = double2{re[p] * a.factor, im[p] * a.factor};
}

// Encode, decimation in time with conjugate twiddles: the block's points gathered from their slots, strides 1 ... 2^(logb-1), natural
// order out; the whole transform ends with the conjugate twist and scale / (n/2), a block of a larger one leaves both to k_embed_inv_top.
__global__ __launch_bounds__(EMB_MAX_THREADS) void k_embed_inv(EmbArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const u32 logh = a.logn - 1, B = 1u << a.logb, T = blockDim.x, tid = threadIdx.x;
    const u32 inst = blockIdx.x >> (logh - a.logb), part = blockIdx.x - (inst << (logh - a.logb));
    double *re = lds, *im = lds + B;
    const double2* z = reinterpret_cast<const double2*>(a.slots_in) + (size_t(inst) << logh);
    const u32* perm = a.perm + (size_t(part) << a.logb);
    for (u32 p = tid; p < B; p += T) {
        const double2 v = z[perm[p]];
        re[p] = v.x; im[p] = v.y;
    }
    __syncthreads();
    for (u32 s = 0; s < a.logb; ++s) {
        const u32 h = 1u << s;
        for (u32 bt = tid; bt < B / 2; bt += T) {
            const u32 j = bt & (h - 1), i = ((bt >> s) << (s + 1)) + j;
            const cplx x{re[i], im[i]}, y = cmul(cplx{re[i + h], im[i + h]}, root<true>(a.roots, j << (a.logn - s)));
            const cplx sum = cadd(x, y), d = csub(x, y);
            re[i] = sum.re; im[i] = sum.im;
            re[i + h] = d.re; im[i + h] = d.im;
        }
        __syncthreads();
    }
    double* c = a.coeffs + (size_t(inst) << a.logn) + (size_t(part) << a.logb);
    const bool whole = a.logb == logh;
    for (u32 p = tid; p < B; p += T) {
        cplx u{re[p], im[p]};
        if (whole) {
            u = cmul(u, root<true>(a.roots, p));
            u.re *= a.factor; u.im *= a.factor;
        }
        c[p] = u.re; c[p + (size_t(1) << logh)] = u.im;
    }
}

// n = 32768: the n/2 = 16384 points are two LDS blocks, and the one stage whose stride (n/4) spans them is a plain pass over the plan
// scratch, in place: thread (instance, j < n/4) reads and writes the four doubles of points j and j + n/4, nobody else's.
// Decode: the twist, then the outermost decimation-in-frequency stage.
__global__ __launch_bounds__(EMB_TOP_THREADS) void k_embed_fwd_top(EmbArgs a) {
    const u32 logq = a.logn - 2, g = blockIdx.x * EMB_TOP_THREADS + threadIdx.x;
    const u32 inst = g >> logq, j = g - (inst << logq), h = 1u << logq;
    double* c = a.coeffs + (size_t(inst) << a.logn);
    const size_t im = size_t(2) << logq;
    const cplx x = cmul(cplx{c[j], c[j + im]}, root<false>(a.roots, j));
    const cplx y = cmul(cplx{c[j + h], c[j + h + im]}, root<false>(a.roots, j + h));
    const cplx sum = cadd(x, y), d = cmul(csub(x, y), root<false>(a.roots, 4 * j));
    c[j] = sum.re; c[j + im] = sum.im;
    c[j + h] = d.re; c[j + h + im] = d.im;
}
// Encode: the outermost decimation-in-time stage, then the conjugate twist with scale / (n/2).
__global__ __launch_bounds__(EMB_TOP_THREADS) void k_embed_inv_top(EmbArgs a) {
    const u32 logq = a.logn - 2, g = blockIdx.x * EMB_TOP_THREADS + threadIdx.x;
    const u32 inst = g >> logq, j = g - (inst << logq), h = 1u << logq;
    double* c = a.coeffs + (size_t(inst) << a.logn);
    const size_t im = size_t(2) << logq;
    const cplx x{c[j], c[j + im]}, y = cmul(cplx{c[j + h], c[j + h + im]}, root<true>(a.roots, 4 * j));
    const cplx sum = cmul(cadd(x, y), root<true>(a.roots, j)), d = cmul(csub(x, y), root<true>(a.roots, j + h));
    c[j] = sum.re * a.factor; c[j + im] = sum.im * a.factor;
    c[j + h] = d.re * a.factor; c[j + h + im] = d.im * a.factor;
}

// ---- real coefficients -> NTT-form limbs ----
struct FromF64Args {
    const KsModF64* mods;       // [K]
    const double* tables;       // [K][4][n]
    const double* coeffs;       // [count][n]
    u64* out;                   // [count][n_limbs][n]
    unsigned* flag;             // the plan's input-range flag
    u32 count, n_limbs;
    unsigned long long tiermap;
};
struct FromF64Opt : NttOpt { static constexpr int XSD = 0; };      // centred inputs, a final range reduction: rns_ops.hip RnsFwdOpt

// k_rns_fwd (rns_ops.hip) with another load: limb-major, one transform per workgroup; every limb's workgroup of an instance reads the
// same n doubles and reduces them modulo its own q_i with f64_arith.hpp f64_to_residue. A coefficient outside the precondition raises
// the flag and enters as 0: no index depends on data, so nothing is read or written out of bounds whatever the doubles are.
template <int LOGN, int LOGE, int LAZY>
__global__ __launch_bounds__(1 << (LOGN - LOGE)) void k_rns_from_f64(FromF64Args a) {
    using G = Geom<LOGN, LOGE>;
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const int tid = threadIdx.x;
    const u32 i = blockIdx.x / a.count, c = blockIdx.x - i * a.count;
    const Mod m = a.mods[i].m;
    const double* tb = a.tables + size_t(i) * 4 * G::N;
    const double* src = a.coeffs + size_t(c) * G::N;
    hxf::RangeMask bad = 0;
    double v[G::E];
#pragma unroll
    for (int r = 0; r < G::E; ++r) {
        const double x = (src + G::idxA(r, 0))[u32(tid)];
        const bool ok = hxf::f64_int_in_range(__builtin_rint(x));
        bad |= __builtin_amdgcn_ballot_w64(!ok);
        v[r] = hxf::f64_to_residue(ok ? x : 0.0, m);
    }
    hxf::report_range(bad, a.flag);
    with_tier<LAZY, LOGN == 14>(a.tiermap, i, [&](auto T) {
        WgNttF64<LOGN, LOGE, decltype(T)::value, FromF64Opt>::template forward<true, true>(v, ldsd, tid, tb, tb + G::N, m);
    });
    u64* dst = a.out + (size_t(c) * a.n_limbs + i) * G::N;
    const u32 tB = u32(G::idxB(0, tid));
#pragma unroll
    for (int r = 0; r < G::E; ++r) (dst + G::idxB(r, 0))[tB] = hxf::from_f64(hxf::lift(v[r], m));
}

template <int LOGN, int LOGE, int LAZY>
static int run_from_f64(hexl_ks_plan* p, const FromF64Args& a) {
    using G = Geom<LOGN, LOGE>;
    if (int rc = hx_lds_optin<k_rns_from_f64<LOGN, LOGE, LAZY>>(p->ctx->device, G::LDS_USED)) return rc;
    hipLaunchKernelGGL((k_rns_from_f64<LOGN, LOGE, LAZY>), dim3(a.count * a.n_limbs), dim3(G::T), G::LDS_USED, p->ctx->stream, a);
    return (int)hipGetLastError();
}

static int launch_from_f64(hexl_ks_plan* p, u64* d_out, const double* d_coeffs, size_t count, u32 n_limbs) {
    const FromF64Args a{p->d_mods_f64, p->d_tables_f64, d_coeffs, d_out, p->d_flag, (u32)count, n_limbs, hx_tiermap(p)};
    return hx_with_f64_geom(p->logn, hx_level_tier(p, n_limbs), [&](auto N, auto E, auto Z) { return run_from_f64<N, E, Z>(p, a); });
}

// ---- coefficient-form limbs -> real coefficients ----
constexpr int GARNER_MAX = 16;                  // K <= 16 (hexl_ks_plan_create)
constexpr u32 CRT_THREADS = 256;
struct CrtArgs {
    const KsModF64* mods;       // [K]
    const double2* garner;      // [16][16]: (q_j^-1 mod q_i centred, fl(./q_i)) at [i][j], j < i
    const u64* in;              // [nb][n_limbs][n] canonical words, coefficients in natural order
    double* out;                // [nb][n]
    u32 logn, n_limbs;
};

// One coefficient per thread. Garner: x = d_0 + d_1 q_0 + d_2 q_0 q_1 + ..., 0 <= d_i < q_i, every step exact on integers held in
// doubles (f64_arith.hpp: the difference of two reduce outputs is inside mul_shoup's 1.5 q_i). The digits of (Q - 1) / 2 are
// (q_i - 1) / 2 for EVERY prefix of the chain (sum_i (q_i - 1)/2 . q_0 ... q_(i-1) telescopes), so the sign is a comparison from the top
// digit down with no table; a negative value is converted as Q - x (digitwise complement plus one), whose high digits vanish when |x|
// is small. Horner from the top digit in double-double (an fma-split product and a two-sum per step): exact while the value is below
// 2^53, and one rounding (2^-53 relative, far inside the 2^-50 asked for) plus terms of order 2^-100 otherwise, whatever n_limbs.
__global__ __launch_bounds__(CRT_THREADS) void k_crt_to_f64(CrtArgs a) {
    const size_t g = size_t(blockIdx.x) * CRT_THREADS + threadIdx.x;
    const size_t inst = g >> a.logn, j = g - (inst << a.logn);
    const u64* src = a.in + ((inst * a.n_limbs) << a.logn) + j;
    double d[GARNER_MAX];
    bool neg = false;
#pragma unroll
    for (int i = 0; i < GARNER_MAX; ++i) {
        if (i < (int)a.n_limbs) {
            const Mod m = a.mods[i].m;
            double t = hxf::reduce(hxf::to_f64(src[size_t(i) << a.logn]), m);
#pragma unroll
            for (int k = 0; k < i; ++k) {
                const double2 c = a.garner[i * GARNER_MAX + k];
                t = hxf::reduce(hxf::mul_shoup(t - hxf::reduce(d[k], m), c.x, c.y, m), m);
            }
            d[i] = hxf::lift(t, m);
            const double half = (m.p - 1.0) * 0.5;
            if (d[i] > half) neg = true;
            else if (d[i] < half) neg = false;
        }
    }
    double carry = neg ? 1.0 : 0.0;
#pragma unroll
    for (int i = 0; i < GARNER_MAX; ++i) {
        if (neg && i < (int)a.n_limbs) {
            const double p = a.mods[i].m.p;
            const double e = (p - 1.0 - d[i]) + carry;
            carry = e == p ? 1.0 : 0.0;
            d[i] = e == p ? 0.0 : e;
        }
    }
    double hi = 0.0, lo = 0.0;
#pragma unroll
    for (int i = GARNER_MAX - 1; i >= 0; --i) {
        if (i < (int)a.n_limbs) {
            const double p = a.mods[i].m.p;
            const double ph = hi * p, pl = __builtin_fma(hi, p, -ph);
            const double s = ph + d[i], bb = s - ph;
            const double se = (ph - (s - bb)) + (d[i] - bb);
            const double l = __builtin_fma(lo, p, pl + se);
            hi = s + l;
            lo = l - (hi - s);
        }
    }
    a.out[g] = neg ? -hi : hi;
}

// ---- plan-owned tables, computed on the host at first use ----
static int embed_tables(hexl_ks_plan* p) {
    if (p->d_emb_roots) return 0;
    const u32 n = p->n, nh = n / 2, logh = p->logn - 1;
    std::vector<double> roots(size_t(4) * n);
    const long double pi = acosl(-1.0L);
    for (u32 t = 0; t < 2 * n; ++t) {
        // the octant's angle, so that the long-double argument is at most pi / 4 and the symmetric entries agree bit for bit
        const u32 o = t % (n / 2) <= n / 4 ? t % (n / 2) : n / 2 - t % (n / 2);
        const long double c = cosl(pi * o / n), s = sinl(pi * o / n);
        const bool swap = t % (n / 2) > n / 4;
        long double re = swap ? s : c, im = swap ? c : s;      // angle within the quadrant
        switch (t / (n / 2)) {                                  // times i^quadrant
            case 1: { const long double r = re; re = -im; im = r; break; }
            case 2: re = -re; im = -im; break;
            case 3: { const long double r = re; re = im; im = -r; break; }
            default: break;
        }
        roots[2 * size_t(t)] = (double)re;
        roots[2 * size_t(t) + 1] = (double)im;
    }
    std::vector<u32> slot_of_s(nh), perm(nh);
    u64 pw = 1;
    for (u32 k = 0; k < nh; ++k) {
        slot_of_s[(pw - 1) / 4] = k;
        pw = pw * 5 % (2 * u64(n));
    }
    for (u32 q = 0; q < nh; ++q) perm[q] = slot_of_s[hxnt::bitrev(q, logh)];
    if (int rc = p->d_emb_perm.upload_once(perm.data(), perm.size())) return rc;
    return p->d_emb_roots.upload_once(roots.data(), roots.size());     // (the roots last: they are what says "both are there")
}

// Garner's constants q_j^-1 mod q_i for j < i < K: those of a prefix of the chain are a prefix of these, so one table serves every level
static int garner_table(hexl_ks_plan* p) {
    if (p->d_garner) return 0;
    std::vector<double> g(size_t(GARNER_MAX) * GARNER_MAX * 2, 0.0);
    for (u32 i = 0; i < p->K; ++i)
        for (u32 j = 0; j < i; ++j) {
            const u64 q = p->moduli[i];
            const double c = hx_centre(hxnt::invmod(p->moduli[j] % q, q), q);
            g[(size_t(i) * GARNER_MAX + j) * 2] = c;
            g[(size_t(i) * GARNER_MAX + j) * 2 + 1] = c / (double)q;
        }
    return p->d_garner.upload_once(g.data(), g.size());
}

// ---- launchers ----
static u32 emb_logb(const hexl_ks_plan* p) { return p->logn - 1 < EMB_MAX_LOGB ? p->logn - 1 : EMB_MAX_LOGB; }
static u32 emb_threads(u32 logb) { return (1u << logb) / 8 < 64 ? 64 : (1u << logb) / 8; }

static int launch_embed(hexl_ks_plan* p, EmbArgs a, size_t nb, bool inverse) {
    const u32 logh = p->logn - 1;
    a.logn = p->logn;
    a.logb = emb_logb(p);
    const size_t lds = (size_t(16) << a.logb);
    if (int rc = hx_lds_optin<k_embed_fwd, k_embed_inv>(p->ctx->device, size_t(16) << EMB_MAX_LOGB)) return rc;
    const dim3 grid((u32)(nb << (logh - a.logb))), block(emb_threads(a.logb));
    const dim3 top_grid((u32)((nb << (p->logn - 2)) / EMB_TOP_THREADS)), top_block(EMB_TOP_THREADS);
    hipStream_t st = p->ctx->stream;
    if (inverse) {
        hipLaunchKernelGGL(k_embed_inv, grid, block, lds, st, a);
        if (a.logb != logh) hipLaunchKernelGGL(k_embed_inv_top, top_grid, top_block, 0, st, a);
    } else {
        if (a.logb != logh) hipLaunchKernelGGL(k_embed_fwd_top, top_grid, top_block, 0, st, a);
        hipLaunchKernelGGL(k_embed_fwd, grid, block, lds, st, a);
    }
    return (int)hipGetLastError();
}

int hx_launch_encode(hexl_ks_plan* p, u64* d_out, const double* d_coeffs, const double* d_slots, size_t count, u32 n_limbs, double scale) {
    if (!count) return 0;
    const size_t n = p->n;
    if (!d_slots) return launch_from_f64(p, d_out, d_coeffs, count, n_limbs);
    if (int rc = embed_tables(p)) return rc;
    const size_t chunk = hx_enc_chunk_of(p, count);
    if (int rc = p->d_enc_coeffs.reserve(chunk * n)) return rc;
    EmbArgs a{};
    a.roots = reinterpret_cast<const double2*>(p->d_emb_roots.get());
    a.perm = p->d_emb_perm;
    a.coeffs = p->d_enc_coeffs;
    a.factor = scale / (double)(n / 2);
    return hx_for_chunks(count, chunk, [&](size_t c0, size_t nb) {
        a.slots_in = d_slots + c0 * n;
        if (int rc = launch_embed(p, a, nb, true)) return rc;
        return launch_from_f64(p, d_out + c0 * n_limbs * n, p->d_enc_coeffs, nb, n_limbs);
    });
}

int hx_launch_decode(hexl_ks_plan* p, double* d_coeffs, double* d_slots, const u64* d_in, size_t count, u32 n_limbs, double scale) {
    if (int rc = garner_table(p)) return rc;
    if (!count) return 0;
    const size_t n = p->n;
    if (d_slots)
        if (int rc = embed_tables(p)) return rc;
    const size_t chunk = hx_enc_chunk_of(p, count);
    if (int rc = p->d_enc_words.reserve(chunk * n_limbs * n)) return rc;
    if (d_slots)
        if (int rc = p->d_enc_coeffs.reserve(chunk * n)) return rc;
    CrtArgs ca{p->d_mods_f64, reinterpret_cast<const double2*>(p->d_garner.get()), p->d_enc_words, nullptr, p->logn, n_limbs};
    EmbArgs a{};
    if (d_slots) {
        a.roots = reinterpret_cast<const double2*>(p->d_emb_roots.get());
        a.perm = p->d_emb_perm;
        a.coeffs = p->d_enc_coeffs;
        a.factor = 1.0 / scale;
    }
    return hx_for_chunks(count, chunk, [&](size_t c0, size_t nb) {
        if (int rc = hx_launch_rns_ntt(p, p->d_enc_words, d_in + c0 * n_limbs * n, nb, n_limbs, true)) return rc;
        ca.out = d_slots ? p->d_enc_coeffs.get() : d_coeffs + c0 * n;
        hipLaunchKernelGGL(k_crt_to_f64, dim3((u32)(nb * n / CRT_THREADS)), dim3(CRT_THREADS), 0, p->ctx->stream, ca);
        if (int rc = (int)hipGetLastError()) return rc;
        if (!d_slots) return 0;
        a.slots_out = d_slots + c0 * n;
        return launch_embed(p, a, nb, false);
    });
}

// ---- entry points of include/hexl_mi355x.h ----
// the checks of hexl_internal.hpp for 1 <= n_limbs <= K, and the [count][n_limbs][n] words apart from the [count][n] doubles
// (coefficients, or n/2 complex slots)
static bool enc_args_ok(const hexl_ks_plan* p, const void* d_words, const void* d_reals, size_t count, u64 n_limbs) {
    if (!d_words || !d_reals || !p || !hx_f64_plan_ok(p, n_limbs, 1, p->K)) return false;
    size_t bytes;
    if (!hx_words_bytes(count, 1, n_limbs, p->n, &bytes) || !hx_wg_grid_ok(count, n_limbs)) return false;
    return !hx_ranges_overlap(d_words, bytes, d_reals, bytes / n_limbs);
}
static bool scale_ok(double scale) { return scale > 0.0 && scale < INFINITY; }

extern "C" int hexl_rns_from_f64(hexl_ks_plan* p, uint64_t* d_out, const double* d_coeffs, size_t count, uint64_t n_limbs) {
    if (!enc_args_ok(p, d_out, d_coeffs, count, n_limbs)) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    return hx_launch_encode(p, d_out, d_coeffs, nullptr, count, (u32)n_limbs, 1.0);
}

extern "C" int hexl_rns_to_f64(hexl_ks_plan* p, double* d_coeffs, const uint64_t* d_in, size_t count, uint64_t n_limbs) {
    if (!enc_args_ok(p, d_in, d_coeffs, count, n_limbs)) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    return hx_launch_decode(p, d_coeffs, nullptr, d_in, count, (u32)n_limbs, 1.0);
}

extern "C" int hexl_ckks_encode(hexl_ks_plan* p, uint64_t* d_out, const double* d_slots, size_t count, uint64_t n_limbs, double scale) {
    if (!enc_args_ok(p, d_out, d_slots, count, n_limbs) || !scale_ok(scale)) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    return hx_launch_encode(p, d_out, nullptr, d_slots, count, (u32)n_limbs, scale);
}

extern "C" int hexl_ckks_decode(hexl_ks_plan* p, double* d_slots, const uint64_t* d_in, size_t count, uint64_t n_limbs, double scale) {
    if (!enc_args_ok(p, d_in, d_slots, count, n_limbs) || !scale_ok(scale)) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    return hx_launch_decode(p, nullptr, d_slots, d_in, count, (u32)n_limbs, scale);
}
