// rns_ops.hip -- what a caller with device-resident ciphertexts needs beside the level operations of ckks_ops.hip (DESIGN.md 4.6.1 "RNS
// transforms and plaintext multiply"):
//   rns_ntt_fwd / rns_ntt_inv   [count][n_limbs][n] to and from NTT form in ONE launch, polynomial (c, i) modulo the plan's q_i on the
//                               plan's own tables and that limb's arithmetic tier: the per-limb transform of the rescale
//                               (ckks_ops.hip k_rs_intt / k_rs_down) without its epilogues                          k_rns_fwd / k_rns_inv
//   multiply_plain              out[b][k][i] (+)= ct[b][k][i] * pt[b or 0][i] mod q_i, word by word in NTT form     k_pt_mul
//   ct_lincomb                  out[b][k][i] = sum_t w[t][i] ct_t[b][k][i] + [k == 0] (pt[b or 0][i] + const[i]) mod q_i: up to eight
//                               ciphertexts, each read once through its first n_limbs limbs     k_ct_lincomb
// FP64 plans only (moduli < 2^52). Nothing here keeps device memory in the plan or reads its keys.
#include "hexl_internal.hpp"
#include "ntt_core_f64.hpp"

using namespace hx;

struct RnsNttArgs {
    const KsModF64* mods;       // [K]
    const double* tables;       // [K][4][n] (keyswitch_f64.hip KsArgsF)
    const u64* in;              // [count][n_limbs][n]
    u64* out;                   // [count][n_limbs][n]; may be `in` (a workgroup holds its whole polynomial before it stores)
    u32 count, n_limbs;
    unsigned long long tiermap; // LAZY = -1: nibble i = reduction period of limb i (keyswitch_f64.hip)
};
// the forward transform of centred residues: the X schedule whose tail FINAL's range reduction finishes
struct RnsFwdOpt : NttOpt { static constexpr int XSD = 0; };

// One transform per workgroup, LIMB-major: workgroup w works on limb w / count of instance w % count, so the workgroups resident at
// any time share one limb's table (128 KiB at N = 16384) in every XCD's L2, where an instance-major
// order would keep all n_limbs of them in flight. Mixed tiers (LAZY = -1) pick among all four schedules at N = 16384: unlike
// k_rs_down there is no second operand to hold across the transform, and the cost is 12 bytes of scratch per lane in the inverse.
template <int LOGN, int LOGE, int LAZY>
__global__ __launch_bounds__(1 << (LOGN - LOGE)) void k_rns_fwd(RnsNttArgs a) {
    using G = Geom<LOGN, LOGE>;
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const int tid = threadIdx.x;
    const u32 i = blockIdx.x / a.count, c = blockIdx.x - i * a.count;
    const Mod m = a.mods[i].m;
    const double* tb = a.tables + size_t(i) * 4 * G::N;
    const size_t poly = (size_t(c) * a.n_limbs + i) * G::N;
    const u64* src = a.in + poly;
    double v[G::E];
#pragma unroll
    for (int r = 0; r < G::E; ++r) v[r] = hxf::reduce(hxf::to_f64((src + G::idxA(r, 0))[u32(tid)]), m);
    // one transform per workgroup: FRESH; FINAL: |v| <= p/2 + 2. Lazy tiers run the X schedule for centred inputs (f64_arith.hpp), as the
    // standalone forward kernel does
    with_tier<LAZY, LOGN == 14>(a.tiermap, i, [&](auto T) {
        WgNttF64<LOGN, LOGE, decltype(T)::value, RnsFwdOpt>::template forward<true, true>(v, ldsd, tid, tb, tb + G::N, m);
    });
    u64* dst = a.out + poly;
    const u32 tB = u32(G::idxB(0, tid));
#pragma unroll
    for (int r = 0; r < G::E; ++r) (dst + G::idxB(r, 0))[tB] = hxf::from_f64(hxf::lift(v[r], m));
}

template <int LOGN, int LOGE, int LAZY>
__global__ __launch_bounds__(1 << (LOGN - LOGE)) void k_rns_inv(RnsNttArgs a) {
    using G = Geom<LOGN, LOGE>;
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const int tid = threadIdx.x;
    const u32 i = blockIdx.x / a.count, c = blockIdx.x - i * a.count;
    const KsModF64 md = a.mods[i];
    const Mod m = md.m;
    const double* tb = a.tables + size_t(i) * 4 * G::N;
    const size_t poly = (size_t(c) * a.n_limbs + i) * G::N;
    const u64* src = a.in + poly;
    const u32 tB = u32(G::idxB(0, tid));
    double v[G::E];
#pragma unroll
    for (int r = 0; r < G::E; ++r) v[r] = hxf::reduce(hxf::to_f64((src + G::idxB(r, 0))[tB]), m);
    // without the w/p table and, in the lazy tiers, on the I schedule: the standalone inverse kernel's transform (ntt.hip)
    with_tier<LAZY, LOGN == 14>(a.tiermap, i, [&](auto T) {
        WgNttF64<LOGN, LOGE, decltype(T)::value, InvNoWpOpt<true>>::template inverse<true>(
            v, ldsd, tid, tb + 2 * G::N, tb + 3 * G::N, m, md.sc);
    });
    u64* dst = a.out + poly;
#pragma unroll
    for (int r = 0; r < G::E; ++r) (dst + G::idxA(r, 0))[u32(tid)] = hxf::from_f64(hxf::lift(v[r], m));
}

template <int LOGN, int LOGE, int LAZY>
static int run_rns_ntt(hexl_ks_plan* p, const RnsNttArgs& a, bool inverse) {
    using G = Geom<LOGN, LOGE>;
    if (int rc = hx_lds_optin<k_rns_fwd<LOGN, LOGE, LAZY>, k_rns_inv<LOGN, LOGE, LAZY>>(p->ctx->device, G::LDS_USED)) return rc;
    const dim3 grid(a.count * a.n_limbs), block(G::T);
    if (inverse) hipLaunchKernelGGL((k_rns_inv<LOGN, LOGE, LAZY>), grid, block, G::LDS_USED, p->ctx->stream, a);
    else hipLaunchKernelGGL((k_rns_fwd<LOGN, LOGE, LAZY>), grid, block, G::LDS_USED, p->ctx->stream, a);
    return (int)hipGetLastError();
}

int hx_launch_rns_ntt(hexl_ks_plan* p, u64* d_out, const u64* d_in, size_t count, u32 n_limbs, bool inverse) {
    if (!count) return 0;
    const RnsNttArgs a{p->d_mods_f64, p->d_tables_f64, d_in, d_out, (u32)count, n_limbs, hx_tiermap(p)};
    return hx_with_f64_geom(p->logn, hx_level_tier(p, n_limbs), [&](auto N, auto E, auto Z) { return run_rns_ntt<N, E, Z>(p, a, inverse); });
}

// ---- plaintext multiply ----
constexpr u32 PT_THREADS = 256, PT_VECS = 2;
constexpr u32 PT_LOG_CHUNK = 10;    // 1024 words of one polynomial per workgroup (the smallest ring): PT_VECS 16-byte vectors per lane
static_assert(PT_THREADS * PT_VECS * 2 == 1u << PT_LOG_CHUNK, "a workgroup covers its chunk exactly");
static_assert(PT_THREADS == HX_WW_THREADS && PT_LOG_CHUNK == HX_WW_LOG_CHUNK, "hx_ww_grid counts these workgroups");

struct PtMulArgs {
    const KsModF64* mods;       // [K]
    const u64* ct;              // [batch][NCOMP][L][n]
    const u64* pt;              // [pt_stride ? batch : 1][L][n]
    u64* out;                   // [batch][NCOMP][L][n]; may be `ct` when ACC = false (a lane reads the words it writes, nobody else's)
    u32 logn, L;
    u32 pt_stride;              // 1: one plaintext per instance, 0: one for all
};

// One workgroup per (instance, limb, chunk of the polynomial): the limb -- and with it the modulus -- is found once per workgroup, and the
// plaintext words are loaded once and meet every component of the instance. Every load of a lane is requested before its first product.
template <int NCOMP, bool ACC>
__global__ __launch_bounds__(PT_THREADS) void k_pt_mul(PtMulArgs a) {
    typedef unsigned long long u2 __attribute__((ext_vector_type(2)));
    const u32 bi = blockIdx.x >> (a.logn - PT_LOG_CHUNK), ch = blockIdx.x - (bi << (a.logn - PT_LOG_CHUNK));
    const u32 b = bi / a.L, i = bi - b * a.L;
    const Mod m = a.mods[i].m;
    const size_t n = size_t(1) << a.logn, within = size_t(i) * n + (size_t(ch) << PT_LOG_CHUNK);
    const u2* pt = reinterpret_cast<const u2*>(a.pt + size_t(b) * a.pt_stride * a.L * n + within);
    u2 t[PT_VECS], c[NCOMP][PT_VECS], prev[ACC ? NCOMP : 1][PT_VECS];
#pragma unroll
    for (u32 j = 0; j < PT_VECS; ++j) t[j] = pt[threadIdx.x + j * PT_THREADS];
#pragma unroll
    for (int k = 0; k < NCOMP; ++k) {
        const size_t poly = (size_t(b) * NCOMP + k) * a.L * n + within;
#pragma unroll
        for (u32 j = 0; j < PT_VECS; ++j) {
            c[k][j] = reinterpret_cast<const u2*>(a.ct + poly)[threadIdx.x + j * PT_THREADS];
            if constexpr (ACC) prev[k][j] = reinterpret_cast<const u2*>(a.out + poly)[threadIdx.x + j * PT_THREADS];
        }
    }
#pragma unroll
    for (int k = 0; k < NCOMP; ++k) {
        const size_t poly = (size_t(b) * NCOMP + k) * a.L * n + within;
#pragma unroll
        for (u32 j = 0; j < PT_VECS; ++j) {
            u2 o;
            if constexpr (ACC) {
                o.x = hxf::from_f64(hxf::pt_mul_acc(hxf::to_f64(c[k][j].x), hxf::to_f64(t[j].x), hxf::to_f64(prev[k][j].x), m));
                o.y = hxf::from_f64(hxf::pt_mul_acc(hxf::to_f64(c[k][j].y), hxf::to_f64(t[j].y), hxf::to_f64(prev[k][j].y), m));
            } else {
                o.x = hxf::from_f64(hxf::pt_mul(hxf::to_f64(c[k][j].x), hxf::to_f64(t[j].x), m));
                o.y = hxf::from_f64(hxf::pt_mul(hxf::to_f64(c[k][j].y), hxf::to_f64(t[j].y), m));
            }
            reinterpret_cast<u2*>(a.out + poly)[threadIdx.x + j * PT_THREADS] = o;
        }
    }
}

int hx_launch_multiply_plain(hexl_ks_plan* p, u64* d_out, const u64* d_ct, const u64* d_pt, size_t batch, u32 n_components, u32 n_limbs,
                             bool per_instance, bool accumulate) {
    if (!batch) return 0;
    const PtMulArgs a{p->d_mods_f64, d_ct, d_pt, d_out, p->logn, n_limbs, per_instance ? 1u : 0u};
    const dim3 grid((u32)hx_ww_grid(p, batch, n_limbs)), block(PT_THREADS);
    auto launch = [&](auto NC) {
        constexpr int NCOMP = decltype(NC)::value;
        if (accumulate) hipLaunchKernelGGL((k_pt_mul<NCOMP, true>), grid, block, 0, p->ctx->stream, a);
        else hipLaunchKernelGGL((k_pt_mul<NCOMP, false>), grid, block, 0, p->ctx->stream, a);
    };
    if (n_components == 1) launch(hx_int<1>{});
    else if (n_components == 2) launch(hx_int<2>{});
    else launch(hx_int<3>{});
    return (int)hipGetLastError();
}

// ---- ciphertext linear combination ----
constexpr u32 LC_MAX_TERMS = 8, LC_MAX_LIMBS = 16;               // hexl_ks_plan::tier has 16 limbs
struct LcWeight { double w, wp; };                                // one term's weight modulo one q_i: centred, and fl(w / q_i) (hxf::lc_term)

// Everything a launch needs travels BY VALUE in the kernel arguments (2.3 KiB of the 4 KiB there are): nothing is uploaded, so there is
// no copy to order in front of the kernel and no device or pinned memory to keep alive behind an asynchronous call.
struct LcArgs {
    const KsModF64* mods;       // [K]
    const u64* ct[LC_MAX_TERMS];    // term t: [batch][NCOMP][in_limbs[t]][n], read through its first L limbs
    const u64* pt;              // nullptr, or [pt_stride ? batch : 1][L][n]: component 0 only
    u64* out;                   // [batch][NCOMP][L][n]; may be ct[t] where in_limbs[t] == L (a lane reads the words it writes, nobody else's)
    u32 in_limbs[LC_MAX_TERMS];
    LcWeight wt[LC_MAX_LIMBS][LC_MAX_TERMS];    // limb-major: a workgroup's NT weights are one contiguous run of scalar loads
    double cst[LC_MAX_LIMBS];   // the constant addend of component 0 modulo q_i, centred (0 when there is none)
    u32 logn, L;
    u32 pt_stride;              // 1: one plaintext per instance, 0: one for all
    u32 has_cst;
};
static_assert(sizeof(LcArgs) <= 4096, "the kernel arguments of k_ct_lincomb must fit the 4 KiB kernarg segment");

// One workgroup per (instance, limb, chunk of the polynomial), as k_pt_mul: the modulus and the NT weights of the limb are found once per
// workgroup (wave-uniform: scalar registers). The component loop runs inside, so the plaintext words and the constant meet component 0
// only. Every load of a component -- NT x PT_VECS 16-byte vectors per lane, 64 VGPRs at NT = 8 -- is requested before its first product;
// when all components together are no more than that (NT * NCOMP <= 8) all of them are, as d_out may be a term and a component's loads
// cannot move above the previous component's stores otherwise. A weight of exactly 1 (wave-uniform test) adds the word as it is.
template <int NT, int NCOMP>
__global__ __launch_bounds__(PT_THREADS) void k_ct_lincomb(LcArgs a) {
    typedef unsigned long long u2 __attribute__((ext_vector_type(2)));
    constexpr bool ALL = NT * NCOMP <= 8;
    const u32 bi = blockIdx.x >> (a.logn - PT_LOG_CHUNK), ch = blockIdx.x - (bi << (a.logn - PT_LOG_CHUNK));
    const u32 b = bi / a.L, i = bi - b * a.L;
    const Mod m = a.mods[i].m;
    const size_t n = size_t(1) << a.logn, chunk = size_t(ch) << PT_LOG_CHUNK;
    const bool has_pt = a.pt != nullptr;
    u2 p[PT_VECS], c[ALL ? NCOMP : 1][NT][PT_VECS];
    if (has_pt) {
        const u2* pt = reinterpret_cast<const u2*>(a.pt + (size_t(b) * a.pt_stride * a.L + i) * n + chunk);
#pragma unroll
        for (u32 j = 0; j < PT_VECS; ++j) p[j] = pt[threadIdx.x + j * PT_THREADS];
    }
    auto load = [&](int k, int slot) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const u2* src = reinterpret_cast<const u2*>(a.ct[t] + ((size_t(b) * NCOMP + k) * a.in_limbs[t] + i) * n + chunk);
#pragma unroll
            for (u32 j = 0; j < PT_VECS; ++j) c[slot][t][j] = src[threadIdx.x + j * PT_THREADS];
        }
    };
    if constexpr (ALL) {
#pragma unroll
        for (int k = 0; k < NCOMP; ++k) load(k, k);
    }
#pragma unroll
    for (int k = 0; k < NCOMP; ++k) {
        if constexpr (!ALL) load(k, 0);
        double acc[PT_VECS][2];
#pragma unroll
        for (u32 j = 0; j < PT_VECS; ++j) acc[j][0] = acc[j][1] = 0.0;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const LcWeight wt = a.wt[i][t];
            const bool one = wt.w == 1.0;                        // the same in every lane: a scalar branch, not a select
#pragma unroll
            for (u32 j = 0; j < PT_VECS; ++j) {
                const u2 v = c[ALL ? k : 0][t][j];
                double x = hxf::to_f64(v.x), y = hxf::to_f64(v.y);
                if (!one) {
                    x = hxf::lc_term(x, wt.w, wt.wp, m);
                    y = hxf::lc_term(y, wt.w, wt.wp, m);
                }
                acc[j][0] = hxf::lc_add(acc[j][0], x, m);
                acc[j][1] = hxf::lc_add(acc[j][1], y, m);
            }
        }
        if (k == 0) {
            if (has_pt) {
#pragma unroll
                for (u32 j = 0; j < PT_VECS; ++j) {
                    acc[j][0] = hxf::lc_add(acc[j][0], hxf::to_f64(p[j].x), m);
                    acc[j][1] = hxf::lc_add(acc[j][1], hxf::to_f64(p[j].y), m);
                }
            }
            if (a.has_cst) {
                const double cst = a.cst[i];
#pragma unroll
                for (u32 j = 0; j < PT_VECS; ++j) {
                    acc[j][0] = hxf::lc_add(acc[j][0], cst, m);
                    acc[j][1] = hxf::lc_add(acc[j][1], cst, m);
                }
            }
        }
        u2* dst = reinterpret_cast<u2*>(a.out + ((size_t(b) * NCOMP + k) * a.L + i) * n + chunk);
#pragma unroll
        for (u32 j = 0; j < PT_VECS; ++j) {
            u2 o;
            o.x = hxf::from_f64(hxf::lc_finish(acc[j][0], m));
            o.y = hxf::from_f64(hxf::lc_finish(acc[j][1], m));
            dst[threadIdx.x + j * PT_THREADS] = o;
        }
    }
}

static int hx_launch_ct_lincomb(hexl_ks_plan* p, const LcArgs& a, size_t batch, u32 n_terms, u32 n_components) {
    if (!batch) return 0;
    const dim3 grid((u32)hx_ww_grid(p, batch, a.L)), block(PT_THREADS);
    auto comps = [&](auto NT) {
        constexpr int T = decltype(NT)::value;
        if (n_components == 1) hipLaunchKernelGGL((k_ct_lincomb<T, 1>), grid, block, 0, p->ctx->stream, a);
        else if (n_components == 2) hipLaunchKernelGGL((k_ct_lincomb<T, 2>), grid, block, 0, p->ctx->stream, a);
        else hipLaunchKernelGGL((k_ct_lincomb<T, 3>), grid, block, 0, p->ctx->stream, a);
    };
    switch (n_terms) {
        case 1: comps(hx_int<1>{}); break;
        case 2: comps(hx_int<2>{}); break;
        case 3: comps(hx_int<3>{}); break;
        case 4: comps(hx_int<4>{}); break;
        case 5: comps(hx_int<5>{}); break;
        case 6: comps(hx_int<6>{}); break;
        case 7: comps(hx_int<7>{}); break;
        default: comps(hx_int<8>{}); break;
    }
    return (int)hipGetLastError();
}

// ---- entry points of include/hexl_mi355x.h (beside their launchers, as in ckks_ops.hip: the CPU staging model needs no stubs for them) ----
// The checks are hexl_internal.hpp's; every limb count here may reach K (the special prime included).
static int rns_ntt(hexl_ks_plan* p, uint64_t* d_out, const uint64_t* d_in, size_t count, uint64_t n_limbs, bool inverse) {
    if (!p || !d_out || !d_in || !hx_f64_plan_ok(p, n_limbs, 1, p->K)) return HEXL_E_BADARG;
    size_t bytes;
    if (!hx_words_bytes(count, 1, n_limbs, p->n, &bytes) || !hx_wg_grid_ok(count, n_limbs)) return HEXL_E_BADARG;
    if (d_out != d_in && hx_ranges_overlap(d_out, bytes, d_in, bytes)) return HEXL_E_BADARG;   // in place, or apart
    HX_CHECK(hipSetDevice(p->ctx->device));
    return hx_launch_rns_ntt(p, d_out, d_in, count, (u32)n_limbs, inverse);
}

extern "C" int hexl_rns_ntt_fwd(hexl_ks_plan* p, uint64_t* d_out, const uint64_t* d_in, size_t count, uint64_t n_limbs) {
    return rns_ntt(p, d_out, d_in, count, n_limbs, false);
}

extern "C" int hexl_rns_ntt_inv(hexl_ks_plan* p, uint64_t* d_out, const uint64_t* d_in, size_t count, uint64_t n_limbs) {
    return rns_ntt(p, d_out, d_in, count, n_limbs, true);
}

extern "C" int hexl_multiply_plain(hexl_ks_plan* p, uint64_t* d_out, const uint64_t* d_ct, const uint64_t* d_pt, size_t batch,
                                   uint64_t n_components, uint64_t n_limbs, size_t pt_batch, int accumulate) {
    if (!p || !d_out || !d_ct || !d_pt || !hx_f64_plan_ok(p, n_limbs, 1, p->K) || !hx_in_range(n_components, 1, 3)) return HEXL_E_BADARG;
    size_t bytes;
    HxPtBatch pt;
    if (!hx_pt_batch(pt_batch, batch, size_t(n_limbs) * p->n * sizeof(u64), &pt)) return HEXL_E_BADARG;
    if (!hx_words_bytes(batch, n_components, n_limbs, p->n, &bytes) || !hx_ww_grid_ok(p, batch, n_limbs)) return HEXL_E_BADARG;
    if (hx_ranges_overlap(d_out, bytes, d_pt, pt.bytes)) return HEXL_E_BADARG;
    // in place over the ciphertext only when the output is written, not accumulated into (d_out would be both addend and factor)
    if ((d_out != d_ct || accumulate) && hx_ranges_overlap(d_out, bytes, d_ct, bytes)) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    return hx_launch_multiply_plain(p, d_out, d_ct, d_pt, batch, (u32)n_components, (u32)n_limbs, pt.stride != 0, accumulate != 0);
}

extern "C" int hexl_ct_lincomb(hexl_ks_plan* p, uint64_t* d_out, const uint64_t* const* d_cts, const uint64_t* in_limbs,
                               const uint64_t* h_weights, size_t n_terms, const uint64_t* d_pt, size_t pt_batch, const uint64_t* h_const,
                               size_t batch, uint64_t n_components, uint64_t n_limbs) {
    if (!p || !d_out || !d_cts || !hx_in_range(n_terms, 1, LC_MAX_TERMS) || !hx_f64_plan_ok(p, n_limbs, 1, p->K) || n_limbs > LC_MAX_LIMBS)
        return HEXL_E_BADARG;
    if (!hx_in_range(n_components, 1, 3)) return HEXL_E_BADARG;
    const size_t poly = size_t(p->n) * sizeof(u64);
    HxPtBatch pt;
    if (d_pt && !hx_pt_batch(pt_batch, batch, size_t(n_limbs) * poly, &pt)) return HEXL_E_BADARG;
    // the largest term has K limbs: if that size fits, every other one does
    size_t bytes;
    if (!hx_words_bytes(batch, n_components, p->K, p->n, &bytes) || !hx_ww_grid_ok(p, batch, n_limbs)) return HEXL_E_BADARG;
    bytes = bytes / p->K * n_limbs;
    LcArgs a{};
    for (size_t t = 0; t < n_terms; ++t) {
        const u64 lt = in_limbs ? in_limbs[t] : n_limbs;
        if (!d_cts[t] || lt < n_limbs || lt > p->K) return HEXL_E_BADARG;
        // in place over a term of the output's own layout, or apart
        if ((d_out != d_cts[t] || lt != n_limbs) && hx_ranges_overlap(d_out, bytes, d_cts[t], batch * n_components * size_t(lt) * poly))
            return HEXL_E_BADARG;
        a.ct[t] = d_cts[t];
        a.in_limbs[t] = (u32)lt;
    }
    if (d_pt && hx_ranges_overlap(d_out, bytes, d_pt, pt.bytes)) return HEXL_E_BADARG;
    for (u64 i = 0; i < n_limbs; ++i) {
        const u64 q = p->moduli[i];
        for (size_t t = 0; t < n_terms; ++t) {
            const u64 w = h_weights ? h_weights[t * n_limbs + i] : 1;
            if (w >= q) return HEXL_E_BADARG;
            const double wc = hx_centre(w, q);
            a.wt[i][t] = LcWeight{wc, wc / (double)q};
        }
        if (h_const) {
            if (h_const[i] >= q) return HEXL_E_BADARG;
            a.cst[i] = hx_centre(h_const[i], q);
        }
    }
    a.mods = p->d_mods_f64;
    a.pt = d_pt;
    a.out = d_out;
    a.logn = p->logn;
    a.L = (u32)n_limbs;
    a.pt_stride = pt.stride;
    a.has_cst = h_const ? 1u : 0u;
    HX_CHECK(hipSetDevice(p->ctx->device));
    return hx_launch_ct_lincomb(p, a, batch, (u32)n_terms, (u32)n_components);
}
