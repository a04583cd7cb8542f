// rns_ops.hip -- what a caller with device-resident ciphertexts needs beside the level operations of ckks_ops.hip (DESIGN.md 4.6.1 "RNS
// transforms and plaintext multiply"):
//   rns_ntt_fwd / rns_ntt_inv   [count][n_limbs][n] to and from NTT form in ONE launch, polynomial (c, i) modulo the plan's q_i on the
//                               plan's own tables and that limb's arithmetic tier: the per-limb transform of the rescale
//                               (ckks_ops.hip k_rs_intt / k_rs_down) without its epilogues                          k_rns_fwd / k_rns_inv
//   multiply_plain              out[b][k][i] (+)= ct[b][k][i] * pt[b or 0][i] mod q_i, word by word in NTT form     k_pt_mul
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
    // the schedule every limb in use admits; LAZY = -1 (per-limb lookup) when they differ, as hx_launch_rescale chooses
    int lazy = p->tier[0];
    for (u32 i = 1; i < n_limbs; ++i)
        if (p->tier[i] != p->tier[0]) lazy = -1;
    const RnsNttArgs a{p->d_mods_f64, p->d_tables_f64, d_in, d_out, (u32)count, n_limbs, hx_tiermap(p)};
    return hx_with_f64_geom(p->logn, lazy, [&](auto N, auto E, auto Z) { return run_rns_ntt<N, E, Z>(p, a, inverse); });
}

// ---- plaintext multiply ----
constexpr u32 PT_THREADS = 256, PT_VECS = 2;
constexpr u32 PT_LOG_CHUNK = 10;    // 1024 words of one polynomial per workgroup (the smallest ring): PT_VECS 16-byte vectors per lane
static_assert(PT_THREADS * PT_VECS * 2 == 1u << PT_LOG_CHUNK, "a workgroup covers its chunk exactly");

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

// workgroups of one hexl_multiply_plain launch
static size_t pt_mul_grid(const hexl_ks_plan* p, size_t batch, u64 n_limbs) { return batch * n_limbs * (p->n >> PT_LOG_CHUNK); }

int hx_launch_multiply_plain(hexl_ks_plan* p, u64* d_out, const u64* d_ct, const u64* d_pt, size_t batch, u32 n_components, u32 n_limbs,
                             bool per_instance, bool accumulate) {
    if (!batch) return 0;
    const PtMulArgs a{p->d_mods_f64, d_ct, d_pt, d_out, p->logn, n_limbs, per_instance ? 1u : 0u};
    const dim3 grid((u32)pt_mul_grid(p, batch, n_limbs)), block(PT_THREADS);
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

// ---- entry points of include/hexl_mi355x.h (beside their launchers, as in ckks_ops.hip: the CPU staging model needs no stubs for them) ----
// FP64 plan of a ring dimension the transforms are built for, 1 <= n_limbs <= K (the special prime included)
static bool rns_plan_ok(const hexl_ks_plan* p, u64 n_limbs) {
    return p && p->use_f64 && p->logn >= 10 && p->logn <= 15 && n_limbs >= 1 && n_limbs <= p->K;
}
constexpr size_t RNS_MAX_GRID = 0x7fffffffu;     // workgroups of one launch (x dimension)

static int rns_ntt(hexl_ks_plan* p, uint64_t* d_out, const uint64_t* d_in, size_t count, uint64_t n_limbs, bool inverse) {
    if (!d_out || !d_in || !rns_plan_ok(p, n_limbs)) return HEXL_E_BADARG;
    const size_t per = size_t(n_limbs) * p->n * sizeof(u64);
    if (count > SIZE_MAX / per || count > RNS_MAX_GRID / n_limbs) return HEXL_E_BADARG;
    if (d_out != d_in && hx_ranges_overlap(d_out, count * per, d_in, count * per)) return HEXL_E_BADARG;   // in place, or apart
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
    if (!d_out || !d_ct || !d_pt || !rns_plan_ok(p, n_limbs)) return HEXL_E_BADARG;
    if (n_components < 1 || n_components > 3) return HEXL_E_BADARG;
    if (pt_batch != 1 && pt_batch != batch) return HEXL_E_BADARG;
    const size_t pt_per = size_t(n_limbs) * p->n * sizeof(u64), per = pt_per * n_components;
    if (batch > SIZE_MAX / per || batch > RNS_MAX_GRID / (n_limbs * (p->n >> PT_LOG_CHUNK))) return HEXL_E_BADARG;
    const size_t bytes = batch * per, pt_bytes = (batch ? pt_batch : 0) * pt_per;
    if (hx_ranges_overlap(d_out, bytes, d_pt, pt_bytes)) return HEXL_E_BADARG;
    // in place over the ciphertext only when the output is written, not accumulated into (d_out would be both addend and factor)
    if ((d_out != d_ct || accumulate) && hx_ranges_overlap(d_out, bytes, d_ct, bytes)) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    return hx_launch_multiply_plain(p, d_out, d_ct, d_pt, batch, (u32)n_components, (u32)n_limbs, pt_batch == batch,
                                    accumulate != 0);
}
