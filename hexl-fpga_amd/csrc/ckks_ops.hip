// ckks_ops.hip -- the two steps of a CKKS level beside multiply + relinearize, on the device (DESIGN.md "CKKS level operations"):
//   rescale   divide by the last prime of the level and drop it (SEAL's rescale_to_next, rounding to nearest) -- the mod-down of the
//             keyswitch (keyswitch_f64.hip k_ksf_intt_sp / k_ksf_moddown) with a data prime in place of the special prime:
//               s   = (INTT_l(c_l) + half) mod q_l,  half = floor(q_l / 2)                                        k_rs_intt
//               out = (c_i - NTT_i((s + fix_i) mod q_i)) * q_l^-1 mod q_i,  fix_i = q_i - (half mod q_i)          k_rs_down
//             = NTT_i(round(X / q_l) mod q_i) for the CRT value X of every coefficient. FP64 plans only (moduli < 2^52).
//   galois    X -> X^g on polynomials in NTT form: a pure index permutation of the transforms' bit-reversed output order,
//               out[j] = in[brv(((2 brv(j) + 1) g mod 2n - 1) / 2)]                                              k_galois
//             no arithmetic, no sign flips, no dependence on the root or the modulus.
//   rotate    (sigma_g(c0), 0) + KeySwitch(sigma_g(c1)): one k_galois launch, then the keyswitch, per slice of instances.
//   hoisted   many rotations of one ciphertext: the entry point is here, the launcher beside the kernels it runs (keyswitch_f64.hip).
//   linear    the hoisted rotations weighted by plaintexts and summed before ONE mod-down (hexl_linear_transform): entry point and the
//             key-free part (k_galois_c0_pt) here, launcher and multiply-accumulate in keyswitch_f64.hip.
#include "hexl_internal.hpp"
#include "ntt_core_f64.hpp"
#include "number_theory.hpp"

using namespace hx;

struct RsArgs {
    const KsModF64* mods;       // [K]
    const double* tables;       // [K][4][n] (keyswitch_f64.hip KsArgsF)
    const KsRescaleF64* rm;     // [l]: constants of the level that drops limb l
    const u64* in;              // [nb][ncomp][l + 1][n]
    u64* out;                   // [nb][ncomp][l][n]
    double* s;                  // [nb][ncomp][n]  s = (INTT_l(c_l) + half) mod q_l, canonical, natural order
    double half;                // floor(q_l / 2)
    u32 l;                      // the limb dropped (n_limbs - 1)
    unsigned long long tiermap; // LAZY = -1: nibble i = reduction period of limb i (keyswitch_f64.hip)
};

__device__ __forceinline__ u32 xcd_item_rs(u32 bid, u32 total) {   // XCD-contiguous work ranges, as keyswitch_f64.hip xcd_item_f
    const u32 q = total >> 3, r = total & 7, xcd = bid & 7, j = bid >> 3;
    return xcd * q + (xcd < r ? xcd : r) + j;
}

// one workgroup per (instance, component): s = (INTT_{q_l}(c_l) + half) mod q_l, as k_ksf_intt_sp does for the special prime
template <int LOGN, int LOGE, int LAZY>
__global__ __launch_bounds__(1 << (LOGN - LOGE)) void k_rs_intt(RsArgs a) {
    using G = Geom<LOGN, LOGE>;
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const int tid = threadIdx.x;
    const u32 item = blockIdx.x;                                  // b*ncomp + k
    const u32 l = a.l;
    const KsModF64 md = a.mods[l];
    const Mod m = md.m;
    const double* tb = a.tables + size_t(l) * 4 * G::N;
    const u64* src = a.in + (size_t(item) * (l + 1) + l) * G::N;
    const u32 tB = u32(G::idxB(0, tid));
    double v[G::E];
#pragma unroll
    for (int r = 0; r < G::E; ++r) v[r] = hxf::reduce(hxf::to_f64((src + G::idxB(r, 0))[tB]), m);
    with_tier<LAZY, false>(a.tiermap, l, [&](auto T) {            // one transform per workgroup: FRESH
        WgNttF64<LOGN, LOGE, decltype(T)::value>::template inverse<true>(v, ldsd, tid, tb + 2 * G::N, tb + 3 * G::N, m, md.sc);
    });
    double* dst = a.s + size_t(item) * G::N;
#pragma unroll
    for (int r = 0; r < G::E; ++r) (dst + G::idxA(r, 0))[u32(tid)] = hxf::rs_round(v[r], a.half, m);
}

// one workgroup per (instance, component, i < l): w = NTT_{q_i}((s + fix_i) mod q_i); out = (c_i - w) * q_l^-1 mod q_i
template <int LOGN, int LOGE, int LAZY>
__global__ __launch_bounds__(1 << (LOGN - LOGE)) void k_rs_down(RsArgs a) {
    using G = Geom<LOGN, LOGE>;
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const int tid = threadIdx.x;
    const u32 l = a.l;
    // (b*ncomp + k)*l + i, XCD-contiguous: the l transforms that read the same s run back to back on one XCD
    const u32 item = __builtin_amdgcn_readfirstlane(xcd_item_rs(blockIdx.x, gridDim.x));
    const u32 bk = item / l, i = item - bk * l;
    const KsModF64 md = a.mods[i];
    const KsRescaleF64 rc = a.rm[i];
    const Mod m = md.m;
    const double* tb = a.tables + size_t(i) * 4 * G::N;
    const double* sk = a.s + size_t(bk) * G::N;
    double v[G::E];
#pragma unroll
    for (int r = 0; r < G::E; ++r) v[r] = hxf::rs_shift((sk + G::idxA(r, 0))[u32(tid)], rc.fix, m);
    const u64* ci = a.in + (size_t(bk) * (l + 1) + i) * G::N;
    const u32 tB = u32(G::idxB(0, tid));
    u64 craw[G::E];
    // FINAL: w range-reduced (|w| <= p/2 + 2), so |c_i - w| <= p + 4 is inside mul_shoup's documented bound. Mixed tiers (LAZY = -1):
    // two schedules, strict and period 3 (valid for every lazy limb), and c_i loaded behind the transform: the four schedules of N = 16384
    // with c_i requested early spill (132 bytes per lane)
    with_tier<LAZY, false>(a.tiermap, i, [&](auto T) {
        using W = WgNttF64<LOGN, LOGE, decltype(T)::value>;
        if constexpr (G::HALF_ONLY || LAZY < 0) {                  // N = 32768: no registers to hold c_i during the transform
            W::template forward<true, true>(v, ldsd, tid, tb, tb + G::N, m);
#pragma unroll
            for (int r = 0; r < G::E; ++r) craw[r] = (ci + G::idxB(r, 0))[tB];
        } else {                                                   // c_i requested behind the cross-wave re-deal
            W::template forward<true, true>(v, ldsd, tid, tb, tb + G::N, m, 0u, [&] {
#pragma unroll
                for (int r = 0; r < G::E; ++r) craw[r] = (ci + G::idxB(r, 0))[tB];
            });
        }
    });
    u64* dst = a.out + (size_t(bk) * l + i) * G::N;
#pragma unroll
    for (int r = 0; r < G::E; ++r)
        (dst + G::idxB(r, 0))[tB] = hxf::from_f64(hxf::rs_down(hxf::to_f64(craw[r]), v[r], rc.qlinv, rc.qlinv_p, m));
}

// ---- Galois automorphism in NTT form (galois_src: ntt_core.hpp) ----

struct GaloisArgs {
    const u64* in;              // [count][n]
    u64* out;                   // [count][n]
    u64* t;                     // rotate: [count / (2 L)][L][n] receives component 1; nullptr: every polynomial goes to `out`
    size_t count;               // polynomials
    u32 logn, g, L;
};

// Polynomial p of the input goes to polynomial p of `out`. Rotate (t != nullptr, p = (b*2 + k)*L + j): component 1 goes to t[b][j]
// instead, and out[b][1][j] is zeroed -- the keyswitch then adds into (sigma(c0), 0).
// LDS (n <= 16384, 128 KiB): a coalesced load of the whole polynomial, the gather from LDS, a coalesced store.
// n = 32768 does not fit: the gather reads global memory (the sources of neighbouring outputs mostly lie within a few words).
// C0_ONLY (hexl_rotate_hoisted, p as for rotate): component 1 of `out` is zeroed and sigma(c1) goes nowhere -- the hoisted
// multiply-accumulate applies sigma to the mod-up output instead; `t` is not read.
template <bool LDS, bool C0_ONLY = false>
__global__ __launch_bounds__(1024) void k_galois(GaloisArgs a) {
    typedef unsigned long long u2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    const u32 n = 1u << a.logn, tid = threadIdx.x, T = blockDim.x;
    for (size_t p = blockIdx.x; p < a.count; p += gridDim.x) {
        const u64* src = a.in + p * n;
        u64* dst = a.out + p * n;
        if constexpr (C0_ONLY) {
            if ((p / a.L) & 1) {
                const u2 zero = {0, 0};
                for (u32 c = tid; c < n / 2; c += T) reinterpret_cast<u2*>(dst)[c] = zero;
                continue;                                         // (p is the same for the whole workgroup)
            }
        } else if (a.t) {
            const size_t bk = p / a.L, j = p - bk * a.L;
            if (bk & 1) {
                const u2 zero = {0, 0};
                for (u32 c = tid; c < n / 2; c += T) reinterpret_cast<u2*>(dst)[c] = zero;
                dst = a.t + ((bk >> 1) * a.L + j) * n;
            }
        }
        if constexpr (LDS) {
            for (u32 c = tid; c < n / 2; c += T) reinterpret_cast<u2*>(lds)[c] = reinterpret_cast<const u2*>(src)[c];
            __syncthreads();
            for (u32 c = tid; c < n / 2; c += T) {
                const u2 w = {lds[galois_src(2 * c, a.logn, a.g)], lds[galois_src(2 * c + 1, a.logn, a.g)]};
                reinterpret_cast<u2*>(dst)[c] = w;
            }
            __syncthreads();                                      // the next polynomial's load overwrites lds
        } else {
            for (u32 c = tid; c < n / 2; c += T) {
                const u2 w = {src[galois_src(2 * c, a.logn, a.g)], src[galois_src(2 * c + 1, a.logn, a.g)]};
                reinterpret_cast<u2*>(dst)[c] = w;
            }
        }
    }
}

template <bool C0_ONLY = false>
static int launch_galois(hexl_ctx* c, hipStream_t st, const GaloisArgs& a) {
    if (!a.count) return 0;
    const u32 n = 1u << a.logn;
    const u32 grid = a.count < 65536 ? (u32)a.count : 65536u;
    if (a.logn <= 14) {
        if (int rc = hx_lds_optin<k_galois<true, C0_ONLY>>(c->device, 16384 * 8)) return rc;
        hipLaunchKernelGGL((k_galois<true, C0_ONLY>), dim3(grid), dim3(n >= 2048 ? 1024 : 512), size_t(n) * 8, st, a);
    } else {
        hipLaunchKernelGGL((k_galois<false, C0_ONLY>), dim3(grid), dim3(1024), 0, st, a);
    }
    return (int)hipGetLastError();
}

int hx_launch_galois(hexl_ctx* c, u64* d_out, const u64* d_in, size_t count, u32 logn, u32 g) {
    GaloisArgs a{d_in, d_out, nullptr, count, logn, g, 1};
    return launch_galois(c, c->stream, a);
}

// d_ct[nb][2][L][n] -> d_out[nb][2][L][n] = (sigma_g(c0), 0): what hexl_rotate_hoisted's mod-down then adds into
int hx_launch_galois_c0(hexl_ctx* c, u64* d_out, const u64* d_ct, size_t nb, u32 L, u32 logn, u32 g) {
    GaloisArgs a{d_ct, d_out, nullptr, nb * 2 * L, logn, g, L};
    return launch_galois<true>(c, c->stream, a);
}

// ---- the part of a linear transform (hexl_linear_transform) that needs no key: what its single mod-down then adds into ----
//     out[b][0][i][j] = sum_r pt_r[i][j] . c0[b][i][galois_src_r(j)] + pt_id[i][j] . c0[b][i][j]
//     out[b][1][i][j] =                                                pt_id[i][j] . c1[b][i][j]      (0 without an identity term)
// every word canonical. One launch per chunk writes both components; the rotations come from the per-call device table.
struct GaloisPtArgs {
    const KsModF64* mods;       // [K]
    const u64* ct;              // [nb][2][L][n]
    u64* out;                   // [nb][2][L][n]
    const HxLtRot* rots;        // [n_rot]: plaintext [> L][n] (rows 0 ... L - 1 are read here) and Galois element
    const u64* pt_id;           // [L][n]; nullptr: no identity term
    u32* range_flag;            // raised for a ciphertext word read here that is not below its modulus; nullptr: nothing is reported
    u32 n_rot, nb, L, logn;
};
constexpr u32 GPT_THREADS = 256, GPT_LOG_CHUNK = 9;     // two adjacent words per lane: 512 words of one polynomial per workgroup
static_assert(GPT_THREADS == HX_WW_THREADS && GPT_THREADS * 2 == 1u << GPT_LOG_CHUNK, "hx_ww_grid(., ., ., GPT_LOG_CHUNK) counts these workgroups");

// One workgroup per (limb, 512-word piece, instance), the instance fastest: the workgroups resident at any time meet the same plaintext
// words, which are read from HBM once and from L2 afterwards. A lane owns two adjacent output words (16-byte plaintext loads and stores)
// and gathers its two c0 words per rotation through L2 -- the whole row is 8 n bytes, and sigma_g maps aligned blocks onto aligned
// blocks (keyswitch_f64.hip k_ksf_mac_galois), so a workgroup's sources are whole cache lines. The sum runs on hxf::lt_mac_acc, the
// multiply-accumulate's own chain. Every c0 word is some lane's source in every rotation, so the range check sees all of them.
template <bool IDENTITY>
__global__ __launch_bounds__(GPT_THREADS) void k_galois_c0_pt(GaloisPtArgs a) {
    typedef unsigned long long u2 __attribute__((ext_vector_type(2)));
    const u32 n = 1u << a.logn;
    const u32 b = blockIdx.x % a.nb, ic = blockIdx.x / a.nb;      // (i * pieces + piece) * nb + b
    const u32 i = ic >> (a.logn - GPT_LOG_CHUNK), piece = ic & ((1u << (a.logn - GPT_LOG_CHUNK)) - 1);
    const u32 j = (piece << GPT_LOG_CHUNK) + 2 * threadIdx.x;
    const Mod m = a.mods[i].m;
    const size_t row = size_t(i) * n;
    const u64* c0 = a.ct + size_t(b) * 2 * a.L * n + row;
    const u64* c1 = c0 + size_t(a.L) * n;
    u64* o0 = a.out + size_t(b) * 2 * a.L * n + row;
    u64* o1 = o0 + size_t(a.L) * n;
    hxf::RangeMask bad = 0;
    double acc[2] = {0.0, 0.0};
    for (u32 r = 0; r < a.n_rot; ++r) {
        const HxLtRot rot = a.rots[r];                            // uniform: scalar loads
        const u2 t = *reinterpret_cast<const u2*>(rot.pt + row + j);
        const u64 w[2] = {c0[galois_src(j, a.logn, (u32)rot.g)], c0[galois_src(j + 1, a.logn, (u32)rot.g)]};
#pragma unroll
        for (int e = 0; e < 2; ++e)
            acc[e] = hxf::lt_mac_acc(hxf::reduce(hxf::to_f64_checked(w[e], m, bad), m), hxf::lt_pt(hxf::to_f64(t[e]), m), acc[e], m);
    }
    u2 out0, out1 = {0, 0};
    if constexpr (IDENTITY) {
        const u2 t = *reinterpret_cast<const u2*>(a.pt_id + row + j);
        const u2 w0 = *reinterpret_cast<const u2*>(c0 + j), w1 = *reinterpret_cast<const u2*>(c1 + j);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const double td = hxf::lt_pt(hxf::to_f64(t[e]), m);
            acc[e] = hxf::lt_mac_acc(hxf::reduce(hxf::to_f64_checked(w0[e], m, bad), m), td, acc[e], m);
            out1[e] = hxf::from_f64(hxf::lift(hxf::lt_mac(hxf::reduce(hxf::to_f64_checked(w1[e], m, bad), m), td, m), m));
        }
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) out0[e] = hxf::from_f64(hxf::lift(acc[e], m));
    *reinterpret_cast<u2*>(o0 + j) = out0;
    *reinterpret_cast<u2*>(o1 + j) = out1;
    if (a.range_flag) hxf::report_range(bad, a.range_flag);      // (uniform)
}

// n_limbs: the limbs of d_ct, d_out and d_pt_identity -- the plan's L, or the level of a hybrid caller (keyswitch_hybrid.hip), whose
// plaintexts are [K][n] and which passes no flag
int hx_launch_galois_c0_pt(hexl_ks_plan* p, u64* d_out, const u64* d_ct, const HxLtRot* d_rots, size_t n_rot, const u64* d_pt_identity,
                           size_t nb, u32 n_limbs, u32* d_range_flag) {
    if (!nb) return 0;
    const GaloisPtArgs a{p->d_mods_f64, d_ct, d_out, d_rots, d_pt_identity, d_range_flag, (u32)n_rot, (u32)nb, n_limbs, p->logn};
    const dim3 grid((u32)hx_ww_grid(p, nb, n_limbs, GPT_LOG_CHUNK)), block(GPT_THREADS);
    if (d_pt_identity) hipLaunchKernelGGL((k_galois_c0_pt<true>), grid, block, 0, p->ctx->stream, a);
    else hipLaunchKernelGGL((k_galois_c0_pt<false>), grid, block, 0, p->ctx->stream, a);
    return (int)hipGetLastError();
}

// ---- the giant steps of hexl_linear_transform_bsgs from the second on: the key-free part is ADDED to what the earlier steps left ----
//     out[b][k][i][j] = (out[b][k][i][j] + t[b][k][i][galois_src(j)]) mod q_i     for k < n_comp; component 1 is left alone when n_comp = 1
// n_comp = 1, g != 1: sigma_g(t[0]) of a rotated giant step (its mod-down then accumulates on top, as after k_galois<., C0_ONLY>);
// n_comp = 2, g = 1: a giant step without a rotation, t itself. Both operands are canonical words (outputs of the mod-down or of
// k_galois_c0_pt), so one conditional subtraction of the integer modulus keeps the sum canonical; the plan's moduli are below 2^52 and
// exact as doubles. Workgroups and lanes as k_galois_c0_pt: (component, limb, 512-word piece, instance), the instance fastest, two
// adjacent words per lane, the gather through L2.
struct GaloisAddArgs {
    const KsModF64* mods;       // [K]
    const u64* t;               // [nb][2][L][n]
    u64* out;                   // [nb][2][L][n]
    u32 nb, L, logn, g;
};

__global__ __launch_bounds__(GPT_THREADS) void k_galois_add(GaloisAddArgs a) {
    typedef unsigned long long u2 __attribute__((ext_vector_type(2)));
    const u32 n = 1u << a.logn;
    const u32 b = blockIdx.x % a.nb, kic = blockIdx.x / a.nb;     // ((k * L + i) * pieces + piece) * nb + b
    const u32 ki = kic >> (a.logn - GPT_LOG_CHUNK), piece = kic & ((1u << (a.logn - GPT_LOG_CHUNK)) - 1);
    const u32 j = (piece << GPT_LOG_CHUNK) + 2 * threadIdx.x;
    const u64 q = (u64)a.mods[ki % a.L].m.p;
    const size_t row = (size_t(b) * 2 * a.L + ki) * n;
    const u64* src = a.t + row;
    u2 o = *reinterpret_cast<const u2*>(a.out + row + j);
    const u64 w[2] = {src[galois_src(j, a.logn, a.g)], src[galois_src(j + 1, a.logn, a.g)]};
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const u64 s = o[e] + w[e];
        o[e] = s >= q ? s - q : s;
    }
    *reinterpret_cast<u2*>(a.out + row + j) = o;
}

// n_limbs: the limbs of d_out and d_t -- the plan's L, or the level of the hybrid caller (keyswitch_hybrid.hip), as hx_launch_galois_c0_pt
int hx_launch_galois_add(hexl_ks_plan* p, u64* d_out, const u64* d_t, size_t nb, u32 g, u32 n_comp, u32 n_limbs) {
    if (!nb) return 0;
    const GaloisAddArgs a{p->d_mods_f64, d_t, d_out, (u32)nb, n_limbs, p->logn, g};
    hipLaunchKernelGGL(k_galois_add, dim3((u32)hx_ww_grid(p, nb * n_comp, n_limbs, GPT_LOG_CHUNK)), dim3(GPT_THREADS), 0, p->ctx->stream, a);
    return (int)hipGetLastError();
}

// ---- rescale ----
template <int LOGN, int LOGE, int LAZY>
static int run_rescale(hexl_ks_plan* p, const RsArgs& a, u32 nb, u32 ncomp) {
    using G = Geom<LOGN, LOGE>;
    if (int rc = hx_lds_optin<k_rs_intt<LOGN, LOGE, LAZY>, k_rs_down<LOGN, LOGE, LAZY>>(p->ctx->device, G::LDS_USED)) return rc;
    hipStream_t st = p->ctx->stream;
    hipLaunchKernelGGL((k_rs_intt<LOGN, LOGE, LAZY>), dim3(nb * ncomp), dim3(G::T), G::LDS_USED, st, a);
    hipLaunchKernelGGL((k_rs_down<LOGN, LOGE, LAZY>), dim3(nb * ncomp * a.l), dim3(G::T), G::LDS_USED, st, a);
    return (int)hipGetLastError();
}

// per-level constants, computed on the host at the first rescale that drops limb l and kept in the plan
static int rescale_constants(hexl_ks_plan* p, u32 l) {
    if (int rc = p->d_rescale.reserve(size_t(16) * 16)) return rc;
    if (p->rescale_levels >> l & 1u) return 0;
    const u64 ql = p->moduli[l], half = ql >> 1;
    KsRescaleF64 rm[16];
    for (u32 i = 0; i < l; ++i) {
        const u64 q = p->moduli[i];
        const double pd = (double)q;
        const u64 inv = hxnt::invmod(ql % q, q);
        rm[i].fix = (double)(q - half % q);                       // in [1, q]
        rm[i].qlinv = hx_centre(inv, q);
        rm[i].qlinv_p = rm[i].qlinv / pd;
        rm[i].half = (double)half;
    }
    HX_CHECK(hipMemcpy(p->d_rescale + size_t(l) * 16, rm, l * sizeof(KsRescaleF64), hipMemcpyHostToDevice));
    p->rescale_levels |= 1u << l;
    return 0;
}

int hx_launch_rescale(hexl_ks_plan* p, u64* d_out, const u64* d_in, size_t batch, u32 n_limbs, u32 ncomp) {
    const u32 l = n_limbs - 1;
    if (int rc = rescale_constants(p, l)) return rc;
    if (!batch) return 0;
    const size_t n = p->n;
    const size_t chunk = hx_ks_chunk_of(p, batch);
    // s: one polynomial per (instance, component) of a chunk
    if (int rc = p->d_rs_s.reserve(chunk * ncomp * n)) return rc;
    const int lazy = hx_level_tier(p, n_limbs);
    RsArgs a;
    a.mods = p->d_mods_f64; a.tables = p->d_tables_f64;
    a.rm = p->d_rescale + size_t(l) * 16;
    a.s = p->d_rs_s;
    a.half = (double)(p->moduli[l] >> 1);
    a.l = l;
    a.tiermap = hx_tiermap(p);
    return hx_for_chunks(batch, chunk, [&](size_t b0, size_t nb) {
        a.in = d_in + b0 * ncomp * n_limbs * n;
        a.out = d_out + b0 * ncomp * l * n;
        // (the (LOGN, LOGE) and tier instantiations of run_chunk_f64, keyswitch_f64.hip)
        return hx_with_f64_geom(p->logn, lazy, [&](auto N, auto E, auto Z) { return run_rescale<N, E, Z>(p, a, (u32)nb, ncomp); });
    });
}

// ---- rotate ----
int hx_launch_rotate(hexl_ks_plan* p, u64* d_out, const u64* d_ct, size_t batch, u32 g) {
    if (!batch) return 0;
    if (!p->have_keys) return HEXL_E_NOKEYS;
    const size_t n = p->n, L = p->L;
    const size_t slice = hx_ks_chunk_of(p, batch);
    if (int rc = p->d_rot_t.reserve(slice * L * n)) return rc;
    return hx_for_chunks(batch, slice, [&](size_t b0, size_t nb) {
        u64* out = d_out + b0 * 2 * L * n;
        GaloisArgs a{d_ct + b0 * 2 * L * n, out, p->d_rot_t, nb * 2 * L, p->logn, g, (u32)L};
        if (int rc = launch_galois(p->ctx, p->ctx->stream, a)) return rc;
        // hx_launch_keyswitch joins its lanes back into the caller's stream before it returns (keyswitch.hip), so the next
        // slice's gather into the same t buffer runs after this keyswitch has read it
        return hx_launch_keyswitch(p, out, p->d_rot_t, nb, 7, nullptr);
    });
}

// ---- entry points of include/hexl_mi355x.h. They live here rather than in capi.hip: the CPU staging model (tests/cpp) compiles
// capi.hip and host_staging.hip against stubs of the launchers those two call, and needs none for these. ----
static bool ring_dimension_ok(u64 n) { return n >= 1024 && n <= 32768 && !(n & (n - 1)); }
static bool galois_elt_ok(u64 g, u64 n) { return (g & 1) && g < 2 * n; }
// a plan of a hoisted call works in p0's scratch with p0's geometry: same context, same FP64 ring
static bool same_ring(const hexl_ks_plan* p, const hexl_ks_plan* p0) {
    return p->ctx == p0->ctx && p->n == p0->n && p->L == p0->L && p->K == p0->K && p->use_f64 && p->moduli == p0->moduli;
}
// bytes of one component [L][n], of one ciphertext, of `batch` of them and of one plaintext [L + 1][n]; false when `bytes` overflows
struct CtBytes { size_t row, per, bytes, pt_bytes; };
static bool ct_bytes(const hexl_ks_plan* p0, size_t batch, CtBytes& s) {
    s.row = size_t(p0->L) * p0->n * sizeof(u64);
    s.per = 2 * s.row;
    s.pt_bytes = s.row + p0->n * sizeof(u64);
    return hx_words_bytes(batch, 2, p0->L, p0->n, &s.bytes);
}

extern "C" int hexl_apply_galois(hexl_ctx* c, uint64_t* d_out, const uint64_t* d_in, size_t count, uint64_t n, uint64_t g) {
    if (!c || !d_out || !d_in || !ring_dimension_ok(n) || !galois_elt_ok(g, n)) return HEXL_E_BADARG;
    size_t bytes;
    if (!hx_words_bytes(count, 1, 1, n, &bytes)) return HEXL_E_BADARG;
    if (hx_ranges_overlap(d_out, bytes, d_in, bytes)) return HEXL_E_BADARG;    // a permutation cannot run in place
    if (!count) return 0;
    u32 logn = 0;
    while ((1ULL << logn) < n) ++logn;
    HX_CHECK(hipSetDevice(c->device));
    return hx_launch_galois(c, d_out, d_in, count, logn, (u32)g);
}

extern "C" int hexl_rescale(hexl_ks_plan* p, uint64_t* d_out, const uint64_t* d_in, size_t batch, uint64_t n_limbs,
                            uint64_t n_components) {
    if (!p || !d_out || !d_in || !hx_f64_plan_ok(p, n_limbs, 2, p->K - 1) || !hx_in_range(n_components, 1, 3)) return HEXL_E_BADARG;
    size_t in_bytes;
    if (!hx_words_bytes(batch, n_components, n_limbs, p->n, &in_bytes)) return HEXL_E_BADARG;
    if (hx_ranges_overlap(d_out, in_bytes / n_limbs * (n_limbs - 1), d_in, in_bytes)) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    return hx_launch_rescale(p, d_out, d_in, batch, (u32)n_limbs, (u32)n_components);
}

extern "C" int hexl_rotate(hexl_ks_plan* p, uint64_t* d_out, const uint64_t* d_ct, size_t batch, uint64_t g) {
    if (!p || !d_out || !d_ct || !galois_elt_ok(g, p->n)) return HEXL_E_BADARG;
    CtBytes s;
    if (!ct_bytes(p, batch, s)) return HEXL_E_BADARG;
    if (hx_ranges_overlap(d_out, s.bytes, d_ct, s.bytes)) return HEXL_E_BADARG;   // component 1 of d_out is zeroed before the keyswitch
    if (!p->have_keys) return HEXL_E_NOKEYS;
    HX_CHECK(hipSetDevice(p->ctx->device));
    return hx_launch_rotate(p, d_out, d_ct, batch, (u32)g);
}

// The three hoisted entry points check in one order: HEXL_E_BADARG for anything malformed in any plan or buffer, then HEXL_E_NOKEYS,
// then nothing to do for an empty batch.
extern "C" int hexl_rotate_hoisted(hexl_ks_plan* const* plans, const uint64_t* galois_elts, size_t n_rot, uint64_t* const* d_outs,
                                   const uint64_t* d_ct, size_t batch) {
    if (!plans || !galois_elts || !d_outs || !d_ct) return HEXL_E_BADARG;
    if (!n_rot) return 0;
    for (size_t r = 0; r < n_rot; ++r)
        if (!plans[r] || !d_outs[r]) return HEXL_E_BADARG;
    const hexl_ks_plan* p0 = plans[0];
    CtBytes s;
    if (!hx_f64_plan_ok(p0) || !ct_bytes(p0, batch, s)) return HEXL_E_BADARG;
    for (size_t r = 0; r < n_rot; ++r) {
        if (!same_ring(plans[r], p0) || !galois_elt_ok(galois_elts[r], p0->n)) return HEXL_E_BADARG;
        if (hx_ranges_overlap(d_outs[r], s.bytes, d_ct, s.bytes)) return HEXL_E_BADARG;
        for (size_t q = 0; q < r; ++q)
            if (hx_ranges_overlap(d_outs[r], s.bytes, d_outs[q], s.bytes)) return HEXL_E_BADARG;
    }
    for (size_t r = 0; r < n_rot; ++r)
        if (!plans[r]->have_keys) return HEXL_E_NOKEYS;
    if (!batch) return 0;
    HX_CHECK(hipSetDevice(p0->ctx->device));
    return hx_launch_rotate_hoisted(plans, galois_elts, n_rot, d_outs, d_ct, batch);
}

extern "C" int hexl_linear_transform(hexl_ks_plan* const* plans, const uint64_t* galois_elts, const uint64_t* const* d_pts, size_t n_rot,
                                     const uint64_t* d_pt_identity, uint64_t* d_out, const uint64_t* d_ct, size_t batch) {
    if (!plans || !galois_elts || !d_pts || !d_out || !d_ct || !n_rot) return HEXL_E_BADARG;
    if (n_rot > SIZE_MAX / sizeof(HxLtRot)) return HEXL_E_BADARG;
    for (size_t r = 0; r < n_rot; ++r)
        if (!plans[r] || !d_pts[r]) return HEXL_E_BADARG;
    const hexl_ks_plan* p0 = plans[0];
    CtBytes s;
    if (!hx_f64_plan_ok(p0) || !ct_bytes(p0, batch, s)) return HEXL_E_BADARG;
    if (hx_ranges_overlap(d_out, s.bytes, d_ct, s.bytes)) return HEXL_E_BADARG;
    if (d_pt_identity && hx_ranges_overlap(d_out, s.bytes, d_pt_identity, s.row)) return HEXL_E_BADARG;
    for (size_t r = 0; r < n_rot; ++r) {
        if (!same_ring(plans[r], p0) || !galois_elt_ok(galois_elts[r], p0->n)) return HEXL_E_BADARG;
        if (hx_ranges_overlap(d_out, s.bytes, d_pts[r], s.pt_bytes)) return HEXL_E_BADARG;
    }
    for (size_t r = 0; r < n_rot; ++r)
        if (!plans[r]->have_keys) return HEXL_E_NOKEYS;
    if (!batch) return 0;
    HX_CHECK(hipSetDevice(p0->ctx->device));
    return hx_launch_linear_transform(plans, galois_elts, d_pts, n_rot, d_pt_identity, d_out, d_ct, batch);
}

extern "C" int hexl_linear_transform_bsgs(hexl_ks_plan* const* baby_plans, const uint64_t* baby_elts, size_t n_baby,
                                          hexl_ks_plan* const* giant_plans, const uint64_t* giant_elts, size_t n_giant,
                                          const uint64_t* const* d_pts, const uint64_t* const* d_pt_identity, uint64_t* d_out,
                                          const uint64_t* d_ct, size_t batch) {
    if (!baby_plans || !baby_elts || !giant_plans || !giant_elts || !d_pts || !d_out || !d_ct || !n_giant) return HEXL_E_BADARG;
    if (n_giant > SIZE_MAX / sizeof(HxLtRot) / 2 || (n_baby && n_giant > SIZE_MAX / sizeof(HxLtRot) / 2 / n_baby)) return HEXL_E_BADARG;
    // the plan that lends scratch, buffers, tier and range flag: baby_plans[0] whenever there is one
    hexl_ks_plan* p0 = nullptr;
    for (size_t i = 0; i < n_baby && !p0; ++i) p0 = baby_plans[i];
    for (size_t j = 0; j < n_giant && !p0; ++j) p0 = giant_plans[j];
    if (!p0) return HEXL_E_BADARG;
    CtBytes s;
    if (!hx_f64_plan_ok(p0) || !ct_bytes(p0, batch, s)) return HEXL_E_BADARG;
    if (n_baby > HX_LT_BSGS_STORE_BYTES / (2 * s.pt_bytes)) return HEXL_E_BADARG;   // not one instance would fit the baby store
    if (hx_ranges_overlap(d_out, s.bytes, d_ct, s.bytes)) return HEXL_E_BADARG;
    for (size_t i = 0; i < n_baby; ++i)
        if ((baby_plans[i] && !same_ring(baby_plans[i], p0)) || !galois_elt_ok(baby_elts[i], p0->n)) return HEXL_E_BADARG;
    for (size_t j = 0; j < n_giant; ++j) {
        if ((giant_plans[j] && !same_ring(giant_plans[j], p0)) || !galois_elt_ok(giant_elts[j], p0->n)) return HEXL_E_BADARG;
        if (!giant_plans[j] && giant_elts[j] != 1) return HEXL_E_BADARG;
        const u64* pt_id = d_pt_identity ? d_pt_identity[j] : nullptr;
        if (pt_id && hx_ranges_overlap(d_out, s.bytes, pt_id, s.row)) return HEXL_E_BADARG;
        bool any = pt_id != nullptr;
        for (size_t i = 0; i < n_baby; ++i)
            if (const u64* pt = d_pts[j * n_baby + i]) {
                if (!baby_plans[i] || hx_ranges_overlap(d_out, s.bytes, pt, s.pt_bytes)) return HEXL_E_BADARG;
                any = true;
            }
        if (!any) return HEXL_E_BADARG;                             // a giant row with no term at all
    }
    for (size_t j = 0; j < n_giant; ++j) {
        if (giant_elts[j] != 1 && !giant_plans[j]->have_keys) return HEXL_E_NOKEYS;
        for (size_t i = 0; i < n_baby; ++i)
            if (d_pts[j * n_baby + i] && !baby_plans[i]->have_keys) return HEXL_E_NOKEYS;
    }
    if (!batch) return 0;
    HX_CHECK(hipSetDevice(p0->ctx->device));
    return hx_launch_linear_transform_bsgs(p0, baby_plans, baby_elts, n_baby, giant_plans, giant_elts, n_giant, d_pts, d_pt_identity, d_out,
                                           d_ct, batch);
}
