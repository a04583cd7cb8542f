// rlwe.hip -- the sampler on the device and the two ends of a flow that need it (DESIGN.md 4.6.6 "Sampling, encrypt and decrypt"):
//   sample         out[c][i] = polynomial `first + c` of the stream (seed, stream, kind) modulo q_i, NTT form
//                  UNIFORM: the words themselves (uniform words are uniform in either domain)            k_sample_uniform
//                  TERNARY / CBD21: one integer polynomial, NTT_i(v mod q_i) in every limb               k_sample_small + k_rns_from_f64
//   rlwe_encrypt   out[b] = (pt + e - a s, a), a = UNIFORM and e = CBD21 of polynomial `first + b`       k_sample_small + k_rns_from_f64
//                                                                                                          + k_rlwe_encrypt
//   rlwe_decrypt   out[b] = c0 + c1 s (+ c2 s^2), Horner                                                  k_rlwe_decrypt
//   pk_encrypt     out[b] = (pk0 u + e0 + pt, pk1 u + e1), u = TERNARY polynomial c = first + b, e0 / e1 =      2 k_sample_small + k_rns_from_f64
//                  CBD21 polynomials 2c / 2c + 1 of (seed, stream)                           + k_pk_encrypt
// The streams are ChaCha20 in counter mode, addressed per word (sample_core.hpp): a result depends on (seed, stream, absolute
// polynomial index, limb, coefficient) only. The three word kernels have k_pt_mul's shape (rns_ops.hip): one workgroup per (instance,
// limb, 1024-word chunk), 256 lanes, the modulus found once per workgroup; a lane owns FOUR CONSECUTIVE words -- 32 contiguous bytes,
// and exactly one UNIFORM block of 64 stream bytes, none of it wasted. FP64 plans only (moduli < 2^52). The small kinds and the error
// of an encryption go through the plan's encode scratch (ckks_encode.hip: d_enc_coeffs, d_enc_words) under encode's chunk rule.
#include "hexl_internal.hpp"
#include "sample_core.hpp"

using hxf::Mod;

constexpr u32 RL_THREADS = 256, RL_LOG_CHUNK = 10;      // 1024 words of one polynomial per workgroup, four per lane
static_assert(RL_THREADS * 4 == 1u << RL_LOG_CHUNK, "a workgroup covers its chunk exactly");
static_assert(RL_THREADS == HX_WW_THREADS && RL_LOG_CHUNK == HX_WW_LOG_CHUNK, "hx_ww_grid counts these workgroups");
typedef unsigned long long rl_u2 __attribute__((ext_vector_type(2)));

struct SampleArgs {
    const KsModF64* mods;       // [K]
    u64* out;                   // uniform: [count][L][n]
    double* coeffs;             // small: [count][n] (plan scratch)
    hxs::Seed seed;             // by value: nothing of the caller's is read after the call returns
    u64 stream, first;          // absolute index of instance 0 of this launch
    u32 logn, L;
    u32 count;                  // small: instances of this launch
    int kind;
};

// the (instance, limb, chunk) of a workgroup and the offset of its chunk inside the polynomial
struct RlWhere { u32 b, i, j0; };
__device__ __forceinline__ RlWhere rl_where(u32 logn, u32 L) {
    const u32 bi = blockIdx.x >> (logn - RL_LOG_CHUNK), ch = blockIdx.x - (bi << (logn - RL_LOG_CHUNK));
    const u32 b = bi / L;
    return {b, bi - b * L, (ch << RL_LOG_CHUNK) + 4 * threadIdx.x};
}
// the four UNIFORM words j0 ... j0 + 3 (j0 a multiple of 4: one block) of polynomial (c, limb i), canonical, as doubles
__device__ __forceinline__ void rl_uniform4(double a[4], const hxs::Seed& seed, u64 stream, u64 c, u32 i, u32 logn, u32 j0, const Mod m) {
    hxs::uniform4(a, seed, stream, c, i, logn, j0, m);
}
__device__ __forceinline__ void rl_store4(u64* dst, const double v[4]) {
    rl_u2 lo, hi;
    lo.x = hxf::from_f64(v[0]); lo.y = hxf::from_f64(v[1]);
    hi.x = hxf::from_f64(v[2]); hi.y = hxf::from_f64(v[3]);
    reinterpret_cast<rl_u2*>(dst)[0] = lo;
    reinterpret_cast<rl_u2*>(dst)[1] = hi;
}
__device__ __forceinline__ void rl_load4(double v[4], const u64* src) {
    const rl_u2 lo = reinterpret_cast<const rl_u2*>(src)[0], hi = reinterpret_cast<const rl_u2*>(src)[1];
    v[0] = hxf::to_f64(lo.x); v[1] = hxf::to_f64(lo.y);
    v[2] = hxf::to_f64(hi.x); v[3] = hxf::to_f64(hi.y);
}

__global__ __launch_bounds__(RL_THREADS) void k_sample_uniform(SampleArgs a) {
    const RlWhere w = rl_where(a.logn, a.L);
    const Mod m = a.mods[w.i].m;
    double v[4];
    rl_uniform4(v, a.seed, a.stream, a.first + w.b, w.i, a.logn, w.j0, m);
    rl_store4(a.out + ((size_t(w.b) * a.L + w.i) << a.logn) + w.j0, v);
}

// One block -- eight coefficients, 64 contiguous bytes of doubles -- per lane: lane g of the launch holds coefficients 8 (g mod n/8) ...
// of instance g / (n/8). The doubles are what hexl_rns_from_f64 takes: k_rns_from_f64 turns them into NTT_i(v mod q_i) for every limb.
__global__ __launch_bounds__(RL_THREADS) void k_sample_small(SampleArgs a) {
    const size_t g = size_t(blockIdx.x) * RL_THREADS + threadIdx.x;
    if (g >= size_t(a.count) << (a.logn - 3)) return;         // an odd count at n = 1024 ends in half a workgroup
    const u32 b = (u32)(g >> (a.logn - 3)), j0 = (u32)(g - (size_t(b) << (a.logn - 3))) << 3;
    const hxs::Block blk = hxs::chacha20_block(a.seed, hxs::counter(a.kind, hxs::small_block(a.first + b, a.logn, j0)), a.stream);
    double2* dst = reinterpret_cast<double2*>(a.coeffs + (size_t(b) << a.logn) + j0);
#pragma unroll
    for (int t = 0; t < 4; ++t)
        dst[t] = double2{(double)hxs::small_value(a.kind, hxs::lane(blk, 2 * t)), (double)hxs::small_value(a.kind, hxs::lane(blk, 2 * t + 1))};
}

struct EncryptArgs {
    const KsModF64* mods;       // [K]
    u64* out;                   // [nb][2][L][n]
    const u64* e;               // [nb][L][n]: NTT_i of the error (plan scratch)
    const u64* pt;              // nullptr, or [pt_stride ? nb : 1][L][n]
    const u64* s;               // [>= L][n]
    hxs::Seed seed;
    u64 stream, first;
    u32 logn, L, pt_stride;
};

// E, pt and s are requested before the block function runs (some 300 32-bit operations that hide their latency); `a` never leaves the
// registers until it is stored as component 1: one read of E / pt / s and one write of the ciphertext.
__global__ __launch_bounds__(RL_THREADS) void k_rlwe_encrypt(EncryptArgs a) {
    const RlWhere w = rl_where(a.logn, a.L);
    const Mod m = a.mods[w.i].m;
    const size_t within = (size_t(w.i) << a.logn) + w.j0, per = size_t(a.L) << a.logn;
    double e[4], s[4], p[4] = {0.0, 0.0, 0.0, 0.0}, u[4], c0[4];
    rl_load4(e, a.e + size_t(w.b) * per + within);
    rl_load4(s, a.s + within);
    if (a.pt) rl_load4(p, a.pt + size_t(w.b) * a.pt_stride * per + within);
    rl_uniform4(u, a.seed, a.stream, a.first + w.b, w.i, a.logn, w.j0, m);
#pragma unroll
    for (int k = 0; k < 4; ++k) c0[k] = hxs::encrypt_c0(u[k], s[k], e[k], p[k], m);
    u64* dst = a.out + size_t(w.b) * 2 * per + within;
    rl_store4(dst, c0);
    rl_store4(dst + per, u);
}

struct PkEncryptArgs {
    const KsModF64* mods;       // [K]
    u64* out;                   // [nb][2][L][n]
    const u64* u;               // [nb][L][n]: NTT_i of the ternary masks (plan scratch)
    const u64* e;               // [nb][2][L][n]: NTT_i of the two errors of every instance (plan scratch, behind u)
    const u64* pt;              // nullptr, or [pt_stride ? nb : 1][L][n]
    const u64* pk;              // [2][pk_limbs][n], rows 0 ... L - 1 of each component read
    u32 logn, L, pk_limbs, pt_stride;
};

// k_rlwe_encrypt's shape with the mask and the key read instead of drawn. The six loads (u, e0, e1, pt, pk0, pk1) are issued before
// the first product; the key's 2 L n words are the same for every instance and come from the cache after the first wave of
// workgroups, so HBM sees four polynomial reads (u, e0, e1, pt) and two writes per (instance, limb). The chains are sample_core.hpp's.
__global__ __launch_bounds__(RL_THREADS) void k_pk_encrypt(PkEncryptArgs a) {
    const RlWhere w = rl_where(a.logn, a.L);
    const Mod m = a.mods[w.i].m;
    const size_t within = (size_t(w.i) << a.logn) + w.j0, per = size_t(a.L) << a.logn;
    double u[4], e0[4], e1[4], p[4] = {0.0, 0.0, 0.0, 0.0}, k0[4], k1[4], c0[4], c1[4];
    rl_load4(u, a.u + size_t(w.b) * per + within);
    rl_load4(e0, a.e + size_t(w.b) * 2 * per + within);
    rl_load4(e1, a.e + (size_t(w.b) * 2 + 1) * per + within);
    if (a.pt) rl_load4(p, a.pt + size_t(w.b) * a.pt_stride * per + within);
    rl_load4(k0, a.pk + within);
    rl_load4(k1, a.pk + (size_t(a.pk_limbs) << a.logn) + within);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double ur = hxs::pk_operand(u[k], m);
        c0[k] = hxs::pk_c0(hxs::pk_operand(k0[k], m), ur, e0[k], p[k], m);
        c1[k] = hxs::pk_c1(hxs::pk_operand(k1[k], m), ur, e1[k], m);
    }
    u64* dst = a.out + size_t(w.b) * 2 * per + within;
    rl_store4(dst, c0);
    rl_store4(dst + per, c1);
}

struct DecryptArgs {
    const KsModF64* mods;       // [K]
    u64* out;                   // [count][L][n]
    const u64* ct;              // [count][NCOMP][L][n]
    const u64* s;               // [>= L][n]
    u32 logn, L;
};

// every component is loaded before the first product; Horner from the top component
template <int NCOMP>
__global__ __launch_bounds__(RL_THREADS) void k_rlwe_decrypt(DecryptArgs a) {
    const RlWhere w = rl_where(a.logn, a.L);
    const Mod m = a.mods[w.i].m;
    const size_t within = (size_t(w.i) << a.logn) + w.j0, per = size_t(a.L) << a.logn;
    double c[NCOMP][4], s[4], r[4];
#pragma unroll
    for (int k = 0; k < NCOMP; ++k) rl_load4(c[k], a.ct + (size_t(w.b) * NCOMP + k) * per + within);
    rl_load4(s, a.s + within);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const double sr = hxf::reduce(s[t], m);
        double acc = hxf::reduce(c[NCOMP - 1][t], m);
#pragma unroll
        for (int k = NCOMP - 2; k >= 0; --k) acc = hxs::horner(acc, sr, c[k][t], m);
        r[t] = hxf::lc_finish(acc, m);
    }
    rl_store4(a.out + size_t(w.b) * per + within, r);
}

// ---- launchers ----
static dim3 rl_grid(const hexl_ks_plan* p, size_t count, u32 n_limbs) { return dim3((u32)hx_ww_grid(p, count, n_limbs)); }

// the small values of instances first ... first + nb - 1 into rows row0 ... row0 + nb - 1 of the plan's d_enc_coeffs (grown by the
// caller), as doubles
static int launch_small(hexl_ks_plan* p, int kind, const hxs::Seed& seed, u64 stream, u64 first, size_t nb, size_t row0 = 0) {
    SampleArgs a{};
    a.coeffs = p->d_enc_coeffs + row0 * p->n;
    a.seed = seed;
    a.stream = stream;
    a.first = first;
    a.logn = p->logn;
    a.count = (u32)nb;
    a.kind = kind;
    hipLaunchKernelGGL(k_sample_small, dim3((u32)(((nb << (p->logn - 3)) + RL_THREADS - 1) / RL_THREADS)), dim3(RL_THREADS), 0, p->ctx->stream, a);
    return (int)hipGetLastError();
}

int hx_launch_sample(hexl_ks_plan* p, u64* d_out, int kind, const u32* seed, u64 stream, u64 first, size_t count, u32 n_limbs) {
    if (!count) return 0;
    hxs::Seed sd;
    for (int k = 0; k < 8; ++k) sd.k[k] = seed[k];
    if (kind == hxs::KIND_UNIFORM) {
        SampleArgs a{};
        a.mods = p->d_mods_f64;
        a.out = d_out;
        a.seed = sd;
        a.stream = stream;
        a.first = first;
        a.logn = p->logn;
        a.L = n_limbs;
        a.kind = kind;
        hipLaunchKernelGGL(k_sample_uniform, rl_grid(p, count, n_limbs), dim3(RL_THREADS), 0, p->ctx->stream, a);
        return (int)hipGetLastError();
    }
    const size_t n = p->n, chunk = hx_enc_chunk_of(p, count);
    if (int rc = p->d_enc_coeffs.reserve(chunk * n)) return rc;
    return hx_for_chunks(count, chunk, [&](size_t c0, size_t nb) {
        if (int rc = launch_small(p, kind, sd, stream, first + c0, nb)) return rc;
        return hx_launch_encode(p, d_out + c0 * n_limbs * n, p->d_enc_coeffs, nullptr, nb, n_limbs, 1.0);
    });
}

// d_enc_words[nb][n_limbs][n] = NTT_i of the CBD21 polynomials first ... first + nb - 1 of (seed, stream), through d_enc_coeffs; nb is at
// most a chunk and both buffers have room for it (the caller's reserve)
int hx_launch_rlwe_error(hexl_ks_plan* p, const u32* seed, u64 stream, u64 first, size_t nb, u32 n_limbs) {
    hxs::Seed sd;
    for (int k = 0; k < 8; ++k) sd.k[k] = seed[k];
    if (int rc = launch_small(p, hxs::KIND_CBD21, sd, stream, first, nb)) return rc;
    return hx_launch_encode(p, p->d_enc_words, p->d_enc_coeffs, nullptr, nb, n_limbs, 1.0);
}

int hx_launch_rlwe_encrypt(hexl_ks_plan* p, u64* d_out, const u64* d_pt, bool per_instance, const u64* d_secret, const u32* seed,
                           u64 stream, u64 first, size_t count, u32 n_limbs) {
    if (!count) return 0;
    const size_t n = p->n, chunk = hx_enc_chunk_of(p, count), per = size_t(n_limbs) * n;
    if (int rc = p->d_enc_coeffs.reserve(chunk * n)) return rc;
    if (int rc = p->d_enc_words.reserve(chunk * per)) return rc;
    EncryptArgs a{};
    a.mods = p->d_mods_f64;
    a.e = p->d_enc_words;
    a.s = d_secret;
    for (int k = 0; k < 8; ++k) a.seed.k[k] = seed[k];
    a.stream = stream;
    a.logn = p->logn;
    a.L = n_limbs;
    a.pt_stride = per_instance ? 1u : 0u;
    return hx_for_chunks(count, chunk, [&](size_t c0, size_t nb) {
        if (int rc = hx_launch_rlwe_error(p, seed, stream, first + c0, nb, n_limbs)) return rc;
        a.out = d_out + c0 * 2 * per;
        a.pt = d_pt ? d_pt + (per_instance ? c0 * per : 0) : nullptr;
        a.first = first + c0;
        hipLaunchKernelGGL(k_rlwe_encrypt, rl_grid(p, nb, n_limbs), dim3(RL_THREADS), 0, p->ctx->stream, a);
        return (int)hipGetLastError();
    });
}

// Per chunk of nb instances the encode scratch holds 3 nb rows: the nb masks, then the 2 nb errors in the order [instance][2] -- CBD21
// polynomials 2 (first + c0) ... are that order already -- and ONE transform launch turns all of them into d_enc_words. A chunk is a
// third of encode's, so the scratch never grows beyond what a full chunk of hexl_rlwe_encrypt reserves.
int hx_launch_pk_encrypt(hexl_ks_plan* p, u64* d_out, const u64* d_pt, bool per_instance, const u64* d_pk, u32 pk_limbs, const u32* seed,
                         u64 stream, u64 first, size_t count, u32 n_limbs) {
    if (!count) return 0;
    const size_t n = p->n, chunk = hx_pk_chunk_of(p, count), per = size_t(n_limbs) * n;
    if (int rc = p->d_enc_coeffs.reserve(3 * chunk * n)) return rc;
    if (int rc = p->d_enc_words.reserve(3 * chunk * per)) return rc;
    hxs::Seed sd;
    for (int k = 0; k < 8; ++k) sd.k[k] = seed[k];
    PkEncryptArgs a{};
    a.mods = p->d_mods_f64;
    a.u = p->d_enc_words;
    a.pk = d_pk;
    a.logn = p->logn;
    a.L = n_limbs;
    a.pk_limbs = pk_limbs;
    a.pt_stride = per_instance ? 1u : 0u;
    return hx_for_chunks(count, chunk, [&](size_t c0, size_t nb) {
        if (int rc = launch_small(p, hxs::KIND_TERNARY, sd, stream, first + c0, nb)) return rc;
        if (int rc = launch_small(p, hxs::KIND_CBD21, sd, stream, 2 * (first + c0), 2 * nb, nb)) return rc;
        if (int rc = hx_launch_encode(p, p->d_enc_words, p->d_enc_coeffs, nullptr, 3 * nb, n_limbs, 1.0)) return rc;
        a.out = d_out + c0 * 2 * per;
        a.e = p->d_enc_words + nb * per;
        a.pt = d_pt ? d_pt + (per_instance ? c0 * per : 0) : nullptr;
        hipLaunchKernelGGL(k_pk_encrypt, rl_grid(p, nb, n_limbs), dim3(RL_THREADS), 0, p->ctx->stream, a);
        return (int)hipGetLastError();
    });
}

int hx_launch_rlwe_decrypt(hexl_ks_plan* p, u64* d_out, const u64* d_ct, const u64* d_secret, size_t count, u32 n_components, u32 n_limbs) {
    if (!count) return 0;
    const DecryptArgs a{p->d_mods_f64, d_out, d_ct, d_secret, p->logn, n_limbs};
    const dim3 grid = rl_grid(p, count, n_limbs), block(RL_THREADS);
    if (n_components == 2) hipLaunchKernelGGL(k_rlwe_decrypt<2>, grid, block, 0, p->ctx->stream, a);
    else hipLaunchKernelGGL(k_rlwe_decrypt<3>, grid, block, 0, p->ctx->stream, a);
    return (int)hipGetLastError();
}

// ---- entry points of include/hexl_mi355x.h ----
// the checks of hexl_internal.hpp for 1 <= n_limbs <= K; *bytes = those of `count` instances of `comps` components, whose workgroups fit
static bool rl_plan_ok(const hexl_ks_plan* p, size_t count, u64 comps, u64 n_limbs, size_t* bytes) {
    return p && hx_f64_plan_ok(p, n_limbs, 1, p->K) && hx_words_bytes(count, comps, n_limbs, p->n, bytes) && hx_ww_grid_ok(p, count, n_limbs);
}
static bool rl_index_ok(u64 first, size_t count) { return first <= hxs::MAX_INDEX && count <= hxs::MAX_INDEX - first; }

extern "C" int hexl_sample(hexl_ks_plan* p, uint64_t* d_out, int kind, const uint32_t seed[8], uint64_t stream, uint64_t first,
                           size_t count, uint64_t n_limbs) {
    size_t bytes;
    if (!d_out || !seed || !rl_plan_ok(p, count, 1, n_limbs, &bytes) || !rl_index_ok(first, count)) return HEXL_E_BADARG;
    if (kind != HEXL_SAMPLE_UNIFORM && kind != HEXL_SAMPLE_TERNARY && kind != HEXL_SAMPLE_CBD21) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    return hx_launch_sample(p, d_out, kind, seed, stream, first, count, (u32)n_limbs);
}

extern "C" int hexl_rlwe_encrypt(hexl_ks_plan* p, uint64_t* d_out, const uint64_t* d_pt, size_t pt_batch, const uint64_t* d_secret,
                                 const uint32_t seed[8], uint64_t stream, uint64_t first, size_t count, uint64_t n_limbs) {
    size_t bytes;
    if (!d_out || !d_secret || !seed || !rl_plan_ok(p, count, 2, n_limbs, &bytes) || !rl_index_ok(first, count)) return HEXL_E_BADARG;
    const size_t per = size_t(n_limbs) * p->n * sizeof(u64);
    HxPtBatch pt;
    if (d_pt && !hx_pt_batch(pt_batch, count, per, &pt)) return HEXL_E_BADARG;
    if (hx_ranges_overlap(d_out, bytes, d_secret, per)) return HEXL_E_BADARG;
    if (d_pt && hx_ranges_overlap(d_out, bytes, d_pt, pt.bytes)) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    return hx_launch_rlwe_encrypt(p, d_out, d_pt, pt.stride != 0, d_secret, seed, stream, first, count, (u32)n_limbs);
}

// TERNARY index c and CBD21 indices 2c, 2c + 1 for c < first + count: first + count <= MAX_INDEX / 2 keeps the latter below MAX_INDEX
static bool pk_index_ok(u64 first, size_t count) { return first <= hxs::MAX_INDEX / 2 && count <= hxs::MAX_INDEX / 2 - first; }

extern "C" int hexl_pk_encrypt(hexl_ks_plan* p, uint64_t* d_out, const uint64_t* d_pt, size_t pt_batch, const uint64_t* d_pk,
                               uint64_t pk_limbs, const uint32_t seed[8], uint64_t stream, uint64_t first, size_t count, uint64_t n_limbs) {
    size_t bytes;
    if (!d_out || !d_pk || !seed || !rl_plan_ok(p, count, 2, n_limbs, &bytes) || !pk_index_ok(first, count)) return HEXL_E_BADARG;
    if (!hx_in_range(pk_limbs, n_limbs, p->K)) return HEXL_E_BADARG;
    const size_t per = size_t(n_limbs) * p->n * sizeof(u64);
    HxPtBatch pt;
    if (d_pt && !hx_pt_batch(pt_batch, count, per, &pt)) return HEXL_E_BADARG;
    if (hx_ranges_overlap(d_out, bytes, d_pk, size_t(2) * pk_limbs * p->n * sizeof(u64))) return HEXL_E_BADARG;
    if (d_pt && hx_ranges_overlap(d_out, bytes, d_pt, pt.bytes)) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    return hx_launch_pk_encrypt(p, d_out, d_pt, pt.stride != 0, d_pk, (u32)pk_limbs, seed, stream, first, count, (u32)n_limbs);
}

extern "C" int hexl_rlwe_decrypt(hexl_ks_plan* p, uint64_t* d_out, const uint64_t* d_ct, const uint64_t* d_secret, size_t count,
                                 uint64_t n_components, uint64_t n_limbs) {
    if (!d_out || !d_ct || !d_secret || !hx_in_range(n_components, 2, 3)) return HEXL_E_BADARG;
    size_t ct_bytes;
    if (!rl_plan_ok(p, count, n_components, n_limbs, &ct_bytes)) return HEXL_E_BADARG;
    const size_t per = size_t(n_limbs) * p->n * sizeof(u64), bytes = ct_bytes / n_components;
    if (hx_ranges_overlap(d_out, bytes, d_ct, ct_bytes) || hx_ranges_overlap(d_out, bytes, d_secret, per)) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    return hx_launch_rlwe_decrypt(p, d_out, d_ct, d_secret, count, (u32)n_components, (u32)n_limbs);
}
