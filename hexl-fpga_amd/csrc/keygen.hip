// keygen.hip -- switching keys that never leave the device (DESIGN.md 4.6.7 "Keys on the device"):
//   install    hexl_ks_set_keys_device: a device buffer in the h_keys layout of hexl_ks_set_keys ([L][2][K][n]) into every copy of the
//              keys the plan holds, each in its own order and word format                                            k_ks_install
//   generate   hexl_ks_gen_keys: the switching key from s' to s, row (d, slot) = (pt + e - a s, a) with
//              pt = [slot == d] (P mod q_i) s'_i, a = UNIFORM and e = CBD21 polynomial first + d of (seed, stream),
//              straight into the FP64 copies -- what hexl_rlwe_encrypt + download + hexl_ks_set_keys leave          k_ks_gen
// Both kernels walk the CALLER'S order: one workgroup per (key row, 1024-word piece), 256 lanes, a lane owns FOUR CONSECUTIVE words --
// exactly one UNIFORM block of the stream (sample_core.hpp), as in rlwe.hip -- computes them once and stores them into every copy at
// the position key_layout.hpp gives. Which copies exist, in which order and format, is hx_ks_key_copies (capi.hip): the list
// hexl_ks_set_keys fills on the host. In a B order the low index bits above the lane's own are thread-index bits, so the lanes of a
// wave that hold one register slot write one contiguous run.
#include "hexl_internal.hpp"
#include "ntt_core.hpp"
#include "sample_core.hpp"

using hxf::Mod;

constexpr u32 KG_THREADS = 256, KG_LOG_CHUNK = 10;
static_assert(KG_THREADS * 4 == 1u << KG_LOG_CHUNK, "a workgroup covers its piece exactly");
static_assert(KG_THREADS == HX_WW_THREADS && KG_LOG_CHUNK == HX_WW_LOG_CHUNK, "hx_ww_grid counts these workgroups");

// key row r = d (L + 1) + slot and the piece of a workgroup; the lane's first word
struct KgWhere { u32 d, slot, i, j0; };
__device__ __forceinline__ KgWhere kg_where(u32 row_piece, u32 logn, u32 L, u32 K) {
    const u32 r = row_piece >> (logn - KG_LOG_CHUNK), ch = row_piece - (r << (logn - KG_LOG_CHUNK));
    const u32 d = r / (L + 1), slot = r - d * (L + 1);
    return {d, slot, slot < L ? slot : K - 1, (ch << KG_LOG_CHUNK) + 4 * threadIdx.x};
}

struct InstallArgs {
    const KsModulus* mods;      // [K]
    const u64* keys;            // [L][2][K][n], any 64-bit words
    HxKeyCopy copies[HX_KEY_MAX_COPIES];
    u32 n_copies, logn, L, K;
};

// blockIdx.x = ((d (L + 1) + slot) 2 + k) pieces + piece: only limbs i < L and i = K - 1 are read, as on the host
__global__ __launch_bounds__(KG_THREADS) void k_ks_install(InstallArgs a) {
    const u32 k = (blockIdx.x >> (a.logn - KG_LOG_CHUNK)) & 1;
    const u32 pieces = 1u << (a.logn - KG_LOG_CHUNK), rk = blockIdx.x >> (a.logn - KG_LOG_CHUNK);
    const KgWhere w = kg_where((rk >> 1) * pieces + (blockIdx.x & (pieces - 1)), a.logn, a.L, a.K);
    const u64 q = a.mods[w.i].q;
    const u64* src = a.keys + (((size_t(w.d) * 2 + k) * a.K + w.i) << a.logn) + w.j0;
    u64 v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = src[t] % q;
    const size_t base = size_t(rk) << a.logn;                     // ((d (L + 1) + slot) 2 + k) n
    for (u32 c = 0; c < a.n_copies; ++c) {
        const HxKeyCopy cp = a.copies[c];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const u32 pos = hxk::pos_of(cp.order, w.j0 + t);
            if (cp.shoup) {
                u64* dst = static_cast<u64*>(cp.dst) + 2 * base;
                dst[pos] = v[t];
                dst[(size_t(1) << a.logn) + pos] = hx::shoup_factor(v[t], q);
            } else {
                static_cast<double*>(cp.dst)[base + pos] = hxk::centre(v[t], q);
            }
        }
    }
}

struct GenArgs {
    const KsModF64* mods;       // [K]
    const u64* e;               // [L][K][n]: NTT_i of the error of key d (plan scratch)
    const u64* s;               // [K][n]
    const u64* from;            // FROM_POLY: [K][n]
    HxKeyCopy copies[HX_KEY_MAX_COPIES];
    hxs::Seed seed;
    u64 stream, first;
    double P;                   // the special prime
    u32 n_copies, logn, L, K, g;
    int kind;
};

// blockIdx.x = (d (L + 1) + slot) pieces + piece. s' is read (or made in registers) only where the plaintext is not zero, slot == d;
// `a` never leaves the registers until it is stored as component 1.
__global__ __launch_bounds__(KG_THREADS) void k_ks_gen(GenArgs a) {
    const KgWhere w = kg_where(blockIdx.x, a.logn, a.L, a.K);
    const Mod m = a.mods[w.i].m;
    const size_t limb = size_t(w.i) << a.logn;
    const u64* pe = a.e + ((size_t(w.d) * a.K) << a.logn) + limb + w.j0;
    const u64* ps = a.s + limb + w.j0;
    double e[4], s[4], pt[4] = {0.0, 0.0, 0.0, 0.0}, u[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { e[t] = hxf::to_f64(pe[t]); s[t] = hxf::to_f64(ps[t]); }
    if (w.slot == w.d) {                                          // uniform per workgroup
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            double f;
            if (a.kind == HEXL_KEY_FROM_POLY) f = hxf::to_f64(a.from[limb + w.j0 + t]);
            else if (a.kind == HEXL_KEY_FROM_SQUARE) f = hxf::pt_mul(s[t], s[t], m);
            else f = hxf::to_f64(a.s[limb + hx::galois_src(w.j0 + t, a.logn, a.g)]);
            pt[t] = hxf::pt_mul(a.P, f, m);
        }
    }
    hxs::uniform4(u, a.seed, a.stream, a.first + w.d, w.i, a.logn, w.j0, m);
    double c0[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) c0[t] = hxs::encrypt_c0(u[t], s[t], e[t], pt[t], m);
    const size_t base = (size_t(blockIdx.x >> (a.logn - KG_LOG_CHUNK)) * 2) << a.logn;     // (d (L + 1) + slot) 2 n
    for (u32 c = 0; c < a.n_copies; ++c) {
        double* dst = static_cast<double*>(a.copies[c].dst) + base;
        const hxk::Order o = a.copies[c].order;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const u32 pos = hxk::pos_of(o, w.j0 + t);
            dst[pos] = hxk::centre_f64(c0[t], m.p);
            dst[(size_t(1) << a.logn) + pos] = hxk::centre_f64(u[t], m.p);
        }
    }
}

// ---- launchers ----
int hx_launch_ks_install(hexl_ks_plan* p, const u64* d_keys) {
    InstallArgs a{};
    a.mods = p->d_mods;
    a.keys = d_keys;
    a.n_copies = (u32)hx_ks_key_copies(p, a.copies);
    a.logn = p->logn; a.L = p->L; a.K = p->K;
    const u32 grid = (u32)hx_ww_grid(p, size_t(p->L) * (p->L + 1), 2);
    hipLaunchKernelGGL(k_ks_install, dim3(grid), dim3(KG_THREADS), 0, p->ctx->stream, a);
    return (int)hipGetLastError();
}

int hx_launch_ks_gen_keys(hexl_ks_plan* p, const u64* d_secret, int from_kind, u32 g, const u64* d_from, const u32* seed, u64 stream,
                          u64 first) {
    const size_t n = p->n, L = p->L, K = p->K;
    // the errors of the L keys at K limbs: one chunk of the encode scratch (L <= 15 instances), as hx_launch_rlwe_encrypt
    if (int rc = p->d_enc_coeffs.reserve(L * n)) return rc;
    if (int rc = p->d_enc_words.reserve(L * K * n)) return rc;
    if (int rc = hx_launch_rlwe_error(p, seed, stream, first, L, (u32)K)) return rc;
    GenArgs a{};
    a.mods = p->d_mods_f64;
    a.e = p->d_enc_words;
    a.s = d_secret;
    a.from = d_from;
    a.n_copies = (u32)hx_ks_key_copies(p, a.copies);
    for (int k = 0; k < 8; ++k) a.seed.k[k] = seed[k];
    a.stream = stream; a.first = first;
    a.P = (double)p->moduli[K - 1];
    a.logn = p->logn; a.L = p->L; a.K = p->K; a.g = g;
    a.kind = from_kind;
    hipLaunchKernelGGL(k_ks_gen, dim3((u32)hx_ww_grid(p, L, L + 1)), dim3(KG_THREADS), 0, p->ctx->stream, a);
    return (int)hipGetLastError();
}

// ---- entry points of include/hexl_mi355x.h ----
extern "C" int hexl_ks_set_keys_device(hexl_ks_plan* p, const uint64_t* d_keys) {
    if (!p || !d_keys) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    if (int rc = hx_launch_ks_install(p, d_keys)) return rc;
    p->have_keys = true;
    return 0;
}

extern "C" int hexl_ks_gen_keys(hexl_ks_plan* p, const uint64_t* d_secret, int from_kind, uint64_t galois_elt, const uint64_t* d_from,
                                const uint32_t seed[8], uint64_t stream, uint64_t first) {
    if (!d_secret || !seed || !hx_f64_plan_ok(p)) return HEXL_E_BADARG;
    if (from_kind != HEXL_KEY_FROM_POLY && from_kind != HEXL_KEY_FROM_SQUARE && from_kind != HEXL_KEY_FROM_GALOIS) return HEXL_E_BADARG;
    if (from_kind == HEXL_KEY_FROM_POLY && !d_from) return HEXL_E_BADARG;
    if (from_kind == HEXL_KEY_FROM_GALOIS && (!(galois_elt & 1) || galois_elt >= 2 * u64(p->n))) return HEXL_E_BADARG;
    if (first > hxs::MAX_INDEX || p->L > hxs::MAX_INDEX - first) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    if (int rc = hx_launch_ks_gen_keys(p, d_secret, from_kind, from_kind == HEXL_KEY_FROM_GALOIS ? (u32)galois_elt : 1u, d_from, seed, stream,
                                       first))
        return rc;
    p->have_keys = true;
    return 0;
}
