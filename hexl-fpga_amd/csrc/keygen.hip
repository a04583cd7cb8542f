// keygen.hip -- switching keys that never leave the device (DESIGN.md 4.6.7 "Keys on the device"):
//   install    hexl_ks_set_keys_device: a device buffer in the h_keys layout of hexl_ks_set_keys ([L][2][K][n]) into every copy of the
//              keys the plan holds, each in its own order and word format                                            k_ks_install
//   generate   hexl_ks_gen_keys: the switching key from s' to s, row (d, slot) = (pt + e - a s, a) with
//              pt = [slot == d] (P mod q_i) s'_i, a = UNIFORM and e = CBD21 polynomial first + d of (seed, stream),
//              straight into the FP64 copies -- what hexl_rlwe_encrypt + download + hexl_ks_set_keys leave          k_ks_gen
//   hybrid     hexl_hks_keygen: one switching key per hybrid object (keyswitch_hybrid.hip) of ONE plan, row (r, d) = (pt + e - a s, a)
//              with pt = [i in G_d] (P mod q_i) s'_(r,i), a and e polynomial first + (rows of the keys before r) + d, straight into
//              each object's centred doubles -- what gen_hybrid_key + hexl_hks_set_keys_device leave  k_hks_gen
// The kernels walk the CALLER'S order: one workgroup per (key row, 1024-word piece), 256 lanes, a lane owns FOUR CONSECUTIVE words --
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

// hexl_hks_keygen: the keys of one call. Key r owns the rows row0 ... row0 + dnum - 1 of the call (row0 = the dnum of the keys before
// it), and row `row` draws polynomial first + row: neither the split of a set into calls nor the split of a call's rows into chunks of
// the encode scratch changes a word.
constexpr u32 HKG_MAX_KEYS = 64;                                  // HEXL_HKS_KEYGEN_MAX_KEYS of the header
static_assert(HKG_MAX_KEYS == HEXL_HKS_KEYGEN_MAX_KEYS, "the header documents this limit");
struct HkgKey {
    double* dst;                // the object's d_keys, [dnum][2][K][n]
    const u64* from;            // FROM_POLY: [K][n]
    u32 g, row0;
    uint16_t alpha, dnum;
    int kind;
};
struct HkgArgs {
    const KsModF64* mods;       // [K]
    const u64* e;               // [nb][K][n]: NTT_i of the error of the chunk's row (plan scratch)
    const u64* s;               // [K][n]
    hxs::Seed seed;
    u64 stream, first;
    double p_mod[16];           // P mod q_i, canonical
    u32 logn, L, K, n_keys, chunk_row0;
    HkgKey keys[HKG_MAX_KEYS];
};
static_assert(sizeof(HkgArgs) <= 4096, "the descriptors travel by value in the kernel arguments");

// blockIdx.x = ((row - chunk_row0) K + i) pieces + piece. s' is read (or made in registers) only where the plaintext is not zero, i in
// G_d; c0 and `a` go to [(d 2 + k) K + i][j] of the key's object as centred doubles, a lane's four as two 16-byte stores each.
__global__ __launch_bounds__(KG_THREADS) void k_hks_gen(HkgArgs a) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    const u32 lp = a.logn - KG_LOG_CHUNK;
    const u32 ri = blockIdx.x >> lp, piece = blockIdx.x - (ri << lp);
    const u32 lrow = ri / a.K, i = ri - lrow * a.K, row = a.chunk_row0 + lrow;
    u32 r = 0;
    while (r + 1 < a.n_keys && a.keys[r + 1].row0 <= row) ++r;   // uniform per workgroup
    const HkgKey key = a.keys[r];
    const u32 d = row - key.row0, j0 = (piece << KG_LOG_CHUNK) + 4 * threadIdx.x;
    const Mod m = a.mods[i].m;
    const size_t limb = size_t(i) << a.logn;
    const u64* pe = a.e + ((size_t(lrow) * a.K) << a.logn) + limb + j0;
    const u64* ps = a.s + limb + j0;
    double e[4], s[4], pt[4] = {0.0, 0.0, 0.0, 0.0}, u[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { e[t] = hxf::to_f64(pe[t]); s[t] = hxf::to_f64(ps[t]); }
    const u32 lo = d * key.alpha, hi = lo + key.alpha < a.L ? lo + key.alpha : a.L;
    if (i >= lo && i < hi) {                                      // uniform per workgroup
        const double P = a.p_mod[i];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            double f;
            if (key.kind == HEXL_KEY_FROM_POLY) f = hxf::to_f64(key.from[limb + j0 + t]);
            else if (key.kind == HEXL_KEY_FROM_SQUARE) f = hxf::pt_mul(s[t], s[t], m);
            else f = hxf::to_f64(a.s[limb + hx::galois_src(j0 + t, a.logn, key.g)]);
            pt[t] = hxf::pt_mul(P, f, m);
        }
    }
    hxs::uniform4(u, a.seed, a.stream, a.first + row, i, a.logn, j0, m);
    double c0[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { c0[t] = hxk::centre_f64(hxs::encrypt_c0(u[t], s[t], e[t], pt[t], m), m.p); u[t] = hxk::centre_f64(u[t], m.p); }
    double* dst = key.dst + (((size_t(d) * 2) * a.K + i) << a.logn) + j0;
    double* dst1 = dst + (size_t(a.K) << a.logn);
    *reinterpret_cast<d2*>(dst) = d2{c0[0], c0[1]};
    *reinterpret_cast<d2*>(dst + 2) = d2{c0[2], c0[3]};
    *reinterpret_cast<d2*>(dst1) = d2{u[0], u[1]};
    *reinterpret_cast<d2*>(dst1 + 2) = d2{u[2], u[3]};
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

// rows of hexl_hks_keygen per chunk of the encode scratch: hx_enc_chunk, or HEXL_HKS_KEYGEN_CHUNK below it (tests; read once per process)
static size_t hkg_chunk(const hexl_ks_plan* p, size_t rows) {
    static const long knob = hx_knob("HEXL_HKS_KEYGEN_CHUNK", 0);
    const size_t chunk = hx_enc_chunk_of(p, rows);
    return knob > 0 && size_t(knob) < chunk ? size_t(knob) : chunk;
}

extern "C" int hexl_hks_keygen(hexl_hks* const* hks, size_t n_keys, const int* from_kinds, const uint64_t* galois_elts,
                               const uint64_t* const* d_froms, const uint64_t* d_secret, const uint32_t seed[8], uint64_t stream,
                               uint64_t first) {
    if (!hks || !from_kinds || !d_secret || !seed || n_keys == 0 || n_keys > HKG_MAX_KEYS) return HEXL_E_BADARG;
    HkgArgs a{};
    hexl_ks_plan* p = nullptr;
    u64 rows = 0;
    for (size_t r = 0; r < n_keys; ++r) {
        if (!hks[r]) return HEXL_E_BADARG;
        for (size_t o = 0; o < r; ++o)
            if (hks[o] == hks[r]) return HEXL_E_BADARG;
        const HxHksKeys k = hx_hks_keys(hks[r]);
        if (r == 0) p = k.plan;
        if (k.plan != p || !hx_f64_plan_ok(p)) return HEXL_E_BADARG;
        const int kind = from_kinds[r];
        if (kind != HEXL_KEY_FROM_POLY && kind != HEXL_KEY_FROM_SQUARE && kind != HEXL_KEY_FROM_GALOIS) return HEXL_E_BADARG;
        if (kind == HEXL_KEY_FROM_POLY && (!d_froms || !d_froms[r])) return HEXL_E_BADARG;
        if (kind == HEXL_KEY_FROM_GALOIS && (!galois_elts || !(galois_elts[r] & 1) || galois_elts[r] >= 2 * u64(p->n))) return HEXL_E_BADARG;
        a.keys[r] = HkgKey{k.d_keys, kind == HEXL_KEY_FROM_POLY ? d_froms[r] : nullptr, kind == HEXL_KEY_FROM_GALOIS ? (u32)galois_elts[r] : 1u,
                           (u32)rows, (uint16_t)k.alpha, (uint16_t)k.dnum, kind};
        rows += k.dnum;
    }
    if (first > hxs::MAX_INDEX || rows > hxs::MAX_INDEX - first) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    const size_t n = p->n, K = p->K, chunk = hkg_chunk(p, rows);
    if (int rc = p->d_enc_coeffs.reserve(chunk * n)) return rc;
    if (int rc = p->d_enc_words.reserve(chunk * K * n)) return rc;
    a.mods = p->d_mods_f64;
    a.e = p->d_enc_words;
    a.s = d_secret;
    for (int k = 0; k < 8; ++k) a.seed.k[k] = seed[k];
    a.stream = stream; a.first = first;
    const double* p_mod = hx_hks_keys(hks[0]).p_mod;              // one plan: the same for every object
    for (size_t i = 0; i < K; ++i) a.p_mod[i] = p_mod[i];
    a.logn = p->logn; a.L = p->L; a.K = p->K; a.n_keys = (u32)n_keys;
    if (int rc = hx_for_chunks(rows, chunk, [&](size_t c0, size_t nb) {
            if (int rc = hx_launch_rlwe_error(p, seed, stream, first + c0, nb, (u32)K)) return rc;
            a.chunk_row0 = (u32)c0;
            hipLaunchKernelGGL(k_hks_gen, dim3((u32)hx_ww_grid(p, nb, K)), dim3(KG_THREADS), 0, p->ctx->stream, a);
            return (int)hipGetLastError();
        }))
        return rc;
    for (size_t r = 0; r < n_keys; ++r) hx_hks_set_keyed(hks[r]);
    return 0;
}
