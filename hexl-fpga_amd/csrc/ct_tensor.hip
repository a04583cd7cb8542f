// ct_tensor.hip -- ciphertext x ciphertext products whose relinearisation is the caller's to place (DESIGN.md 4.6.8 "Tensor sums and
// lazy relinearisation"):
//   ct_tensor_sum               out[b][0..2][i] = sum_t (a_t0 b_t0, a_t0 b_t1 + a_t1 b_t0, a_t1 b_t1) mod q_i: up to eight pairs of
//                               two-component ciphertexts, each read once through its first n_limbs limbs          k_ct_tensor_sum
//   relinearize                 [batch][3][L][n] -> [batch][2][L][n] = (c0, c1) + KeySwitch(c2): the components are moved apart slice by
//                               slice and the keyswitch is the one hexl_keyswitch runs                             k_relin_split
//   multiply_sum_relinearize    the two in one call: the tensor kernel writes components 0-1 into the output and component 2 into the
//                               keyswitch's t_target slice, so the three-component sum never exists
// The tensor kernel is FP64 arithmetic (moduli < 2^52); k_relin_split moves words and serves every plan. Nothing here touches a keyswitch
// kernel: hx_launch_keyswitch is called as hx_launch_rotate (ckks_ops.hip) calls it, on the same slice buffer (hexl_ks_plan::d_rot_t).
#include "hexl_internal.hpp"

using hxf::Mod;

constexpr u32 TS_THREADS = 256, TS_VECS = 2;
constexpr u32 TS_LOG_CHUNK = 10;    // 1024 words of one polynomial per workgroup (the smallest ring): TS_VECS 16-byte vectors per lane
static_assert(TS_THREADS * TS_VECS * 2 == 1u << TS_LOG_CHUNK, "a workgroup covers its piece exactly");
static_assert(TS_THREADS == HX_WW_THREADS && TS_LOG_CHUNK == HX_WW_LOG_CHUNK, "hx_ww_grid counts these workgroups");
// TsArgs, the kernel's arguments, is hexl_internal.hpp's: the hybrid multiply (keyswitch_hybrid.hip) fills one too
static_assert(sizeof(TsArgs) <= 4096, "the kernel arguments of k_ct_tensor_sum must fit the 4 KiB kernarg segment");

// One workgroup per (instance, limb, piece of the polynomial), as k_pt_mul and k_ct_lincomb: the limb -- and with it the modulus -- is
// found once per workgroup (wave-uniform: scalar registers). A term is four operand polynomials (a0, a1, b0, b1), TS_VECS 16-byte vectors
// per lane each: 32 VGPRs. Eight terms would not fit, so two terms' worth are kept: every load of term t + 1 is requested before the
// first product of term t, and term t's registers take term t + 2. The three partial sums are 24 VGPRs.
// The term loop is unrolled (NT is a template argument), so the wait in front of term t's products counts the loads of term t + 1 as
// still in flight (s_waitcnt vmcnt(8)): a rolled loop merges its two ways in and waits for everything. Left to itself the scheduler
// then hoists the loads of up to all eight terms to the top (254 VGPRs at seven terms: two waves per SIMD; capped at 128 registers it
// spills), so each stage ends in a scheduling barrier: nothing moves across, and the loads stay where the source puts them.
template <int NT>
__global__ __launch_bounds__(TS_THREADS) void k_ct_tensor_sum(TsArgs s) {
    typedef unsigned long long u2 __attribute__((ext_vector_type(2)));
    const u32 bi = blockIdx.x >> (s.logn - TS_LOG_CHUNK), ch = blockIdx.x - (bi << (s.logn - TS_LOG_CHUNK));
    const u32 b = bi / s.L, i = bi - b * s.L;
    const Mod m = s.mods[i].m;
    const size_t n = size_t(1) << s.logn, piece = size_t(ch) << TS_LOG_CHUNK;
    u2 w[2][4][TS_VECS];                                          // [slot][a0, a1, b0, b1][vector]
    // A lane takes TS_VECS ADJACENT vectors of every polynomial -- the same words of all of them, which is all a word-wise kernel needs --
    // so every address is a wave-uniform base (scalar registers) plus ONE 32-bit lane offset plus an immediate: no address lives in
    // vector registers (with the vectors a workgroup-width apart, as in k_pt_mul, the 4096-byte step does not fit the immediate and
    // each load of the second vector costs a 64-bit address pair, computed early and kept)
    const u32 lane = threadIdx.x * TS_VECS * (u32)sizeof(u2);
    auto at = [&](const u64* base, u32 j) { return reinterpret_cast<const char*>(base) + lane + j * (u32)sizeof(u2); };
    auto vec = [&](const u64* base, u32 j) { return *reinterpret_cast<const u2*>(at(base, j)); };
    auto load = [&](int t, int slot) {
        const u64* pa = s.a[t] + (size_t(b) * 2 * s.la[t] + i) * n + piece;
        const u64* pb = s.b[t] + (size_t(b) * 2 * s.lb[t] + i) * n + piece;
        const u64* pa1 = pa + size_t(s.la[t]) * n;                // the second component
        const u64* pb1 = pb + size_t(s.lb[t]) * n;
#pragma unroll
        for (u32 j = 0; j < TS_VECS; ++j) {
            w[slot][0][j] = vec(pa, j);
            w[slot][1][j] = vec(pa1, j);
            w[slot][2][j] = vec(pb, j);
            w[slot][3][j] = vec(pb1, j);
        }
    };
    double d[3][TS_VECS][2];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (u32 j = 0; j < TS_VECS; ++j) d[k][j][0] = d[k][j][1] = 0.0;
    auto word = [&](double* d0, double* d1, double* d2, u64 wa0, u64 wa1, u64 wb0, u64 wb1) {
        const double a0 = hxf::ts_operand(hxf::to_f64(wa0), m), a1 = hxf::ts_operand(hxf::to_f64(wa1), m);
        const double b0 = hxf::ts_operand(hxf::to_f64(wb0), m), b1 = hxf::ts_operand(hxf::to_f64(wb1), m);
        *d0 = hxf::ts_mac(*d0, a0, b0, m);
        *d1 = hxf::ts_mac(hxf::ts_mac(*d1, a0, b1, m), a1, b0, m);
        *d2 = hxf::ts_mac(*d2, a1, b1, m);
    };
    load(0, 0);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t + 1 < NT) load(t + 1, (t + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
        const int c = t & 1;
#pragma unroll
        for (u32 j = 0; j < TS_VECS; ++j) {
            word(&d[0][j][0], &d[1][j][0], &d[2][j][0], w[c][0][j].x, w[c][1][j].x, w[c][2][j].x, w[c][3][j].x);
            word(&d[0][j][1], &d[1][j][1], &d[2][j][1], w[c][0][j].y, w[c][1][j].y, w[c][2][j].y, w[c][3][j].y);
        }
        // the partial sums pass through an empty volatile statement: it is ordered with the loads and the barriers, so the
        // accumulation of term t ends here (instruction selection otherwise sinks the additions of all terms to the end of the
        // kernel and keeps every term's products alive until then: 16 VGPRs per term)
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (u32 j = 0; j < TS_VECS; ++j) {
                asm volatile("" : "+v"(d[k][j][0]));
                asm volatile("" : "+v"(d[k][j][1]));
            }
        __builtin_amdgcn_sched_barrier(0);
    }
    const size_t within = size_t(i) * n + piece;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        u64* poly = k < 2 ? s.out01 + size_t(b) * s.stride01 + size_t(k) * s.L * n + within : s.out2 + size_t(b) * s.stride2 + within;
#pragma unroll
        for (u32 j = 0; j < TS_VECS; ++j) {
            u2 o;
            o.x = hxf::from_f64(hxf::ts_finish(d[k][j][0], m));
            o.y = hxf::from_f64(hxf::ts_finish(d[k][j][1], m));
            *reinterpret_cast<u2*>(const_cast<char*>(at(poly, j))) = o;
        }
    }
}

// nb instances: `s` with its operand and output pointers at the first of them
int hx_launch_tensor(hexl_ks_plan* p, const TsArgs& s, size_t nb) {
    const dim3 grid((u32)hx_ww_grid(p, nb, s.L)), block(TS_THREADS);
    hipStream_t st = p->ctx->stream;
    switch (s.n_terms) {
        case 1: hipLaunchKernelGGL(k_ct_tensor_sum<1>, grid, block, 0, st, s); break;
        case 2: hipLaunchKernelGGL(k_ct_tensor_sum<2>, grid, block, 0, st, s); break;
        case 3: hipLaunchKernelGGL(k_ct_tensor_sum<3>, grid, block, 0, st, s); break;
        case 4: hipLaunchKernelGGL(k_ct_tensor_sum<4>, grid, block, 0, st, s); break;
        case 5: hipLaunchKernelGGL(k_ct_tensor_sum<5>, grid, block, 0, st, s); break;
        case 6: hipLaunchKernelGGL(k_ct_tensor_sum<6>, grid, block, 0, st, s); break;
        case 7: hipLaunchKernelGGL(k_ct_tensor_sum<7>, grid, block, 0, st, s); break;
        default: hipLaunchKernelGGL(k_ct_tensor_sum<8>, grid, block, 0, st, s); break;
    }
    return (int)hipGetLastError();
}

// ---- relinearize: the components of a slice moved apart ----
struct RelinSplitArgs {
    const u64* ct3;             // [nb][3][L][n]
    u64* out;                   // [nb][2][L][n] = components 0-1
    u64* t;                     // [nb][L][n]    = component 2
    u32 logn, L;
};

// One workgroup per (instance, row of the 3 L, piece): words are moved, never interpreted, so integer-kernel plans are served too.
__global__ __launch_bounds__(TS_THREADS) void k_relin_split(RelinSplitArgs a) {
    typedef unsigned long long u2 __attribute__((ext_vector_type(2)));
    const u32 br = blockIdx.x >> (a.logn - TS_LOG_CHUNK), ch = blockIdx.x - (br << (a.logn - TS_LOG_CHUNK));
    const u32 b = br / (3 * a.L), r = br - b * 3 * a.L;          // r = k L + i
    const size_t n = size_t(1) << a.logn, piece = size_t(ch) << TS_LOG_CHUNK;
    const u2* src = reinterpret_cast<const u2*>(a.ct3 + (size_t(b) * 3 * a.L + r) * n + piece);
    u64* row = r < 2 * a.L ? a.out + (size_t(b) * 2 * a.L + r) * n : a.t + (size_t(b) * a.L + (r - 2 * a.L)) * n;
    u2 v[TS_VECS];
#pragma unroll
    for (u32 j = 0; j < TS_VECS; ++j) v[j] = src[threadIdx.x + j * TS_THREADS];
#pragma unroll
    for (u32 j = 0; j < TS_VECS; ++j) reinterpret_cast<u2*>(row + piece)[threadIdx.x + j * TS_THREADS] = v[j];
}

// The slice loop of hx_launch_rotate (ckks_ops.hip): fill(b0, nb, out, t) writes components 0-1 of instances b0 ... b0 + nb - 1 to `out`
// and their component 2 to the plan's slice buffer `t`; the keyswitch then accumulates into `out`. hx_launch_keyswitch joins its lanes
// back into the caller's stream before it returns (keyswitch.hip), so the next slice's fill of the same t buffer runs after this
// keyswitch has read it.
template <class F>
static int relin_slices(hexl_ks_plan* p, u64* d_out, size_t batch, F fill) {
    const size_t n = p->n, L = p->L;
    const size_t slice = hx_ks_chunk_of(p, batch);
    if (int rc = p->d_rot_t.reserve(slice * L * n)) return rc;
    return hx_for_chunks(batch, slice, [&](size_t b0, size_t nb) {
        u64* out = d_out + b0 * 2 * L * n;
        if (int rc = fill(b0, nb, out, (u64*)p->d_rot_t)) return rc;
        return hx_launch_keyswitch(p, out, p->d_rot_t, nb, 7, nullptr);
    });
}

// ---- entry points of include/hexl_mi355x.h (beside their launchers, as in ckks_ops.hip and rns_ops.hip: the CPU staging model needs no
// stubs for them) ----
// The operands of a tensor sum, checked and laid into `s` (pointers at instance 0): HEXL_E_BADARG for a null entry, a limb count outside
// n_limbs ... K, or an operand that shares a byte with [d_out, d_out + out_bytes) -- the layouts differ, so there is no in-place form.
int hx_tensor_operands(const hexl_ks_plan* p, const u64* const* d_as, const u64* const* d_bs, const u64* in_limbs, size_t n_terms,
                       size_t batch, u64 n_limbs, const u64* d_out, size_t out_bytes, TsArgs& s) {
    const size_t poly = size_t(p->n) * sizeof(u64);
    for (size_t t = 0; t < n_terms; ++t) {
        const u64 la = in_limbs ? in_limbs[2 * t] : n_limbs, lb = in_limbs ? in_limbs[2 * t + 1] : n_limbs;
        if (!d_as[t] || !d_bs[t] || !hx_in_range(la, n_limbs, p->K) || !hx_in_range(lb, n_limbs, p->K)) return HEXL_E_BADARG;
        if (hx_ranges_overlap(d_out, out_bytes, d_as[t], batch * 2 * size_t(la) * poly) ||
            hx_ranges_overlap(d_out, out_bytes, d_bs[t], batch * 2 * size_t(lb) * poly)) return HEXL_E_BADARG;
        s.a[t] = d_as[t];
        s.b[t] = d_bs[t];
        s.la[t] = (u32)la;
        s.lb[t] = (u32)lb;
    }
    s.mods = p->d_mods_f64;
    s.logn = p->logn;
    s.L = (u32)n_limbs;
    s.n_terms = (u32)n_terms;
    return 0;
}

extern "C" int hexl_ct_tensor_sum(hexl_ks_plan* p, uint64_t* d_out, const uint64_t* const* d_as, const uint64_t* const* d_bs,
                                  const uint64_t* in_limbs, size_t n_terms, size_t batch, uint64_t n_limbs) {
    if (!p || !d_out || !d_as || !d_bs || !hx_in_range(n_terms, 1, TS_MAX_TERMS) || !hx_f64_plan_ok(p, n_limbs, 1, p->K) ||
        n_limbs > TS_MAX_LIMBS)
        return HEXL_E_BADARG;
    // the largest operand has K limbs: if that size fits, every other one does
    size_t bytes, out_bytes;
    if (!hx_words_bytes(batch, 2, p->K, p->n, &bytes) || !hx_words_bytes(batch, 3, n_limbs, p->n, &out_bytes) ||
        !hx_ww_grid_ok(p, batch, n_limbs))
        return HEXL_E_BADARG;
    TsArgs s{};
    if (int rc = hx_tensor_operands(p, d_as, d_bs, in_limbs, n_terms, batch, n_limbs, d_out, out_bytes, s)) return rc;
    if (!batch) return 0;
    s.out01 = d_out;
    s.out2 = d_out + 2 * size_t(n_limbs) * p->n;
    s.stride01 = s.stride2 = 3ull * n_limbs * p->n;
    HX_CHECK(hipSetDevice(p->ctx->device));
    return hx_launch_tensor(p, s, batch);
}

extern "C" int hexl_relinearize(hexl_ks_plan* p, uint64_t* d_out, const uint64_t* d_ct3, size_t batch) {
    if (!p || !d_out || !d_ct3) return HEXL_E_BADARG;
    size_t in_bytes;
    if (!hx_words_bytes(batch, 3, p->L, p->n, &in_bytes)) return HEXL_E_BADARG;
    if (hx_ranges_overlap(d_out, in_bytes / 3 * 2, d_ct3, in_bytes)) return HEXL_E_BADARG;
    if (!p->have_keys) return HEXL_E_NOKEYS;
    if (!batch) return 0;
    if (!hx_ww_grid_ok(p, hx_ks_chunk_of(p, batch), 3 * u64(p->L))) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    const size_t n = p->n, L = p->L;
    return relin_slices(p, d_out, batch, [&](size_t b0, size_t nb, u64* out, u64* t) {
        const RelinSplitArgs a{d_ct3 + b0 * 3 * L * n, out, t, p->logn, (u32)L};
        hipLaunchKernelGGL(k_relin_split, dim3((u32)hx_ww_grid(p, nb, 3 * L)), dim3(TS_THREADS), 0, p->ctx->stream, a);
        return (int)hipGetLastError();
    });
}

extern "C" int hexl_multiply_sum_relinearize(hexl_ks_plan* p, uint64_t* d_out, const uint64_t* const* d_as, const uint64_t* const* d_bs,
                                             const uint64_t* in_limbs, size_t n_terms, size_t batch) {
    if (!p || !d_out || !d_as || !d_bs || !hx_in_range(n_terms, 1, TS_MAX_TERMS) || !hx_f64_plan_ok(p, p->L, 1, TS_MAX_LIMBS))
        return HEXL_E_BADARG;
    size_t bytes, out_bytes;
    if (!hx_words_bytes(batch, 2, p->K, p->n, &bytes) || !hx_words_bytes(batch, 2, p->L, p->n, &out_bytes) ||
        !hx_ww_grid_ok(p, hx_ks_chunk_of(p, batch), p->L))
        return HEXL_E_BADARG;
    TsArgs s{};
    if (int rc = hx_tensor_operands(p, d_as, d_bs, in_limbs, n_terms, batch, p->L, d_out, out_bytes, s)) return rc;
    if (!p->have_keys) return HEXL_E_NOKEYS;
    if (!batch) return 0;
    HX_CHECK(hipSetDevice(p->ctx->device));
    const size_t n = p->n, L = p->L;
    s.stride01 = 2 * L * n;
    s.stride2 = L * n;
    return relin_slices(p, d_out, batch, [&](size_t b0, size_t nb, u64* out, u64* t) {
        TsArgs c = s;
        for (size_t k = 0; k < n_terms; ++k) {
            c.a[k] += b0 * 2 * c.la[k] * n;
            c.b[k] += b0 * 2 * c.lb[k] * n;
        }
        c.out01 = out;
        c.out2 = t;
        return hx_launch_tensor(p, c, nb);
    });
}
