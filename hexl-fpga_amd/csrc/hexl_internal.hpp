// hexl_internal.hpp -- host-side state shared by the launcher translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/hexl_mi355x.h"
#include "f64_arith.hpp"
#include "key_layout.hpp"

typedef uint64_t u64;
typedef uint32_t u32;
typedef unsigned __int128 u128;

#define HX_CHECK(expr)                                                                       \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            fprintf(stderr, "[hexl_mi355x] %s failed: %s (%s:%d)\n", #expr,                  \
                    hipGetErrorString(_e), __FILE__, __LINE__);                              \
            return (int)_e;                                                                  \
        }                                                                                    \
    } while (0)

// The > 64 KiB dynamic-LDS opt-in of a set of kernels, the first time their launcher runs on a device: hipFuncSetAttribute applies
// to the CURRENT device's copy of a kernel, and the launchers may run on one host thread per device (NUM_DEV > 1), so every set of
// kernels (= every instantiation of this function) keeps its own per-device "done" bits behind a mutex.
template <auto... Kernels>
int hx_lds_optin(int device, size_t bytes) {
    static std::mutex m;
    static uint64_t done = 0;
    std::lock_guard<std::mutex> g(m);
    const uint64_t bit = 1ull << (device & 63);
    if (done & bit) return 0;
    for (const void* k : {(const void*)Kernels...})
        HX_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done |= bit;
    return 0;
}

// ---- environment knobs: one parser; a knob read in more than one place has one accessor here. A `static` in an
// accessor = read once per process; the others are read by every call (of hexl_ks_plan_create, of a launcher).
constexpr long HX_KNOB_UNSET = LONG_MIN;
inline long hx_knob(const char* name, long dflt) {
    const char* e = getenv(name);
    return e ? atol(e) : dflt;
}
// HEXL_KS_PER_LIMB: 0 = the plan-wide tier for every limb (read per plan); 2 = the (b, d)-major and the latency kernels look the tier
// up per transform for every batch (tests; read once per process)
inline int hx_knob_ks_per_limb() { return (int)hx_knob("HEXL_KS_PER_LIMB", 1); }
// HEXL_KS_LAT: 0 = no lone-keyswitch path, 1 = the three-kernel path of keyswitch_f64.hip for every batch of that pipeline, 2 = the
// quarter-transform path of keyswitch_lat.hip for every batch that fits a scratch chunk (tests)
inline int hx_knob_ks_lat() { static const int v = (int)hx_knob("HEXL_KS_LAT", -1); return v; }
// HEXL_KS_PIPE: 1 = FP64 plans keep the (b, d)-major pipeline and integer plans run the first-generation kernels, 3 = the slot-major
// pipeline for every batch (tests, comparisons)
inline int hx_knob_ks_pipe() { static const int v = (int)hx_knob("HEXL_KS_PIPE", 2); return v; }
// HEXL_KS_FUSE: bit 0 clear = the (b, d)-major pipeline runs steps 1-2 as one transform per workgroup even for large batches
inline int hx_knob_ks_fuse() { static const int v = (int)hx_knob("HEXL_KS_FUSE", 1); return v; }

// ---- owned device / pinned memory (DESIGN.md 4.7 "Host scaffold"). HxBuf<T> is one grow-only allocation of `capacity()` elements that
// releases itself with its owner; HOST_FLAGS < 0: device memory (HxDevBuf), else pinned host memory of those hipHostMalloc flags
// (HxPinBuf). The drain rule is fixed at construction: before a grown buffer's old memory is released, everything that may still use
// it has to finish -- the stream of the context given, or the whole device when there is none (a plan's buffers: lanes on the plan's
// auxiliary streams use them). The destructor does NOT wait: hexl_ctx_destroy / hexl_ks_plan_destroy synchronise first.
struct hexl_ctx;
inline int hx_drain(hexl_ctx* ctx);
template <class T, int HOST_FLAGS = -1>
class HxBuf {
public:
    explicit HxBuf(hexl_ctx* drain = nullptr) : drain_(drain) {}
    HxBuf(const HxBuf&) = delete;
    HxBuf& operator=(const HxBuf&) = delete;
    ~HxBuf() { release(); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t capacity() const { return cap_; }
    // room for `count` elements; contents are NOT kept when the buffer grows
    int reserve(size_t count) {
        if (cap_ >= count) return 0;
        if (p_) {
            if (int rc = hx_drain(drain_)) return rc;
            HX_CHECK(free_mem(p_));
            p_ = nullptr; cap_ = 0;
        }
        HX_CHECK(alloc_mem((void**)&p_, count * sizeof(T)));
        cap_ = count;
        return 0;
    }
    // an allocate-once table: `count` elements copied from the host at the first call (later calls do nothing); a failure leaves it empty
    int upload_once(const T* host, size_t count) {
        if (p_) return 0;
        if (int rc = reserve(count)) return rc;
        const hipError_t e = hipMemcpy(p_, host, count * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) release();
        return (int)e;
    }
    void release() {
        if (p_) (void)free_mem(p_);
        p_ = nullptr; cap_ = 0;
    }

private:
    static hipError_t alloc_mem(void** p, size_t bytes) {
        if constexpr (HOST_FLAGS < 0) return hipMalloc(p, bytes);
        else return hipHostMalloc(p, bytes, (unsigned)HOST_FLAGS);
    }
    static hipError_t free_mem(void* p) {
        if constexpr (HOST_FLAGS < 0) return hipFree(p);
        else return hipHostFree(p);
    }
    T* p_ = nullptr;
    size_t cap_ = 0;
    hexl_ctx* drain_;
};
template <class T> using HxDevBuf = HxBuf<T>;
template <class T, int HOST_FLAGS = (int)hipHostMallocDefault> using HxPinBuf = HxBuf<T, HOST_FLAGS>;

struct hexl_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;      // stream launches go to (own or caller's)
    hipEvent_t ev_switch = nullptr;    // orders a new stream behind the previous one (capi.hip switch_stream; created at the first switch)
    int num_cu = 0;
    // grow-only device scratch + pinned staging used by the *_host entry points
    HxDevBuf<char> d_stage{this};
    HxDevBuf<char> d_shared{this};                          // small shared arrays of device-resident callers
    HxPinBuf<char> h_stage{this};
    // COHERENT (fine-grained) pinned slabs of the zero-copy lone keyswitch, whose host side reads result limbs the RUNNING kernel has just
    // published (host_staging.hip keyswitch_host_lone). The staging pipeline's slabs stay default: with coherent ones its copy-engine
    // transfers ran a third slower (worksize 128: 13.4 k against 21 k keyswitch/s through the C++ API)
    HxPinBuf<char, (int)hipHostMallocCoherent> h_lone{this};
    uint32_t lone_epoch = 0;                                // zero-copy lone keyswitches so far (their completion words carry it)
    // host-pointer pipeline: copy streams + events (created lazily), see run_pipeline() in host_staging.hip
    hipStream_t s_up = nullptr, s_down = nullptr;
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_comp[2] = {nullptr, nullptr}, ev_down[2] = {nullptr, nullptr};
    HxDevBuf<char> d_meta{this};                            // dyadic per-(item,modulus) constants
    HxDevBuf<u32> d_ntt_redo{this};                         // N = 32768 standalone NTT: polynomials left to the integer butterflies (ntt.hip k_ntt_redo_*)
    HxDevBuf<char> d_ntt_tab{this};                         // standalone NTT fast path: violation counters + derived double tables
    uint32_t ntt_seq = 0;                                   // launches so far (selects the violation counter)
    // "these tables are not Shoup tables" hints from the fast-path kernels to the host (ntt.hip NttHint): four pinned words
    HxPinBuf<unsigned long long, (int)hipHostMallocMapped> h_ntt_hint{this};
    unsigned long long* d_ntt_hint = nullptr;               // the device's address of h_ntt_hint
    char name[256] = {0};
};

inline int hx_drain(hexl_ctx* ctx) {
    HX_CHECK(ctx ? hipStreamSynchronize(ctx->stream) : hipDeviceSynchronize());
    return 0;
}
void hx_pin_own_thread();    // a host thread of the library (copy pool, unpack lane) asks for the NUMA node of the devices in use (capi.hip)
// ring dimensions: 1024..16384 as the reference (keyswitch) / 16384 (NTT); 32768 is beyond its envelope
inline bool hx_supported_ntt_n(u64 n) { return n == 1024 || n == 2048 || n == 4096 || n == 8192 || n == 16384 || n == 32768; }

// per-modulus constants of a keyswitch plan (device copy is an array of K of these)
struct KsModulus {
    u64 q;          // modulus
    u64 qbarr;      // floor(2^64/q)                      (fpga.cpp:1053)
    u64 inv_n, inv_n_p;       // n^-1 mod q and its Shoup factor (fpga.cpp:1070-1089)
    u64 inv_n_w, inv_n_w_p;   // n^-1 * W_last and its Shoup factor
    u64 msf, msf_p;           // modswitch factor reduced mod q (fpga.cpp:1057-1061) + Shoup factor
    u64 fix;        // q - (floor(q_sp/2) mod q)          (intt2_redu.hpp:31-32)
    u64 half;       // floor(q_sp/2)                      (intt2_redu.hpp:25)
    u64 len;        // floor(log2 q) - 1                  (128->64 Barrett, as fpga.cpp:366-373)
    u64 barr_lo;    // floor(2^(len+64)/q)
};

// the same constants for the FP64 path (keyswitch_f64.hip); residues centred, *_p = fl(value / p)
struct KsModF64 {
    hxf::Mod m;
    hxf::InvScale sc;
    double msf, msf_p;   // modswitch factor
    double fix;          // q - (floor(q_sp/2) mod q), in [1, q]
    double half;         // floor(q_sp/2)
};

// per-level constants of the rescale that drops limb l (ckks_ops.hip), one per limb i < l; residues centred, *_p = fl(value / p)
struct KsRescaleF64 {
    double fix;          // q_i - (floor(q_l/2) mod q_i), in [1, q_i]
    double qlinv, qlinv_p;   // q_l^-1 mod q_i
    double half;         // floor(q_l/2)
};

// lanes (auxiliary streams) the chunks of one keyswitch call alternate between: 2 in production; HEXL_KS_LANES=3|4 is the
// experiment that bounds what a single launch per chunk could gain (tools/experiments/README.md, round 4)
constexpr int HX_KS_MAX_LANES = 4;
int hx_ks_lanes();

struct hexl_ks_plan {
    hexl_ctx* ctx = nullptr;
    u32 n = 0, logn = 0, L = 0, K = 0, rns = 0;
    std::vector<u64> moduli;
    // device memory of the plan: every buffer is an HxDevBuf (the plan-wide drain rule: the whole device) and goes with the plan
    HxDevBuf<KsModulus> d_mods;       // [K]
    HxDevBuf<u64> d_tables;           // [K][4][n]: roots, precon, inv_roots(HEXL idx), inv_precon
    HxDevBuf<u64> d_keys;             // [L][L+1][2][n] in forward-output ("B") order
    u32 int_loge = 5;                 // elements-per-thread exponent of the integer kernels (fixes that B order)
    bool have_keys = false;
    // FP64 path (all moduli < 2^52): same tables / keys as centred doubles
    bool use_f64 = false;
    int f64_lazy = 0;                 // forward reduction period of the lazy kernels (3, 6, 12 by modulus size); 0 = strict -- the tier every
                                      // modulus of the plan admits (chosen from the LARGEST one)
    // Per-limb arithmetic tier (round 5): a transform runs modulo ONE q_i, so its reduction period depends on that modulus alone, as
    // every NTT engine of the reference runs on its own modulus (device/keyswitch/ntt_core.hpp:285-291, ntt1.hpp:107-128).
    // tier[i] = forward reduction period for limb i (0 = strict); `mixed` = some limb the plan uses admits a longer period than f64_lazy
    // (e.g. bridge-seal's chain 52,30,30,40,27,27,27: one strict limb, six at period 12). HEXL_KS_PER_LIMB=0 keeps the plan-wide tier.
    unsigned char tier[16] = {};
    bool mixed = false;
    u32 f64_loge = 4;                 // elements-per-thread exponent of the FP64 kernels (fixes the keys' B order)
    HxDevBuf<KsModF64> d_mods_f64;    // [K]
    HxDevBuf<double> d_tables_f64;    // [K][4][n]
    HxDevBuf<double> d_keys_f64;      // [L][L+1][2][n]
    HxDevBuf<double> d_keys_x;        // the same keys in the B order of the slot-major pipeline's geometry (keyswitch_x.hip)
    u32 x_loge = 5;                   // ... whose elements-per-thread exponent this is
    // scratch for `cap` keyswitches per lane; two lanes (aux streams) work on alternating chunks so that kernels
    // of different kinds -- FP64-bound transforms and the HBM-bound multiply-accumulate -- share the chip and one
    // chunk's ragged last wave of workgroups is filled by the other's
    HxDevBuf<u64> d_scratch;          // [lanes][cap * scratch_words * n] (grow-only: hx_ks_reserve_scratch)
    size_t cap = 0;                   // instances per lane d_scratch has room for
    hipStream_t aux[HX_KS_MAX_LANES] = {};
    hipEvent_t ev_start = nullptr, ev_done[HX_KS_MAX_LANES] = {};
    HxDevBuf<u32> d_flag;             // two device words + their pinned host mirrors: [0] the kernels' input-range flag (HEXL_W_RANGE), [1] HEXL_KS_VALIDATE's (HEXL_E_RANGE)
    HxPinBuf<u32> h_flag;
    HxDevBuf<double> d_keys_nat;      // N = 16384 FP64 plans: the keys as centred doubles in NATURAL order (latency path, keyswitch_lat.hip)
    bool x_skip = false;              // slot-major lazy kernels: moduli within LAZY_SKIP_MAX_RATIO of each other -> c_d and s' enter the
                                      // transforms without a range reduction (keyswitch_x.hip SKIP variants; HEXL_KSX_SKIP=0 turns it off)
    bool overwrite_result = false;    // host-pointer path, (b, d)-major FP64 kernels: write `result` instead of accumulating into it
    // zero-copy lone keyswitch of the host-pointer entry point (host_staging.hip keyswitch_host_lone; set around ONE launch, else null):
    // per-quarter-limb completion words and the range flag in pinned host memory (keyswitch_lat.hip KsArgsQ)
    u32* host_done = nullptr;
    u32* host_flag = nullptr;
    u32 host_epoch = 0;
    hipStream_t cur = nullptr;        // stream the chunk being launched goes to
    u64* cur_scratch = nullptr;
    // CKKS level operations (ckks_ops.hip), all allocated at first use
    HxDevBuf<KsRescaleF64> d_rescale; // [16][16]: row l = constants of the rescale that drops limb l (filled at its first call)
    u32 rescale_levels = 0;           // bit l: row l is filled
    HxDevBuf<double> d_rs_s;          // rescale scratch: s of every (instance, component) pair of a chunk, n doubles each (grow-only)
    HxDevBuf<u64> d_rot_t;            // rotate: sigma_g(c1) of one slice of instances, [slice][L][n] (grow-only); relinearize and
                                      // multiply_sum_relinearize (ct_tensor.hip): component 2 of one slice -- one buffer for all three, as
                                      // each call's keyswitch has read it before the call returns to the stream
    // baby-step/giant-step linear transform (keyswitch_f64.hip hx_launch_linear_transform_bsgs), both grow-only
    HxDevBuf<double> d_bsgs_b;        // baby store: [n_baby][chunk][2][L+1][n] multiply-accumulate outputs in B order
    HxDevBuf<u64> d_bsgs_t;           // one giant step's inner sum t_j: [chunk][2][L][n] canonical words
    // device-side encode / decode (ckks_encode.hip), all allocated at first use
    HxDevBuf<double> d_emb_roots;     // [2n][2]: zeta^t = exp(i pi t / n) as (re, im), computed in long double and rounded once
    HxDevBuf<u32> d_emb_perm;         // [n/2]: slot k held by position p of the embedding FFT's bit-reversed side (5^k = 4 bitrev(p) + 1 mod 2n)
    HxDevBuf<double> d_garner;        // [16][16][2]: row i, column j < i = (q_j^-1 mod q_i centred, fl(./q_i)): Garner's constants for every prefix
    HxDevBuf<double> d_enc_coeffs;    // real coefficients of a chunk's instances, n doubles each (grow-only; rlwe.hip: the small samples)
    HxDevBuf<u64> d_enc_words;        // coefficient-form limbs of a chunk's (instance, limb) polynomials, n words each (grow-only; rlwe.hip:
                                      // NTT_i of an encryption's error)
};

// launcher prototypes implemented per translation unit
int hx_launch_ntt_fwd(hexl_ctx*, u64* d_x, size_t batch, const u64* roots, const u64* precon, u64 q, u64 n);
int hx_launch_ntt_inv(hexl_ctx*, u64* d_x, size_t batch, const u64* iroots, const u64* iprecon, u64 q,
                      u64 inv_n, u64 inv_n_p, u64 inv_n_w, u64 inv_n_w_p, u64 n);
int hx_launch_dyadic(hexl_ctx*, u64* d_out, const u64* d_a, const u64* d_b, size_t batch, u64 n,
                     const u64* d_moduli, u64 n_moduli);
int hx_launch_keyswitch(hexl_ks_plan*, u64* d_result, const u64* d_t_target, size_t batch, int stage_mask,
                        hipEvent_t* ev /* optional [4] */);
// one scratch chunk (nb <= plan->cap) on the FP64 path
int hx_launch_keyswitch_f64(hexl_ks_plan*, u64* d_result, const u64* d_t_target, size_t nb, int stage_mask,
                            hipEvent_t* ev);
// the same on the slot-major pipeline (keyswitch_x.hip; N = 16384, large chunks)
int hx_launch_keyswitch_x(hexl_ks_plan*, u64* d_result, const u64* d_t_target, size_t nb, int stage_mask,
                          hipEvent_t* ev);
bool hx_ks_x_applies(const hexl_ks_plan*, size_t nb);
size_t hx_ks_chunk(const hexl_ks_plan*);      // instances per scratch chunk (HEXL_KS_CHUNK or the default for the ring dimension)
bool hx_ks_chunk_forced();                    // HEXL_KS_CHUNK is set: hx_ks_chunk is that number whatever the plan
// true when a batch of nb runs entirely on kernels that honour hexl_ks_plan::overwrite_result
bool hx_ks_can_overwrite(const hexl_ks_plan*, size_t nb);
// the lone-keyswitch latency path (keyswitch_lat.hip): N = 16384, FP64 plans; one instance per call on p->cur / p->cur_scratch
bool hx_ks_lat_applies(const hexl_ks_plan*, size_t nb);
int hx_launch_keyswitch_lat(hexl_ks_plan*, u64* d_result, const u64* d_t_target, size_t nb);
int hx_launch_multiply_relinearize(hexl_ks_plan*, u64* d_out, const u64* d_a, const u64* d_b, size_t batch);
// CKKS level operations (ckks_ops.hip); arguments checked by their entry points (hexl_apply_galois, hexl_rescale, hexl_rotate)
int hx_launch_galois(hexl_ctx*, u64* d_out, const u64* d_in, size_t count, u32 logn, u32 g);
int hx_launch_rescale(hexl_ks_plan*, u64* d_out, const u64* d_in, size_t batch, u32 n_limbs, u32 n_components);
int hx_launch_rotate(hexl_ks_plan*, u64* d_out, const u64* d_ct, size_t batch, u32 g);
// hexl_rotate_hoisted (keyswitch_f64.hip): the keyswitch's steps 1-2 once per chunk on plans[0]'s scratch, steps 3-7 per rotation;
// hx_launch_galois_c0 (ckks_ops.hip) writes (sigma_g(c0), 0) for nb instances on the context's stream
int hx_launch_rotate_hoisted(hexl_ks_plan* const* plans, const u64* galois_elts, size_t n_rot, u64* const* d_outs, const u64* d_ct,
                             size_t batch);
int hx_launch_galois_c0(hexl_ctx*, u64* d_out, const u64* d_ct, size_t nb, u32 L, u32 logn, u32 g);
// hexl_linear_transform (keyswitch_f64.hip): the hoisted rotations weighted by plaintexts and summed in the extended basis, one mod-down
// per chunk. HxLtRot: one rotation of the per-call device table (in the context's d_shared) that hx_launch_galois_c0_pt (ckks_ops.hip)
// walks: d_out[nb][2][L][n] = (sum_r pt_r . sigma_{g_r}(c0) + pt_id . c0, pt_id . c1), canonical words, on the context's stream; the
// range flag given (the plan's d_flag; nullptr: none) is raised for a ciphertext word it reads that is not below its modulus. n_limbs:
// the limbs of d_ct, d_out and d_pt_identity -- p->L, or the level of hexl_hks_linear_transform (keyswitch_hybrid.hip)
struct HxLtRot { const u64* pt; u64 g; };                       // pt: [L + 1][n] ([K][n] for the hybrid caller), the kernel reads rows 0 ... n_limbs - 1
int hx_launch_linear_transform(hexl_ks_plan* const* plans, const u64* galois_elts, const u64* const* d_pts, size_t n_rot,
                               const u64* d_pt_identity, u64* d_out, const u64* d_ct, size_t batch);
int hx_launch_galois_c0_pt(hexl_ks_plan* p, u64* d_out, const u64* d_ct, const HxLtRot* d_rots, size_t n_rot, const u64* d_pt_identity,
                           size_t nb, u32 n_limbs, u32* d_range_flag);
// hexl_linear_transform_bsgs (keyswitch_f64.hip): the mod-up once, one key multiply-accumulate per baby step into the plan's baby store,
// then per giant step a key-free weighted sum of the stored products, one mod-down into the plan's t buffer and one hoisted rotation
// accumulated into d_out. `p0` (the first non-NULL plan, baby plans first) lends scratch, buffers, tier and range flag. Arguments checked
// by the entry point (ckks_ops.hip). hx_lt_bsgs_chunk: instances per chunk -- the keyswitch's, cut so that the baby store stays within
// HX_LT_BSGS_STORE_BYTES unless HEXL_KS_CHUNK forces it. hx_launch_galois_add (ckks_ops.hip): d_out[nb][2][n_limbs][n] += sigma_g of the
// first n_comp components of d_t, word by word modulo q_i, on the context's stream; n_limbs: p->L, or the level of
// hexl_hks_linear_transform_bsgs (keyswitch_hybrid.hip).
constexpr size_t HX_LT_BSGS_STORE_BYTES = size_t(2) << 30;
size_t hx_lt_bsgs_chunk(const hexl_ks_plan* p, size_t n_baby, size_t batch);
int hx_launch_linear_transform_bsgs(hexl_ks_plan* p0, hexl_ks_plan* const* baby_plans, const u64* baby_elts, size_t n_baby,
                                    hexl_ks_plan* const* giant_plans, const u64* giant_elts, size_t n_giant, const u64* const* d_pts,
                                    const u64* const* d_pt_identity, u64* d_out, const u64* d_ct, size_t batch);
int hx_launch_galois_add(hexl_ks_plan* p, u64* d_out, const u64* d_t, size_t nb, u32 g, u32 n_comp, u32 n_limbs);
// plan-driven RNS transforms and the plaintext multiply (rns_ops.hip); arguments checked by their entry points (hexl_rns_ntt_fwd,
// hexl_rns_ntt_inv, hexl_multiply_plain)
int hx_launch_rns_ntt(hexl_ks_plan*, u64* d_out, const u64* d_in, size_t count, u32 n_limbs, bool inverse);
int hx_launch_multiply_plain(hexl_ks_plan*, u64* d_out, const u64* d_ct, const u64* d_pt, size_t batch, u32 n_components, u32 n_limbs,
                             bool per_instance, bool accumulate);
// The ciphertext tensor sum (ct_tensor.hip k_ct_tensor_sum). Pointers and limb counts travel BY VALUE in the kernel arguments, as
// k_ct_lincomb's (rns_ops.hip): nothing is uploaded, so the host arrays are the caller's again when the call returns. The output goes
// through TWO descriptors -- components 0-1 of instance b at out01 + b stride01 (laid out [2][L][n]), component 2 at out2 + b stride2
// ([L][n]) -- so that one kernel writes hexl_ct_tensor_sum's [batch][3][L][n] buffer and, for the fused multiplies
// (hexl_multiply_sum_relinearize; keyswitch_hybrid.hip hexl_hks_multiply_sum_*), a two-component buffer and the key switch's input slice.
constexpr u32 TS_MAX_TERMS = 8, TS_MAX_LIMBS = 16;                // hexl_ks_plan::tier has 16 limbs
struct TsArgs {
    const KsModF64* mods;       // [K]
    const u64* a[TS_MAX_TERMS]; // term t: [batch][2][la[t]][n], read through its first L limbs
    const u64* b[TS_MAX_TERMS]; //         [batch][2][lb[t]][n]; may be a[t] (a square)
    u32 la[TS_MAX_TERMS], lb[TS_MAX_TERMS];
    u64* out01;
    u64* out2;
    unsigned long long stride01, stride2;       // words between instances
    u32 logn, L, n_terms;
};
// The operands of a tensor sum, checked and laid into `s` (pointers at instance 0): HEXL_E_BADARG for a null entry, a limb count outside
// n_limbs ... K, or an operand that shares a byte with [d_out, d_out + out_bytes). hx_launch_tensor: nb instances on the context's
// stream, `s` with its operand and output pointers at the first of them.
int hx_tensor_operands(const hexl_ks_plan* p, const u64* const* d_as, const u64* const* d_bs, const u64* in_limbs, size_t n_terms,
                       size_t batch, u64 n_limbs, const u64* d_out, size_t out_bytes, TsArgs& s);
int hx_launch_tensor(hexl_ks_plan* p, const TsArgs& s, size_t nb);
// device-side encode / decode (ckks_encode.hip); arguments checked by their entry points (hexl_rns_from_f64, hexl_rns_to_f64,
// hexl_ckks_encode, hexl_ckks_decode). d_slots = nullptr: the real coefficients themselves are the caller's (d_coeffs).
int hx_launch_encode(hexl_ks_plan*, u64* d_out, const double* d_coeffs, const double* d_slots, size_t count, u32 n_limbs, double scale);
int hx_launch_decode(hexl_ks_plan*, double* d_coeffs, double* d_slots, const u64* d_in, size_t count, u32 n_limbs, double scale);
// instances per chunk of the encode scratch (d_enc_coeffs, d_enc_words): 256 at n = 16384 and the same number of coefficients at every other n
inline size_t hx_enc_chunk(const hexl_ks_plan* p) { return (size_t(256) << 14) >> p->logn; }
inline size_t hx_enc_chunk_of(const hexl_ks_plan* p, size_t count) { return count < hx_enc_chunk(p) ? count : hx_enc_chunk(p); }
// the sampler, symmetric encryption and decryption (rlwe.hip); arguments checked by their entry points (hexl_sample, hexl_rlwe_encrypt,
// hexl_rlwe_decrypt). The small kinds and the error of an encryption pass through d_enc_coeffs / d_enc_words in chunks of hx_enc_chunk.
int hx_launch_sample(hexl_ks_plan*, u64* d_out, int kind, const u32* seed, u64 stream, u64 first, size_t count, u32 n_limbs);
int hx_launch_rlwe_encrypt(hexl_ks_plan*, u64* d_out, const u64* d_pt, bool per_instance, const u64* d_secret, const u32* seed, u64 stream,
                           u64 first, size_t count, u32 n_limbs);
int hx_launch_rlwe_decrypt(hexl_ks_plan*, u64* d_out, const u64* d_ct, const u64* d_secret, size_t count, u32 n_components, u32 n_limbs);
// public-key encryption (rlwe.hip; arguments checked by hexl_pk_encrypt): per chunk the mask and the two errors of every instance pass
// through the encode scratch as 3 rows, so a chunk is a third of encode's -- 85 instances at n = 16384, 1365 at n = 1024
inline size_t hx_pk_chunk(const hexl_ks_plan* p) { return hx_enc_chunk(p) / 3; }
inline size_t hx_pk_chunk_of(const hexl_ks_plan* p, size_t count) { return count < hx_pk_chunk(p) ? count : hx_pk_chunk(p); }
int hx_launch_pk_encrypt(hexl_ks_plan*, u64* d_out, const u64* d_pt, bool per_instance, const u64* d_pk, u32 pk_limbs, const u32* seed,
                         u64 stream, u64 first, size_t count, u32 n_limbs);
// the error of nb <= chunk encryptions, NTT_i(CBD21 polynomial first + b) at n_limbs limbs, into d_enc_words (reserved by the caller)
int hx_launch_rlwe_error(hexl_ks_plan*, const u32* seed, u64 stream, u64 first, size_t nb, u32 n_limbs);
// switching keys without a host round trip (keygen.hip); arguments checked by their entry points (hexl_ks_set_keys_device,
// hexl_ks_gen_keys). HxKeyCopy: one copy of the keys a plan holds -- [L][L + 1][2][n] limbs at `dst`, the n words of a limb in `order`
// (key_layout.hpp), as centred doubles, or (shoup: the integer kernels' copy) as u64 [limb][2][n] = the word and floor(word 2^64 / q).
// hx_ks_key_copies (capi.hip) is the ONE list of them: hexl_ks_set_keys fills what it names on the host, the kernels of keygen.hip on
// the device. It fixes hexl_ks_plan::x_loge, as hexl_ks_set_keys always did.
struct HxKeyCopy { void* dst; hxk::Order order; bool shoup; };
constexpr int HX_KEY_MAX_COPIES = 3;
int hx_ks_key_copies(hexl_ks_plan* p, HxKeyCopy out[HX_KEY_MAX_COPIES]);
int hx_launch_ks_install(hexl_ks_plan*, const u64* d_keys);
int hx_launch_ks_gen_keys(hexl_ks_plan*, const u64* d_secret, int from_kind, u32 g, const u64* d_from, const u32* seed, u64 stream, u64 first);
u32 hx_ks_x_loge();
// What hexl_hks_keygen (keygen.hip) needs of a hybrid object; keyswitch_hybrid.hip owns the struct. d_keys: [dnum][2][K][n] centred doubles,
// the layout k_hks_install writes. p_mod: [K], P mod q_i canonical (exact as a double), P the product of the plan's moduli L ... K - 1,
// computed when the object is created.
struct HxHksKeys { hexl_ks_plan* plan; double* d_keys; const double* p_mod; u32 alpha, dnum; };
HxHksKeys hx_hks_keys(hexl_hks*);
void hx_hks_set_keyed(hexl_hks*);         // the keys were written on the context's stream: the object answers no HEXL_E_NOKEYS any more
// index of coefficient held in register r of thread tid after a forward transform ("B layout")
u32 hx_idxB(u32 logn, u32 r, u32 tid);
u32 hx_loge_for(u32 logn);


static inline u64 hx_shoup(u64 y, u64 q) { return (u64)(((u128)(y % q) << 64) / q); }
// residue v < q as the centred double in (-q/2, q/2] the FP64 kernels work on
static inline double hx_centre(u64 v, u64 q) { return hxk::centre(v, q); }
// nibble i = forward reduction period of limb i (the kernels built with LAZY = -1 look their schedule up here)
static inline unsigned long long hx_tiermap(const hexl_ks_plan* p) {
    unsigned long long m = 0;
    for (u32 i = 0; i < p->K; ++i) m |= (unsigned long long)(p->tier[i] & 15u) << (4 * i);
    return m;
}
// [a, a + abytes) and [b, b + bbytes) share a byte
static inline bool hx_ranges_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
    return (const char*)a < (const char*)b + bbytes && (const char*)b < (const char*)a + abytes;
}
// instances of a batch that go into one scratch chunk
static inline size_t hx_ks_chunk_of(const hexl_ks_plan* p, size_t batch) { return batch < hx_ks_chunk(p) ? batch : hx_ks_chunk(p); }
// the plan's keyswitch scratch for chunks of `chunk` instances on every lane (keyswitch.hip; keeps hexl_ks_plan::cap)
int hx_ks_reserve_scratch(hexl_ks_plan* p, size_t chunk);
// f(first, nb) for every chunk of `count` instances, in order; stops at the first status that is not 0
template <class F>
static inline int hx_for_chunks(size_t count, size_t chunk, F f) {
    for (size_t c0 = 0; c0 < count; c0 += chunk)
        if (int rc = f(c0, count - c0 < chunk ? count - c0 : chunk)) return rc;
    return 0;
}
// the forward reduction period every one of the first n_limbs limbs shares, else -1 (the kernels built with LAZY = -1 look it up per limb)
static inline int hx_level_tier(const hexl_ks_plan* p, u32 n_limbs) {
    for (u32 i = 1; i < n_limbs; ++i)
        if (p->tier[i] != p->tier[0]) return -1;
    return p->tier[0];
}

// ---- the argument checks of the plan-level entry points (DESIGN.md 4.7 "Host scaffold"); all of them decide HEXL_E_BADARG ----
constexpr size_t HX_MAX_GRID = 0x7fffffffu;      // workgroups of one launch (x dimension)
static inline bool hx_in_range(u64 v, u64 lo, u64 hi) { return v >= lo && v <= hi; }
// FP64 plan of a ring dimension the workgroup transforms exist for (1024 ... 32768) ...
static inline bool hx_f64_plan_ok(const hexl_ks_plan* p) { return p && p->use_f64 && p->logn >= 10 && p->logn <= 15; }
// ... and lo <= n_limbs <= hi
static inline bool hx_f64_plan_ok(const hexl_ks_plan* p, u64 n_limbs, u64 lo, u64 hi) { return hx_f64_plan_ok(p) && hx_in_range(n_limbs, lo, hi); }
// *bytes = the size of [count][comps][limbs][n] 64-bit words (or doubles); false when it does not fit a size_t
static inline bool hx_words_bytes(size_t count, u64 comps, u64 limbs, u64 n, size_t* bytes) {
    const size_t per = size_t(comps) * limbs * n * sizeof(u64);
    if (per && count > SIZE_MAX / per) return false;
    *bytes = count * per;
    return true;
}
// one workgroup per (instance, limb) -- the workgroup transforms: the launch fits
static inline bool hx_wg_grid_ok(size_t count, u64 limbs) { return count <= HX_MAX_GRID / limbs; }
// The word-wise kernels (k_pt_mul, k_ct_lincomb, the rlwe.hip kernels; with 512-word pieces the k_galois_c0_pt family): HX_WW_THREADS
// lanes and one workgroup per (instance, limb, piece of 2^log_chunk words). The kernels read constants of their own, tied to these
// by a static_assert beside each.
constexpr u32 HX_WW_THREADS = 256, HX_WW_LOG_CHUNK = 10;
static inline size_t hx_ww_grid(const hexl_ks_plan* p, size_t count, u64 limbs, u32 log_chunk = HX_WW_LOG_CHUNK) {
    return count * limbs * (p->n >> log_chunk);
}
static inline bool hx_ww_grid_ok(const hexl_ks_plan* p, size_t count, u64 limbs) { return count <= HX_MAX_GRID / hx_ww_grid(p, 1, limbs); }
// The plaintext operand of a batched call: one for all instances (pt_batch == 1) or one per instance (pt_batch == batch); anything else
// is refused. stride: 1 per instance, 0 shared; bytes: what the call reads of it (per_bytes each; nothing for an empty batch).
struct HxPtBatch { u32 stride = 0; size_t bytes = 0; };
static inline bool hx_pt_batch(size_t pt_batch, size_t batch, size_t per_bytes, HxPtBatch* pb) {
    if (pt_batch != 1 && pt_batch != batch) return false;
    pb->stride = pt_batch == batch ? 1u : 0u;
    pb->bytes = (batch ? pt_batch : 0) * per_bytes;
    return true;
}

// The <LOGN, LOGE, LAZY> instantiations of the FP64 (b, d)-major kernels and of the kernels built on their geometry (rescale):
// f(<LOGN>, <LOGE>, <LAZY>) for ring dimension 2^logn and forward reduction period `lazy` (f64_arith.hpp: 0 = strict, < 0 = looked up
// per limb). N = 16384 has the periods 3 / 6 / 12, the other rings keep 3 (a shorter period is always valid: fewer kernel variants).
template <int V> using hx_int = std::integral_constant<int, V>;
template <class F>
static int hx_with_f64_geom(u32 logn, int lazy, F f) {
    auto tiers = [&](auto N, auto E) {
        if (lazy < 0) return f(N, E, hx_int<-1>{});
        if (lazy == 0) return f(N, E, hx_int<0>{});
        if constexpr (decltype(N)::value == 14) {
            if (lazy == 12) return f(N, E, hx_int<12>{});
            if (lazy == 6) return f(N, E, hx_int<6>{});
        }
        return f(N, E, hx_int<3>{});
    };
    switch (logn) {
        case 10: return tiers(hx_int<10>{}, hx_int<4>{});
        case 11: return tiers(hx_int<11>{}, hx_int<5>{});
        case 12: return tiers(hx_int<12>{}, hx_int<5>{});
        case 13: return tiers(hx_int<13>{}, hx_int<5>{});
        case 14: return tiers(hx_int<14>{}, hx_int<4>{});
        case 15: return tiers(hx_int<15>{}, hx_int<5>{});      // beyond the reference: N = 32768
        default: return (int)HEXL_E_BADARG;
    }
}
