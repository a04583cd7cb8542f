// capi.hip -- the extern "C" launcher ABI of include/hexl_mi355x.h on device pointers: contexts, the K1-K3 entry points, keyswitch
// plans (host precompute + upload) and the hipEvent timing hook. The host-pointer (*_host) entry points are host_staging.hip.
#include <string.h>

#include <atomic>

#include "hexl_internal.hpp"
#include "number_theory.hpp"

// ------------------------------------------------------------------------------- context
// NUMA node the library's own host threads (copy pool, unpack lane) ask for: the node of the devices in use when they all hang off one
// node, else no preference (host_simd.cpp; round 6: +16 % on the host-pointer KeySwitch at worksize 128). -2 = no context yet.
int hx_numa_node_of_pci(const char* bdf);
bool hx_pin_this_thread_to_node(int node);
static std::atomic<int> g_host_node{-2};
static void note_device_node(int device) {
    static const bool pin = hx_knob("HEXL_HOST_PIN", 1) != 0;
    if (!pin) { g_host_node.store(-1); return; }
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, sizeof bdf, device) != hipSuccess) { (void)hipGetLastError(); bdf[0] = 0; }
    for (char* c = bdf; *c; ++c) if (*c >= 'A' && *c <= 'F') *c = char(*c - 'A' + 'a');     // sysfs names are lower case
    const int node = hx_numa_node_of_pci(bdf);
    int seen = g_host_node.load();
    while (!g_host_node.compare_exchange_weak(seen, seen == -2 ? node : (seen == node ? node : -1))) {}
}
void hx_pin_own_thread() { (void)hx_pin_this_thread_to_node(g_host_node.load()); }

extern "C" int hexl_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return count;
}

extern "C" int hexl_ctx_create(int device, hexl_ctx** out) {
    if (!out) return HEXL_E_BADARG;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device >= count) return HEXL_E_NODEVICE;
    HX_CHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HX_CHECK(hipGetDeviceProperties(&prop, device));
    hexl_ctx* c = new hexl_ctx();
    c->device = device;
    c->num_cu = prop.multiProcessorCount;
    snprintf(c->name, sizeof(c->name), "hexl_mi355x: device %d %s (%s), %d CUs, %.1f GiB", device, prop.name,
             prop.gcnArchName, prop.multiProcessorCount, prop.totalGlobalMem / 1073741824.0);
    HX_CHECK(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    note_device_node(device);
    *out = c;
    return 0;
}

extern "C" int hexl_ctx_destroy(hexl_ctx* c) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->s_up) (void)hipStreamDestroy(c->s_up);
    if (c->s_down) (void)hipStreamDestroy(c->s_down);
    for (int i = 0; i < 2; ++i) {
        if (c->ev_up[i]) (void)hipEventDestroy(c->ev_up[i]);
        if (c->ev_comp[i]) (void)hipEventDestroy(c->ev_comp[i]);
        if (c->ev_down[i]) (void)hipEventDestroy(c->ev_down[i]);
    }
    if (c->ev_switch) (void)hipEventDestroy(c->ev_switch);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;                                                     // every HxBuf member releases its memory (the stream was drained above)
    return 0;
}

// A context and its plans keep ONE set of scratch buffers (derived NTT tables, dyadic constants, keyswitch / rescale / rotate scratch,
// the range flag), safe on one stream because launch k + 1 is ordered behind launch k. A switch keeps that order: the new stream waits
// for an event recorded behind everything queued on the old one. The host does not wait.
static int switch_stream(hexl_ctx* c, hipStream_t to) {
    if (to == c->stream) return 0;
    HX_CHECK(hipSetDevice(c->device));
    if (!c->ev_switch) HX_CHECK(hipEventCreateWithFlags(&c->ev_switch, hipEventDisableTiming));
    HX_CHECK(hipEventRecord(c->ev_switch, c->stream));
    HX_CHECK(hipStreamWaitEvent(to, c->ev_switch, 0));
    c->stream = to;
    return 0;
}
extern "C" int hexl_ctx_set_stream(hexl_ctx* c, void* s) {
    if (!c) return HEXL_E_BADARG;
    return switch_stream(c, (hipStream_t)s);
}
extern "C" int hexl_ctx_use_own_stream(hexl_ctx* c) {
    if (!c) return HEXL_E_BADARG;
    return switch_stream(c, c->own_stream);
}
extern "C" int hexl_ctx_sync(hexl_ctx* c) {
    if (!c) return HEXL_E_BADARG;
    HX_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" int hexl_ctx_describe(hexl_ctx* c, char* buf, size_t len) {
    if (!c || !buf || !len) return HEXL_E_BADARG;
    snprintf(buf, len, "%s", c->name);
    return 0;
}

// ------------------------------------------------------------------------------- K1..K3
extern "C" int hexl_ntt_fwd(hexl_ctx* c, uint64_t* x, size_t batch, const uint64_t* roots, const uint64_t* precon,
                            uint64_t q, uint64_t n) {
    if (!c || !x || !roots || !precon || !q || !hx_supported_ntt_n(n) || batch > 0x7fffffffu) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(c->device));
    return hx_launch_ntt_fwd(c, x, batch, roots, precon, q, n);
}

extern "C" int hexl_ntt_inv(hexl_ctx* c, uint64_t* x, size_t batch, const uint64_t* ir, const uint64_t* ip, uint64_t q,
                            uint64_t inv_n, uint64_t inv_n_w, uint64_t n) {
    if (!c || !x || !ir || !ip || !q || !hx_supported_ntt_n(n) || batch > 0x7fffffffu) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(c->device));
    // floor(y*2^64/q) once on the host; the reference recomputes it per element on the device
    // (MultiplyUIntModLazy3, device/mod_ops.hpp:135-151)
    return hx_launch_ntt_inv(c, x, batch, ir, ip, q, inv_n, hx_shoup(inv_n, q), inv_n_w, hx_shoup(inv_n_w, q), n);
}

extern "C" int hexl_dyadic_multiply(hexl_ctx* c, uint64_t* out, const uint64_t* a, const uint64_t* b, size_t batch,
                                    uint64_t n, const uint64_t* moduli, uint64_t n_moduli) {
    if (!c || !out || !a || !b || !moduli) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(c->device));
    return hx_launch_dyadic(c, out, a, b, batch, n, moduli, n_moduli);
}

// ------------------------------------------------------------------------------- K4 plan
// elements-per-thread exponent of the keyswitch kernels (must match run_chunk<> / run_chunk_f64<> dispatch)
static u32 ks_loge(u32 logn, bool f64) { return logn <= 10 ? 4 : (f64 && logn == 14 ? 4 : 5); }
// perm[pos] = the caller's word index stored at position pos of a limb in that order (key_layout.hpp); empty: natural order
static std::vector<u32> ks_perm(u32 n, const hxk::Order o) {
    std::vector<u32> perm(o.loge ? n : 0);
    for (u32 pos = 0; pos < (u32)perm.size(); ++pos) perm[pos] = hxk::src_of(o, pos);
    return perm;
}

// The copies of the keys this plan holds, in the order hexl_ks_set_keys has always filled them (hexl_internal.hpp HxKeyCopy):
//   integer plans   d_keys: B order of the integer kernels' geometry, the word beside its Shoup factor -- FP64 plans never run those
//                   kernels and hold no integer copy (22 MB of device memory and a host pass per key set for nothing)
//   FP64 plans      d_keys_f64: centred doubles in the B order of the (b, d)-major kernels
//   d_keys_x        ... in the B order of the slot-major pipeline's geometry. N = 32768: every transform of that pipeline is two
//                   16384-point halves (keyswitch_x.hip k_ksh_*), so NTT-domain block h of a key row is kept in the B order of THAT geometry
//   d_keys_nat      ... in natural order (latency path)
int hx_ks_key_copies(hexl_ks_plan* p, HxKeyCopy out[HX_KEY_MAX_COPIES]) {
    int c = 0;
    if (!p->use_f64) out[c++] = {p->d_keys.get(), {p->logn, p->int_loge}, true};
    else out[c++] = {p->d_keys_f64.get(), {p->logn, p->f64_loge}, false};
    if (p->d_keys_x) {
        p->x_loge = p->logn == 14 ? hx_ks_x_loge() : 4;
        out[c++] = {p->d_keys_x.get(), {p->logn < 15 ? p->logn : 14, p->logn < 15 ? p->x_loge : 4}, false};
    }
    if (p->d_keys_nat) out[c++] = {p->d_keys_nat.get(), {p->logn, 0}, false};
    return c;
}

extern "C" int hexl_ks_plan_create(hexl_ctx* c, uint64_t n, uint64_t L, uint64_t K, uint64_t rns, uint64_t kcc,
                                   const uint64_t* h_moduli, const uint64_t* h_modswitch, const uint64_t* h_twiddles,
                                   hexl_ks_plan** out) {
    if (!c || !out || !h_moduli || !h_modswitch) return HEXL_E_BADARG;
    if (!hx_supported_ntt_n(n) || kcc != 2 || L == 0 || K < 2 || L >= K || K > 16 || rns == 0) return HEXL_E_BADARG;
    for (u64 i = 0; i < K; ++i)
        if (h_moduli[i] < (1ULL << 16) || h_moduli[i] >= (1ULL << 60)) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(c->device));
    u32 logn = 0;
    while ((1ULL << logn) < n) ++logn;

    hexl_ks_plan* p = new hexl_ks_plan();
    struct Guard {                                                // every failing exit below releases the plan and what it holds so far
        hexl_ks_plan* p;
        ~Guard() { (void)hexl_ks_plan_destroy(p); }               // (null once the plan is the caller's)
    } guard{p};
    p->ctx = c; p->n = (u32)n; p->logn = logn; p->L = (u32)L; p->K = (u32)K; p->rns = (u32)rns;
    p->moduli.assign(h_moduli, h_moduli + K);

    const u64 q_sp = h_moduli[K - 1];
    std::vector<KsModulus> mods(K);
    std::vector<u64> tables(size_t(K) * 4 * n);
    std::vector<u64> inv0(n);
    for (u64 i = 0; i < K; ++i) {
        const u64 q = h_moduli[i];
        u64* roots = &tables[(i * 4 + 0) * n];
        u64* precon = &tables[(i * 4 + 1) * n];
        u64* iroots = &tables[(i * 4 + 2) * n];
        u64* iprecon = &tables[(i * 4 + 3) * n];
        if (h_twiddles) {
            // caller blocks [inv_roots | precon_inv | roots | precon_roots]; like the reference's
            // twiddle_generator.hpp:35-79 only blocks 0 and 2 are consumed
            memcpy(inv0.data(), h_twiddles + i * 4 * n, n * sizeof(u64));
            memcpy(roots, h_twiddles + (i * 4 + 2) * n, n * sizeof(u64));
        } else {
            const u64 w = hxnt::minimal_primitive_root(2 * n, q);      // fpga.cpp:1097-1109
            hxnt::forward_roots(n, logn, q, w, roots);
            hxnt::inverse_roots_from0(n, q, roots, inv0.data());
        }
        // internal inverse table uses the standalone kernel's indexing (first entry at index 1)
        iroots[0] = 1;
        for (u64 r = 1; r < n; ++r) iroots[r] = inv0[r - 1];
        for (u64 r = 0; r < n; ++r) {
            precon[r] = hx_shoup(roots[r], q);
            iprecon[r] = hx_shoup(iroots[r], q);
        }
        KsModulus& m = mods[i];
        m.q = q;
        m.qbarr = (u64)(((u128)1 << 64) / q);                           // fpga.cpp:1053
        m.inv_n = hxnt::invmod(n, q);                                   // fpga.cpp:1073
        m.inv_n_p = hx_shoup(m.inv_n, q);
        m.inv_n_w = hxnt::mulmod(m.inv_n, iroots[n - 1] % q, q);        // last-stage W folded into the scaling
        m.inv_n_w_p = hx_shoup(m.inv_n_w, q);
        u64 msf = h_modswitch[i];                                       // ReduceMod<8>, fpga.cpp:1057-1061
        if (msf >= 4 * q) msf -= 4 * q;
        if (msf >= 2 * q) msf -= 2 * q;
        if (msf >= q) msf -= q;
        m.msf = msf;
        m.msf_p = hx_shoup(msf, q);
        m.half = q_sp >> 1;
        m.fix = q - (m.half % q);                                       // intt2_redu.hpp:31-32
        u32 fl = 63;
        while (!(q >> fl)) --fl;
        m.len = fl - 1;
        m.barr_lo = (u64)(((u128)1 << (m.len + 64)) / q);
    }
    // FP64 path: every modulus below 2^52 (the reference's own bound); HEXL_KS_INT=1 forces the integer kernels
    bool f64_ok = hx_knob("HEXL_KS_INT", 0) != 1;
    for (u64 i = 0; i < K; ++i) f64_ok = f64_ok && h_moduli[i] < (1ULL << 52);
    if (logn == 15 && !f64_ok) return HEXL_E_BADARG;              // N = 32768: FP64 kernels only (moduli < 2^52)
    p->use_f64 = f64_ok;
    p->f64_lazy = 0;
    p->f64_loge = ks_loge(logn, true);
    p->int_loge = ks_loge(logn, false);
    if (logn == 14) {                                             // HEXL_KSI_LOGE=4: 16 coefficients x 1024 threads
        const long e = hx_knob("HEXL_KSI_LOGE", 0);
        if (e == 4 || e == 5) p->int_loge = (u32)e;
    }
    if (f64_ok && hx_knob("HEXL_KS_NOLAZY", 0) != 1) {
        double qmax = 0;
        for (u64 i = 0; i < K; ++i) qmax = (double)h_moduli[i] > qmax ? (double)h_moduli[i] : qmax;
        p->f64_lazy = hxf::lazy_period_for(qmax);
        double qmin = qmax;
        for (u64 i = 0; i < K; ++i) qmin = (double)h_moduli[i] < qmin ? (double)h_moduli[i] : qmin;
        // HEXL_KSX_SKIP=0: keep the range reductions (tests)
        p->x_skip = p->f64_lazy && qmax <= hxf::LAZY_SKIP_MAX_RATIO * qmin && hx_knob("HEXL_KSX_SKIP", 1) != 0;
        const long e = hx_knob("HEXL_KS_PERIOD", 12);           // testing: force a SHORTER period (always valid)
        const int cap = (e == 3 || e == 6) ? (int)e : 12;
        if (p->f64_lazy > cap) p->f64_lazy = cap;
        // per-limb tiers: limb i's transforms run modulo q_i alone (hexl_internal.hpp); HEXL_KS_PER_LIMB=0: the plan-wide tier for all
        const bool per_limb = hx_knob_ks_per_limb() != 0;
        for (u64 i = 0; i < K; ++i) {
            int t = per_limb ? hxf::lazy_period_for((double)h_moduli[i]) : p->f64_lazy;
            if (t > cap) t = cap;
            p->tier[i] = (unsigned char)t;
            if ((i < L || i == K - 1) && t != p->f64_lazy) p->mixed = true;
        }
    }
    if (f64_ok) {
        std::vector<KsModF64> fm(K);
        std::vector<double> ft(size_t(K) * 4 * n);
        for (u64 i = 0; i < K; ++i) {
            const u64 q = h_moduli[i];
            const double pd = (double)q;
            auto centre = [&](u64 v) { return hx_centre(v % q, q); };
            for (int blk = 0; blk < 4; blk += 2)                   // blocks 0 / 2 hold w, blocks 1 / 3 hold fl(w/p)
                for (u64 r = 0; r < n; ++r) {
                    const double w = centre(tables[(i * 4 + blk) * n + r]);
                    ft[(i * 4 + blk) * n + r] = w;
                    ft[(i * 4 + blk + 1) * n + r] = w / pd;
                }
            KsModF64& f = fm[i];
            f.m.p = pd; f.m.pinv = 1.0 / pd;
            f.sc.n = centre(mods[i].inv_n);     f.sc.n_p = f.sc.n / pd;
            f.sc.nw = centre(mods[i].inv_n_w);  f.sc.nw_p = f.sc.nw / pd;
            f.msf = centre(mods[i].msf);        f.msf_p = f.msf / pd;
            f.fix = (double)mods[i].fix;
            f.half = (double)mods[i].half;
        }
        const size_t key_words = size_t(L) * (L + 1) * 2 * n;
        if (int rc = p->d_mods_f64.upload_once(fm.data(), K)) return rc;
        if (int rc = p->d_tables_f64.upload_once(ft.data(), ft.size())) return rc;
        if (int rc = p->d_keys_f64.reserve(key_words)) return rc;
        if (logn >= 10 && logn <= 15)
            if (int rc = p->d_keys_x.reserve(key_words)) return rc;
        if (logn == 14)
            if (int rc = p->d_keys_nat.reserve(key_words)) return rc;
    }
    // input-range flag of the FP64 kernels (hexl_ks_range_check) + its pinned mirror; HEXL_KS_VALIDATE shares them
    // word 0: the kernels' range flag (HEXL_W_RANGE); word 1: HEXL_KS_VALIDATE's own (HEXL_E_RANGE) -- two statuses, two words
    // (word 2: the output gate of the zero-copy lone keyswitch, keyswitch_lat.hip k_ksq_down)
    if (int rc = p->d_flag.reserve(4)) return rc;
    HX_CHECK(hipMemset(p->d_flag, 0, 4 * sizeof(u32)));
    if (int rc = p->h_flag.reserve(2)) return rc;
    if (int rc = p->d_mods.upload_once(mods.data(), K)) return rc;
    if (int rc = p->d_tables.upload_once(tables.data(), tables.size())) return rc;
    // integer-kernel keys (key words + Shoup factors): only plans that run the integer kernels hold them
    if (!f64_ok)
        if (int rc = p->d_keys.reserve(size_t(L) * (L + 1) * 4 * n)) return rc;
    guard.p = nullptr;
    *out = p;
    return 0;
}

extern "C" int hexl_ks_plan_destroy(hexl_ks_plan* p) {
    if (!p) return 0;
    (void)hipSetDevice(p->ctx->device);
    (void)hipDeviceSynchronize();
    for (int l = 0; l < HX_KS_MAX_LANES; ++l) {
        if (p->aux[l]) (void)hipStreamDestroy(p->aux[l]);
        if (p->ev_done[l]) (void)hipEventDestroy(p->ev_done[l]);
    }
    if (p->ev_start) (void)hipEventDestroy(p->ev_start);
    delete p;                                                     // every HxBuf member releases its memory (the device was drained above)
    return 0;
}

// The reference packs keys into 3x256-bit DDR words (KeySwitch_load_keys, fpga.cpp:1167-1248); the GPU
// keeps plain 64-bit words but permutes each (d, slot, k) limb into the forward transform's register
// order so the key multiply-accumulate reads them fully coalesced.
extern "C" int hexl_ks_set_keys(hexl_ks_plan* p, const uint64_t* const* h_keys) {
    if (!p || !h_keys) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    const u64 n = p->n, L = p->L, K = p->K;
    for (u64 d = 0; d < L; ++d)
        if (!h_keys[d]) return HEXL_E_BADARG;
    HX_CHECK(hipStreamSynchronize(p->ctx->stream));
    const size_t words = size_t(L) * (L + 1) * 2 * n;
    // one target layout: word j of limb (d, slot, k) is the caller's word perm[j] (no perm: natural order) reduced modulo the
    // limb's q -> store(first word of the limb, j, value, q)
    auto relayout = [&](const std::vector<u32>& perm, auto store) {
        for (u64 d = 0; d < L; ++d)
            for (u64 slot = 0; slot <= L; ++slot) {
                const u64 i = slot < L ? slot : K - 1;
                const u64 q = p->moduli[i];
                for (u64 k = 0; k < 2; ++k) {
                    const u64* src = h_keys[d] + (k * K + i) * n;            // fpga.cpp:1186-1190
                    const size_t base = ((d * (L + 1) + slot) * 2 + k) * n;
                    for (u64 j = 0; j < n; ++j) store(base, j, src[perm.empty() ? j : perm[j]] % q, q);
                }
            }
    };
    HxKeyCopy copies[HX_KEY_MAX_COPIES];
    const int n_copies = hx_ks_key_copies(p, copies);
    for (int c = 0; c < n_copies; ++c) {
        const std::vector<u32> perm = ks_perm((u32)n, copies[c].order);
        if (copies[c].shoup) {                                    // [d][slot][k][0] = key mod q, [..][1] = floor(that * 2^64 / q)
            std::vector<u64> h(2 * words);
            relayout(perm, [&](size_t base, u64 j, u64 v, u64 q) {
                h[2 * base + j] = v;
                h[2 * base + n + j] = (u64)(((u128)v << 64) / q);
            });
            HX_CHECK(hipMemcpy(copies[c].dst, h.data(), h.size() * sizeof(u64), hipMemcpyHostToDevice));
        } else {                                                  // the same limbs as centred doubles
            std::vector<double> h(words);
            relayout(perm, [&](size_t base, u64 j, u64 v, u64 q) { h[base + j] = hx_centre(v, q); });
            HX_CHECK(hipMemcpy(copies[c].dst, h.data(), words * sizeof(double), hipMemcpyHostToDevice));
        }
    }
    p->have_keys = true;
    return 0;
}

extern "C" int hexl_keyswitch(hexl_ks_plan* p, uint64_t* d_result, const uint64_t* d_t_target, size_t batch) {
    if (!p || !d_result || !d_t_target) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    return hx_launch_keyswitch(p, d_result, d_t_target, batch, 7, nullptr);
}

extern "C" int hexl_ks_plan_tiers(const hexl_ks_plan* p, int* tiers) {
    if (!p || !tiers) return HEXL_E_BADARG;
    for (u32 i = 0; i < p->K; ++i) tiers[i] = p->use_f64 ? (int)p->tier[i] : -1;
    return p->use_f64 && p->mixed ? 1 : 0;
}

extern "C" int hexl_ks_range_check(hexl_ks_plan* p) {
    if (!p) return HEXL_E_BADARG;
    hexl_ctx* c = p->ctx;
    HX_CHECK(hipSetDevice(c->device));
    HX_CHECK(hipMemcpyAsync(p->h_flag, p->d_flag, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HX_CHECK(hipMemsetAsync(p->d_flag, 0, sizeof(u32), c->stream));
    HX_CHECK(hipStreamSynchronize(c->stream));
    return *p->h_flag ? HEXL_W_RANGE : 0;
}

extern "C" int hexl_multiply_relinearize(hexl_ks_plan* p, uint64_t* d_out, const uint64_t* d_a, const uint64_t* d_b,
                                         size_t batch) {
    if (!p || !d_out || !d_a || !d_b) return HEXL_E_BADARG;
    // d_out is written while d_a / d_b are still being read (component 0 is stored before component 1's operands are loaded)
    const size_t bytes = batch * 2 * size_t(p->L) * p->n * sizeof(u64);
    if (hx_ranges_overlap(d_out, bytes, d_a, bytes) || hx_ranges_overlap(d_out, bytes, d_b, bytes)) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    return hx_launch_multiply_relinearize(p, d_out, d_a, d_b, batch);
}

extern "C" int hexl_ks_time_stages(hexl_ks_plan* p, uint64_t* d_result, const uint64_t* d_t_target, size_t batch,
                                   int iters, float* ms_out) {
    if (!p || !ms_out || iters <= 0) return HEXL_E_BADARG;
    HX_CHECK(hipSetDevice(p->ctx->device));
    hipEvent_t ev[4] = {};
    struct Guard {                                                // the events go on every exit
        hipEvent_t* ev;
        ~Guard() { for (int i = 0; i < 4; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]); }
    } guard{ev};
    for (auto& e : ev) HX_CHECK(hipEventCreate(&e));
    float acc[4] = {0, 0, 0, 0};
    for (int it = 0; it < iters; ++it) {
        int rc = hx_launch_keyswitch(p, d_result, d_t_target, batch, 7, ev);
        if (rc) return rc;
        HX_CHECK(hipEventSynchronize(ev[3]));
        float t;
        HX_CHECK(hipEventElapsedTime(&t, ev[0], ev[3])); acc[0] += t;
        for (int s = 0; s < 3; ++s) { HX_CHECK(hipEventElapsedTime(&t, ev[s], ev[s + 1])); acc[1 + s] += t; }
    }
    for (int s = 0; s < 4; ++s) ms_out[s] = acc[s] / iters;
    return 0;
}
