// devbuf_selftest.cpp -- TEST INFRASTRUCTURE, CPU only: the host scaffold of hexl-fpga_amd/csrc/hexl_internal.hpp (the owning buffer type
// HxBuf and the argument-check vocabulary) on the CPU shim of the HIP host API, through the REAL capi.hip: a context and a plan are
// created by the C-ABI, every buffer either of them owns is reserved, reserved smaller (pointer and capacity stay), reserved larger
// (capacity grows) and the allocate-once helper is run, then both are destroyed. Built with -fsanitize=address,undefined: a buffer
// that escaped the release is a leak report, a double release a heap error, and either fails tests/test_devbuf_selftest.py.
// The second half calls every predicate of the vocabulary at its edges and asserts the decisions the entry points made before the
// predicates were shared (each is quoted beside its checks).
//   g++ -std=c++17 -g -fsanitize=address,undefined -Ihip_shim -x c++ devbuf_selftest.cpp ../../hexl-fpga_amd/csrc/capi.hip
//       stage_model_stubs.cpp ../../hexl-fpga_amd/csrc/host_simd.cpp
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "../../hexl-fpga_amd/csrc/hexl_internal.hpp"

// the shim's hipMalloc reports a failed posix_memalign: the allocator has to return null for the size the failure test asks for
extern "C" const char* __asan_default_options() { return "allocator_may_return_null=1"; }

static int g_failed = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

static bool is_prime(u64 q) {
    for (u64 d = 3; d * d <= q; d += 2)
        if (q % d == 0) return false;
    return q > 2 && (q & 1);
}
// `count` primes = 1 mod 2n below 2^bits
static std::vector<u64> primes(u64 n, int bits, int count) {
    std::vector<u64> out;
    for (u64 q = ((1ULL << bits) / (2 * n)) * 2 * n + 1 - 2 * n; (int)out.size() < count; q -= 2 * n)
        if (is_prime(q)) out.push_back(q);
    return out;
}

// grow-only: first reservation, a smaller one (nothing moves), a larger one (capacity grows)
template <class B>
static void exercise(B& buf, const char* name) {
    const size_t had = buf.capacity(), first = had + 100;
    CHECK(buf.reserve(first) == 0);
    CHECK(buf.get() != nullptr && buf.capacity() == first);
    const void* at = buf.get();
    CHECK(buf.reserve(first / 2) == 0);
    CHECK(buf.get() == at && buf.capacity() == first);
    CHECK(buf.reserve(first) == 0);
    CHECK(buf.get() == at && buf.capacity() == first);
    CHECK(buf.reserve(2 * first) == 0);
    CHECK(buf.get() != nullptr && buf.capacity() == 2 * first);
    std::memset(buf.get(), 0x5a, 2 * first * sizeof(*buf.get()));    // the whole capacity is ours (ASan watches the bounds)
    CHECK(static_cast<const void*>(buf) == buf.get());
    std::printf("  %-14s %zu -> %zu -> %zu elements\n", name, had, first, 2 * first);
}

// allocate-once: filled from the host at the first call, untouched by the second, empty after a failure
template <class T>
static void exercise_upload(HxDevBuf<T>& buf, const char* name) {
    buf.release();
    CHECK(buf.get() == nullptr && buf.capacity() == 0);
    std::vector<T> host(37), other(64);
    std::memset(host.data(), 0x11, host.size() * sizeof(T));
    std::memset(other.data(), 0x22, other.size() * sizeof(T));
    // a size no allocator grants: the helper reports it and leaves the member empty
    CHECK(buf.upload_once(host.data(), SIZE_MAX / sizeof(T) / 2) != 0);
    CHECK(buf.get() == nullptr && buf.capacity() == 0);
    CHECK(buf.upload_once(host.data(), host.size()) == 0);
    CHECK(buf.get() != nullptr && buf.capacity() == host.size());
    CHECK(std::memcmp(buf.get(), host.data(), host.size() * sizeof(T)) == 0);      // (the shim's device memory is host memory)
    const void* at = buf.get();
    CHECK(buf.upload_once(other.data(), other.size()) == 0);
    CHECK(buf.get() == at && buf.capacity() == host.size());
    CHECK(std::memcmp(buf.get(), host.data(), host.size() * sizeof(T)) == 0);
    std::printf("  %-14s uploaded once\n", name);
}

static void test_buffers() {
    std::printf("buffers\n");
    const u64 n = 1024, L = 2, K = 3;
    const std::vector<u64> q = primes(n, 30, (int)K);
    const std::vector<u64> msf(K, 1);
    hexl_ctx* c = nullptr;
    hexl_ks_plan* p = nullptr;
    CHECK(hexl_ctx_create(0, &c) == 0 && c);
    CHECK(hexl_ks_plan_create(c, n, L, K, L, 2, q.data(), msf.data(), nullptr, &p) == 0 && p);
    if (!c || !p) return;
    CHECK(p->use_f64 && p->d_mods_f64.capacity() == K && p->d_tables_f64.capacity() == K * 4 * n);
    CHECK(p->d_mods.capacity() == K && p->d_tables.capacity() == K * 4 * n && p->d_flag.capacity() == 4 && p->h_flag.capacity() == 2);
    CHECK(p->d_keys_f64.capacity() == L * (L + 1) * 2 * n && p->d_keys_x.capacity() == L * (L + 1) * 2 * n);
    CHECK(!p->d_keys && !p->d_keys_nat);                            // integer keys: integer plans; natural-order keys: n = 16384
    // a plan's tables stay where plan_create put them when the helper runs again
    const void* mods_at = p->d_mods_f64.get();
    const KsModF64 dummy[3] = {};
    CHECK(p->d_mods_f64.upload_once(dummy, 3) == 0 && p->d_mods_f64.get() == mods_at);
#define EX(owner, member) exercise(owner->member, #member)
    EX(c, d_stage); EX(c, d_shared); EX(c, h_stage); EX(c, h_lone); EX(c, d_meta); EX(c, d_ntt_redo); EX(c, d_ntt_tab); EX(c, h_ntt_hint);
    EX(p, d_mods); EX(p, d_tables); EX(p, d_keys); EX(p, d_mods_f64); EX(p, d_tables_f64); EX(p, d_keys_f64); EX(p, d_keys_x);
    EX(p, d_keys_nat); EX(p, d_scratch); EX(p, d_flag); EX(p, h_flag); EX(p, d_rescale); EX(p, d_rs_s); EX(p, d_rot_t); EX(p, d_bsgs_b);
    EX(p, d_bsgs_t); EX(p, d_emb_roots); EX(p, d_emb_perm); EX(p, d_garner); EX(p, d_enc_coeffs); EX(p, d_enc_words);
#undef EX
    exercise_upload(p->d_emb_roots, "d_emb_roots");
    exercise_upload(p->d_emb_perm, "d_emb_perm");
    exercise_upload(p->d_garner, "d_garner");
    exercise_upload(p->d_rescale, "d_rescale");
    // a buffer on its own: released by hand, then released again by its destructor
    {
        HxDevBuf<u64> lone;
        CHECK(lone.reserve(8) == 0 && lone.capacity() == 8);
        lone.release();
        CHECK(!lone && lone.capacity() == 0);
        CHECK(lone.reserve(4) == 0 && lone.capacity() == 4);
    }
    CHECK(hexl_ks_plan_destroy(p) == 0);
    CHECK(hexl_ctx_destroy(c) == 0);
}

static void test_checks() {
    std::printf("argument checks\n");
    hexl_ks_plan p;                                                // fields only: nothing here touches the device
    p.n = 1024; p.logn = 10; p.L = 2; p.K = 3; p.use_f64 = true;
    const u64 K = p.K;

    // "p && p->use_f64 && p->logn >= 10 && p->logn <= 15 && n_limbs >= 1 && n_limbs <= p->K" (rns_plan_ok, rl_plan_ok, enc_args_ok)
    CHECK(!hx_f64_plan_ok(&p, 0, 1, K));
    CHECK(hx_f64_plan_ok(&p, 1, 1, K));
    CHECK(hx_f64_plan_ok(&p, K, 1, K));
    CHECK(!hx_f64_plan_ok(&p, K + 1, 1, K));
    // "n_limbs < 2 || n_limbs > p->K - 1" refused (hexl_rescale)
    CHECK(!hx_f64_plan_ok(&p, 0, 2, K - 1));
    CHECK(!hx_f64_plan_ok(&p, 1, 2, K - 1));
    CHECK(hx_f64_plan_ok(&p, K - 1, 2, K - 1));
    CHECK(!hx_f64_plan_ok(&p, K, 2, K - 1));
    CHECK(!hx_f64_plan_ok(&p, K + 1, 2, K - 1));
    CHECK(!hx_f64_plan_ok(nullptr) && !hx_f64_plan_ok(nullptr, 1, 1, 1));
    CHECK(hx_f64_plan_ok(&p));
    p.use_f64 = false; CHECK(!hx_f64_plan_ok(&p) && !hx_f64_plan_ok(&p, 1, 1, K)); p.use_f64 = true;
    p.logn = 9;  CHECK(!hx_f64_plan_ok(&p));
    p.logn = 16; CHECK(!hx_f64_plan_ok(&p));
    p.logn = 15; CHECK(hx_f64_plan_ok(&p));
    p.logn = 10;
    // "n_components < 1 || n_components > 3" refused; hexl_rlwe_decrypt: 2 or 3
    CHECK(!hx_in_range(0, 1, 3) && hx_in_range(1, 1, 3) && hx_in_range(3, 1, 3) && !hx_in_range(4, 1, 3));
    CHECK(!hx_in_range(1, 2, 3) && hx_in_range(2, 2, 3));

    // "count > SIZE_MAX / per" refused, per = comps * limbs * n * 8 bytes
    for (u64 comps = 1; comps <= 3; ++comps) {
        const size_t per = size_t(comps) * K * p.n * sizeof(u64), most = SIZE_MAX / per;
        size_t bytes = 1;
        CHECK(hx_words_bytes(0, comps, K, p.n, &bytes) && bytes == 0);
        CHECK(hx_words_bytes(1, comps, K, p.n, &bytes) && bytes == per);
        CHECK(hx_words_bytes(most, comps, K, p.n, &bytes) && bytes == most * per);
        CHECK(!hx_words_bytes(most + 1, comps, K, p.n, &bytes));
        CHECK(!hx_words_bytes(SIZE_MAX, comps, K, p.n, &bytes));
    }
    // hexl_apply_galois: "count > (SIZE_MAX / sizeof(u64)) / n" refused
    {
        size_t bytes;
        const size_t most = (SIZE_MAX / sizeof(u64)) / 32768;
        CHECK(hx_words_bytes(most, 1, 1, 32768, &bytes) && bytes == most * 32768 * 8);
        CHECK(!hx_words_bytes(most + 1, 1, 1, 32768, &bytes));
    }
    // the workgroup transforms: "count > MAX_GRID / n_limbs" refused, MAX_GRID = 0x7fffffff
    static_assert(HX_MAX_GRID == 0x7fffffffu, "the x dimension of a launch");
    CHECK(hx_wg_grid_ok(0, K) && hx_wg_grid_ok(0x7fffffffu / K, K) && !hx_wg_grid_ok(0x7fffffffu / K + 1, K));
    CHECK(hx_wg_grid_ok(0x7fffffffu, 1) && !hx_wg_grid_ok(0x80000000u, 1));
    // the word-wise kernels: "batch > MAX_GRID / (n_limbs * (n >> 10))" refused; grid = instances x limbs x n / 1024
    static_assert(HX_WW_THREADS == 256 && HX_WW_LOG_CHUNK == 10, "256 lanes, 1024-word pieces");
    CHECK(hx_ww_grid(&p, 5, K) == 5 * K && hx_ww_grid(&p, 5, K, 9) == 5 * K * 2);
    CHECK(hx_ww_grid_ok(&p, 0x7fffffffu / K, K) && !hx_ww_grid_ok(&p, 0x7fffffffu / K + 1, K));
    p.n = 32768; p.logn = 15;
    CHECK(hx_ww_grid(&p, 5, K) == 5 * K * 32 && hx_ww_grid(&p, 5, 2, 9) == 5 * 2 * 64);
    CHECK(hx_ww_grid_ok(&p, 0x7fffffffu / (K * 32), K) && !hx_ww_grid_ok(&p, 0x7fffffffu / (K * 32) + 1, K));
    p.n = 1024; p.logn = 10;

    // "pt_batch != 1 && pt_batch != batch" refused; per instance when pt_batch == batch; "(batch ? pt_batch : 0) * per" bytes read
    const size_t per = 4096;
    HxPtBatch pb;
    CHECK(!hx_pt_batch(0, 3, per, &pb));
    CHECK(hx_pt_batch(1, 3, per, &pb) && pb.stride == 0 && pb.bytes == per);
    CHECK(hx_pt_batch(3, 3, per, &pb) && pb.stride == 1 && pb.bytes == 3 * per);
    CHECK(!hx_pt_batch(4, 3, per, &pb));
    CHECK(!hx_pt_batch(2, 3, per, &pb));
    CHECK(hx_pt_batch(0, 0, per, &pb) && pb.stride == 1 && pb.bytes == 0);
    CHECK(hx_pt_batch(1, 0, per, &pb) && pb.stride == 0 && pb.bytes == 0);
    CHECK(!hx_pt_batch(2, 0, per, &pb));
    CHECK(hx_pt_batch(1, 1, per, &pb) && pb.stride == 1 && pb.bytes == per);
    CHECK(!hx_pt_batch(0, 1, per, &pb) && !hx_pt_batch(2, 1, per, &pb));

    // "[a, a + abytes) and [b, b + bbytes) share a byte"
    alignas(16) static char mem[64];
    CHECK(!hx_ranges_overlap(mem, 16, mem + 16, 16) && !hx_ranges_overlap(mem + 16, 16, mem, 16));      // they touch
    CHECK(hx_ranges_overlap(mem, 17, mem + 16, 16) && hx_ranges_overlap(mem + 16, 16, mem, 17));        // one byte shared
    CHECK(hx_ranges_overlap(mem, 16, mem, 16) && hx_ranges_overlap(mem, 64, mem + 8, 1));
    // an empty range (the plaintext of an empty batch) shares nothing at either end of the other one; strictly inside, the formula says yes
    CHECK(!hx_ranges_overlap(mem, 0, mem, 16) && !hx_ranges_overlap(mem + 16, 0, mem, 16) && !hx_ranges_overlap(mem, 16, mem + 16, 0));
    CHECK(!hx_ranges_overlap(mem, 0, mem + 8, 0) && hx_ranges_overlap(mem + 8, 0, mem, 16));

    // "lazy = tier[0]; any tier[i] != tier[0] for 1 <= i < n_limbs: lazy = -1"
    p.tier[0] = 3; p.tier[1] = 3; p.tier[2] = 12;
    CHECK(hx_level_tier(&p, 1) == 3 && hx_level_tier(&p, 2) == 3 && hx_level_tier(&p, 3) == -1);
    p.tier[0] = 0; p.tier[1] = 12;
    CHECK(hx_level_tier(&p, 1) == 0 && hx_level_tier(&p, 2) == -1);
    p.tier[1] = 0; p.tier[2] = 0;
    CHECK(hx_level_tier(&p, 3) == 0);

    // "for (c0 = 0; c0 < count; c0 += chunk) { nb = min(count - c0, chunk); if (rc) return rc; }"
    std::vector<std::pair<size_t, size_t>> seen;
    CHECK(hx_for_chunks(10, 4, [&](size_t c0, size_t nb) { seen.push_back({c0, nb}); return 0; }) == 0);
    CHECK((seen == std::vector<std::pair<size_t, size_t>>{{0, 4}, {4, 4}, {8, 2}}));
    seen.clear();
    CHECK(hx_for_chunks(8, 4, [&](size_t c0, size_t nb) { seen.push_back({c0, nb}); return 0; }) == 0);
    CHECK((seen == std::vector<std::pair<size_t, size_t>>{{0, 4}, {4, 4}}));
    seen.clear();
    CHECK(hx_for_chunks(3, 3, [&](size_t c0, size_t nb) { seen.push_back({c0, nb}); return 0; }) == 0 && seen.size() == 1);
    seen.clear();
    CHECK(hx_for_chunks(0, 0, [&](size_t c0, size_t nb) { seen.push_back({c0, nb}); return 0; }) == 0 && seen.empty());
    CHECK(hx_for_chunks(10, 4, [&](size_t c0, size_t nb) { seen.push_back({c0, nb}); return c0 ? 7 : 0; }) == 7 && seen.size() == 2);
}

int main() {
    test_buffers();
    test_checks();
    if (g_failed) { std::printf("%d check(s) FAILED\n", g_failed); return 1; }
    std::printf("ALL PASSED\n");
    return 0;
}
