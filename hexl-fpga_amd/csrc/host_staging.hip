// host_staging.hip -- the host-pointer (*_host) entry points of include/hexl_mi355x.h and the host runtime behind them: the
// copy-thread pool, the helper lane, the three-stream staging pipeline and the zero-copy lone keyswitch. Calls the device-pointer
// entry points of capi.hip; the CPU staging model (tests/cpp) compiles this file and capi.hip with g++ against a shim of the HIP host API.
//
// The reference stages every batch through device-visible memory (FPGAObject_*::fill_in_data / fill_out_data,
// host/src/fpga.cpp:329-518) with one batch in flight while the previous one is read back (:1517-1545). Here a
// batch is cut into sub-batches that flow through a 3-stage pipeline with double-buffered pinned and device
// slabs: CPU pack (parallel memcpy) -> H2D on its own stream -> kernels on the context stream -> D2H on a third
// stream -> CPU unpack, so PCIe traffic in both directions, the kernels and the host copies overlap.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "hexl_internal.hpp"

// the host's `result += output` per limb (host_simd.cpp)
void hx_add_mod_u64(uint64_t* r, const uint64_t* o, size_t n, uint64_t q);

static unsigned host_threads() {                                   // (thread-safe static: several device runners call this)
    static const unsigned n = [] {
        // 8: swept on the 256-thread boxes of this pool (round 3, HEXL_HOST_THREADS sweep of tests/cpp/bench_cxx_api): 2 / 4 / 8 / 12 / 32 / 64 copy threads move 12 / 21 / 26 / 27 /
        // 19 / 12 k keyswitch/s through the host-pointer API at worksize 1024 -- the copies are memory-bound, more threads only contend
        // (round 4: those pods run under a CFS quota of 16 cores, bench.py cpu_baseline.cgroup_cpu_quota_cores -- a host without one may want more)
        const unsigned v = (unsigned)hx_knob("HEXL_HOST_THREADS", std::min(8u, std::max(1u, std::thread::hardware_concurrency() / 2)));
        return v ? v : 1u;
    }();
    return n;
}

// Persistent host workers for the staging copies (spawning threads per sub-batch cost more than the copies:
// 64 threads measured slower than 8). Jobs are index ranges; several jobs may be in flight (the unpack of one
// sub-batch runs beside the pack of the next), workers drain them front to back.
namespace {
struct HostJob {
    std::function<void(size_t)> fn;
    size_t count = 0;
    std::atomic<size_t> next{0}, done{0};
};
class HostPool {
  public:
    static HostPool& get() { static HostPool p; return p; }
    std::shared_ptr<HostJob> submit(size_t count, std::function<void(size_t)> fn) {
        auto j = std::make_shared<HostJob>();
        j->fn = std::move(fn); j->count = count;
        if (!count) return j;
        { std::lock_guard<std::mutex> g(m_); jobs_.push_back(j); }
        cv_.notify_all();
        return j;
    }
    void wait(const std::shared_ptr<HostJob>& j) {
        if (!j) return;
        work_on(j.get());                                         // the caller helps instead of sleeping
        std::unique_lock<std::mutex> g(m_);
        done_cv_.wait(g, [&] { return j->done.load() >= j->count; });
    }
  private:
    HostPool() {
        const unsigned n = host_threads();
        for (unsigned t = 0; t + 1 < n; ++t) th_.emplace_back([this] { loop(); });
    }
    ~HostPool() {
        { std::lock_guard<std::mutex> g(m_); stop_ = true; }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    void work_on(HostJob* j) {
        for (size_t i; (i = j->next.fetch_add(1)) < j->count;) {
            j->fn(i);
            if (j->done.fetch_add(1) + 1 == j->count) { std::lock_guard<std::mutex> g(m_); done_cv_.notify_all(); }
        }
    }
    void loop() {
        hx_pin_own_thread();                                             // (the pool is created by the first copy: contexts exist by then)
        for (;;) {
            std::shared_ptr<HostJob> j;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [&] {
                    while (!jobs_.empty() && jobs_.front()->next.load() >= jobs_.front()->count) jobs_.pop_front();
                    return stop_ || !jobs_.empty();
                });
                if (stop_) return;
                j = jobs_.front();
            }
            work_on(j.get());
        }
    }
    std::mutex m_;
    std::condition_variable cv_, done_cv_;
    std::deque<std::shared_ptr<HostJob>> jobs_;
    std::vector<std::thread> th_;
    bool stop_ = false;
};
}  // namespace

static void parallel_for(size_t count, const std::function<void(size_t)>& fn) {
    if (count <= 1 || host_threads() <= 1) { for (size_t i = 0; i < count; ++i) fn(i); return; }
    HostPool::get().wait(HostPool::get().submit(count, fn));
}

// One persistent helper thread per calling thread (= per device runner): runs the posted jobs in order. The unpack of
// sub-batch k runs here beside the pack of sub-batch k + 2; a thread spawned per sub-batch (std::async) cost ~40 us each,
// a third of a single keyswitch's end-to-end time at worksize 1.
namespace {
class AsyncLane {
  public:
    AsyncLane() : th_([this] { loop(); }) {}
    ~AsyncLane() {
        { std::lock_guard<std::mutex> g(m_); stop_ = true; }
        cv_.notify_all();
        th_.join();
    }
    size_t post(std::function<void()> fn) {                       // returns the job's ticket
        size_t t;
        { std::lock_guard<std::mutex> g(m_); q_.push_back(std::move(fn)); t = ++posted_; }
        cv_.notify_all();
        return t;
    }
    void wait(size_t ticket) {
        std::unique_lock<std::mutex> g(m_);
        done_cv_.wait(g, [&] { return finished_ >= ticket; });
    }
  private:
    void loop() {
        hx_pin_own_thread();
        std::unique_lock<std::mutex> g(m_);
        for (;;) {
            cv_.wait(g, [&] { return stop_ || !q_.empty(); });
            if (q_.empty()) return;                               // stop requested and nothing left
            std::function<void()> fn = std::move(q_.front());
            q_.pop_front();
            g.unlock();
            fn();
            g.lock();
            ++finished_;
            done_cv_.notify_all();
        }
    }
    std::mutex m_;
    std::condition_variable cv_, done_cv_;
    std::deque<std::function<void()>> q_;
    size_t posted_ = 0, finished_ = 0;
    bool stop_ = false;
    std::thread th_;                                              // last member: starts after the others exist
};
}  // namespace

static int pipe_init(hexl_ctx* c) {
    if (c->s_up) return 0;
    HX_CHECK(hipStreamCreateWithFlags(&c->s_up, hipStreamNonBlocking));
    HX_CHECK(hipStreamCreateWithFlags(&c->s_down, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        HX_CHECK(hipEventCreateWithFlags(&c->ev_up[i], hipEventDisableTiming));
        HX_CHECK(hipEventCreateWithFlags(&c->ev_comp[i], hipEventDisableTiming));
        HX_CHECK(hipEventCreateWithFlags(&c->ev_down[i], hipEventDisableTiming));
    }
    return 0;
}

// pack(first, count, h_in)      fill the pinned input slab for items [first, first+count)
// compute(count, d_in, d_out)   enqueue kernels on c->stream
// unpack(first, count, h_out)   consume the pinned output slab
// `shared_bytes` at the head of every input slab is filled by pack_shared once per slab (tables, moduli).
struct PipeShape { size_t in1, out1, shared, sub; bool in_place; };

// HEXL_HOST_TRACE=1: microseconds since the call started at each step of a host-pointer call (stderr)
struct HostTrace {
    const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
    void operator()(const char* what, long sub /* sub-batch; < 0: the zero-copy lone keyswitch */) const {
        static const bool trace = hx_knob("HEXL_HOST_TRACE", 0) == 1;
        if (!trace) return;
        char where[32] = "zero-copy  ";
        if (sub >= 0) snprintf(where, sizeof where, "sub-batch %ld", sub);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[hexl host] %-22s %s  +%8.1f us  @%12.1f us\n", what, where, std::chrono::duration<double, std::micro>(now - t_begin).count(),
                fmod(std::chrono::duration<double, std::micro>(now.time_since_epoch()).count(), 1e8));
    }
};

static int run_pipeline(hexl_ctx* c, size_t batch, const PipeShape& sh,
                        const std::function<void(char*)>& pack_shared,
                        const std::function<void(size_t, size_t, char*)>& pack,
                        const std::function<int(size_t, char*, char*)>& compute,
                        const std::function<void(size_t, size_t, const char*)>& unpack) {
    int rc = pipe_init(c);
    if (rc) return rc;
    const HostTrace stamp;
    // at least four sub-batches once there are four items -- eight from 64 items up -- so that the stages overlap for small windows
    // too: the window's first upload and last unpack are exposed, and they shrink with the sub-batch (round 6 trace at worksize 128,
    // profiles/r06_host_trace_worksize128.txt: 1.7 ms of ramp-up with four sub-batches of 32)
    const size_t S = std::min(sh.sub, std::max<size_t>(1, batch >= 64 ? (batch + 7) / 8 : (batch + 3) / 4));
    const size_t in_slab = (sh.shared + S * sh.in1 + 255) & ~size_t(255);
    // in-place primitives compute inside the device input slab, but on the HOST side the download areas are separate from the upload
    // areas and there are FOUR of them (two of everything else): the unpack -- for a keyswitch the host's `result +=`, the slowest
    // stage of the pipeline -- of sub-batch k then only has to be finished before the download of sub-batch k + 4 is enqueued, not k + 2
    // (round 6: with two, every other download waited for an unpack and the copy engine idled behind the host)
    constexpr size_t HOUT = 4;
    const size_t out_slab = (S * (sh.in_place ? sh.in1 : sh.out1) + 255) & ~size_t(255);
    const size_t dset = in_slab + (sh.in_place ? 0 : out_slab);
    rc = c->d_stage.reserve(2 * dset);
    if (!rc) rc = c->h_stage.reserve(2 * in_slab + HOUT * out_slab);
    if (rc) return rc;
    // Sub-batch sizes: S each, but from 64 objects up the window OPENS with S/4 and S/2 and CLOSES with S/2 and S/4: the first upload +
    // kernels + download and the last unpack are exposed (nothing to overlap with), and they shrink with their sub-batch -- in steady
    // state the pipeline runs at the PCIe download rate (round 6: 16 objects per 0.55 ms at L = 6 = 45 GB/s), so a window costs that
    // plus ramp and tail (worksize 128: 1.2 ms of ramp with eight equal sub-batches)
    std::vector<size_t> sub_first, sub_cnt;
    {
        std::vector<size_t> head, tail;
        if (batch >= 64 && S >= 8) { head = {S / 4, S / 2}; tail = {S / 2, S / 4}; }
        size_t at = 0, closing = 0;
        for (size_t t : tail) closing += t;
        for (size_t h : head) { sub_first.push_back(at); sub_cnt.push_back(h); at += h; }
        while (at + closing < batch) { const size_t cnt = std::min(S, batch - closing - at); sub_first.push_back(at); sub_cnt.push_back(cnt); at += cnt; }
        for (size_t t : tail) { sub_first.push_back(at); sub_cnt.push_back(t); at += t; }
    }
    const size_t nsub = sub_first.size();
    auto h_in = [&](size_t k) { return c->h_stage + (k & 1) * in_slab; };
    auto d_in = [&](size_t k) { return c->d_stage + (k & 1) * dset; };
    auto h_out = [&](size_t k) { return c->h_stage + 2 * in_slab + (k % HOUT) * out_slab; };
    auto d_out = [&](size_t k) { return sh.in_place ? d_in(k) + sh.shared : d_in(k) + in_slab; };
    if (nsub == 1) {
        // one sub-batch: nothing to overlap with -- one stream, one synchronisation, the unpack on the calling thread
        if (sh.shared) pack_shared(h_in(0));
        pack(0, batch, h_in(0) + sh.shared);
        stamp("packed", 0);
        HX_CHECK(hipMemcpyAsync(d_in(0), h_in(0), sh.shared + batch * sh.in1, hipMemcpyHostToDevice, c->stream));
        rc = compute(batch, d_in(0), d_out(0));
        if (rc) return rc;
        HX_CHECK(hipMemcpyAsync(h_out(0), d_out(0), batch * (sh.in_place ? sh.in1 : sh.out1), hipMemcpyDeviceToHost, c->stream));
        stamp("enqueued", 0);
        HX_CHECK(hipStreamSynchronize(c->stream));
        stamp("download complete", 0);
        unpack(0, batch, h_out(0));
        stamp("done", 1);
        return 0;
    }
    // unpack(k) runs on the helper lane beside pack(k+2), strictly in submission order (a keyswitch unpack ACCUMULATES
    // into the caller's result, and the same result may appear in several sub-batches, benchmark/bench_keyswitch.cpp:
    // 113-131); it must be finished before the download of sub-batch k + HOUT is enqueued (same host download area)
    static thread_local AsyncLane lane;
    size_t ticket[HOUT] = {}, last_ticket = 0;
    struct Drain {                                                // the posted jobs reference this frame: never leave before them
        AsyncLane& l; size_t& t;
        ~Drain() { l.wait(t); }
    } drain{lane, last_ticket};
    for (size_t it = 0; it < nsub + 2; ++it) {
        if (it >= 2) {                                            // drain sub-batch it-2 (frees slab set it&1)
            const size_t k = it - 2, first = sub_first[k], cnt = sub_cnt[k];
            HX_CHECK(hipEventSynchronize(c->ev_down[k & 1]));
            stamp("download complete", k);
            const char* src = h_out(k);
            last_ticket = ticket[k % HOUT] = lane.post([&unpack, &stamp, first, cnt, src, k] { unpack(first, cnt, src); stamp("unpacked", k); });
        }
        if (it < nsub) {
            const size_t first = sub_first[it], cnt = sub_cnt[it];
            if (sh.shared) pack_shared(h_in(it));
            pack(first, cnt, h_in(it) + sh.shared);
            stamp("packed", it);
            HX_CHECK(hipMemcpyAsync(d_in(it), h_in(it), sh.shared + cnt * sh.in1, hipMemcpyHostToDevice, c->s_up));
            HX_CHECK(hipEventRecord(c->ev_up[it & 1], c->s_up));
            HX_CHECK(hipStreamWaitEvent(c->stream, c->ev_up[it & 1], 0));
            rc = compute(cnt, d_in(it), d_out(it));
            if (rc) break;
            HX_CHECK(hipEventRecord(c->ev_comp[it & 1], c->stream));
            HX_CHECK(hipStreamWaitEvent(c->s_down, c->ev_comp[it & 1], 0));
            lane.wait(ticket[it % HOUT]);                         // (the unpack of sub-batch it - HOUT: this download area's last reader)
            HX_CHECK(hipMemcpyAsync(h_out(it), d_out(it), cnt * (sh.in_place ? sh.in1 : sh.out1), hipMemcpyDeviceToHost,
                                    c->s_down));
            HX_CHECK(hipEventRecord(c->ev_down[it & 1], c->s_down));
            stamp("enqueued", it);
        }
    }
    lane.wait(last_ticket);
    stamp("done", nsub);
    return rc;
}

static size_t sub_batch_for(size_t bytes_per_item) {              // ~128 MB slabs (32 MB measured 15-25 % slower at worksize 1024)
    const size_t target = (size_t)hx_knob("HEXL_HOST_SUB_MB", 128) << 20;      // (read by every call)
    return std::max<size_t>(1, target / std::max<size_t>(1, bytes_per_item));
}

// ------------------------------------------------------------------------------- device-resident callers
// The reference's API takes plain pointers; callers that already keep their ciphertexts in device (or managed)
// memory can pass those pointers to the same entry points: no staging, the kernels run where the data lies.
// All payload pointers of one call must be of the same kind; small shared arrays (tables, moduli) may be either.
static bool on_device(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // plain host memory
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}
// 0: every pointer is host memory, 1: every pointer is device memory, -1: mixed
static int payload_kind(std::initializer_list<std::pair<const void* const*, size_t>> lists) {
    size_t dev = 0, total = 0;
    for (auto& l : lists)
        for (size_t i = 0; i < l.second; ++i) { dev += on_device(l.first[i]) ? 1 : 0; ++total; }
    return dev == 0 ? 0 : dev == total ? 1 : -1;
}
// a device copy of a small shared array that may live on either side (`slot` = which quarter of the scratch)
static int shared_to_device(hexl_ctx* c, const void* src, size_t bytes, int slot, const void** out) {
    if (on_device(src)) { *out = src; return 0; }
    const size_t quarter = (bytes + 255) & ~size_t(255);
    int rc = c->d_shared.reserve(4 * quarter);
    if (rc) return rc;
    char* dst = c->d_shared + slot * quarter;
    HX_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    *out = dst;
    return 0;
}

// f(first, count) for every maximal run of items that lie back to back in device memory: adjacent(j) = item j follows item j - 1
template <class Adj, class F>
static int for_each_run(size_t batch, Adj adjacent, F f) {
    int rc = 0;
    for (size_t i = 0, j; !rc && i < batch; i = j) {
        for (j = i + 1; j < batch && adjacent(j); ++j) {}
        rc = f(i, j - i);
    }
    return rc;
}

// both directions of the standalone transform: ntt(x, count, t0, t1) = hexl_ntt_fwd / hexl_ntt_inv on device pointers
template <class Ntt>
static int ntt_host(hexl_ctx* c, uint64_t* const* h_x, size_t batch, const uint64_t* h_t0, const uint64_t* h_t1, uint64_t n, Ntt ntt) {
    if (!c || !h_x || !h_t0 || !h_t1 || !hx_supported_ntt_n(n)) return HEXL_E_BADARG;
    if (!batch) return 0;
    HX_CHECK(hipSetDevice(c->device));
    const size_t one = n * 8;
    const int kind = payload_kind({{(const void* const*)h_x, batch}});
    if (kind < 0) return HEXL_E_BADARG;
    if (kind == 1) {                                               // device-resident polynomials: maximal contiguous runs
        const void *dr, *dp;
        int rc = shared_to_device(c, h_t0, one, 0, &dr);
        if (!rc) rc = shared_to_device(c, h_t1, one, 1, &dp);
        if (!rc) rc = for_each_run(batch, [&](size_t j) { return h_x[j] == h_x[j - 1] + n; },
                                   [&](size_t i, size_t cnt) { return ntt(h_x[i], cnt, (const u64*)dr, (const u64*)dp); });
        return rc ? rc : (int)hipStreamSynchronize(c->stream);
    }
    PipeShape sh{one, one, 2 * one, sub_batch_for(one), true};
    return run_pipeline(c, batch, sh,
        [&](char* h) { memcpy(h, h_t0, one); memcpy(h + one, h_t1, one); },
        [&](size_t first, size_t cnt, char* h) { parallel_for(cnt, [&](size_t b) { memcpy(h + b * one, h_x[first + b], one); }); },
        [&](size_t cnt, char* d, char* dout) { return ntt((u64*)dout, cnt, (const u64*)d, (const u64*)(d + one)); },
        [&](size_t first, size_t cnt, const char* h) { parallel_for(cnt, [&](size_t b) { memcpy(h_x[first + b], h + b * one, one); }); });
}

extern "C" int hexl_ntt_fwd_host(hexl_ctx* c, uint64_t* const* h_x, size_t batch, const uint64_t* h_roots,
                                 const uint64_t* h_precon, uint64_t q, uint64_t n) {
    return ntt_host(c, h_x, batch, h_roots, h_precon, n,
                    [&](u64* x, size_t cnt, const u64* r, const u64* p) { return hexl_ntt_fwd(c, x, cnt, r, p, q, n); });
}

extern "C" int hexl_ntt_inv_host(hexl_ctx* c, uint64_t* const* h_x, size_t batch, const uint64_t* h_ir,
                                 const uint64_t* h_ip, uint64_t q, uint64_t inv_n, uint64_t inv_n_w, uint64_t n) {
    return ntt_host(c, h_x, batch, h_ir, h_ip, n,
                    [&](u64* x, size_t cnt, const u64* r, const u64* p) { return hexl_ntt_inv(c, x, cnt, r, p, q, inv_n, inv_n_w, n); });
}

extern "C" int hexl_dyadic_multiply_host(hexl_ctx* c, uint64_t* const* h_out, const uint64_t* const* h_a,
                                         const uint64_t* const* h_b, size_t batch, uint64_t n,
                                         const uint64_t* const* h_moduli, uint64_t n_moduli) {
    if (!c || !h_out || !h_a || !h_b || !h_moduli) return HEXL_E_BADARG;
    if (!batch) return 0;
    HX_CHECK(hipSetDevice(c->device));
    const size_t op1 = 2 * n_moduli * n * 8, out1 = 3 * n_moduli * n * 8, mod1 = n_moduli * 8;
    const int kind = payload_kind({{(const void* const*)h_out, batch}, {(const void* const*)h_a, batch},
                                   {(const void* const*)h_b, batch}});
    if (kind < 0) return HEXL_E_BADARG;
    if (kind == 1)                                                 // device-resident operands and results
        return for_each_run(batch, [&](size_t j) { return h_out[j] == h_out[j - 1] + out1 / 8 && h_a[j] == h_a[j - 1] + op1 / 8 && h_b[j] == h_b[j - 1] + op1 / 8; },
                            [&](size_t i, size_t cnt) {
            // per-item moduli: gather the run's lists into one device array
            const void* dm = h_moduli[i];
            if (on_device(dm)) {                                   // must then be one contiguous device array, too
                for (size_t k = i + 1; k < i + cnt; ++k)
                    if (h_moduli[k] != h_moduli[k - 1] + n_moduli) return (int)HEXL_E_BADARG;
            } else {
                std::vector<u64> mods(cnt * n_moduli);
                for (size_t k = 0; k < cnt; ++k) memcpy(&mods[k * n_moduli], h_moduli[i + k], mod1);
                if (int rc = c->d_shared.reserve(mods.size() * 8)) return rc;
                HX_CHECK(hipMemcpy(c->d_shared, mods.data(), mods.size() * 8, hipMemcpyHostToDevice));
                dm = c->d_shared;
            }
            const int rc = hexl_dyadic_multiply(c, h_out[i], h_a[i], h_b[i], cnt, n, (const u64*)dm, n_moduli);
            return rc ? rc : (int)hipStreamSynchronize(c->stream);    // d_shared is reused by the next run
        });
    const size_t in1 = 2 * op1 + ((mod1 + 15) & ~size_t(15));   // per item: [a | b | moduli(padded)]
    PipeShape sh{in1, out1, 0, sub_batch_for(in1 + out1), false};
    // layout inside a slab holding cnt items: a[cnt] | b[cnt] | moduli[cnt] (contiguous batches for the kernel);
    // cnt*(2*op1 + mod1) <= cnt*in1 bytes, which is what the pipeline uploads
    return run_pipeline(c, batch, sh, [](char*) {},
        [&](size_t first, size_t cnt, char* h) {
            parallel_for(cnt, [&](size_t k) {
                memcpy(h + k * op1, h_a[first + k], op1);
                memcpy(h + cnt * op1 + k * op1, h_b[first + k], op1);
                memcpy(h + 2 * cnt * op1 + k * mod1, h_moduli[first + k], mod1);
            });
        },
        [&](size_t cnt, char* d, char* dout) {
            return hexl_dyadic_multiply(c, (u64*)dout, (u64*)d, (u64*)(d + cnt * op1), cnt, n, (u64*)(d + 2 * cnt * op1),
                                        n_moduli);
        },
        [&](size_t first, size_t cnt, const char* h) { parallel_for(cnt, [&](size_t k) { memcpy(h_out[first + k], h + k * out1, out1); }); });
}

// the host's `result += output` for one limb of one object (limb = k * L + i)
static void add_limb(const hexl_ks_plan* p, u64* res, const u64* out, size_t limb) {
    hx_add_mod_u64(res + limb * p->n, out + limb * p->n, p->n, p->moduli[limb % p->L]);   // host_simd.cpp (AVX-512 / AVX2 / portable)
}
// objects that share a result array must be added in order
static bool results_distinct(uint64_t* const* r, size_t cnt) {
    for (size_t a = 0; a < cnt; ++a)
        for (size_t b = a + 1; b < cnt; ++b)
            if (r[a] == r[b]) return false;
    return true;
}

// A LONE keyswitch (the SEAL bridge's call shape: set_worksize_KeySwitch(1), experimental/bridge-seal/tests/fpga_context.h:13-16) through
// the host-pointer entry point, ZERO-COPY (round 5). The staged pipeline spent 212 us per call at L = 6: pack 10, seven enqueues 22,
// [hipMemcpyAsync 0.8 MB up 29.5, four kernels 50, hipMemcpyAsync 1.6 MB down 43, gaps] 121, host accumulate 37, hand-overs 20
// (HEXL_HOST_TRACE=1). Here the kernels of the quarter-transform path (keyswitch_lat.hip) work on the pinned slabs themselves:
// k_ksq_intt pulls t_target across PCIe while it transforms, k_ksq_down pushes the output the same way (tools/zero_copy_probe: 18.7 us
// and 31.6 us for those bytes, overlapped with the arithmetic, against 29.5 + 43.2 us of copies around it) and publishes every finished
// quarter limb in a pinned word, so the host adds limb i into the caller's `result` (the reference's contract: the HOST accumulates,
// FPGAObject_KeySwitch::fill_out_data, fpga.cpp:441-475) while limbs i + 1 ... are still in flight. No copy engine, no memset, no
// stream synchronisation on the critical path; the range flag is a pinned word too.
static int keyswitch_host_lone(hexl_ks_plan* p, uint64_t* const* h_results, const uint64_t* const* h_t_targets, size_t batch) {
    hexl_ctx* c = p->ctx;
    const size_t n = p->n, L = p->L, tt = L * n * 8, rs = 2 * tt;
    const HostTrace trace;
    auto stamp = [&](const char* what) { trace(what, -1); };
    const size_t in_bytes = (batch * tt + 255) & ~size_t(255), out_bytes = (batch * rs + 255) & ~size_t(255);
    const size_t nflag = batch * 2 * L * 4;                                   // one word per quarter limb
    int rc = c->h_lone.reserve(in_bytes + out_bytes + 256 + nflag * sizeof(u32));
    if (rc) return rc;
    char* h_in = c->h_lone;
    char* h_out = h_in + in_bytes;
    u32* flag = (u32*)(h_out + out_bytes);
    u32* done = flag + 64;
    for (size_t b = 0; b < batch; ++b) memcpy(h_in + b * tt, h_t_targets[b], tt);
    __atomic_store_n(flag, 0u, __ATOMIC_RELAXED);                             // flag[0]: input-range flag, flag[1]: "the last kernel has started"
    __atomic_store_n(flag + 1, 0u, __ATOMIC_RELAXED);
    memset(done, 0, nflag * sizeof(u32));
    stamp("packed");
    const u32 epoch = ++c->lone_epoch ? c->lone_epoch : ++c->lone_epoch;      // never 0
    p->host_done = done; p->host_flag = flag; p->host_epoch = epoch; p->overwrite_result = true;
    rc = hexl_keyswitch(p, (u64*)h_out, (const u64*)h_in, batch);              // pinned slabs: device-visible at their host addresses
    p->host_done = nullptr; p->host_flag = nullptr; p->overwrite_result = false;
    if (rc) return rc;
    stamp("enqueued");
    // a quarter limb has landed when its word shows this call's epoch (released by the kernel behind the data); a launch that died
    // never publishes: give up after the stream has gone idle without it
    // (spinning pool workers share the process-wide HostPool with other device runners: after a few thousand polls they yield)
    auto relax = [](unsigned spins) {
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
        if ((spins & 0xFFF) == 0xFFF) std::this_thread::yield();
    };
    std::atomic<bool> lost{false};
    auto wait_word = [&](const u32* w) -> bool {
        for (unsigned spins = 0; __atomic_load_n(w, __ATOMIC_ACQUIRE) != epoch; ++spins) {
            if (lost.load(std::memory_order_relaxed)) return false;
            if ((spins & 0xFFFF) == 0xFFFF && hipStreamQuery(c->stream) != hipErrorNotReady && __atomic_load_n(w, __ATOMIC_ACQUIRE) != epoch) {
                lost.store(true);
                return false;
            }
            relax(spins);
        }
        return true;
    };
    auto wait_limb = [&](size_t x) {                                            // x = b * 2L + limb: its four quarters
        return wait_word(done + x * 4) && wait_word(done + x * 4 + 1) && wait_word(done + x * 4 + 2) && wait_word(done + x * 4 + 3);
    };
    if (results_distinct(h_results, batch)) {
        // the calling thread alone until the LAST kernel starts (its arithmetic takes ~15 us before the first limb crosses PCIe) ...
        wait_word(flag + 1);
        stamp("last kernel started");
        // ... then one job per limb: the pool's workers wake up during that arithmetic and add limb x while limbs x + 1 ... are in flight
        parallel_for(batch * 2 * L, [&](size_t x) { if (wait_limb(x)) add_limb(p, h_results[x / (2 * L)], (const u64*)(h_out + (x / (2 * L)) * rs), x % (2 * L)); });
    } else {
        HX_CHECK(hipStreamSynchronize(c->stream));
        for (size_t b = 0; b < batch; ++b)
            for (size_t limb = 0; limb < 2 * L; ++limb) add_limb(p, h_results[b], (const u64*)(h_out + b * rs), limb);
    }
    if (lost.load()) {
        const hipError_t e = hipStreamSynchronize(c->stream);
        fprintf(stderr, "[hexl_mi355x] lone keyswitch: the launch finished without publishing its results (%s)\n", hipGetErrorString(e));
        return e != hipSuccess ? (int)e : (int)hipErrorUnknown;
    }
    // every quarter limb of the LAST kernel has been published, so the launch is over as far as these slabs and the plan's scratch
    // are concerned; the next launch on the stream is ordered behind it anyway
    stamp("done");
    return __atomic_load_n(flag, __ATOMIC_ACQUIRE) ? HEXL_W_RANGE : 0;
}

extern "C" int hexl_keyswitch_host(hexl_ks_plan* p, uint64_t* const* h_results, const uint64_t* const* h_t_targets,
                                   size_t batch) {
    if (!p || !h_results || !h_t_targets) return HEXL_E_BADARG;
    if (!batch) return 0;
    hexl_ctx* c = p->ctx;
    HX_CHECK(hipSetDevice(c->device));
    const size_t n = p->n, L = p->L;
    const size_t tt = L * n * 8, rs = 2 * tt;
    const int kind = payload_kind({{(const void* const*)h_results, batch}, {(const void* const*)h_t_targets, batch}});
    if (kind < 0) return HEXL_E_BADARG;
    if (kind == 1) {
        // device-resident ciphertexts: the kernels accumulate straight into `result`. A run ends where the arrays stop
        // being contiguous or a result array repeats (two instances of one launch must not update the same words;
        // launches on one stream are ordered, which keeps the reference's submission-order semantics)
        int rc = 0;
        // the status covers THIS call's objects, as on the staged path below: whatever an earlier hexl_keyswitch on the plan left in
        // the flag is for hexl_ks_range_check before this call (only the staged branch cleared it)
        if (p->use_f64) HX_CHECK(hipMemsetAsync(p->d_flag, 0, sizeof(u32), c->stream));
        rc = for_each_run(batch, [&](size_t j) { return h_results[j] == h_results[j - 1] + rs / 8 && h_t_targets[j] == h_t_targets[j - 1] + tt / 8; },
                          [&](size_t i, size_t cnt) { return hexl_keyswitch(p, h_results[i], h_t_targets[i], cnt); });
        // the status covers this call, as on the staged path below: the kernels' range flag is read (and cleared) here too
        if (!rc) rc = p->use_f64 ? hexl_ks_range_check(p) : (int)hipStreamSynchronize(c->stream);
        return rc;
    }
    // a lone keyswitch (or the few that still take the quarter-transform path): zero-copy, no staging pipeline. HEXL_HOST_ZERO_COPY=0
    // keeps the staged route (comparisons)
    static const bool zero_copy = hx_knob("HEXL_HOST_ZERO_COPY", 1) != 0;
    // (one quarter-transform launch must cover the whole call -- its completion words and output gate are per launch: a batch that
    // HEXL_KS_CHUNK would cut into several chunks takes the staged route)
    if (zero_copy && p->use_f64 && p->have_keys && batch <= 8 && batch <= hx_ks_chunk(p) && hx_ks_lat_applies(p, batch) && hx_ks_can_overwrite(p, batch))
        return keyswitch_host_lone(p, h_results, h_t_targets, batch);
    // The FP64 kernels flag t_target words that are not below their modulus (the device-side result buffer starts at zero or
    // is written here, so `result` is the host's business). The status covers THIS call: the flag is cleared on the stream
    // before the first launch (whatever earlier hexl_keyswitch launches on the plan left in it is for hexl_ks_range_check,
    // before this call), every sub-batch's launch is followed by a 4-byte copy of the still accumulating flag into the pinned
    // mirror, and the pipeline's own last synchronisation covers the last copy -- no extra stream synchronisation per call.
    if (p->use_f64) { *p->h_flag = 0; HX_CHECK(hipMemsetAsync(p->d_flag, 0, sizeof(u32), c->stream)); }
    PipeShape sh{tt, rs, 0, sub_batch_for(tt + rs), false};
    // Like the reference, the device produces the keyswitch output only (the kernels accumulate into a zeroed
    // buffer) and the HOST adds it into the caller's result in submission order
    // (FPGAObject_KeySwitch::fill_out_data, fpga.cpp:441-475). This keeps the semantics when several objects of a
    // batch alias the same result array, as benchmark/bench_keyswitch.cpp:113-131 does; it also means `result`
    // never crosses PCIe upwards.
    const int rc_pipe = run_pipeline(c, batch, sh, [](char*) {},
        [&](size_t first, size_t cnt, char* h) {
            if (cnt >= 4) parallel_for(cnt, [&](size_t b) { memcpy(h + b * tt, h_t_targets[first + b], tt); });
            else for (size_t b = 0; b < cnt; ++b) memcpy(h + b * tt, h_t_targets[first + b], tt);
        },
        [&](size_t cnt, char* d, char* dout) {
            // small sub-batches run on kernels that can WRITE their output: no zeroed buffer to prepare and to read back
            const bool ow = hx_ks_can_overwrite(p, cnt);
            if (!ow) HX_CHECK(hipMemsetAsync(dout, 0, cnt * rs, c->stream));
            p->overwrite_result = ow;
            const int rc = hexl_keyswitch(p, (u64*)dout, (u64*)d, cnt);
            p->overwrite_result = false;
            if (!rc && p->use_f64) HX_CHECK(hipMemcpyAsync(p->h_flag, p->d_flag, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
            return rc;
        },
        [&](size_t first, size_t cnt, const char* h) {
            // distinct results: one job per (item, limb) -- a lone keyswitch (worksize 1) still spreads over 2 L threads
            if (results_distinct(h_results + first, cnt))
                parallel_for(cnt * 2 * L, [&](size_t x) { add_limb(p, h_results[first + x / (2 * L)], (const u64*)(h + (x / (2 * L)) * rs), x % (2 * L)); });
            else
                for (size_t b = 0; b < cnt; ++b)
                    for (size_t limb = 0; limb < 2 * L; ++limb) add_limb(p, h_results[first + b], (const u64*)(h + b * rs), limb);
        });
    if (rc_pipe) return rc_pipe;
    return (p->use_f64 && *p->h_flag) ? HEXL_W_RANGE : 0;
}
