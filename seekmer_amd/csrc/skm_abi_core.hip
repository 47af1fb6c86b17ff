// C ABI of libseekmer_hip.so: this thread's error message, the device calls, the page-locked arena
// and the diagnostic probes (gathers, scan, sort).
#include "skm_abi.h"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>

using namespace skm;
using namespace skm::abi;

namespace {

thread_local std::string g_error;

}  // namespace

namespace skm {
namespace abi __attribute__((visibility("hidden"))) {

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
    return code;
}

const std::string &last_message() { return g_error; }
void set_message(const std::string &message) { g_error = message; }

int set_device(int device)
{
    HIP_TRY(hipSetDevice(device));
    return SKM_OK;
}

int check_device(int device)
{
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (device < 0 || device >= n_dev) return fail(SKM_ERR_ARG, "device %d out of range", device);
    return SKM_OK;
}

}  // namespace abi
}  // namespace skm

// ------------------------------------------------------------------- errors
extern "C" const char *skm_last_error(void) { return g_error.c_str(); }

extern "C" int skm_device_count(int *count)
{
    if (!count) return fail(SKM_ERR_ARG, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        *count = 0;
        return fail(SKM_ERR_NO_DEVICE, "no HIP device: %s", hipGetErrorString(e));
    }
    *count = n;
    return SKM_OK;
}

extern "C" int skm_device_malloc(int device, int64_t bytes, void **out)
{
    if (!out || bytes < 0) return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(set_device(device));
    HIP_TRY(hipMalloc(out, (size_t)std::max<int64_t>(bytes, 1)));
    return SKM_OK;
}

extern "C" int skm_device_free(int device, void *ptr)
{
    SKM_TRY(set_device(device));
    if (ptr) HIP_TRY(hipFree(ptr));
    return SKM_OK;
}

extern "C" int skm_device_upload(int device, void *dst, const void *src, int64_t bytes)
{
    if (!dst || !src || bytes < 0) return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(set_device(device));
    HIP_TRY(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyHostToDevice));
    return SKM_OK;
}

extern "C" int skm_device_download(int device, void *dst, const void *src, int64_t bytes)
{
    if (!dst || !src || bytes < 0) return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(set_device(device));
    HIP_TRY(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost));
    return SKM_OK;
}

extern "C" int skm_device_synchronize(int device)
{
    SKM_TRY(set_device(device));
    HIP_TRY(hipDeviceSynchronize());
    return SKM_OK;
}

// Page-locked host memory: a batch handed over from it crosses the link at the full PCIe rate
// and asynchronously (no staging copy by the runtime).  Plain C allocator signatures so that
// libseekmer_host.so's FASTQ reader can take them as its slab allocator (skm_fastq_set_allocator).
namespace {

std::atomic<int> g_pinned_device{0};

void *pinned_direct(size_t bytes)
{
    void *p = nullptr;
    const int want = g_pinned_device.load();
    int current = 0;
    if (hipGetDevice(&current) != hipSuccess) return nullptr;
    if (current != want && hipSetDevice(want) != hipSuccess) return nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable);
    if (current != want) (void)hipSetDevice(current);
    return e == hipSuccess ? p : nullptr;
}

// One page-locked arena per process for the FASTQ readers' pieces.  Page-locking is slow
// (hipHostMalloc: about a millisecond per megabyte, one call at a time inside the driver) and a
// reader asks for a few dozen pieces of a megabyte or two in its first milliseconds -- measured: 19
// concurrent calls that end 15 ms later, the parse waiting behind them.  The arena is page-locked
// ONCE, by a helper thread that skm_pinned_set_device starts (infer.run calls it before it loads the
// index, so the reservation runs under the index upload), and handed out first-fit; a request it
// cannot serve (too large, arena full, no arena) is page-locked on its own as before.
struct PinnedArena {
    std::mutex mu;
    std::condition_variable cv;
    bool started = false, ready = false;
    std::thread helper;
    char *base = nullptr;
    size_t bytes = 0;
    std::map<size_t, size_t> free_at;          // offset -> length of every free range
    std::unordered_map<size_t, size_t> live;   // offset -> length handed out
    ~PinnedArena() { if (helper.joinable()) helper.join(); }
} g_arena;

size_t arena_size()
{
    size_t mb = 128;
    if (const char *v = getenv("SKM_PINNED_ARENA_MB")) mb = (size_t)std::max(0L, atol(v));
    return mb << 20;
}

}  // namespace

extern "C" int skm_pinned_set_device(int device)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(SKM_ERR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= count) return fail(SKM_ERR_ARG, "no GPU %d", device);
    g_pinned_device.store(device);
    std::lock_guard<std::mutex> hold(g_arena.mu);
    if (!g_arena.started && arena_size() > 0) {
        g_arena.started = true;
        g_arena.helper = std::thread([device]() {
            const size_t want = arena_size();
            void *p = nullptr;
            if (hipSetDevice(device) != hipSuccess || hipHostMalloc(&p, want, hipHostMallocPortable) != hipSuccess) p = nullptr;
            std::lock_guard<std::mutex> hold(g_arena.mu);
            g_arena.base = (char *)p;
            g_arena.bytes = p ? want : 0;
            if (p) g_arena.free_at[0] = want;
            g_arena.ready = true;
            g_arena.cv.notify_all();
        });
    }
    return SKM_OK;
}

// (called from the FASTQ readers' worker threads, which never chose a device: page-lock against the
// process's GPU, not against GPU 0, and portably, so that any device of the process may copy from it)
extern "C" void *skm_pinned_alloc(size_t bytes)
{
    const size_t need = (std::max<size_t>(bytes, 1) + 4095) & ~(size_t)4095;
    {
        std::unique_lock<std::mutex> hold(g_arena.mu);
        if (g_arena.started && need <= arena_size() / 8) {
            // (a reservation in progress is worth waiting for: a call of our own would queue behind it)
            g_arena.cv.wait(hold, [] { return g_arena.ready; });
            for (auto it = g_arena.free_at.begin(); it != g_arena.free_at.end(); ++it) {
                if (it->second < need) continue;
                const size_t at = it->first, rest = it->second - need;
                g_arena.free_at.erase(it);
                if (rest) g_arena.free_at[at + need] = rest;
                g_arena.live[at] = need;
                return g_arena.base + at;
            }
        }
    }
    return pinned_direct(bytes);
}

extern "C" void skm_pinned_free(void *p)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> hold(g_arena.mu);
        if (g_arena.base && (char *)p >= g_arena.base && (char *)p < g_arena.base + g_arena.bytes) {
            const size_t at = (size_t)((char *)p - g_arena.base);
            auto it = g_arena.live.find(at);
            if (it == g_arena.live.end()) return;
            size_t len = it->second, from = at;
            g_arena.live.erase(it);
            auto next = g_arena.free_at.lower_bound(from);          // merge with the free neighbours
            if (next != g_arena.free_at.end() && next->first == from + len) { len += next->second; next = g_arena.free_at.erase(next); }
            if (next != g_arena.free_at.begin()) {
                auto prev = std::prev(next);
                if (prev->first + prev->second == from) { from = prev->first; len += prev->second; g_arena.free_at.erase(prev); }
            }
            g_arena.free_at[from] = len;
            return;
        }
    }
    (void)hipHostFree(p);
}

// Diagnostic: random 16-byte gathers over a zero-filled table of `table_bytes`
// (power of two).  chain=0: independent gathers (throughput); chain=1: each
// address depends on the previous slot (latency under load).
extern "C" int skm_device_gather_ceiling(int device, int64_t table_bytes, int blocks, int per_lane,
                                         int chain, double *gathers_per_second)
{
    if (!gathers_per_second || table_bytes < 4096 || (table_bytes & (table_bytes - 1)) || blocks < 1
            || per_lane < 4)
        return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(set_device(device));
    DevMem table, sink;
    HIP_TRY(hipMalloc(table.out(), (size_t)table_bytes));
    HIP_TRY(hipMalloc(sink.out(), 8));
    HIP_TRY(hipMemset(table, 0, (size_t)table_bytes));
    Event e0, e1;
    HIP_TRY(hipEventCreate(e0.out()));
    HIP_TRY(hipEventCreate(e1.out()));
    launch_gather_probe(table, (uint64_t)table_bytes / 16, blocks, per_lane, chain, (unsigned long long *)sink.get(),
                        nullptr);   // warm-up
    HIP_TRY(hipEventRecord(e0, nullptr));
    launch_gather_probe(table, (uint64_t)table_bytes / 16, blocks, per_lane, chain, (unsigned long long *)sink.get(),
                        nullptr);
    HIP_TRY(hipEventRecord(e1, nullptr));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    *gathers_per_second = (double)blocks * 256.0 * per_lane / (ms * 1e-3);
    return SKM_OK;
}

// Diagnostics: the scan and the stable radix sort of skm_quant_setup.hip on the caller's arrays, as the class
// views, the unit grouping and the census run them -- upload, the production call, download (tests pin them to numpy).
// The device outputs are filled with 0xff first: an entry the kernels fail to write then shows as that, not as whatever
// the pool's block held before (the right answer of an earlier call, perhaps).
extern "C" int skm_device_scan_probe(int device, const int64_t *in, int64_t n, int in_place, int64_t *out)
{
    SKM_TRY(check_device(device));
    if (n < 0 || n >= (1LL << 31) || !out || (n && !in)) return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(set_device(device));
    DBuf<int64_t> d_in, d_out;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    SKM_TRY(d_out.ensure((size_t)n + 1));
    if (!in_place) SKM_TRY(d_in.ensure((size_t)std::max<int64_t>(n, 1)));
    int64_t *src = in_place ? d_out.p : d_in.p;
    HIP_TRY(hipMemsetAsync(d_out.p, 0xff, ((size_t)n + 1) * 8, nullptr));
    if (n) HIP_TRY(hipMemcpy(src, in, (size_t)n * 8, hipMemcpyHostToDevice));
    if (exclusive_scan_total_i64(src, d_out.p, n, nullptr) != 0)
        return fail(SKM_ERR_HIP, "scanning %lld values: %s", (long long)n, quant_setup_failure());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost));
    drain.dismiss();                          // (the copy home has waited for the kernels)
    return SKM_OK;
}

namespace {

template <class K>
int sort_probe(int (*sort)(const K *, K *, const int32_t *, int32_t *, int64_t, int, hipStream_t), const void *keys,
               const int32_t *vals, int64_t n, int end_bit, void *keys_out, int32_t *vals_out)
{
    DBuf<K> d_keys, d_keys_out; DBuf<int32_t> d_vals, d_vals_out;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    const size_t room = (size_t)n;
    SKM_TRY(d_keys.ensure(room)); SKM_TRY(d_keys_out.ensure(room)); SKM_TRY(d_vals.ensure(room)); SKM_TRY(d_vals_out.ensure(room));
    HIP_TRY(hipMemsetAsync(d_keys_out.p, 0xff, room * sizeof(K), nullptr));
    HIP_TRY(hipMemsetAsync(d_vals_out.p, 0xff, room * 4, nullptr));
    HIP_TRY(hipMemcpy(d_keys.p, keys, room * sizeof(K), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_vals.p, vals, room * 4, hipMemcpyHostToDevice));
    if (sort(d_keys.p, d_keys_out.p, d_vals.p, d_vals_out.p, n, end_bit, nullptr) != 0)
        return fail(SKM_ERR_HIP, "sorting %lld pairs: %s", (long long)n, quant_setup_failure());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(keys_out, d_keys_out.p, room * sizeof(K), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(vals_out, d_vals_out.p, room * 4, hipMemcpyDeviceToHost));
    drain.dismiss();                          // (the copies home have waited for the kernels)
    return SKM_OK;
}

}  // namespace

extern "C" int skm_device_sort_probe(int device, int key_kind, const void *keys, const int32_t *vals, int64_t n, int end_bit,
                                     void *keys_out, int32_t *vals_out)
{
    SKM_TRY(check_device(device));
    if (n < 0 || n >= (1LL << 31) || key_kind < 0 || key_kind > 2 || end_bit < 0 || end_bit > (key_kind == 1 ? 64 : 32)
            || (n && (!keys || !vals || !keys_out || !vals_out)))
        return fail(SKM_ERR_ARG, "bad argument");
    if (n == 0) return SKM_OK;
    SKM_TRY(set_device(device));
    if (key_kind == 0) return sort_probe<uint32_t>(sort_pairs_u32, keys, vals, n, end_bit, keys_out, vals_out);
    if (key_kind == 1) return sort_probe<unsigned long long>(sort_pairs_u64, keys, vals, n, end_bit, keys_out, vals_out);
    return sort_probe<int32_t>(sort_pairs_i32, keys, vals, n, end_bit, keys_out, vals_out);
}
