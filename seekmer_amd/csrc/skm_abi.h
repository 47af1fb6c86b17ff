// What the units of the C ABI glue (skm_abi*.hip) share: error reporting, the early-return macros,
// and the owners of device buffers and other HIP resources.  For those units only (each names `skm` and
// `skm::abi` with using-directives of its own).  Internal to libseekmer_hip.so: the
// namespace is hidden wherever it is opened, headers and units alike (the attribute covers only the block
// it stands on), so nothing shared between units reaches the dynamic symbol table.
#pragma once
#include "../../include/seekmer_hip.h"
#include "skm_kernels.h"
#include "skm_pool.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>

namespace skm {
namespace abi __attribute__((visibility("hidden"))) {

// records this thread's message (what skm_last_error returns) and hands `code` back
int fail(int code, const char *fmt, ...);
// this thread's message: a worker reads it to keep it with the failed job, the thread that waits for the job
// sets it again (the variable itself stays in skm_abi_core.hip)
const std::string &last_message();
void set_message(const std::string &message);

#define HIP_TRY(call)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(SKM_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                               \
    } while (0)

// SKM_TRACE_STALE=1: report (and clear) a HIP error that some earlier call left behind (tuning aid)
#define STALE_CHECK(where)                                                                           \
    do {                                                                                             \
        static const bool trace_stale_ = getenv("SKM_TRACE_STALE") != nullptr;                       \
        if (trace_stale_) {                                                                          \
            const hipError_t s_ = hipGetLastError();                                                 \
            if (s_ != hipSuccess) fprintf(stderr, "[skm] stale HIP error at %s: %s\n", where, hipGetErrorString(s_)); \
        }                                                                                            \
    } while (0)

#define SKM_TRY(call)          \
    do {                       \
        int rc_ = (call);      \
        if (rc_ != SKM_OK) return rc_; \
    } while (0)

// device buffer that only ever grows; its block goes back to the pool with it (a block that a
// stream may still use: drain that stream before the buffer goes)
template <class T>
struct DBuf {
    T *p = nullptr;
    size_t cap = 0;      // elements
    DBuf() = default;
    DBuf(const DBuf &) = delete;
    DBuf &operator=(const DBuf &) = delete;
    DBuf(DBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DBuf &operator=(DBuf &&o) noexcept
    {
        if (this != &o) { pool_free(p); p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); }
        return *this;
    }
    ~DBuf() { pool_free(p); }
    int ensure(size_t n, bool keep = false, hipStream_t stream = nullptr)
    {
        if (n <= cap) return SKM_OK;
        size_t want = std::max(n, cap + cap / 2);
        T *q = nullptr;
        HIP_TRY(pool_alloc((void **)&q, want * sizeof(T)));
        want = pool_round(want * sizeof(T)) / sizeof(T);
        if (keep && p && cap) {
            HIP_TRY(hipMemcpyAsync(q, p, cap * sizeof(T), hipMemcpyDeviceToDevice, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
        pool_free(p);
        p = q;
        cap = want;
        return SKM_OK;
    }
};

// One HIP resource of another kind -- a stream, an event, a pinned block, hipMalloc'd memory --
// handed back by `Free` (to the pool or to the runtime) when its owner goes.  Reads as the handle.
template <class H, auto Free>
class Own {
public:
    Own() = default;
    explicit Own(H h) : h_(h) {}
    Own(const Own &) = delete;
    Own &operator=(const Own &) = delete;
    ~Own() { reset(); }
    operator H() const { return h_; }
    H get() const { return h_; }
    H operator->() const { return h_; }
    H *out() { reset(); return &h_; }          // for the call that acquires a new one
    void reset(H h = nullptr) { if (h_) (void)Free(h_); h_ = h; }
    H release() { return std::exchange(h_, nullptr); }     // hand the resource to another owner

private:
    H h_ = nullptr;
};

inline void pool_event_release_plain(hipEvent_t e) { pool_event_release(e, false); }
inline void pool_event_release_timing(hipEvent_t e) { pool_event_release(e, true); }

using PoolStream = Own<hipStream_t, pool_stream_release>;
using PoolEvent = Own<hipEvent_t, pool_event_release_plain>;
using PoolTimingEvent = Own<hipEvent_t, pool_event_release_timing>;
using PoolPinned = Own<unsigned long long *, pool_pinned_release>;
using Stream = Own<hipStream_t, hipStreamDestroy>;
using Event = Own<hipEvent_t, hipEventDestroy>;
using HostPinned = Own<unsigned long long *, hipHostFree>;
using DevMem = Own<void *, hipFree>;

// runs a clean-up on every exit of the enclosing scope unless dismissed (the HIP_TRY / SKM_TRY
// macros return from the middle of a function)
template <class F>
struct ScopeGuard {
    F f;
    bool armed = true;
    explicit ScopeGuard(F fn) : f(fn) {}
    ~ScopeGuard() { if (armed) f(); }
    void dismiss() { armed = false; }
};
template <class F> ScopeGuard<F> on_exit(F f) { return ScopeGuard<F>(f); }
// (scratch that kernels on a stream use goes back to the pool, where another stream may get it at
// once, only after that stream has drained: a function declares its scratch BEFORE the guard that
// synchronises the stream on an early return -- destroyed in reverse order, the guard runs first)

int set_device(int device);
// SKM_ERR_NO_DEVICE without a GPU, SKM_ERR_ARG for a `device` outside [0, skm_device_count)
int check_device(int device);

}  // namespace abi
}  // namespace skm

