// Device memory of libkoemorph_hip.so: the ONE place that calls the runtime's allocator.
//
// Ownership rule: whatever holds device memory holds it as a DevBuf member (or a local DevBuf for a scratch buffer), so freeing is
// the destructor's work and no entry point keeps a list of what to free.  A pointer INTO somebody else's allocation (a carved
// region, a slot handed to a launcher) stays a plain non-owning T*.  Every create / init / reserve entry point allocates first
// and writes the fields later calls use as their guard (n_streams, tr.windows, uploaded, ...) after the last allocation succeeded.
#pragma once

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdint>
#include <utility>

#include "koemorph.h"

namespace km {

int fail(int code, const char* fmt, ...);
// An allocation cannot be captured: inside a stream capture growth_refused fails with KM_ERR_WORKSPACE, before any HIP call.
int growth_refused(void* stream, const char* what, int64_t need, int64_t cap);

// bytes held by all live DevBufs of the process (km_live_device_bytes)
inline std::atomic<int64_t> g_live_device_bytes{0};

}  // namespace km

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                                                                        \
            (void)hipGetLastError(); /* the runtime keeps a failed call as its last error: do not leave it to the next launch check */ \
            return ::km::fail(KM_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));                                                     \
        }                                                                                                                              \
    } while (0)

namespace km {

// `n` elements of T on the device.  Non-copyable, movable; reads as a T* wherever the raw pointer used to stand.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    int64_t n = 0;      // capacity in elements

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    ~DevBuf() { release(); }

    operator T*() const { return p; }
    int64_t bytes() const { return n * (int64_t)sizeof(T); }

    // never fails: a buffer the runtime would not free is forgotten, not freed twice
    void release() {
        if (p) {
            if (hipFree(p) != hipSuccess) (void)hipGetLastError();
            g_live_device_bytes -= bytes();
        }
        p = nullptr; n = 0;
    }

    // a fresh allocation of `count` elements (contents undefined); empty on failure
    int alloc(int64_t count, const char* what) {
        release();
        if (count < 0 || (uint64_t)count > SIZE_MAX / sizeof(T)) return fail(KM_ERR_HIP, "%s: %lld elements cannot be allocated", what, (long long)count);
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, (size_t)count * sizeof(T));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(KM_ERR_HIP, "%s: hipMalloc of %lld bytes: %s", what, (long long)(count * (int64_t)sizeof(T)), hipGetErrorString(e));
        }
        p = static_cast<T*>(q); n = count;
        g_live_device_bytes += bytes();
        return KM_OK;
    }

    // grow-only: nothing when `need` fits; otherwise, once the stream has drained, a fresh allocation of `need` elements
    // (contents undefined).  Refused inside a stream capture, before any HIP call.
    int grow(int64_t need, void* stream, const char* what) {
        if (need <= n) return KM_OK;
        if (int rc = growth_refused(stream, what, need, n)) return rc;
        if (p) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        return alloc(need, what);
    }
};

// an event or a stream of the runtime, destroyed with its owner; reads as the raw handle
template <typename H, hipError_t (*Destroy)(H)>
struct DevHandle {
    H h = nullptr;
    DevHandle() = default;
    DevHandle(const DevHandle&) = delete;
    DevHandle& operator=(const DevHandle&) = delete;
    DevHandle(DevHandle&& o) noexcept : h(o.h) { o.h = nullptr; }
    DevHandle& operator=(DevHandle&& o) noexcept {
        if (this != &o) { reset(); h = o.h; o.h = nullptr; }
        return *this;
    }
    DevHandle& operator=(H created) { reset(); h = created; return *this; }
    ~DevHandle() { reset(); }
    operator H() const { return h; }
    void reset() {
        if (h && Destroy(h) != hipSuccess) (void)hipGetLastError();
        h = nullptr;
    }
};
using DevEvent = DevHandle<hipEvent_t, hipEventDestroy>;
using DevStream = DevHandle<hipStream_t, hipStreamDestroy>;

}  // namespace km
