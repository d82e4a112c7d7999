// device_memory.h -- who owns device memory, and how a failed HIP call or a C++ exception becomes a return code.  Host code only.
//   DevAlloc / DevFree   the only callers of hipMalloc / hipFree in csrc/, with a process-wide count of the live bytes
//   DevBuf<T>            move-only owner of a device array; DevEvent / DevStream own a hipEvent_t / hipStream_t
//   HIP_TRY(ctx, expr)   a HIP call of a function that returns a cgpt_status: on failure "<expr> failed: <hip text>" and CGPT_ERR_HIP
//   Guarded(ctx, what, f) the wall in front of the C ABI: nothing f throws unwinds through it
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <exception>
#include <mutex>
#include <unordered_map>

#include "cpugpupt_abi.h"

namespace cgpt {

// the message of a failed call; ctx null: the text cgpt_last_error(nullptr) returns (cgpt_ctx_create has no context yet)
int CtxFail(cgpt_ctx* ctx, int code, const char* fmt, ...);

inline int HipFail(cgpt_ctx* ctx, const char* call, hipError_t e) { return CtxFail(ctx, CGPT_ERR_HIP, "%s failed: %s", call, hipGetErrorString(e)); }

#define HIP_TRY(ctx, expr)                                                   \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess) return ::cgpt::HipFail((ctx), #expr, e_);      \
    } while (0)

template <class F> int Guarded(cgpt_ctx* ctx, const char* what, F&& body)
{
    try {
        return body();
    } catch (const std::exception& e) {
        return CtxFail(ctx, CGPT_ERR_INVALID, "%s: %s", what, e.what());
    } catch (...) {
        return CtxFail(ctx, CGPT_ERR_INVALID, "%s: unknown exception", what);
    }
}

// The bytes asked of hipMalloc and not yet given back (cgpt_debug_live_device_bytes).  A group's worker threads allocate their pools
// side by side: the count is atomic, the sizes by pointer sit behind a mutex.  Never destroyed: contexts may outlive static destructors.
struct DevLedger {
    std::atomic<uint64_t> live{ 0 };
    std::mutex m;
    std::unordered_map<void*, size_t> bytes;
};
inline DevLedger& Ledger() { static DevLedger* const l = new DevLedger; return *l; }

inline hipError_t DevAlloc(void** p, size_t bytes)
{
    *p = nullptr;
    const hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) { *p = nullptr; return e; }
    DevLedger& l = Ledger();
    std::lock_guard<std::mutex> lk(l.m);
    l.bytes[*p] = bytes;
    l.live += bytes;
    return hipSuccess;
}

inline void DevFree(void* p)
{
    if (!p) return;
    {
        DevLedger& l = Ledger();
        std::lock_guard<std::mutex> lk(l.m);
        const auto it = l.bytes.find(p);
        if (it != l.bytes.end()) { l.live -= it->second; l.bytes.erase(it); }
    }
    (void)hipFree(p);
}

// n elements at p, released with the owner.  How a buffer changes size is its site's policy: Alloc is "exactly n, whatever was there",
// Grow "at least n"; neither waits for the device (launch_common.h: Grow(DevBuf&, n) of the persistent launcher does first).
template <typename T> struct DevBuf {
    T* p = nullptr;
    size_t n = 0;

    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { Reset(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    ~DevBuf() { Reset(); }

    void Reset() { DevFree(p); p = nullptr; n = 0; }
    hipError_t Alloc(size_t count)
    {
        Reset();
        const hipError_t e = DevAlloc((void**)&p, count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    hipError_t Grow(size_t count) { return n >= count ? hipSuccess : Alloc(count); }
};

struct DevEvent {
    hipEvent_t e = nullptr;
    DevEvent() = default;
    DevEvent(const DevEvent&) = delete;
    DevEvent& operator=(const DevEvent&) = delete;
    ~DevEvent() { if (e) (void)hipEventDestroy(e); }
    hipError_t Create() { return hipEventCreate(&e); }
};

struct DevStream {
    hipStream_t s = nullptr;
    DevStream() = default;
    DevStream(const DevStream&) = delete;
    DevStream& operator=(const DevStream&) = delete;
    ~DevStream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t Create(unsigned flags) { return hipStreamCreateWithFlags(&s, flags); }
};

}  // namespace cgpt
