// launch_common.h -- host plumbing shared by the voted launchers, LaunchWavefront (wavefront_kernels.hip) and LaunchPersistent
// (persistent_kernel.hip), and the ShadeVariant every render launcher takes.  Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "cpugpupt_abi.h"
#include "device_memory.h"
#include "kernel_variant.h"

namespace cgpt {

// Which instantiation of its render kernels a launcher runs: counters of cgpt_stats, lobe level (kernel_variant.h), resampled NEE (shade_device.hpp,
// above shade_bounce), top-level tree.  ChooseVariant (ctx_internal.h) makes it; the render mode and the call's size pick the rest inside the launcher.
struct ShadeVariant { bool count; uint32_t lobe_level; bool ris; bool tree; };
static inline uint32_t KernelLevel(ShadeVariant v) { return (uint32_t)KernelLevel((int)v.lobe_level, v.tree); }   // of the megakernel and the persistent kernel

// a HIP call of a launcher: on failure the context's error names the call (as HIP_TRY's does) and the launcher returns -1
#define LAUNCH_TRY(expr)                                                     \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess) { HipFail(ctx, #expr, e_); return -1; }        \
    } while (0)

// One knob table per launcher, for cgpt_set_tuning (per context, any time between renders) and the environment (process-wide
// defaults, read when a context first needs the launcher's state: prefix + name in upper case, clamped into the range)
template <typename T> struct Knob { const char* name; uint32_t T::*field; uint32_t lo, hi; };

template <typename T, size_t N> void LoadKnobsFromEnv(const Knob<T> (&knobs)[N], const char* prefix, T& tune)
{
    for (const Knob<T>& k : knobs) {
        char env[64];
        size_t n = 0;
        for (const char* c = prefix; *c && n + 1 < sizeof(env); ++c) env[n++] = *c;
        for (const char* c = k.name; *c && n + 1 < sizeof(env); ++c) env[n++] = (char)toupper((unsigned char)*c);
        env[n] = 0;
        const char* v = getenv(env);
        if (v && *v) tune.*(k.field) = (uint32_t)std::min<long>(std::max<long>(strtol(v, nullptr, 10), k.lo), k.hi);
    }
}

template <typename T, size_t N> const Knob<T>* FindKnob(const Knob<T> (&knobs)[N], const char* name)
{
    for (const Knob<T>& k : knobs)
        if (strcmp(k.name, name) == 0) return &k;
    return nullptr;
}

template <typename T> int SetKnob(cgpt_ctx* ctx, const Knob<T>* k, T& tune, const char* name, uint32_t value)
{
    if (!k) return CtxFail(ctx, CGPT_ERR_INVALID, "unknown tuning knob '%s'", name);
    if (value < k->lo || value > k->hi) return CtxFail(ctx, CGPT_ERR_INVALID, "tuning knob %s: %u outside [%u, %u]", name, value, k->lo, k->hi);
    tune.*(k->field) = value;
    return CGPT_OK;
}

inline hipError_t QueryCuCount(uint32_t& n_cus)                              // once per launcher state
{
    if (n_cus) return hipSuccess;
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) n_cus = (uint32_t)cus;
    return e;
}

// entries of a kernel table, of a slice of one, or of the host array that mirrors it
template <typename A> constexpr size_t TableCount(const A& table) { return sizeof(A) / sizeof(std::remove_all_extents_t<A>); }

// resident blocks per CU (at least 1) of n kernels of a table with `lds` bytes of dynamic LDS; beyond the default 48 KiB a kernel opts in
template <typename F> hipError_t QueryOccupancy(const F* kernels, uint32_t* blocks_per_cu, size_t n, int block_threads, size_t lds)
{
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < n && e == hipSuccess; ++i) {
        int b = 0;
        if (lds > 48u * 1024u) e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernels[i]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, kernels[i], block_threads, lds);
        blocks_per_cu[i] = (uint32_t)std::max(1, b);
    }
    return e;
}

// a launcher's buffer only grows; reallocating waits for the device first (earlier launches may still use the old one)
template <typename T> hipError_t Grow(DevBuf<T>& b, size_t n)
{
    if (b.n >= n) return hipSuccess;
    const hipError_t e = hipDeviceSynchronize();
    return e == hipSuccess ? b.Alloc(n) : e;
}

// hipEvent pairs around the launches of the last render, grow-only: ReserveEvents before it, hipEventRecord(NextEvent()) before and
// after each launch, ForEachPair once its device work has completed
struct EventPairs { hipEvent_t* ev = nullptr; uint32_t cap = 0, used = 0; };

inline int ReserveEvents(cgpt_ctx* ctx, EventPairs& e, uint32_t n)
{
    if (e.cap < n) {
        hipEvent_t* grown = static_cast<hipEvent_t*>(realloc(e.ev, (size_t)n * sizeof(hipEvent_t)));
        if (!grown) { CtxFail(ctx, CGPT_ERR_INVALID, "out of host memory"); return -1; }
        e.ev = grown;
        for (; e.cap < n; ++e.cap) LAUNCH_TRY(hipEventCreate(&e.ev[e.cap]));
    }
    e.used = 0;
    return 0;
}

inline hipEvent_t NextEvent(EventPairs& e) { return e.ev[e.used++]; }

template <typename F> void ForEachPair(EventPairs& e, F&& each)             // each(pair index, ms) of every pair that could be timed
{
    for (uint32_t i = 0; i + 1u < e.used; i += 2u) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, e.ev[i], e.ev[i + 1u]) == hipSuccess) each(i / 2u, ms);
    }
    e.used = 0;
}

inline void FreeEvents(EventPairs& e)
{
    for (uint32_t i = 0; i < e.cap; ++i) (void)hipEventDestroy(e.ev[i]);
    free(e.ev);
    e = EventPairs{};
}

}  // namespace cgpt
