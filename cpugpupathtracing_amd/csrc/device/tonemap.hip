// tonemap.hip -- the display stage (gfx950): cgpt_tonemap, cgpt_read_exposure, cgpt_exposure_reset.
// Linear radiance -- the accumulator, a filter call's result, or an uploaded image -- to {r, g, b, 1} and packed pixels: auto exposure
// from a luminance histogram, a tone curve, the sRGB transfer function.  csrc/host/tonemap.h states every step once, for these kernels
// and the host mirror (tonemap.cpp); nothing below restates arithmetic.  Three kernels on the context's stream, no host wait between:
//   luminance_histogram<FROM_ACCUMULATOR>   the 256 bin counts and the ignored pixels' tally, into the context's table
//   exposure_resolve                        one block: metering, adaptation, exposure -> the record; clears the table
//   tonemap_pixels<CURVE, TRANSFER, FROM_ACCUMULATOR>   curve, transfer, pack; reads the exposure from the record (manual mode: an argument)
// The counts are integers: the order in which the atomics arrive does not change them.  There is no CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "cpugpupt_abi.h"
#include "ctx_internal.h"
#include "tonemap.h"

namespace cgpt {
namespace {

constexpr uint32_t kBlock = 256, kWaves = kBlock / 64u;
constexpr uint32_t kTableWords = kTonemapBins + 1u;                            // the counts, then the ignored pixels
constexpr uint32_t kPixelsPerBlock = 4u * kBlock;                              // a block strides over at least this many (TonemapGrid)

template <bool FROM_ACCUMULATOR>
__device__ __forceinline__ float4 source_pixel(const float4* __restrict__ src, size_t i, float n)
{
    float4 c = src[i];                                                         // 16 bytes a lane, consecutive lanes on consecutive pixels
    if (FROM_ACCUMULATOR) { c.x = AccumulatorChannel(c.x, n); c.y = AccumulatorChannel(c.y, n); c.z = AccumulatorChannel(c.z, n); }
    return c;
}

// One histogram per wave in LDS (4 KB a block): the lanes of a wave contend only among themselves.  After the barrier thread t sums bin
// t of the four and adds a non-zero sum to the table with one device-scope atomic, so a block issues at most 257 of them whatever it read.
template <bool FROM_ACCUMULATOR>
__global__ void __launch_bounds__(kBlock) luminance_histogram(const float4* __restrict__ src, size_t n_pixels, float n_samples, uint32_t* __restrict__ table)
{
    __shared__ uint32_t bins[kWaves][kTonemapBins];
    __shared__ uint32_t ignored[kWaves];
    const uint32_t t = threadIdx.x, wave = t >> 6;
    for (uint32_t w = 0; w < kWaves; ++w) bins[w][t] = 0u;
    if (t < kWaves) ignored[t] = 0u;
    __syncthreads();
    uint32_t my_ignored = 0;
    for (size_t i = (size_t)blockIdx.x * kBlock + t; i < n_pixels; i += (size_t)gridDim.x * kBlock) {
        const float4 c = source_pixel<FROM_ACCUMULATOR>(src, i, n_samples);
        const int b = LuminanceBin(Luminance(c.x, c.y, c.z));
        if (b >= 0) atomicAdd(&bins[wave][b], 1u);
        else my_ignored += 1u;
    }
    if (my_ignored) atomicAdd(&ignored[wave], my_ignored);
    __syncthreads();
    const uint32_t sum = (bins[0][t] + bins[1][t]) + (bins[2][t] + bins[3][t]);
    if (sum) atomicAdd(&table[t], sum);
    if (t == 0) {
        const uint32_t ig = (ignored[0] + ignored[1]) + (ignored[2] + ignored[3]);
        if (ig) atomicAdd(&table[kTonemapBins], ig);
    }
}

struct ResolveArgs {
    uint32_t* table;
    cgpt_exposure_info* record;
    double m_adapted;                                                          // the context's, as it was before this call
    uint32_t have_adapted;
    float low_fraction, high_fraction, alpha, key, exposure_scale;
    int32_t ev_bias;
};

// One block.  Every thread moves its bin from the table to the record and clears the table's word; thread 0 then meters the 256 counts
// with tonemap.h's own loop (256 short steps on one lane: a few microseconds, and one statement of the trimming) and writes the record.
__global__ void __launch_bounds__(kBlock) exposure_resolve(const ResolveArgs a)
{
    __shared__ uint32_t counts[kTonemapBins];
    const uint32_t t = threadIdx.x;
    const uint32_t c = a.table[t];
    counts[t] = c;
    a.record->histogram[t] = c;
    a.table[t] = 0u;
    __syncthreads();
    if (t != 0) return;
    const uint32_t n_ignored = a.table[kTonemapBins];
    a.table[kTonemapBins] = 0u;
    double m = 0.0, m_adapted = a.m_adapted;
    uint64_t n_counted = 0;
    uint32_t valid = a.have_adapted ? CGPT_EXPOSURE_ADAPTED : 0u;
    if (MeterHistogram(counts, a.low_fraction, a.high_fraction, &m, &n_counted)) {
        m_adapted = AdaptIndex(a.m_adapted, a.have_adapted != 0u, m, a.alpha);
        valid = CGPT_EXPOSURE_ADAPTED | CGPT_EXPOSURE_METERED;
    }
    cgpt_exposure_info* const r = a.record;
    r->mean_index = m;
    r->adapted_index = m_adapted;
    r->exposure = (valid & CGPT_EXPOSURE_ADAPTED) ? AutoExposure(m_adapted, a.key, a.exposure_scale, a.ev_bias) : ManualExposure(a.exposure_scale, a.ev_bias);
    r->valid = valid;
    r->n_counted = n_counted;
    r->n_ignored = n_ignored;
}

// record null: manual mode, the exposure is the argument; otherwise exposure_resolve's (a uniform address: a scalar load)
template <uint32_t CURVE, uint32_t TRANSFER, bool FROM_ACCUMULATOR>
__global__ void __launch_bounds__(kBlock) tonemap_pixels(const float4* __restrict__ src, size_t n_pixels, float n_samples, const cgpt_exposure_info* __restrict__ record,
                                                         float manual_exposure, float white, float4* __restrict__ out, uint32_t* __restrict__ pixels)
{
    const float exposure = record ? record->exposure : manual_exposure;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_pixels; i += (size_t)gridDim.x * kBlock) {
        const float4 c = source_pixel<FROM_ACCUMULATOR>(src, i, n_samples);
        const float r = ApplyTransfer<TRANSFER>(ApplyCurve<CURVE>(c.x, exposure, white));
        const float g = ApplyTransfer<TRANSFER>(ApplyCurve<CURVE>(c.y, exposure, white));
        const float b = ApplyTransfer<TRANSFER>(ApplyCurve<CURVE>(c.z, exposure, white));
        out[i] = float4{ r, g, b, 1.0f };
        pixels[i] = PackPixel(r, g, b);
    }
}

using PixelKernel = decltype(&tonemap_pixels<0u, 0u, false>);
template <uint32_t CURVE> PixelKernel PixelKernelOf(uint32_t transfer, bool acc)
{
    return transfer == CGPT_TRANSFER_SRGB ? (acc ? tonemap_pixels<CURVE, CGPT_TRANSFER_SRGB, true> : tonemap_pixels<CURVE, CGPT_TRANSFER_SRGB, false>)
                                          : (acc ? tonemap_pixels<CURVE, CGPT_TRANSFER_LINEAR, true> : tonemap_pixels<CURVE, CGPT_TRANSFER_LINEAR, false>);
}
PixelKernel PickPixelKernel(uint32_t curve, uint32_t transfer, bool acc)
{
    switch (curve) {
    case CGPT_CURVE_REINHARD: return PixelKernelOf<CGPT_CURVE_REINHARD>(transfer, acc);
    case CGPT_CURVE_ACES: return PixelKernelOf<CGPT_CURVE_ACES>(transfer, acc);
    case CGPT_CURVE_HABLE: return PixelKernelOf<CGPT_CURVE_HABLE>(transfer, acc);
    default: return PixelKernelOf<CGPT_CURVE_CLAMP>(transfer, acc);
    }
}

// The grid of the two pixel kernels: eight blocks a CU -- the 2 048 threads a CU holds, so one wave of blocks covers the chip -- and never
// more blocks than there are runs of kPixelsPerBlock pixels, so a small image is strided too.  The global atomics of a histogram are at
// most 257 a block: bounded by the chip, not by the image.
uint32_t TonemapGrid(uint32_t n_cus, size_t n_pixels)
{
    const size_t runs = (n_pixels + kPixelsPerBlock - 1u) / kPixelsPerBlock;
    return (uint32_t)std::min<size_t>((size_t)n_cus * 8u, std::max<size_t>(runs, 1u));
}

struct Source {
    cgpt_ctx* dev;                 // the one-device context whose device, stream and buffers do the work
    const float4* pixels;          // null for CGPT_TONEMAP_HOST until the upload
    size_t n;
    float n_samples;               // the accumulator's divisor
    bool accumulator;
};

// the source of a call, or its refusal; nothing is launched or copied here except a multi-device context's gather
int ResolveSource(cgpt_ctx* ctx, const cgpt_tonemap_params& p, Source& s)
{
    cgpt_ctx* const d = ctx->group ? GroupFirstMember(ctx) : ctx;
    s.dev = d; s.pixels = nullptr; s.n_samples = 1.0f; s.accumulator = false;
    if (p.source == CGPT_TONEMAP_HOST) { s.n = (size_t)p.src_width * p.src_height; return CGPT_OK; }
    if (!ctx->has_scene || !d->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "cgpt_tonemap: no scene uploaded");
    uint32_t width = ctx->width, rows = ctx->n_rows, num_accumulated = ctx->num_accumulated, debug = ctx->last_debug_mode;
    if (ctx->group) { GroupFrameInfo(ctx, &width, &rows, &num_accumulated, &debug); }
    else if (!ctx->fb.accumulator.p) width = 0;
    if (width == 0) return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_tonemap: nothing rendered yet");
    if (p.source == CGPT_TONEMAP_DENOISED) {
        if (!d->denoised) return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_tonemap: no denoised result: no filter call has succeeded since the last render, reset or restore");
        s.pixels = d->denoised; s.n = d->denoised_n;
        return CGPT_OK;
    }
    if (num_accumulated == 0) return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_tonemap: nothing accumulated (num_accumulated is 0)");
    if (debug != 0u) return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_tonemap: the last render was a debug view (debug_render_mode %u): its pixels are not radiance", debug);
    s.n = (size_t)width * rows; s.n_samples = (float)num_accumulated; s.accumulator = true;
    s.pixels = ctx->fb.accumulator.p;                                          // a group's: the gathered frame, once the outputs are checked
    return CGPT_OK;
}

// the device half of a call that was accepted: upload, the kernels, the read-back, and on success the context's state
int Launch(cgpt_ctx* ctx, const cgpt_tonemap_params& p, Source& s, float* dst_rgba, uint32_t* dst_pixels)
{
    cgpt_ctx* const d = s.dev;
    TonemapBuffers& tm = d->tm;
    const bool automatic = (p.flags & CGPT_TONEMAP_AUTO_EXPOSURE) != 0u;
    HIP_TRY(ctx, hipSetDevice(d->device));
    HIP_TRY(ctx, QueryCuCount(d->tonemap_cus));
    HIP_TRY(ctx, tm.out.Grow(s.n));
    HIP_TRY(ctx, tm.pixels.Grow(s.n));
    if (p.source == CGPT_TONEMAP_HOST) {
        HIP_TRY(ctx, tm.src.Grow(s.n));
        HIP_TRY(ctx, hipMemcpyAsync(tm.src.p, p.src_rgba, s.n * sizeof(float4), hipMemcpyHostToDevice, d->stream));
        s.pixels = tm.src.p;
    }
    const dim3 grid(TonemapGrid(d->tonemap_cus, s.n)), block(kBlock);
    if (automatic) {
        if (!tm.table.p) {
            HIP_TRY(ctx, tm.table.Alloc(kTableWords));
            HIP_TRY(ctx, tm.record.Alloc(1));
            HIP_TRY(ctx, hipMemsetAsync(tm.table.p, 0, kTableWords * sizeof(uint32_t), d->stream));
        }
        hipLaunchKernelGGL((s.accumulator ? luminance_histogram<true> : luminance_histogram<false>), grid, block, 0, d->stream, s.pixels, s.n, s.n_samples, tm.table.p);
        HIP_TRY(ctx, hipGetLastError());
        const ResolveArgs a = { tm.table.p, tm.record.p, d->m_adapted_valid ? d->m_adapted : 0.0, d->m_adapted_valid ? 1u : 0u,   // no reading: reported as 0
                                p.low_fraction, p.high_fraction, p.alpha, p.key, p.exposure_scale, p.ev_bias };
        hipLaunchKernelGGL(exposure_resolve, dim3(1), block, 0, d->stream, a);
        HIP_TRY(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(PickPixelKernel(p.curve, p.transfer, s.accumulator), grid, block, 0, d->stream, s.pixels, s.n, s.n_samples,
                       automatic ? (const cgpt_exposure_info*)tm.record.p : nullptr, ManualExposure(p.exposure_scale, p.ev_bias), p.white, tm.out.p, tm.pixels.p);
    HIP_TRY(ctx, hipGetLastError());
    cgpt_exposure_info info;
    if (automatic) HIP_TRY(ctx, hipMemcpyAsync(&info, tm.record.p, sizeof(info), hipMemcpyDeviceToHost, d->stream));
    if (dst_rgba) HIP_TRY(ctx, hipMemcpyAsync(dst_rgba, tm.out.p, s.n * sizeof(float4), hipMemcpyDeviceToHost, d->stream));
    if (dst_pixels) HIP_TRY(ctx, hipMemcpyAsync(dst_pixels, tm.pixels.p, s.n * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(ctx, hipStreamSynchronize(d->stream));
    if (automatic) {                                                           // the call succeeded: its reading becomes the context's
        d->exposure_info = info; d->exposure_info_valid = true;
        d->m_adapted = info.adapted_index; d->m_adapted_valid = (info.valid & CGPT_EXPOSURE_ADAPTED) != 0u;
    }
    return CGPT_OK;
}

int Tonemap(cgpt_ctx* ctx, const cgpt_tonemap_params* params, float* dst_rgba, size_t n_floats, uint32_t* dst_pixels, size_t n_pixels)
{
    const cgpt_tonemap_params p = params ? *params : kTonemapDefaults;
    if (const char* why = TonemapParamsError(p)) return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_tonemap: %s", why);
    Source s;
    int rc = ResolveSource(ctx, p, s);
    if (rc != CGPT_OK) return rc;
    if (!dst_rgba && !dst_pixels) return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_tonemap: both outputs are null");
    if (dst_rgba && n_floats != 4 * s.n) return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_tonemap: expected a buffer of %zu floats (4 per pixel)", 4 * s.n);
    if (dst_pixels && n_pixels != s.n) return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_tonemap: expected a buffer of %zu pixels", s.n);
    if (s.accumulator && ctx->group && (rc = GroupGatherUncounted(ctx, &s.pixels)) != CGPT_OK) return rc;
    if ((rc = Launch(ctx, p, s, dst_rgba, dst_pixels)) != CGPT_OK) ResetAll(s.dev->tm.table, s.dev->tm.record);   // the table may hold counts: the next call starts anew
    return rc;
}

}  // namespace
}  // namespace cgpt

using namespace cgpt;

extern "C" {

int cgpt_tonemap(cgpt_ctx* ctx, const cgpt_tonemap_params* params, float* dst_rgba, size_t n_floats, uint32_t* dst_pixels, size_t n_pixels)
{
    if (!ctx) return CGPT_ERR_INVALID;
    return Guarded(ctx, __func__, [&] { return Tonemap(ctx, params, dst_rgba, n_floats, dst_pixels, n_pixels); });
}

int cgpt_read_exposure(cgpt_ctx* ctx, cgpt_exposure_info* out)
{
    if (!ctx) return CGPT_ERR_INVALID;
    const cgpt_ctx* const d = ctx->group ? GroupFirstMember(ctx) : ctx;
    if (!out) return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_read_exposure: out is null");
    if (!d->exposure_info_valid) return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_read_exposure: no auto-exposure call has succeeded on this context");
    *out = d->exposure_info;
    return CGPT_OK;
}

int cgpt_exposure_reset(cgpt_ctx* ctx)
{
    if (!ctx) return CGPT_ERR_INVALID;
    (ctx->group ? GroupFirstMember(ctx) : ctx)->m_adapted_valid = false;
    return CGPT_OK;
}

}  // extern "C"
