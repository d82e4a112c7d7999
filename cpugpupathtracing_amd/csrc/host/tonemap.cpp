// tonemap.cpp -- the host mirror of the display stage (cgpth_tonemap; include/cpugpupt_host.h): tonemap.h's arithmetic over a host image,
// one pixel after the other.  Needs no GPU; allocates nothing.  The device kernels (csrc/device/tonemap.hip) call the same functions.
#include <cstring>
#include <string>

#include "cpugpupt_host.h"
#include "tonemap.h"

namespace cgpt {
void HostSetError(const char* msg);                                           // host_capi.cpp: the text cgpth_last_error returns
}

using namespace cgpt;

namespace {

int Fail(const std::string& msg) { HostSetError(msg.c_str()); return CGPT_ERR_INVALID; }

template <uint32_t CURVE, uint32_t TRANSFER>
void MapPixels(const float* src, size_t n, float exposure, float white, float* dst_rgba, uint32_t* dst_pixels)
{
    for (size_t i = 0; i < n; ++i) {
        const float r = ApplyTransfer<TRANSFER>(ApplyCurve<CURVE>(src[4 * i + 0], exposure, white));
        const float g = ApplyTransfer<TRANSFER>(ApplyCurve<CURVE>(src[4 * i + 1], exposure, white));
        const float b = ApplyTransfer<TRANSFER>(ApplyCurve<CURVE>(src[4 * i + 2], exposure, white));
        if (dst_rgba) { dst_rgba[4 * i + 0] = r; dst_rgba[4 * i + 1] = g; dst_rgba[4 * i + 2] = b; dst_rgba[4 * i + 3] = 1.0f; }
        if (dst_pixels) dst_pixels[i] = PackPixel(r, g, b);
    }
}

template <uint32_t CURVE>
void MapPixelsOf(uint32_t transfer, const float* src, size_t n, float exposure, float white, float* dst_rgba, uint32_t* dst_pixels)
{
    if (transfer == CGPT_TRANSFER_SRGB) MapPixels<CURVE, CGPT_TRANSFER_SRGB>(src, n, exposure, white, dst_rgba, dst_pixels);
    else MapPixels<CURVE, CGPT_TRANSFER_LINEAR>(src, n, exposure, white, dst_rgba, dst_pixels);
}

int Mirror(const cgpt_tonemap_params* params, cgpth_exposure_state* state, float* dst_rgba, size_t n_floats, uint32_t* dst_pixels, size_t n_pixels,
           cgpt_exposure_info* info_out);

}  // namespace

// nothing may unwind through the C ABI (a message's std::string can throw)
extern "C" int cgpth_tonemap(const cgpt_tonemap_params* params, cgpth_exposure_state* state, float* dst_rgba, size_t n_floats, uint32_t* dst_pixels,
                             size_t n_pixels, cgpt_exposure_info* info_out)
{
    try {
        return Mirror(params, state, dst_rgba, n_floats, dst_pixels, n_pixels, info_out);
    } catch (...) {
        HostSetError("cgpth_tonemap: out of host memory");
        return CGPT_ERR_INVALID;
    }
}

extern "C" int cgpth_luminance_bin(float luminance) { return LuminanceBin(luminance); }

namespace {

int Mirror(const cgpt_tonemap_params* params, cgpth_exposure_state* state, float* dst_rgba, size_t n_floats, uint32_t* dst_pixels, size_t n_pixels,
           cgpt_exposure_info* info_out)
{
    if (!params) return Fail("cgpth_tonemap: params is null (the mirror has no accumulator to default to)");
    const cgpt_tonemap_params& p = *params;
    if (const char* why = TonemapParamsError(p)) return Fail(std::string("cgpth_tonemap: ") + why);
    if (p.source != CGPT_TONEMAP_HOST) return Fail("cgpth_tonemap: the mirror maps host images only (source CGPT_TONEMAP_HOST)");
    const bool automatic = (p.flags & CGPT_TONEMAP_AUTO_EXPOSURE) != 0u;
    if (automatic && !state) return Fail("cgpth_tonemap: auto exposure needs a state");
    const size_t n = (size_t)p.src_width * p.src_height;
    if (!dst_rgba && !dst_pixels) return Fail("cgpth_tonemap: both outputs are null");
    if (dst_rgba && n_floats != 4 * n) return Fail("cgpth_tonemap: expected a buffer of " + std::to_string(4 * n) + " floats (4 per pixel)");
    if (dst_pixels && n_pixels != n) return Fail("cgpth_tonemap: expected a buffer of " + std::to_string(n) + " pixels");
    const float* const src = p.src_rgba;
    float exposure = ManualExposure(p.exposure_scale, p.ev_bias);
    if (automatic) {
        cgpt_exposure_info info{};
        for (size_t i = 0; i < n; ++i) {
            const int b = LuminanceBin(Luminance(src[4 * i + 0], src[4 * i + 1], src[4 * i + 2]));
            if (b >= 0) info.histogram[b] += 1u;
            else info.n_ignored += 1u;
        }
        const bool have = state->valid != 0u;
        double m = 0.0;
        info.adapted_index = have ? state->adapted_index : 0.0;               // no reading: reported as 0
        info.valid = have ? CGPT_EXPOSURE_ADAPTED : 0u;
        if (MeterHistogram(info.histogram, p.low_fraction, p.high_fraction, &m, &info.n_counted)) {
            info.adapted_index = AdaptIndex(state->adapted_index, have, m, p.alpha);
            info.valid = CGPT_EXPOSURE_ADAPTED | CGPT_EXPOSURE_METERED;
        }
        info.mean_index = m;
        if (info.valid & CGPT_EXPOSURE_ADAPTED) exposure = AutoExposure(info.adapted_index, p.key, p.exposure_scale, p.ev_bias);
        info.exposure = exposure;
        state->adapted_index = info.adapted_index;
        state->valid = (info.valid & CGPT_EXPOSURE_ADAPTED) ? 1u : 0u;
        if (info_out) *info_out = info;
    }
    switch (p.curve) {
    case CGPT_CURVE_REINHARD: MapPixelsOf<CGPT_CURVE_REINHARD>(p.transfer, src, n, exposure, p.white, dst_rgba, dst_pixels); break;
    case CGPT_CURVE_ACES: MapPixelsOf<CGPT_CURVE_ACES>(p.transfer, src, n, exposure, p.white, dst_rgba, dst_pixels); break;
    case CGPT_CURVE_HABLE: MapPixelsOf<CGPT_CURVE_HABLE>(p.transfer, src, n, exposure, p.white, dst_rgba, dst_pixels); break;
    default: MapPixelsOf<CGPT_CURVE_CLAMP>(p.transfer, src, n, exposure, p.white, dst_rgba, dst_pixels); break;
    }
    return CGPT_OK;
}

}  // namespace
