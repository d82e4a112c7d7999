// tonemap.h -- the display stage's arithmetic, stated once for the host mirror (tonemap.cpp: cgpth_tonemap) and the device kernels
// (csrc/device/tonemap.hip), which share every function below as tree_cost.h's users share its terms.  tests/tonemap_ref.py states the
// same in numpy; DESIGN.md 5.37.  Host-only: no HIP include; under hipcc the functions are __host__ __device__.
//
// Everything but the sRGB curve's powf uses + - * /, floor, ldexp, integer operations and comparisons, compiled with -ffp-contract=off:
// the device, the mirror and numpy agree bit for bit.
//   luminance   Y = (0.2126f r + 0.7152f g) + 0.0722f b                       (the denoiser's, denoise.hip)
//   histogram   256 bins over [2^-16, 2^16), eight an octave, from the float's bits: bin = clamp((bits(Y) >> 20) - ((127 - 16) << 3), 0, 255)
//               for a finite Y > 0; any other Y (<= 0, NaN, +inf) is not counted but tallied in n_ignored
//   metering    N = the counted pixels; the lowest floor(low_fraction N) and the highest floor(high_fraction N) of them are dropped (double
//               products; boundary bins are trimmed partially); of the rest m = (sum of c_i (2 i + 1)) 0.5 / (sum of c_i): the mean
//               log-luminance in eighths of an octave above 2^-16.  N = 0: the frame has no reading
//   adaptation  first reading: m_adapted = m; later: m_adapted + (m - m_adapted) (double)alpha; no reading: m_adapted stays
//   exposure    q = m_adapted / 8 - 16, L = ldexp(1 + (q - floor q), (int)floor q) (the inverse of the binning: a bin's centre),
//               exposure = ((float)((double)key / L) * bias) * exposure_scale, bias = (float)ldexp(1.0, ev_bias).  No reading ever, or
//               manual mode: the metered factor is 1
//   curve       per channel on x = c exposure, x > 0 ? x : 0 (a NaN becomes 0), in the operation order written below; the rational
//               curves take min(x, 2^32); a NaN result (0 / 0 where white^2 underflows) becomes 0
//   transfer    LINEAR nothing; SRGB on y < 1 ? y : 1: y <= 0.0031308f ? 12.92f y : 1.055f powf(y, 1 / 2.4f) - 0.055f
//   output      {r, g, b, 1} and the pixel as Vec4ToUint packs it (ref: Include/MathLib.h:144-152; rt_device.hpp: vec4_to_uint)
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "cpugpupt_abi.h"

#ifdef __HIP__
#define CGPT_TONEMAP_FN __host__ __device__ inline
#else
#define CGPT_TONEMAP_FN inline
#endif

namespace cgpt {

constexpr uint32_t kTonemapBins = 256;
// NULL params (cgpt_tonemap): common defaults, not tuned on this renderer's scenes
constexpr cgpt_tonemap_params kTonemapDefaults = { CGPT_TONEMAP_ACCUMULATOR, CGPT_CURVE_ACES, CGPT_TRANSFER_SRGB, CGPT_TONEMAP_AUTO_EXPOSURE,
                                                   1.0f, 0, 4.0f, 0.18f, 0.5f, 0.02f, 1.0f, nullptr, 0u, 0u };

CGPT_TONEMAP_FN float Luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// the bin of a luminance, or -1 for one that is not counted
CGPT_TONEMAP_FN int LuminanceBin(float y)
{
    if (!(y > 0.0f) || !(y <= FLT_MAX)) return -1;
    const int b = (int)(__builtin_bit_cast(uint32_t, y) >> 20) - ((127 - 16) << 3);
    return b < 0 ? 0 : (b > 255 ? 255 : b);
}

// the accumulator's pixel as pack_pixels_kernel divides it (path_kernels.hip): n = (float)num_accumulated
CGPT_TONEMAP_FN float AccumulatorChannel(float sum, float n) { return sum / n; }

// Metering: counts[256] -> m.  False: nothing was counted (no reading).  n_counted is N before the trimming
CGPT_TONEMAP_FN bool MeterHistogram(const uint32_t* counts, float low_fraction, float high_fraction, double* m, uint64_t* n_counted)
{
    uint64_t n = 0;
    for (uint32_t i = 0; i < kTonemapBins; ++i) n += counts[i];
    *n_counted = n;
    if (n == 0) return false;
    uint64_t drop_lo = (uint64_t)floor((double)low_fraction * (double)n), drop_hi = (uint64_t)floor((double)high_fraction * (double)n);
    // the highest bin the low trim reaches, and what it leaves there; the bins below it are empty afterwards
    uint32_t lo = 0;
    uint64_t lo_left = 0;
    for (; lo < kTonemapBins; ++lo) {
        const uint64_t c = counts[lo];
        if (c > drop_lo) { lo_left = c - drop_lo; break; }
        drop_lo -= c;
    }
    uint64_t den = 0, num2 = 0;                                               // sum of c_i and of c_i (2 i + 1) over what remains: exact
    for (uint32_t k = kTonemapBins; k-- > lo;) {
        uint64_t c = k == lo ? lo_left : (uint64_t)counts[k];
        const uint64_t t = c < drop_hi ? c : drop_hi;
        c -= t; drop_hi -= t;
        den += c; num2 += c * (uint64_t)(2u * k + 1u);
    }
    if (den == 0) return false;                                               // (cannot happen while low + high < 1)
    *m = ((double)num2 * 0.5) / (double)den;
    return true;
}

CGPT_TONEMAP_FN double AdaptIndex(double m_adapted, bool have_adapted, double m, float alpha)
{
    return have_adapted ? m_adapted + (m - m_adapted) * (double)alpha : m;
}

// the luminance at the histogram index m: the inverse of LuminanceBin (index i + 0.5 is bin i's centre)
CGPT_TONEMAP_FN double IndexLuminance(double m)
{
    const double q = m / 8.0 - 16.0, f = floor(q);
    return ldexp(1.0 + (q - f), (int)f);
}

CGPT_TONEMAP_FN float ExposureBias(int32_t ev_bias) { return (float)ldexp(1.0, (int)ev_bias); }
CGPT_TONEMAP_FN float ExposureFromFactor(float metered, float exposure_scale, int32_t ev_bias) { return (metered * ExposureBias(ev_bias)) * exposure_scale; }
CGPT_TONEMAP_FN float AutoExposure(double m_adapted, float key, float exposure_scale, int32_t ev_bias)
{
    return ExposureFromFactor((float)((double)key / IndexLuminance(m_adapted)), exposure_scale, ev_bias);
}
CGPT_TONEMAP_FN float ManualExposure(float exposure_scale, int32_t ev_bias) { return ExposureFromFactor(1.0f, exposure_scale, ev_bias); }

// ---- the curves -------------------------------------------------------------------------------------------------------------------------
CGPT_TONEMAP_FN float CurveReinhard(float x, float white) { return (x * (1.0f + x / (white * white))) / (1.0f + x); }
// Narkowicz 2015, "ACES Filmic Tone Mapping Curve"
CGPT_TONEMAP_FN float CurveAces(float x) { return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f); }
// Hable 2010, "Filmic Tonemapping Operators" (Uncharted 2): A shoulder, B linear strength, C linear angle, D toe strength, E toe numerator, F toe denominator
CGPT_TONEMAP_FN float HablePartial(float x)
{
    const float A = 0.15f, B = 0.50f, C = 0.10f, D = 0.20f, E = 0.02f, F = 0.30f;
    return ((x * (A * x + C * B) + D * E) / (x * (A * x + B) + D * F)) - E / F;
}
CGPT_TONEMAP_FN float CurveHable(float x, float white) { return HablePartial(x) / HablePartial(white); }

// The three rational curves take min(x, 2^32): x^2 stays finite in float, so a pixel that overflowed (+inf) or is absurdly bright maps
// to the curve's saturated end, not through inf / inf to black.  Every curve has saturated to float precision long before.
constexpr float kCurveMaxInput = 4294967296.0f;

template <uint32_t CURVE>
CGPT_TONEMAP_FN float ApplyCurve(float c, float exposure, float white)
{
    float x = c * exposure;
    x = x > 0.0f ? x : 0.0f;
    float y = x;                                                              // CGPT_CURVE_CLAMP: the reference's (the pack clamps)
    if (CURVE != CGPT_CURVE_CLAMP) x = x < kCurveMaxInput ? x : kCurveMaxInput;
    if (CURVE == CGPT_CURVE_REINHARD) y = CurveReinhard(x, white);
    if (CURVE == CGPT_CURVE_ACES) y = CurveAces(x);
    if (CURVE == CGPT_CURVE_HABLE) y = CurveHable(x, white);
    return y == y ? y : 0.0f;
}

template <uint32_t TRANSFER>
CGPT_TONEMAP_FN float ApplyTransfer(float y)
{
    if (TRANSFER == CGPT_TRANSFER_LINEAR) return y;
    y = y < 1.0f ? y : 1.0f;
    return y <= 0.0031308f ? 12.92f * y : 1.055f * powf(y, 1.0f / 2.4f) - 0.055f;
}

// Vec4ToUint (ref: Include/MathLib.h:144-152), as rt_device.hpp: vec4_to_uint restates it for the device
CGPT_TONEMAP_FN uint32_t PackPixel(float x, float y, float z)
{
    const float one = 1.0f;
    const float fr = 255.0f * (x < one ? x : one), fg = 255.0f * (y < one ? y : one), fb = 255.0f * (z < one ? z : one);
    const uint32_t r = (uint32_t)(int32_t)(fr < 0.0f ? 0.0f : fr) & 0xFFu;
    const uint32_t g = (uint32_t)(int32_t)(fg < 0.0f ? 0.0f : fg) & 0xFFu;
    const uint32_t b = (uint32_t)(int32_t)(fb < 0.0f ? 0.0f : fb) & 0xFFu;
    return (255u << 24) + (b << 16) + (g << 8) + r;
}

// ---- what a call refuses before it looks at its source or its outputs: nullptr, or the reason --------------------------------------------
inline bool FinitePositive(float v) { return std::isfinite(v) && v > 0.0f; }
inline const char* TonemapParamsError(const cgpt_tonemap_params& p)
{
    if (p.source > CGPT_TONEMAP_HOST) return "unknown source";
    if (p.curve > CGPT_CURVE_HABLE) return "unknown curve";
    if (p.transfer > CGPT_TRANSFER_SRGB) return "unknown transfer";
    if (p.flags & ~(uint32_t)CGPT_TONEMAP_AUTO_EXPOSURE) return "unknown flags";
    if (!FinitePositive(p.exposure_scale)) return "exposure_scale must be finite and > 0";
    if (!FinitePositive(p.white)) return "white must be finite and > 0";
    if (p.ev_bias < -64 || p.ev_bias > 64) return "ev_bias outside [-64, 64]";
    if (p.flags & CGPT_TONEMAP_AUTO_EXPOSURE) {
        if (!FinitePositive(p.key)) return "key must be finite and > 0";
        if (!(p.low_fraction >= 0.0f && p.low_fraction < 1.0f) || !(p.high_fraction >= 0.0f && p.high_fraction < 1.0f)) return "a fraction outside [0, 1)";
        if (!((double)p.low_fraction + (double)p.high_fraction < 1.0)) return "low_fraction + high_fraction must be < 1";
        if (!(p.alpha >= 0.0f && p.alpha <= 1.0f)) return "alpha outside [0, 1]";
    }
    if (p.source == CGPT_TONEMAP_HOST && (!p.src_rgba || p.src_width == 0u || p.src_height == 0u)) return "a host source needs an image: src_rgba, src_width and src_height";
    return nullptr;
}

}  // namespace cgpt
