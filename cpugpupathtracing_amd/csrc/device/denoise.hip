// denoise.hip -- an edge-avoiding a-trous filter guided by first-hit buffers (gfx950): cgpt_read_guides, cgpt_denoise,
// the temporal reprojection in front of it: cgpt_denoise_temporal, cgpt_temporal_reset, cgpt_read_temporal_history,
// and its variance-guided form: cgpt_denoise_variance_guided, cgpt_read_variance.
//
// Guides: the reference does not jitter primary rays (SURVEY A-14), so every sample of a pixel has the same first hit, and one primary
// trace per camera gives each pixel's position, normal and albedo.  guides_kernel computes that hit with the render paths' own device
// functions -- camera_ray with primary_ray's u, v (trace_steps.hpp), intersect_scene with the LDS stack set up as intersect_rays_kernel
// does, get_hit, load_material -- so the guides are the render's primary hit bit for bit.  The context keeps them until the camera, the
// band or the scene changes (every upload and in-place edit bumps cgpt_ctx::scene_generation).
//
// Filter (tests/denoise_ref.py states it in numpy): pass i = 0 .. I-1 has step s = 2^i and taps q = p + s (dx, dy),
// dx, dy in -2..2, skipped outside the band; weight h(dx) h(dy) exp(-|c(q) - c(p)|^2 / (sigma_c 2^-i)^2) times, when p and q both hit,
// exp(-|n(q) - n(p)|^2 / sigma_n^2) exp(-(n(p).(x(q) - x(p)))^2 / sigma_x^2); a hit and a miss never mix.  denoise_prepare divides the
// accumulator by num_accumulated (data.pixels' division) and by the albedo (demodulation); the last pass multiplies the albedo back and
// packs the pixels as data.pixels are packed.  One launch per pass, 16x16-pixel blocks, ping-pong float4 buffers of the context.
//
// Temporal stage (cgpt_denoise_temporal; tests/temporal_ref.py states it in numpy): between denoise_prepare and the
// passes, temporal_merge reprojects the history of the earlier frames -- merged colour and history length H per pixel, with that frame's
// guides and camera -- onto the current camera through the current first hits, validates the four bilinear taps against the current hit
// (same object, normal, tangent plane) and merges c = (He c_h + N c_0) / (He + N).  The passes then run on c.
// With CGPT_TEMPORAL_FOLLOW_TRANSFORMS (tests/motion_ref.py) a history outlives cgpt_scene_update_transforms calls: the
// hits on the objects whose matrices changed are first carried back through M_prev M_cur^-1 (temporal_merge<.., MOTION = true>).
// With CGPT_TEMPORAL_FOLLOW_POSES (tests/pose_motion_ref.py) it outlives cgpt_scene_skin_mesh calls: pose_carry_back
// computes, per pixel, where the hit's surface point was under the pose the history was stored with (cgpt_read_previous_hits), from
// the first hit's triangle (guides_tri_kernel) and the history's joint matrices, and temporal_merge<.., POSE = true> reprojects from there.
// With CGPT_TEMPORAL_FOLLOW_MORPHS (tests/morph_motion_ref.py) it outlives cgpt_scene_morph_mesh calls, and poses of an
// object that has both targets and a skin: morph_carry_back computes the same records from the history's weights (and matrices).
//
// Variance-guided edge stopping (cgpt_denoise_variance_guided, cgpt_read_variance; tests/variance_ref.py states it in
// numpy): the colour edge-stop of the passes becomes exp(-|l(c_q) - l(c_p)| / (sigma_l sqrt(gbar(p)) + 1e-6)), l the luminance and gbar
// a 3x3 Gaussian of the pixel's variance.  variance_estimate puts that variance into the .w lane of pass 0's input: the weighted variance
// of l over a 7x7 window, or -- with the temporal stage in front, where temporal_merge<false, true> keeps {mean, variance, samples} of l
// beside the colour history -- the temporal estimate once a pixel's history is long enough.  variance_pass filters it along with the colour.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "cpugpupt_abi.h"
#include "ctx_internal.h"
#include "device_scene.h"
#include "morph.h"
#include "rt_device.hpp"
#include "shade_device.hpp"
#include "skinning.h"
#include "tonemap.h"

namespace cgpt {

using namespace dev;

extern __shared__ uint32_t denoise_lds[];

namespace {

constexpr uint32_t kTile = 16;                   // 16x16 pixels = one 256-thread block
constexpr uint32_t kMaxIterations = 10;
constexpr cgpt_denoise_params kDefaults = { 5u, CGPT_DENOISE_DEMODULATE_ALBEDO, 4.0f, 0.2f, 0.3f };

// pixel of a thread: 16x16 tiles in row-major tile order (a 1-D grid: no limit on the frame's height)
__device__ __forceinline__ void tile_pixel(uint32_t width, uint32_t& px, uint32_t& row)
{
    const uint32_t tiles_x = (width + kTile - 1u) / kTile;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    px = tx * kTile + (threadIdx.x & (kTile - 1u));
    row = ty * kTile + threadIdx.x / kTile;
}

// One thread per pixel of the band (global rows first_row ..): {x.xyz, t | n.xyz, bits(obj) | albedo.xyz, bits(mat_index)} and the
// demodulation albedo (the albedo per channel where it is >= 1e-3 on a hit that is not a light, else 1).
// SMOOTH: the scene has an object with smooth normals (cgpt_scene_update_smooth_normals): n is get_hit's interpolated normal there.
// XFORM: it has an object with a transform (cgpt_scene_update_transforms): the trace and the normal honour it (this instantiation carries
// SMOOTH too, as lobe level 4 does).  TREE: the trace goes through the top-level tree (cgpt_set_top_level(1)); the same hit, so the cached
// guides of one mode serve the other.
// The body is stated once, as text: shared through a device function, guides_kernel's instantiations did not keep their instruction
// streams.  TRI_STATEMENT runs on a hit, WRITE_TRI after the stores.
#define CGPT_GUIDES_BODY(SMOOTH_, XFORM_, TREE_, TRI_STATEMENT, WRITE_TRI)                                                                     \
    uint32_t px, row;                                                                                                                          \
    tile_pixel(width, px, row);                                                                                                                \
    if (px >= width || row >= n_rows) return;                                                                                                  \
    uint32_t* const stack = denoise_lds + threadIdx.x;                                                                                         \
    const uint32_t py = first_row + row;                                                                                                       \
    Ray ray = camera_ray(cam, (float)px * (1.0f / (float)width), (float)py * (1.0f / (float)height));   /* primary_ray's u, v */                \
    Counters cnt = { 0, 0, 0, 0, 0 };                                          /* not booked: cgpt_stats does not grow */                      \
    intersect_scene<false, XFORM_, TREE_>(sc, ray, stack, blockDim.x, cnt);                                                                    \
    float4 g0 = make_float4(0.0f, 0.0f, 0.0f, 1e34f);                                                                                          \
    float4 g1 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(kNoHit));                                                                        \
    float4 g2 = g1;                                                                                                                            \
    float4 m = make_float4(1.0f, 1.0f, 1.0f, 0.0f);                                                                                            \
    if (ray.obj != kNoHit) {                                                                                                                   \
        const Hit h = get_hit<false, SMOOTH_, XFORM_>(sc, ray, cnt);                                                                           \
        const Mat mat = load_material(sc, h.mat);                                                                                              \
        TRI_STATEMENT;                                                                                                                         \
        g0 = make_float4(h.pos.x, h.pos.y, h.pos.z, ray.t);                                                                                    \
        g1 = make_float4(h.normal.x, h.normal.y, h.normal.z, __uint_as_float(ray.obj));                                                        \
        g2 = make_float4(mat.albedo.x, mat.albedo.y, mat.albedo.z, __uint_as_float(h.mat));                                                    \
        if (!mat.is_light) {                                                                                                                   \
            m.x = mat.albedo.x >= 1e-3f ? mat.albedo.x : 1.0f;                                                                                 \
            m.y = mat.albedo.y >= 1e-3f ? mat.albedo.y : 1.0f;                                                                                 \
            m.z = mat.albedo.z >= 1e-3f ? mat.albedo.z : 1.0f;                                                                                 \
        }                                                                                                                                      \
    }                                                                                                                                          \
    const size_t i = (size_t)row * width + px;                                                                                                 \
    guides[3 * i] = g0; guides[3 * i + 1] = g1; guides[3 * i + 2] = g2;                                                                        \
    demod[i] = m;                                                                                                                              \
    WRITE_TRI

template <bool SMOOTH, bool XFORM = false, bool TREE = false>
__global__ void __launch_bounds__(256) guides_kernel(const DevScene sc, const DevCamera cam, uint32_t width, uint32_t height, uint32_t first_row,
                                                     uint32_t n_rows, float4* __restrict__ guides, float4* __restrict__ demod)
{
    CGPT_GUIDES_BODY(SMOOTH, XFORM, TREE, (void)0, (void)0);
}

// The guides of a context that holds a skin (cgpt_scene_set_skin) or morph targets (cgpt_scene_set_morph_targets), whichever features its scene has: guides_kernel<true, true, TREE> -- it
// reads the smooth and transform flags per object, so a scene without either gets the bits of its own instantiation; TREE follows
// cgpt_set_top_level as it does there -- which also writes the first hit's triangle, in its object's original order, beside the
// guides: what CGPT_TEMPORAL_FOLLOW_POSES and CGPT_TEMPORAL_FOLLOW_MORPHS carry a hit back through.  0 for anything but a mesh: a stand-alone triangle object's
// Ray::tri is whatever an earlier mesh left there, and get_hit reads 0 for it.  A kernel of its own name: guides_kernel's
// instantiations keep their signature.
template <bool TREE>
__global__ void __launch_bounds__(256) guides_tri_kernel(const DevScene sc, const DevCamera cam, uint32_t width, uint32_t height, uint32_t first_row,
                                                         uint32_t n_rows, float4* __restrict__ guides, float4* __restrict__ demod, uint32_t* __restrict__ tri_out)
{
    uint32_t tri = 0u;
    CGPT_GUIDES_BODY(true, true, TREE, tri = sc.objects[ray.obj].kind == 0u ? ray.tri : 0u, tri_out[i] = tri);
}
#undef CGPT_GUIDES_BODY

struct PassArgs {
    const float4* src;        // the previous pass's output (pass 0: denoise_prepare's)
    float4* dst;
    uint32_t* pixels;         // last pass
    const float4* guides;
    const float4* demod;
    uint32_t width, n_rows, step, demodulate;
    float color_scale;        // atrous_pass: 1 / (sigma_c 2^-i)^2 of this pass; variance_pass: sigma_luminance
    float inv_normal, inv_position;   // 1 / sigma^2
};
struct VarPassArgs : PassArgs {};   // src is {c, var}: the same layout under the name variance_pass has in the code object

// c_0 = acc / num_accumulated (data.pixels' division, ref: Main.cpp:741), divided by the albedo with demodulation.  Once per pixel here
// rather than in each of pass 0's 25 taps: 150 IEEE divisions per pixel took that pass to 256 VGPRs, one wave per SIMD.
__global__ void __launch_bounds__(256) denoise_prepare(const float4* __restrict__ acc, const float4* __restrict__ demod, float4* __restrict__ dst,
                                                       size_t n_pixels, float n, uint32_t demodulate)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    const float4 a = acc[i];
    float4 c = make_float4(a.x / n, a.y / n, a.z / n, 0.0f);
    if (demodulate) {
        const float4 m = demod[i];
        c.x = c.x / m.x; c.y = c.y / m.y; c.z = c.z / m.z;
    }
    dst[i] = c;
}

// h(d) of the B3 spline 1/16 (1, 4, 6, 4, 1): 3/8, 1/4, 1/16
__device__ __forceinline__ constexpr float tap(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1 ? 0.25f : 0.0625f); }

// l(c), the luminance the variance-guided filter measures
__device__ __forceinline__ float luminance(float r, float g, float b) { return Luminance(r, g, b); }   // tonemap.h states it

// a tap's coordinate clamped into [0, n): a tap outside the band is loaded from the nearest pixel inside it and masked by a select.
// (A row's clamp is written on its row_in instead: through this helper the kernels' instruction streams moved.)
template <typename T> __device__ __forceinline__ size_t clamp_tap(T q, T n) { return (size_t)(q < 0 ? 0 : (q < n ? q : n - 1)); }

// the geometry term of a tap's exponent, for two hits: |n_q - n_p|^2 / sigma_n^2 + (n_p . (x_q - x_p))^2 / sigma_x^2
__device__ __forceinline__ float geometry_exponent(const float4& xq, const float4& nq, const V3& x_p, const V3& n_p, float inv_normal, float inv_position)
{
    const V3 dn = mk(nq.x, nq.y, nq.z) - n_p;
    const float dplane = dot(n_p, mk(xq.x, xq.y, xq.z) - x_p);               // distance to p's tangent plane
    return dot(dn, dn) * inv_normal + dplane * dplane * inv_position;
}

// what a call's last kernel writes: the albedo multiplied back (demodulation), w = 1, and the pixel packed as data.pixels is
__device__ __forceinline__ void write_output(float r, float g, float b, uint32_t demodulate, const float4* demod, float4* dst, uint32_t* pixels, size_t i)
{
    if (demodulate) {
        const float4 m = demod[i];
        r *= m.x; g *= m.y; b *= m.z;
    }
    dst[i] = make_float4(r, g, b, 1.0f);
    pixels[i] = vec4_to_uint(r, g, b);
}

template <bool LAST>
__global__ void __launch_bounds__(256) atrous_pass(const PassArgs a)
{
    uint32_t px, row;
    tile_pixel(a.width, px, row);
    if (px >= a.width || row >= a.n_rows) return;
    const size_t i = (size_t)row * a.width + px;
    const float4 xp4 = a.guides[3 * i], np4 = a.guides[3 * i + 1];
    const V3 x_p = mk(xp4.x, xp4.y, xp4.z), n_p = mk(np4.x, np4.y, np4.z);
    const bool hit_p = __float_as_uint(np4.w) != kNoHit;
    const float4 cp4 = a.src[i];
    const V3 c_p = mk(cp4.x, cp4.y, cp4.z);
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, wsum = 0.0f;
    // A row of five taps at a time: first all their loads, each from the tap's position clamped into the band, then the weights, where a
    // tap outside the band (skipped, not clamped) or across a hit / miss edge gets none.  Selects, not branches: a branch would pull the
    // loads after it, and every tap would wait for its own.
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const long long qy = (long long)row + (long long)dy * a.step;
        const bool row_in = qy >= 0 && qy < (long long)a.n_rows;
        const size_t qy_c = (size_t)(qy < 0 ? 0 : (row_in ? qy : (long long)a.n_rows - 1));   // clamp_tap on row_in's comparison
        float4 xq[5], nq[5];
        V3 cq[5];
        bool in[5];
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const long long qx = (long long)px + (long long)(t - 2) * a.step;
            in[t] = row_in && qx >= 0 && qx < (long long)a.width;
            const size_t j = qy_c * a.width + clamp_tap(qx, (long long)a.width);
            xq[t] = a.guides[3 * j]; nq[t] = a.guides[3 * j + 1];
            const float4 c4 = a.src[j];
            cq[t] = mk(c4.x, c4.y, c4.z);
        }
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const bool hit_q = __float_as_uint(nq[t].w) != kNoHit;
            const V3 dc = cq[t] - c_p;
            const float e_geo = geometry_exponent(xq[t], nq[t], x_p, n_p, a.inv_normal, a.inv_position);
            const float e = dot(dc, dc) * a.color_scale + (hit_p && hit_q ? e_geo : 0.0f);
            const float w = (tap(t - 2) * tap(dy)) * __expf(-e);                // the centre tap: e = 0, w = h
            const bool use = in[t] && hit_q == hit_p;                         // a hit and a miss never mix
            sr = use ? sr + cq[t].x * w : sr;
            sg = use ? sg + cq[t].y * w : sg;
            sb = use ? sb + cq[t].z * w : sb;
            wsum = use ? wsum + w : wsum;
        }
        __builtin_amdgcn_sched_barrier(0);                                    // one row's loads in flight at a time: the registers of five taps
    }
    const V3 r = mk(sr / wsum, sg / wsum, sb / wsum);
    if (LAST) write_output(r.x, r.y, r.z, a.demodulate, a.demod, a.dst, a.pixels, i);
    else a.dst[i] = make_float4(r.x, r.y, r.z, 0.0f);
}

// iterations = 0: the accumulator / num_accumulated, packed as data.pixels is (the same division and packing: the same bits)
__global__ void __launch_bounds__(256) denoise_identity(const float4* __restrict__ acc, float4* __restrict__ dst, uint32_t* __restrict__ pixels,
                                                        size_t n_pixels, float n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    const float4 a = acc[i];
    const float r = a.x / n, g = a.y / n, b = a.z / n;
    dst[i] = make_float4(r, g, b, 1.0f);
    pixels[i] = vec4_to_uint(r, g, b);
}

// ---- the temporal stage --------------------------------------------------------------------------------------------------------
constexpr cgpt_temporal_params kTemporalDefaults = { 64.0f, 0.9f, 0.01f, 0u };
enum TemporalMode : uint32_t { kNoHistory = 0, kSameCamera = 1, kReproject = 2 };   // of a whole call: wave-uniform in the kernel

struct TemporalArgs {
    const float4* guides;          // this frame's, 3 float4 per pixel
    const float4* demod;
    const float4* materials;       // DevScene::materials, 4 float4 per material: the view-dependent rule reads specular and refractivity
    const float4* hist;            // the history {c, H} and its guides (2 float4 per pixel); read only when mode != kNoHistory
    const float4* hist_guides;
    float4* hist_out;              // the new history
    float4* hist_guides_out;
    float4* color;                 // in: c_0 (denoise_prepare's output); out: the merged c (FINAL: c m, w = 1)
    uint32_t* pixels;              // FINAL
    uint32_t width, n_rows, mode, drop_view_dependent, demodulate;
    float n_samples, max_history, normal_cos_min, plane_tolerance;
    float minv[9];                 // rows of the inverse of [top_left - pos | top_right - top_left | bottom_left - top_left] of the history's camera
    float pos_prev[3];
    float height, first_row;       // fy = (c / a) height - first_row
    // MOMENTS only (cgpt_denoise_variance_guided)
    const float4* moments;         // {mu, v, K, 0} beside hist; read only when have_moments != 0
    float4* moments_out;
    float* variance;               // out: var_t or -1
    uint32_t have_moments;         // the moments belong to hist (no cgpt_denoise_temporal call updated the colour since)
    float min_history_n;           // min_history_frames N
    // MOTION only (CGPT_TEMPORAL_FOLLOW_TRANSFORMS)
    const float4* motion;          // 6 float4 per object: transform_math.h's MotionRecord
    // POSE only (CGPT_TEMPORAL_FOLLOW_POSES)
    const float4* pose;            // 2 float4 per pixel: pose_carry_back's records
};

// One thread per pixel.  The geometry of the reprojection -- (a, b, c) = Minv (x - pos_prev), fx, fy, the bilinear weights and the two
// validity tests -- is double arithmetic on the float guides: in float the sample position moved by up to 1e-4 pixel, which times the
// difference between neighbouring history pixels at 1 spp is more than the 1e-4 the output is held to, and the accept / reject decisions
// near a threshold differed from the float64 statement's on more pixels.  It is some 150 instructions next to 15 loads of 16 bytes.
// All four taps' loads (colour and two guide float4s each, from positions clamped into the band) and the material's come before any
// validity arithmetic, which masks with selects (the lesson of atrous_pass).
// FINAL (iterations = 0): the output is c m packed as data.pixels is, with w = 1.
// MOMENTS (cgpt_denoise_variance_guided with CGPT_VARIANCE_TEMPORAL; tests/variance_ref.py): the luminance moments
// {mu, v, K} kept beside the colour history go through the same four taps, validity tests and weights, and merge with the N samples of
// l0 = l(c_0) by the pooled-variance update; the pixel's entry of the variance map becomes var_t = v' N / (Ke + N), or -1 where
// Ke + N < min_history_frames N (variance_estimate then puts var_s there).  The colour's arithmetic is the same instructions either way.
// MOTION (CGPT_TEMPORAL_FOLLOW_TRANSFORMS, a call in which an object moved; always mode kReproject; tests/motion_ref.py):
// the pixel's record -- gathered by its object index, a miss reads record 0 and is masked -- carries the hit back to where the object
// was when the history was stored, x' = D x and n' = normalize(N n) in double, each rounded to float once, and the arithmetic below runs
// on x', n', the unchanged t and object index.  A pixel of an unmoved object takes x and n untouched by a select (an identity product
// would change bits), one of a dropped object takes no history.  The record's six loads are issued as soon as the object index is
// known and before anything waits for them; the taps' addresses depend on them.  The new history stores the frame's own guides.
// POSE (CGPT_TEMPORAL_FOLLOW_POSES, a call in which a skinned object was re-posed; always mode kReproject; DESIGN.md 5.27;
// tests/pose_motion_ref.py): the pixel's record of pose_carry_back (below) names where its hit was under the history's pose.  State 1
// takes x and n from the record, state 0 the guides' untouched by a select, state 2 no history.  MOTION then runs on that x and n:
// an object that was re-posed and moved is carried back through its pose and then through D, two roundings to float.
template <bool FINAL, bool MOMENTS = false, bool MOTION = false, bool POSE = false>
__global__ void __launch_bounds__(256) temporal_merge(const TemporalArgs a)
{
    uint32_t px, row;
    tile_pixel(a.width, px, row);
    if (px >= a.width || row >= a.n_rows) return;
    const size_t i = (size_t)row * a.width + px;
    const float4 g0 = a.guides[3 * i], g1 = a.guides[3 * i + 1], g2 = a.guides[3 * i + 2];
    const float4 c0 = a.color[i];
    float hr = 0.0f, hg = 0.0f, hb = 0.0f, H = 0.0f;                            // c_h and H; H = 0: no history
    float mu_h = 0.0f, v_h = 0.0f, K_h = 0.0f;                                 // MOMENTS; K_h = 0: no moments
    if (a.mode == kSameCamera) {                                               // same scene and camera: the same hit, no validation
        const float4 h = a.hist[i];
        hr = h.x; hg = h.y; hb = h.z; H = h.w;
        if constexpr (MOMENTS) {
            if (a.have_moments != 0u) {
                const float4 m = a.moments[i];
                mu_h = m.x; v_h = m.y; K_h = H > 0.0f ? m.z : 0.0f;
            }
        }
    } else if (a.mode == kReproject) {
        const uint32_t obj = __float_as_uint(g1.w), mat = __float_as_uint(g2.w);
        const bool hit = obj != kNoHit;
        float4 x4 = g0, n4 = g1;                                               // the hit the reprojection runs on: POSE and MOTION carry it back
        bool dropped = false;
        if constexpr (POSE) {
            const float4 p0 = a.pose[2 * i], p1 = a.pose[2 * i + 1];
            const uint32_t state = __float_as_uint(p0.w);                      // pose_carry_back: 0 for a miss and for every object without a new pose
            const bool posed = state == 1u;
            dropped = state == 2u;
            x4.x = posed ? p0.x : g0.x; x4.y = posed ? p0.y : g0.y; x4.z = posed ? p0.z : g0.z;
            n4.x = posed ? p1.x : g1.x; n4.y = posed ? p1.y : g1.y; n4.z = posed ? p1.z : g1.z;
        }
        if constexpr (MOTION) {
            const float4 xs = x4, ns = n4;                                     // the guides' own without POSE
            const float4* const rec = a.motion + 6u * (hit ? (size_t)obj : 0u);
            const float4 d0 = rec[0], d1 = rec[1], d2 = rec[2], n0 = rec[3], n1 = rec[4], n2 = rec[5];
            const uint32_t state = hit ? __float_as_uint(n0.w) : 0u;           // transform_math.h: 0 unmoved, 1 moved, 2 drop
            const double x = (double)xs.x, y = (double)xs.y, z = (double)xs.z;
            const double cx = (((double)d0.x * x + (double)d0.y * y) + (double)d0.z * z) + (double)d0.w;
            const double cy = (((double)d1.x * x + (double)d1.y * y) + (double)d1.z * z) + (double)d1.w;
            const double cz = (((double)d2.x * x + (double)d2.y * y) + (double)d2.z * z) + (double)d2.w;
            const double nx = (double)ns.x, ny = (double)ns.y, nz = (double)ns.z;
            const double vx = ((double)n0.x * nx + (double)n0.y * ny) + (double)n0.z * nz;
            const double vy = ((double)n1.x * nx + (double)n1.y * ny) + (double)n1.z * nz;
            const double vz = ((double)n2.x * nx + (double)n2.y * ny) + (double)n2.z * nz;
            const double len = sqrt((vx * vx + vy * vy) + vz * vz);
            const bool moved = state == 1u;
            dropped = dropped || state == 2u;
            x4.x = moved ? (float)cx : xs.x; x4.y = moved ? (float)cy : xs.y; x4.z = moved ? (float)cz : xs.z;
            n4.x = moved ? (float)(vx / len) : ns.x; n4.y = moved ? (float)(vy / len) : ns.y; n4.z = moved ? (float)(vz / len) : ns.z;
        }
        const double dx = (double)x4.x - (double)a.pos_prev[0], dy = (double)x4.y - (double)a.pos_prev[1], dz = (double)x4.z - (double)a.pos_prev[2];
        const double pa = ((double)a.minv[0] * dx + (double)a.minv[1] * dy) + (double)a.minv[2] * dz;
        const double pb = ((double)a.minv[3] * dx + (double)a.minv[4] * dy) + (double)a.minv[5] * dz;
        const double pc = ((double)a.minv[6] * dx + (double)a.minv[7] * dy) + (double)a.minv[8] * dz;
        const bool in_front = hit && pa > 0.0;                                 // a <= 0: behind the history's camera
        const double pa_s = in_front ? pa : 1.0;
        double fx = (pb / pa_s) * (double)a.width, fy = (pc / pa_s) * (double)a.height - (double)a.first_row;
        // two pixels outside the band every tap is outside it: clamp there, so that the integer conversion is defined (a NaN goes to a bound)
        fx = fmin(fmax(fx, -2.0), (double)a.width + 1.0);
        fy = fmin(fmax(fy, -2.0), (double)a.n_rows + 1.0);
        const double flx = floor(fx), fly = floor(fy);
        const long long x0 = (long long)flx, y0 = (long long)fly;
        const double wx = fx - flx, wy = fy - fly;
        float4 hc[4], hx[4], hn[4], hm[4];
        bool in[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long qx = x0 + (k & 1), qy = y0 + (k >> 1);
            in[k] = qx >= 0 && qx < (long long)a.width && qy >= 0 && qy < (long long)a.n_rows;
            const size_t qx_c = clamp_tap(qx, (long long)a.width), qy_c = clamp_tap(qy, (long long)a.n_rows);
            const size_t j = qy_c * a.width + qx_c;
            hc[k] = a.hist[j]; hx[k] = a.hist_guides[2 * j]; hn[k] = a.hist_guides[2 * j + 1];
            if constexpr (MOMENTS) hm[k] = a.have_moments != 0u ? a.moments[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        const size_t m_c = hit ? (size_t)mat : 0u;                             // a miss reads material 0 and is masked below
        const float specular = a.materials[4 * m_c].w, refractivity = a.materials[4 * m_c + 1].x;
        const bool view_dependent = a.drop_view_dependent != 0u && (specular > 0.0f || refractivity > 0.0f);
        const double tol = (double)a.plane_tolerance * (double)g0.w;
        double wsum = 0.0;
        float sr = 0.0f, sg = 0.0f, sb = 0.0f, sh = 0.0f;
        float smu = 0.0f, sv = 0.0f, sk = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double ndot = ((double)hn[k].x * (double)n4.x + (double)hn[k].y * (double)n4.y) + (double)hn[k].z * (double)n4.z;
            const double dplane = ((double)n4.x * ((double)hx[k].x - (double)x4.x) + (double)n4.y * ((double)hx[k].y - (double)x4.y)) +
                                  (double)n4.z * ((double)hx[k].z - (double)x4.z);
            const bool valid = in[k] && __float_as_uint(hn[k].w) == obj && ndot >= (double)a.normal_cos_min && fabs(dplane) <= tol;
            const double w = valid ? ((k & 1) ? wx : 1.0 - wx) * ((k >> 1) ? wy : 1.0 - wy) : 0.0;
            const float wf = (float)w;
            wsum += w;
            sr += wf * hc[k].x; sg += wf * hc[k].y; sb += wf * hc[k].z; sh += wf * hc[k].w;
            if constexpr (MOMENTS) { smu += wf * hm[k].x; sv += wf * hm[k].y; sk += wf * hm[k].z; }
        }
        const bool use = in_front && !view_dependent && wsum > 0.01 && !((MOTION || POSE) && dropped);   // in_front: a hit, so an equal object index is a hit's
        const float inv = 1.0f / (use ? (float)wsum : 1.0f);
        hr = sr * inv; hg = sg * inv; hb = sb * inv;
        H = use ? sh * inv : 0.0f;
        if constexpr (MOMENTS) { mu_h = smu * inv; v_h = sv * inv; K_h = use ? sk * inv : 0.0f; }   // no colour history: no moments
    }
    const float He = fminf(H, a.max_history), N = a.n_samples;
    const float inv = 1.0f / (He + N);
    float r = c0.x, g = c0.y, b = c0.z;
    if (He > 0.0f) {                                                           // no history: c = c_0 bit for bit
        r = (He * hr + N * c0.x) * inv; g = (He * hg + N * c0.y) * inv; b = (He * hb + N * c0.z) * inv;
    }
    a.hist_out[i] = make_float4(r, g, b, fminf(He + N, a.max_history));
    a.hist_guides_out[2 * i] = g0; a.hist_guides_out[2 * i + 1] = g1;
    if constexpr (MOMENTS) {
        const float l0 = luminance(c0.x, c0.y, c0.z);
        const float Ke = fminf(K_h, a.max_history), tot = Ke + N;
        float mu = l0, v = 0.0f, K = N;
        if (Ke > 0.0f) {
            mu = (Ke * mu_h + N * l0) / tot;
            const float dm = mu_h - mu, dl = l0 - mu;
            v = (Ke * (v_h + dm * dm) + N * (dl * dl)) / tot;
            K = fminf(tot, a.max_history);
        }
        a.moments_out[i] = make_float4(mu, v, K, 0.0f);
        a.variance[i] = tot >= a.min_history_n ? v * N / tot : -1.0f;
    }
    if (FINAL) write_output(r, g, b, a.demodulate, a.demod, a.color, a.pixels, i);
    else a.color[i] = make_float4(r, g, b, 0.0f);
}

// ---- following poses (CGPT_TEMPORAL_FOLLOW_POSES; tests/pose_motion_ref.py states it in numpy) ----------------------
struct PoseArgs {
    const float4* guides;          // this frame's
    const uint32_t* tri;           // the first hit's triangle, beside the guides (guides_tri_kernel)
    const PoseRecord* table;       // one record per object (ctx_internal.h), built by PreparePoses
    const float4* matrices;        // the history's joint matrices of every re-posed skin, 3 float4 per joint
    float4* out;                   // 2 float4 per pixel {x_p.xyz, bits(state) | n_p.xyz, 0}
    uint32_t width, n_rows;
};

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }

// One thread per pixel: where the pixel's first hit was under the pose the temporal history was stored with.  A pose is always computed
// from the bind pose, so that place is a function of the history's joint matrices alone: the hit's barycentric coordinates on the
// current triangle (tri_orig), applied to the same triangle posed -- by skinning.h's float arithmetic, the bits skin_triangles wrote
// then -- with the history's matrices.  Everything around that is double on the float inputs and rounded to float once, as
// temporal_merge's geometry is and for its reason.  In order:
//  1. P, the hit in object space: x, or Ainv x + binv with the scene's float inverse for an object with a transform;
//  2. e1 = p1 - p0, e2 = p2 - p0, w = P - p0, g = e1 x e2, gg = g.g, u = ((w x e2).g) / gg, v = ((e1 x w).g) / gg (smooth_normal's
//     steps 2-3, not clamped); gg zero or not finite: state 2;
//  3. q_c, m_c: SkinBlend / SkinCorner on bind[tri], joints[tri], weights[tri] and the history's matrices;
//  4. x' = (q0 + u (q1 - q0)) + v (q2 - q0);
//  5. n' = m0, or with the smooth flag ((1 - u - v) m0 + u m1) + v m2 over its length (m0 where the squared length is not > 1e-12);
//     smooth_normal's side fallback (its step 5) is not replayed: n' only feeds temporal_merge's two validity tests;
//  6. x_p = A x' + b, n_p = normalize(Ainv^T n') through the object's current transform; an object without one takes x', n' as they are;
//     anything not finite: state 2.
// A miss, a hit on an object that was not re-posed and a state-2 pixel write their own x and n.
// The joint matrices are read through the vector cache, not staged in LDS as skin_triangles stages them: a frame can hold several
// skins, a 16x16 tile would stage up to 48 KB to use a handful of rows, and the pixels of a tile hit neighbouring triangles that share
// their joints, so the rows a tile reads are few and stay in L1.  The gathers of a pixel -- the table record, then the triangle's
// corners, skin and current positions, then the 36 matrix rows -- are each issued together before anything reads them.
__global__ void __launch_bounds__(256) pose_carry_back(const DevScene sc, const PoseArgs a)
{
    uint32_t px, row;
    tile_pixel(a.width, px, row);
    if (px >= a.width || row >= a.n_rows) return;
    const size_t i = (size_t)row * a.width + px;
    const float4 g0 = a.guides[3 * i], g1 = a.guides[3 * i + 1];
    const uint32_t obj = __float_as_uint(g1.w);
    const bool hit = obj != kNoHit;
    const PoseRecord* const rec = a.table + (hit ? (size_t)obj : 0u);           // a miss reads record 0 and is masked
    uint32_t state = hit ? rec->state : 0u;
    float ox = g0.x, oy = g0.y, oz = g0.z, onx = g1.x, ony = g1.y, onz = g1.z;
    if (state == 1u) {
        const uint32_t tri_base = rec->tri_base, smooth = rec->smooth, n_tris = rec->n_tris;
        const float2* const bind = rec->bind;
        const uint2* const joints = rec->joints;
        const float4* const weights = rec->weights;
        const float4* const mat = a.matrices + 3u * (size_t)rec->matrix_base;
        float A[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) A[k] = rec->xform[k];
        const bool xf = has_xform(sc, obj);
        const Xform inv = load_xform(sc, obj);
        const uint32_t tau = a.tri[i];                                         // read here only: a call without a state-1 object may have no index buffer
        const size_t t = tau < n_tris ? tau : n_tris - 1u;                      // a mesh's tri_idx was validated at upload
        const float4* const orig = sc.tri_orig + 3u * ((size_t)tri_base + t);
        const float4 c0 = orig[0], c1 = orig[1], c2 = orig[2];
        uint2 jw[3];
        float4 w[3];
        float2 b[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            jw[c] = joints[3 * t + c];
            w[c] = weights[3 * t + c];
            b[c][0] = bind[9 * t + 3 * c]; b[c][1] = bind[9 * t + 3 * c + 1]; b[c][2] = bind[9 * t + 3 * c + 2];
        }
        float4 rows[3][4][3];                                                  // [corner][influence][row]
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t j[4] = { jw[c].x & 0xFFFFu, jw[c].x >> 16, jw[c].y & 0xFFFFu, jw[c].y >> 16 };
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int r = 0; r < 3; ++r) rows[c][k][r] = mat[3u * j[k] + r];
        }
        float q[3][6];                                                         // the history pose's corners {pos, normal}: skin_triangles' arithmetic
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float m[12];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float4 a0 = rows[c][0][r], a1 = rows[c][1][r], a2 = rows[c][2][r], a3 = rows[c][3][r];
                m[4 * r] = SkinBlend(w[c].x, a0.x, w[c].y, a1.x, w[c].z, a2.x, w[c].w, a3.x);
                m[4 * r + 1] = SkinBlend(w[c].x, a0.y, w[c].y, a1.y, w[c].z, a2.y, w[c].w, a3.y);
                m[4 * r + 2] = SkinBlend(w[c].x, a0.z, w[c].y, a1.z, w[c].z, a2.z, w[c].w, a3.z);
                m[4 * r + 3] = SkinBlend(w[c].x, a0.w, w[c].y, a1.w, w[c].z, a2.w, w[c].w, a3.w);
            }
            const float pn[6] = { b[c][0].x, b[c][0].y, b[c][1].x, b[c][1].y, b[c][2].x, b[c][2].y };
            SkinCorner(m, pn, q[c]);
        }
        // 1. the hit in object space
        const double gx = (double)g0.x, gy = (double)g0.y, gz = (double)g0.z;
        const double Px = xf ? dot3((double)inv.r0.x, (double)inv.r0.y, (double)inv.r0.z, gx, gy, gz) + (double)inv.r0.w : gx;
        const double Py = xf ? dot3((double)inv.r1.x, (double)inv.r1.y, (double)inv.r1.z, gx, gy, gz) + (double)inv.r1.w : gy;
        const double Pz = xf ? dot3((double)inv.r2.x, (double)inv.r2.y, (double)inv.r2.z, gx, gy, gz) + (double)inv.r2.w : gz;
        // 2. its coordinates on the current triangle
        const double e1x = (double)c1.x - (double)c0.x, e1y = (double)c1.y - (double)c0.y, e1z = (double)c1.z - (double)c0.z;
        const double e2x = (double)c2.x - (double)c0.x, e2y = (double)c2.y - (double)c0.y, e2z = (double)c2.z - (double)c0.z;
        const double wx = Px - (double)c0.x, wy = Py - (double)c0.y, wz = Pz - (double)c0.z;
        const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;   // g = e1 x e2
        const double gg = dot3(nx, ny, nz, nx, ny, nz);
        const double u = dot3(wy * e2z - wz * e2y, wz * e2x - wx * e2z, wx * e2y - wy * e2x, nx, ny, nz) / gg;
        const double v = dot3(e1y * wz - e1z * wy, e1z * wx - e1x * wz, e1x * wy - e1y * wx, nx, ny, nz) / gg;
        // 4. the same point of the history pose's triangle
        const double xx = ((double)q[0][0] + u * ((double)q[1][0] - (double)q[0][0])) + v * ((double)q[2][0] - (double)q[0][0]);
        const double xy = ((double)q[0][1] + u * ((double)q[1][1] - (double)q[0][1])) + v * ((double)q[2][1] - (double)q[0][1]);
        const double xz = ((double)q[0][2] + u * ((double)q[1][2] - (double)q[0][2])) + v * ((double)q[2][2] - (double)q[0][2]);
        // 5. and its normal
        double mx = (double)q[0][3], my = (double)q[0][4], mz = (double)q[0][5];
        if (smooth != 0u) {
            const double w0 = 1.0 - u - v;
            const double sx = (w0 * mx + u * (double)q[1][3]) + v * (double)q[2][3];
            const double sy = (w0 * my + u * (double)q[1][4]) + v * (double)q[2][4];
            const double sz = (w0 * mz + u * (double)q[1][5]) + v * (double)q[2][5];
            const double l2 = dot3(sx, sy, sz, sx, sy, sz);
            if (l2 > 1e-12) {
                const double len = sqrt(l2);
                mx = sx / len; my = sy / len; mz = sz / len;
            }
        }
        // 6. back into the world
        double wxp = xx, wyp = xy, wzp = xz, wnx = mx, wny = my, wnz = mz;
        if (xf) {
            wxp = dot3((double)A[0], (double)A[1], (double)A[2], xx, xy, xz) + (double)A[3];
            wyp = dot3((double)A[4], (double)A[5], (double)A[6], xx, xy, xz) + (double)A[7];
            wzp = dot3((double)A[8], (double)A[9], (double)A[10], xx, xy, xz) + (double)A[11];
            const double tx = dot3((double)inv.r0.x, (double)inv.r1.x, (double)inv.r2.x, mx, my, mz);
            const double ty = dot3((double)inv.r0.y, (double)inv.r1.y, (double)inv.r2.y, mx, my, mz);
            const double tz = dot3((double)inv.r0.z, (double)inv.r1.z, (double)inv.r2.z, mx, my, mz);
            const double len = sqrt(dot3(tx, ty, tz, tx, ty, tz));
            wnx = tx / len; wny = ty / len; wnz = tz / len;
        }
        const float fx = (float)wxp, fy = (float)wyp, fz = (float)wzp, fnx = (float)wnx, fny = (float)wny, fnz = (float)wnz;
        const bool ok = gg != 0.0 && isfinite(gg) && isfinite(fx) && isfinite(fy) && isfinite(fz) && isfinite(fnx) && isfinite(fny) && isfinite(fnz);
        state = ok ? 1u : 2u;
        ox = ok ? fx : ox; oy = ok ? fy : oy; oz = ok ? fz : oz;
        onx = ok ? fnx : onx; ony = ok ? fny : ony; onz = ok ? fnz : onz;
    }
    a.out[2 * i] = make_float4(ox, oy, oz, __uint_as_float(state));
    a.out[2 * i + 1] = make_float4(onx, ony, onz, 0.0f);
}

// ---- following morphs (CGPT_TEMPORAL_FOLLOW_MORPHS; tests/morph_motion_ref.py states it in numpy) -------------------
struct MorphCarryArgs {
    PoseArgs pose;                 // as pose_carry_back's
    const MorphRecord* morph_table;   // one record per object beside pose.table (ctx_internal.h), built by PreparePoses
    const uint2* active;           // the history's active tables {target, bits(weight)} of every re-posed object with targets
};

// pose_carry_back for a call in which an object with morph targets was re-posed; it runs in that kernel's place (one pass and one record
// buffer for a frame that has both kinds), and a kernel of its own name so that pose_carry_back keeps its instruction stream.  The six
// steps are that kernel's and so is their arithmetic; step 3, the history pose's corners of triangle tau, depends on the object's
// MorphRecord:
//   kMorphRecordMorph  x[18] = the base record of tau; for each entry {k, w} of the history's active table in order MorphAccumulate(x, w,
//                      target k's record); with a non-empty table MorphNormalise(base, x) -- morph.h's float arithmetic, contraction off,
//                      the bits morph_triangles held in registers then.  LEAF: the record's nine float2 planes lie at
//                      data[(9 s + p) n + slot_of_tri[tau]], otherwise at data[9 (s n + tau) + p].  Without the flag x is the skin's bind record;
//   kMorphRecordSkin   each corner of x goes through SkinBlend / SkinCorner with the history's matrices (morph_triangles<SKIN>'s order:
//                      the morph first); without the flag the corners are x.
// The active table's length is per lane (a tile mostly shares one object).  Two targets are in flight at a time: their eighteen float2
// loads are issued before the first accumulate; a lane whose table has an odd length loads its last entry twice and accumulates it once
// (a zero weight must not be accumulated: -0 + 0 d is +0).  The morph runs first, into x; only then are the 36 matrix rows fetched.
__global__ void __launch_bounds__(256) morph_carry_back(const DevScene sc, const MorphCarryArgs ma)
{
    const PoseArgs& a = ma.pose;
    uint32_t px, row;
    tile_pixel(a.width, px, row);
    if (px >= a.width || row >= a.n_rows) return;
    const size_t i = (size_t)row * a.width + px;
    const float4 g0 = a.guides[3 * i], g1 = a.guides[3 * i + 1];
    const uint32_t obj = __float_as_uint(g1.w);
    const bool hit = obj != kNoHit;
    const PoseRecord* const rec = a.table + (hit ? (size_t)obj : 0u);           // a miss reads record 0 and is masked
    const MorphRecord* const mrec = ma.morph_table + (hit ? (size_t)obj : 0u);
    uint32_t state = hit ? rec->state : 0u;
    float ox = g0.x, oy = g0.y, oz = g0.z, onx = g1.x, ony = g1.y, onz = g1.z;
    if (state == 1u) {
        const uint32_t tri_base = rec->tri_base, smooth = rec->smooth, n_tris = rec->n_tris;
        const uint32_t mflags = mrec->flags;
        float A[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) A[k] = rec->xform[k];
        const bool xf = has_xform(sc, obj);
        const Xform inv = load_xform(sc, obj);
        const uint32_t tau = a.tri[i];
        const size_t t = tau < n_tris ? tau : n_tris - 1u;                      // a mesh's tri_idx was validated at upload
        const float4* const orig = sc.tri_orig + 3u * ((size_t)tri_base + t);
        const float4 c0 = orig[0], c1 = orig[1], c2 = orig[2];
        // 3. the history pose's corners: the morph ...
        float x[18];
        if (mflags & kMorphRecordMorph) {
            const float2* const data = mrec->data;
            const uint2* const active = ma.active + mrec->active_base;
            const uint32_t n_active = mrec->n_active;
            const bool leaf = (mflags & kMorphRecordLeaf) != 0u;
            const size_t n = n_tris;
            const size_t first = leaf ? (size_t)mrec->slot_of_tri[t] : 9u * t, plane = leaf ? n : 1u;   // plane p of set s: data[9 s n + first + p plane]
            float base[18];
#pragma unroll
            for (int p = 0; p < 9; ++p) {
                const float2 v = data[first + (size_t)p * plane];
                base[2 * p] = v.x; base[2 * p + 1] = v.y;
            }
#pragma unroll
            for (int j = 0; j < 18; ++j) x[j] = base[j];
            for (uint32_t e = 0; e < n_active; e += 2u) {
                const bool two = e + 1u < n_active;
                const uint2 k0 = active[e], k1 = active[two ? e + 1u : e];
                const float2* const s0 = data + 9u * n * ((size_t)k0.x + 1u) + first;
                const float2* const s1 = data + 9u * n * ((size_t)k1.x + 1u) + first;
                float2 v0[9], v1[9];
#pragma unroll
                for (int p = 0; p < 9; ++p) { v0[p] = s0[(size_t)p * plane]; v1[p] = s1[(size_t)p * plane]; }
                float d[18];
#pragma unroll
                for (int p = 0; p < 9; ++p) { d[2 * p] = v0[p].x; d[2 * p + 1] = v0[p].y; }
                MorphAccumulate(x, __uint_as_float(k0.y), d);
                if (two) {
#pragma unroll
                    for (int p = 0; p < 9; ++p) { d[2 * p] = v1[p].x; d[2 * p + 1] = v1[p].y; }
                    MorphAccumulate(x, __uint_as_float(k1.y), d);
                }
            }
            if (n_active != 0u) MorphNormalise(base, x);
        } else {
            const float2* const bind = rec->bind;
#pragma unroll
            for (int p = 0; p < 9; ++p) {
                const float2 v = bind[9 * t + p];
                x[2 * p] = v.x; x[2 * p + 1] = v.y;
            }
        }
        // ... and the skin
        float q[3][6];
        if (mflags & kMorphRecordSkin) {
            const uint2* const joints = rec->joints;
            const float4* const weights = rec->weights;
            const float4* const mat = a.matrices + 3u * (size_t)rec->matrix_base;
            uint2 jw[3];
            float4 w[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { jw[c] = joints[3 * t + c]; w[c] = weights[3 * t + c]; }
            float4 rows[3][4][3];                                              // [corner][influence][row]
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t j[4] = { jw[c].x & 0xFFFFu, jw[c].x >> 16, jw[c].y & 0xFFFFu, jw[c].y >> 16 };
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int r = 0; r < 3; ++r) rows[c][k][r] = mat[3u * j[k] + r];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float m[12];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float4 a0 = rows[c][0][r], a1 = rows[c][1][r], a2 = rows[c][2][r], a3 = rows[c][3][r];
                    m[4 * r] = SkinBlend(w[c].x, a0.x, w[c].y, a1.x, w[c].z, a2.x, w[c].w, a3.x);
                    m[4 * r + 1] = SkinBlend(w[c].x, a0.y, w[c].y, a1.y, w[c].z, a2.y, w[c].w, a3.y);
                    m[4 * r + 2] = SkinBlend(w[c].x, a0.z, w[c].y, a1.z, w[c].z, a2.z, w[c].w, a3.z);
                    m[4 * r + 3] = SkinBlend(w[c].x, a0.w, w[c].y, a1.w, w[c].z, a2.w, w[c].w, a3.w);
                }
                SkinCorner(m, x + 6 * c, q[c]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < 6; ++k) q[c][k] = x[6 * c + k];
        }
        // 1. the hit in object space
        const double gx = (double)g0.x, gy = (double)g0.y, gz = (double)g0.z;
        const double Px = xf ? dot3((double)inv.r0.x, (double)inv.r0.y, (double)inv.r0.z, gx, gy, gz) + (double)inv.r0.w : gx;
        const double Py = xf ? dot3((double)inv.r1.x, (double)inv.r1.y, (double)inv.r1.z, gx, gy, gz) + (double)inv.r1.w : gy;
        const double Pz = xf ? dot3((double)inv.r2.x, (double)inv.r2.y, (double)inv.r2.z, gx, gy, gz) + (double)inv.r2.w : gz;
        // 2. its coordinates on the current triangle
        const double e1x = (double)c1.x - (double)c0.x, e1y = (double)c1.y - (double)c0.y, e1z = (double)c1.z - (double)c0.z;
        const double e2x = (double)c2.x - (double)c0.x, e2y = (double)c2.y - (double)c0.y, e2z = (double)c2.z - (double)c0.z;
        const double wx = Px - (double)c0.x, wy = Py - (double)c0.y, wz = Pz - (double)c0.z;
        const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;   // g = e1 x e2
        const double gg = dot3(nx, ny, nz, nx, ny, nz);
        const double u = dot3(wy * e2z - wz * e2y, wz * e2x - wx * e2z, wx * e2y - wy * e2x, nx, ny, nz) / gg;
        const double v = dot3(e1y * wz - e1z * wy, e1z * wx - e1x * wz, e1x * wy - e1y * wx, nx, ny, nz) / gg;
        // 4. the same point of the history pose's triangle
        const double xx = ((double)q[0][0] + u * ((double)q[1][0] - (double)q[0][0])) + v * ((double)q[2][0] - (double)q[0][0]);
        const double xy = ((double)q[0][1] + u * ((double)q[1][1] - (double)q[0][1])) + v * ((double)q[2][1] - (double)q[0][1]);
        const double xz = ((double)q[0][2] + u * ((double)q[1][2] - (double)q[0][2])) + v * ((double)q[2][2] - (double)q[0][2]);
        // 5. and its normal
        double mx = (double)q[0][3], my = (double)q[0][4], mz = (double)q[0][5];
        if (smooth != 0u) {
            const double w0 = 1.0 - u - v;
            const double sx = (w0 * mx + u * (double)q[1][3]) + v * (double)q[2][3];
            const double sy = (w0 * my + u * (double)q[1][4]) + v * (double)q[2][4];
            const double sz = (w0 * mz + u * (double)q[1][5]) + v * (double)q[2][5];
            const double l2 = dot3(sx, sy, sz, sx, sy, sz);
            if (l2 > 1e-12) {
                const double len = sqrt(l2);
                mx = sx / len; my = sy / len; mz = sz / len;
            }
        }
        // 6. back into the world
        double wxp = xx, wyp = xy, wzp = xz, wnx = mx, wny = my, wnz = mz;
        if (xf) {
            wxp = dot3((double)A[0], (double)A[1], (double)A[2], xx, xy, xz) + (double)A[3];
            wyp = dot3((double)A[4], (double)A[5], (double)A[6], xx, xy, xz) + (double)A[7];
            wzp = dot3((double)A[8], (double)A[9], (double)A[10], xx, xy, xz) + (double)A[11];
            const double tx = dot3((double)inv.r0.x, (double)inv.r1.x, (double)inv.r2.x, mx, my, mz);
            const double ty = dot3((double)inv.r0.y, (double)inv.r1.y, (double)inv.r2.y, mx, my, mz);
            const double tz = dot3((double)inv.r0.z, (double)inv.r1.z, (double)inv.r2.z, mx, my, mz);
            const double len = sqrt(dot3(tx, ty, tz, tx, ty, tz));
            wnx = tx / len; wny = ty / len; wnz = tz / len;
        }
        const float fx = (float)wxp, fy = (float)wyp, fz = (float)wzp, fnx = (float)wnx, fny = (float)wny, fnz = (float)wnz;
        const bool ok = gg != 0.0 && isfinite(gg) && isfinite(fx) && isfinite(fy) && isfinite(fz) && isfinite(fnx) && isfinite(fny) && isfinite(fnz);
        state = ok ? 1u : 2u;
        ox = ok ? fx : ox; oy = ok ? fy : oy; oz = ok ? fz : oz;
        onx = ok ? fnx : onx; ony = ok ? fny : ony; onz = ok ? fnz : onz;
    }
    a.out[2 * i] = make_float4(ox, oy, oz, __uint_as_float(state));
    a.out[2 * i + 1] = make_float4(onx, ony, onz, 0.0f);
}

// ---- the variance-guided filter (cgpt_denoise_variance_guided; tests/variance_ref.py states it in numpy) ----------
constexpr cgpt_variance_params kVarianceDefaults = { 4.0f, 4u, 0u };

struct VarianceArgs {
    float4* color;             // the image the passes will read (c_0 or the merged c); out: .w = var
    const float4* guides;
    float* variance;           // in (have_temporal): var_t or -1 of temporal_merge<false, true>; out: var
    uint32_t width, n_rows, have_temporal;
    float inv_normal, inv_position;   // 1 / sigma^2 of pass 0
};

// var_s of a pixel: the weighted variance of the luminance over the 7x7 window around it, d_q = l(c_q) - l(c_p) shifted by the centre so
// that a smooth region does not cancel; the weights are the filter's geometry term (two hits), 1 (two misses), none (a hit and a miss, or
// outside the band).  A row of seven taps at a time, loads first, selects for the masks (atrous_pass's lessons).  A pixel that has its
// var_t skips the window: after a few static frames that is the whole frame, and the kernel is one load and two stores per pixel.
__global__ void __launch_bounds__(256) variance_estimate(const VarianceArgs a)
{
    uint32_t px, row;
    tile_pixel(a.width, px, row);
    if (px >= a.width || row >= a.n_rows) return;
    const size_t i = (size_t)row * a.width + px;
    float var = a.have_temporal != 0u ? a.variance[i] : -1.0f;
    if (var < 0.0f) {
        const float4 xp4 = a.guides[3 * i], np4 = a.guides[3 * i + 1];
        const V3 x_p = mk(xp4.x, xp4.y, xp4.z), n_p = mk(np4.x, np4.y, np4.z);
        const bool hit_p = __float_as_uint(np4.w) != kNoHit;
        const float4 cp4 = a.color[i];
        const float l_p = luminance(cp4.x, cp4.y, cp4.z);
        float sw = 0.0f, swd = 0.0f, swd2 = 0.0f;
#pragma unroll
        for (int dy = -3; dy <= 3; ++dy) {
            const int qy = (int)row + dy;
            const bool row_in = qy >= 0 && qy < (int)a.n_rows;
            const size_t qy_c = (size_t)(qy < 0 ? 0 : (row_in ? qy : (int)a.n_rows - 1));
            float4 xq[7], nq[7], cq[7];
            bool in[7];
#pragma unroll
            for (int t = 0; t < 7; ++t) {
                const int qx = (int)px + t - 3;
                in[t] = row_in && qx >= 0 && qx < (int)a.width;
                const size_t j = qy_c * a.width + clamp_tap(qx, (int)a.width);
                xq[t] = a.guides[3 * j]; nq[t] = a.guides[3 * j + 1]; cq[t] = a.color[j];
            }
#pragma unroll
            for (int t = 0; t < 7; ++t) {
                const bool hit_q = __float_as_uint(nq[t].w) != kNoHit;
                const float e_geo = geometry_exponent(xq[t], nq[t], x_p, n_p, a.inv_normal, a.inv_position);
                const float w = hit_p && hit_q ? __expf(-e_geo) : 1.0f;       // the centre tap: e = 0, w = 1
                const float d = luminance(cq[t].x, cq[t].y, cq[t].z) - l_p;
                const bool use = in[t] && hit_q == hit_p;
                sw = use ? sw + w : sw;
                swd = use ? swd + w * d : swd;
                swd2 = use ? swd2 + (w * d) * d : swd2;
            }
            __builtin_amdgcn_sched_barrier(0);                                // one row's loads in flight at a time
        }
        const float m1 = swd / sw;
        var = fmaxf(0.0f, swd2 / sw - m1 * m1);
    }
    a.variance[i] = var;
    reinterpret_cast<float*>(a.color)[4 * i + 3] = var;                       // the .w lane the passes carry it in
}

// atrous_pass with the colour edge-stop in standard deviations of the pixel: exp(-|l(c_q) - l(c_p)| / (sigma_l sqrt(gbar(p)) + 1e-6)),
// gbar the 3x3 Gaussian of the variance over p's immediate neighbours (step 1 in every pass; over the taps in the band with p's hit /
// miss state, renormalised), and the variance filtered along with the colour: var' = sum w^2 var_q / (sum w)^2 in the .w lane.
// 1 / (sigma_l sqrt(gbar) + 1e-6) once per pixel, from nine loads of their own in front of the rows; the luminance term joins the
// geometry term in one exponent, so a tap still costs one __expf.
template <bool LAST>
__global__ void __launch_bounds__(256) variance_pass(const VarPassArgs a)
{
    uint32_t px, row;
    tile_pixel(a.width, px, row);
    if (px >= a.width || row >= a.n_rows) return;
    const size_t i = (size_t)row * a.width + px;
    const float4 xp4 = a.guides[3 * i], np4 = a.guides[3 * i + 1];
    const V3 x_p = mk(xp4.x, xp4.y, xp4.z), n_p = mk(np4.x, np4.y, np4.z);
    const bool hit_p = __float_as_uint(np4.w) != kNoHit;
    const float4 cp4 = a.src[i];
    const float l_p = luminance(cp4.x, cp4.y, cp4.z);
    float inv_l;
    {
        float vq[9], hq[9];
        bool in[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int qx = (int)px + k % 3 - 1, qy = (int)row + k / 3 - 1;
            in[k] = qx >= 0 && qx < (int)a.width && qy >= 0 && qy < (int)a.n_rows;
            const size_t j = clamp_tap(qy, (int)a.n_rows) * a.width + clamp_tap(qx, (int)a.width);
            vq[k] = reinterpret_cast<const float*>(a.src)[4 * j + 3];
            hq[k] = reinterpret_cast<const float*>(a.guides)[12 * j + 7];
        }
        float num = 0.0f, den = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float g = ((k % 3 == 1 ? 2.0f : 1.0f) * (k / 3 == 1 ? 2.0f : 1.0f)) * 0.0625f;
            const bool use = in[k] && (__float_as_uint(hq[k]) != kNoHit) == hit_p;
            num = use ? num + g * vq[k] : num;
            den = use ? den + g : den;
        }
        inv_l = 1.0f / (a.color_scale * sqrtf(num / den) + 1e-6f);
    }
    __builtin_amdgcn_sched_barrier(0);                                        // gbar's loads are done before the rows' begin
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const long long qy = (long long)row + (long long)dy * a.step;
        const bool row_in = qy >= 0 && qy < (long long)a.n_rows;
        const size_t qy_c = (size_t)(qy < 0 ? 0 : (row_in ? qy : (long long)a.n_rows - 1));   // clamp_tap on row_in's comparison
        float4 xq[5], nq[5], cq[5];
        bool in[5];
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const long long qx = (long long)px + (long long)(t - 2) * a.step;
            in[t] = row_in && qx >= 0 && qx < (long long)a.width;
            const size_t j = qy_c * a.width + clamp_tap(qx, (long long)a.width);
            xq[t] = a.guides[3 * j]; nq[t] = a.guides[3 * j + 1]; cq[t] = a.src[j];
        }
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const bool hit_q = __float_as_uint(nq[t].w) != kNoHit;
            const float dl = fabsf(luminance(cq[t].x, cq[t].y, cq[t].z) - l_p);
            const float e_geo = geometry_exponent(xq[t], nq[t], x_p, n_p, a.inv_normal, a.inv_position);
            const float e = dl * inv_l + (hit_p && hit_q ? e_geo : 0.0f);
            const float w = (tap(t - 2) * tap(dy)) * __expf(-e);                // the centre tap: e = 0, w = h
            const bool use = in[t] && hit_q == hit_p;
            sr = use ? sr + cq[t].x * w : sr;
            sg = use ? sg + cq[t].y * w : sg;
            sb = use ? sb + cq[t].z * w : sb;
            sv += (use ? w * w : 0.0f) * cq[t].w;                              // the weight masked, not the sum: a select on the sum
                                                                              // let the compiler put this lane's load behind a branch
            wsum = use ? wsum + w : wsum;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    const V3 r = mk(sr / wsum, sg / wsum, sb / wsum);
    if (LAST) write_output(r.x, r.y, r.z, a.demodulate, a.demod, a.dst, a.pixels, i);
    else a.dst[i] = make_float4(r.x, r.y, r.z, sv / (wsum * wsum));
}

// iterations = 0 behind the temporal stage: the merged c times the albedo, packed, w = 1 -- temporal_merge<true>'s output
__global__ void __launch_bounds__(256) variance_identity(const float4* __restrict__ src, const float4* __restrict__ demod, float4* __restrict__ dst,
                                                         uint32_t* __restrict__ pixels, size_t n_pixels, uint32_t demodulate)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    const float4 c = src[i];
    write_output(c.x, c.y, c.z, demodulate, demod, dst, pixels, i);
}

// what a call works on: a one-device context's contiguous band, or a multi-device context's full frame on its first member
struct Frame {
    cgpt_ctx* dev;            // the one-device context whose device, stream, scene and buffers do the work
    uint32_t width, height, first_row, n_rows, num_accumulated;
};

int ResolveFrame(cgpt_ctx* ctx, bool denoise, const cgpt_camera* camera, Frame& f)
{
    uint32_t width, height, num_accumulated, debug;
    if (ctx->group) {
        if (!ctx->has_scene || !GroupFirstMember(ctx)->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "no scene uploaded");
        GroupFrameInfo(ctx, &width, &height, &num_accumulated, &debug);
        if (width == 0) return CtxFail(ctx, CGPT_ERR_INVALID, "nothing rendered yet");
        f.dev = GroupFirstMember(ctx); f.first_row = 0; f.n_rows = height;
    } else {
        if (!ctx->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "no scene uploaded");
        if (!ctx->fb.accumulator.p) return CtxFail(ctx, CGPT_ERR_INVALID, "nothing rendered yet");
        width = ctx->width; height = ctx->height; num_accumulated = ctx->num_accumulated; debug = ctx->last_debug_mode;
        f.dev = ctx; f.first_row = ctx->band_key[0]; f.n_rows = ctx->n_rows;
    }
    if (denoise && num_accumulated == 0) return CtxFail(ctx, CGPT_ERR_INVALID, "nothing accumulated (num_accumulated is 0)");
    if (debug != 0u) return CtxFail(ctx, CGPT_ERR_INVALID, "the last render was a debug view (debug_render_mode %u): its pixels are not radiance", debug);
    if (!ctx->group && (ctx->band_key[2] != 0u || ctx->band_key[3] != 0u))
        return CtxFail(ctx, CGPT_ERR_INVALID, "an interleaved band: its rows are not neighbours (a multi-device context filters the gathered frame)");
    if (!camera) return CtxFail(ctx, CGPT_ERR_INVALID, "camera is null");
    f.width = width; f.height = height; f.num_accumulated = num_accumulated;
    return CGPT_OK;
}

// the frame's 16x16 tiles: the grid of every kernel that tile_pixel places
uint32_t Tiles(const Frame& f) { return ((f.width + kTile - 1u) / kTile) * ((f.n_rows + kTile - 1u) / kTile); }

// [kGuideLevels - 1 - guide level] (ctx_internal.h: ChooseGuideLevel): from the top level down, the order the instantiations have in the code object
decltype(&guides_kernel<false>) const kGuideKernels[kGuideLevels] = { guides_kernel<true, true, true>, guides_kernel<true, true>, guides_kernel<true>, guides_kernel<false> };

// the context holds a skin: its guides come with the triangle index (guides_tri_kernel)
bool HoldsSkin(const cgpt_ctx* d)
{
    for (const SkinBuffers& sk : d->skins)
        if (sk.n_joints != 0u) return true;
    return false;
}
// ... or morph targets: likewise (CGPT_TEMPORAL_FOLLOW_MORPHS carries a hit back through the same index)
bool HoldsMorphTargets(const cgpt_ctx* d)
{
    for (const MorphBuffers& mb : d->morphs)
        if (mb.n_targets != 0u) return true;
    return false;
}

int EnsureGuides(cgpt_ctx* ctx, const Frame& f, const cgpt_camera* camera)
{
    cgpt_ctx* d = f.dev;
    const uint32_t key[4] = { f.width, f.height, f.first_row, f.n_rows };
    const bool with_tri = HoldsSkin(d) || HoldsMorphTargets(d);                                      // guides cached without the index are stale for a context that now needs it
    if (d->guides_valid && d->guide_generation == d->scene_generation && memcmp(d->guide_frame, key, sizeof(key)) == 0 &&
        memcmp(&d->guide_camera, camera, sizeof(cgpt_camera)) == 0 && (d->guide_tri_valid || !with_tri))
        return CGPT_OK;
    d->guides_valid = d->guide_tri_valid = false;
    const size_t n = (size_t)f.width * f.n_rows;
    if (d->dn.guide_demod.n != n) {                                            // any other size: both anew (the second one's count is the key)
        ResetAll(d->dn.guides, d->dn.guide_demod);
        HIP_TRY(ctx, d->dn.guides.Alloc(3 * n));
        HIP_TRY(ctx, d->dn.guide_demod.Alloc(n));
    }
    DevCamera cam;
    static_assert(sizeof(DevCamera) == sizeof(cgpt_camera), "camera layouts");
    memcpy(&cam, camera, sizeof(cam));
    const size_t lds = (size_t)d->scene.stack_depth * 256u * sizeof(uint32_t);   // intersect_rays_kernel's stack
    if (with_tri) {
        if (d->dn.guide_tri.n != n) HIP_TRY(ctx, d->dn.guide_tri.Alloc(n));
        hipLaunchKernelGGL((d->top_level ? guides_tri_kernel<true> : guides_tri_kernel<false>), dim3(Tiles(f)), dim3(256), lds, d->stream, d->scene, cam, f.width, f.height, f.first_row, f.n_rows,
                           d->dn.guides.p, d->dn.guide_demod.p, d->dn.guide_tri.p);
    } else
        hipLaunchKernelGGL(kGuideKernels[kGuideLevels - 1 - ChooseGuideLevel(d)], dim3(Tiles(f)), dim3(256), lds, d->stream, d->scene, cam, f.width, f.height, f.first_row, f.n_rows,
                           d->dn.guides.p, d->dn.guide_demod.p);
    HIP_TRY(ctx, hipGetLastError());
    memcpy(d->guide_frame, key, sizeof(key));
    memcpy(&d->guide_camera, camera, sizeof(cgpt_camera));
    d->guide_generation = d->scene_generation;
    d->guides_valid = true;
    d->guide_tri_valid = with_tri;
    return CGPT_OK;
}

int EnsureFilterBuffers(cgpt_ctx* ctx, cgpt_ctx* d, size_t n)
{
    if (d->dn.filter_pixels.n == n) return CGPT_OK;                            // any other size: all three anew (the last one's count is the key)
    ResetAll(d->dn.filter[0], d->dn.filter[1], d->dn.filter_pixels);
    HIP_TRY(ctx, d->dn.filter[0].Alloc(n));
    HIP_TRY(ctx, d->dn.filter[1].Alloc(n));
    HIP_TRY(ctx, d->dn.filter_pixels.Alloc(n));
    return CGPT_OK;
}

int ReadBack(cgpt_ctx* ctx, cgpt_ctx* d, size_t n, const float4* out, float* dst_rgba, uint32_t* dst_pixels)
{
    if (dst_rgba) HIP_TRY(ctx, hipMemcpyAsync(dst_rgba, out, n * sizeof(float4), hipMemcpyDeviceToHost, d->stream));
    if (dst_pixels) HIP_TRY(ctx, hipMemcpyAsync(dst_pixels, d->dn.filter_pixels.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(ctx, hipStreamSynchronize(d->stream));
    return CGPT_OK;
}

int CheckParams(cgpt_ctx* ctx, const cgpt_denoise_params& p)
{
    if (p.iterations > kMaxIterations) return CtxFail(ctx, CGPT_ERR_INVALID, "iterations %u outside [0, %u]", p.iterations, kMaxIterations);
    if (p.flags & ~(uint32_t)CGPT_DENOISE_DEMODULATE_ALBEDO) return CtxFail(ctx, CGPT_ERR_INVALID, "unknown denoise flags 0x%x", p.flags);
    const float s[3] = { p.sigma_color, p.sigma_normal, p.sigma_position };
    for (float v : s)
        if (!std::isfinite(v) || !(v > 0.0f)) return CtxFail(ctx, CGPT_ERR_INVALID, "sigmas must be finite and > 0, got %g, %g, %g", s[0], s[1], s[2]);
    return CGPT_OK;
}

int CheckTemporalParams(cgpt_ctx* ctx, const cgpt_temporal_params& t)
{
    if (!std::isfinite(t.max_history) || !(t.max_history >= 1.0f)) return CtxFail(ctx, CGPT_ERR_INVALID, "max_history must be finite and >= 1, got %g", t.max_history);
    if (!(t.normal_cos_min >= -1.0f && t.normal_cos_min <= 1.0f)) return CtxFail(ctx, CGPT_ERR_INVALID, "normal_cos_min %g outside [-1, 1]", t.normal_cos_min);
    if (!std::isfinite(t.plane_tolerance) || !(t.plane_tolerance > 0.0f)) return CtxFail(ctx, CGPT_ERR_INVALID, "plane_tolerance must be finite and > 0, got %g", t.plane_tolerance);
    if (t.flags & ~(uint32_t)(CGPT_TEMPORAL_KEEP_VIEW_DEPENDENT | CGPT_TEMPORAL_FOLLOW_TRANSFORMS | CGPT_TEMPORAL_FOLLOW_POSES | CGPT_TEMPORAL_FOLLOW_MORPHS)) return CtxFail(ctx, CGPT_ERR_INVALID, "unknown temporal flags 0x%x", t.flags);
    return CGPT_OK;
}

// Minv of a camera: the inverse (adjugate / determinant) of the matrix with the columns top_left - pos, top_right - top_left,
// bottom_left - top_left, in double from the float entries, each entry rounded to float once (as InvertTransform, transform_math.h).
// False for a singular camera or a result that is not finite.
bool InvertCamera(const cgpt_camera& c, float out[9])
{
    double m[3][3];
    for (int r = 0; r < 3; ++r) {
        m[r][0] = (double)c.top_left[r] - (double)c.pos[r];
        m[r][1] = (double)c.top_right[r] - (double)c.top_left[r];
        m[r][2] = (double)c.bottom_left[r] - (double)c.top_left[r];
    }
    const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1], c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2], c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    const double det = (m[0][0] * c00 + m[0][1] * c01) + m[0][2] * c02;
    if (det == 0.0 || !std::isfinite(det)) return false;
    const double inv[9] = {
        c00 / det, (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det, (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det,
        c01 / det, (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det, (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det,
        c02 / det, (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det, (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det,
    };
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite((float)inv[i])) return false;
    for (int i = 0; i < 9; ++i) out[i] = (float)inv[i];
    return true;
}

int EnsureHistoryBuffers(cgpt_ctx* ctx, cgpt_ctx* d, size_t n)
{
    if (d->dn.history_guides[1].n == 2 * n) return CGPT_OK;                    // any other size: all four anew (the last one's count is the key)
    d->temporal_valid = false;
    ResetAll(d->dn.history[0], d->dn.history[1], d->dn.history_guides[0], d->dn.history_guides[1]);
    HIP_TRY(ctx, d->dn.history[0].Alloc(n));
    HIP_TRY(ctx, d->dn.history[1].Alloc(n));
    HIP_TRY(ctx, d->dn.history_guides[0].Alloc(2 * n));
    HIP_TRY(ctx, d->dn.history_guides[1].Alloc(2 * n));
    return CGPT_OK;
}

// the history a call may use: stored by a call that succeeded, for this band, scene and demodulation.  The edits since it was stored
// fall into four classes, counted by the four generations: cgpt_scene_update_transforms calls (scene - shape), kept with `follow`
// (CGPT_TEMPORAL_FOLLOW_TRANSFORMS); cgpt_scene_skin_mesh calls (pose), kept with `follow_poses` (CGPT_TEMPORAL_FOLLOW_POSES); accepted
// cgpt_scene_morph_mesh calls (morph), kept with `follow_morphs` (CGPT_TEMPORAL_FOLLOW_MORPHS); every other edit (shape - pose - morph),
// never kept.  Each flag keeps its own class only.
bool HistoryMatches(const cgpt_ctx* d, const uint32_t key[4], uint32_t demodulate, bool follow, bool follow_poses, bool follow_morphs)
{
    const uint64_t edits = d->scene_generation - d->temporal_generation, shape_edits = d->shape_generation - d->temporal_shape_generation;
    const uint64_t poses = d->pose_generation - d->temporal_pose_generation, morphs = d->morph_generation - d->temporal_morph_generation;
    const bool scene = edits == 0 || (shape_edits == poses + morphs && (edits == shape_edits || follow) && (poses == 0 || follow_poses) && (morphs == 0 || follow_morphs));
    return d->temporal_valid && scene && d->temporal_demodulate == demodulate && memcmp(d->temporal_frame, key, sizeof(d->temporal_frame)) == 0;
}

// CGPT_TEMPORAL_FOLLOW_TRANSFORMS with a usable history: the records of every object against the matrices the history was stored for,
// in d->motion_records and -- when an object moved -- in d->dn.motion (an asynchronous copy on the stream: motion_records lives on).
// `moved`: an object is not unmoved, so the call reprojects through temporal_merge<.., MOTION = true>.
int PrepareMotion(cgpt_ctx* ctx, cgpt_ctx* d, bool& moved)
{
    moved = false;
    const size_t n = d->top_state.xform.size() / 12;
    if (n == 0) return CGPT_OK;
    try { d->motion_records.resize(n); } catch (const std::exception& e) { return CtxFail(ctx, CGPT_ERR_INVALID, "out of host memory: %s", e.what()); }
    if (CompareTransforms(d->temporal_xform.data(), d->temporal_xform.size() / 12, d->top_state.xform.data(), n, d->motion_records.data()) == 0) return CGPT_OK;
    HIP_TRY(ctx, d->dn.motion.Grow(6 * n));                                    // hipFree waits for the device
    static_assert(sizeof(MotionRecord) == 6 * sizeof(float4), "6 float4 per object");
    HIP_TRY(ctx, hipMemcpyAsync(d->dn.motion.p, d->motion_records.data(), n * sizeof(MotionRecord), hipMemcpyHostToDevice, d->stream));
    moved = true;
    return CGPT_OK;
}

// which object's skin posed the copy object j shows, per object: -1 where no pose is known.  A pose through one skin makes every
// other skin of the copy unknown (refit.hip: SkinMesh), so a copy has at most one.
void PoseOwners(const cgpt_ctx* d, std::vector<int32_t>& owner)
{
    owner.assign(d->h_objects.size(), -1);
    for (size_t k = 0; k < d->skins.size(); ++k) {
        if (d->skins[k].n_joints == 0u || !d->skins[k].pose_known) continue;
        for (size_t j = 0; j < owner.size(); ++j)
            if (d->mesh_group[j] == d->mesh_group[k]) owner[j] = (int32_t)k;
    }
}

// the poses a call's history is stored for (empty for a context without a skin)
void SnapshotPoses(const cgpt_ctx* d, PoseSnapshot& snap)
{
    snap = PoseSnapshot{};
    if (!HoldsSkin(d)) return;
    PoseOwners(d, snap.owner);
    snap.serial.assign(snap.owner.size(), 0);
    snap.matrices.resize(snap.owner.size());
    for (const int32_t k : snap.owner)
        if (k >= 0 && snap.serial[k] == 0) { snap.serial[k] = d->skins[k].serial; snap.matrices[k] = d->skins[k].pose; }
}

// which object's morph targets posed the copy object j shows, per object: -1 where none did or no pose is known.  A pose through one
// object's targets makes every other placement's targets and skin unknown (refit.hip: PoseObject), so a copy has at most one, and none
// beside a skin that PoseOwners names.
void MorphOwners(const cgpt_ctx* d, std::vector<int32_t>& owner)
{
    owner.assign(d->h_objects.size(), -1);
    for (size_t k = 0; k < d->morphs.size(); ++k) {
        if (d->morphs[k].n_targets == 0u || !d->morphs[k].pose_known) continue;
        for (size_t j = 0; j < owner.size(); ++j)
            if (d->mesh_group[j] == d->mesh_group[k]) owner[j] = (int32_t)k;
    }
}

// the morphed poses a call's history is stored for (empty for a context without targets)
void SnapshotMorphs(const cgpt_ctx* d, MorphSnapshot& snap)
{
    snap = MorphSnapshot{};
    if (!HoldsMorphTargets(d)) return;
    MorphOwners(d, snap.owner);
    snap.key.resize(snap.owner.size());
    for (const int32_t k : snap.owner)
        if (k >= 0 && snap.key[k].serial == 0) {
            const MorphBuffers& mb = d->morphs[k];
            snap.key[k].serial = mb.serial; snap.key[k].weights = mb.weights;
            snap.key[k].skin_serial = mb.pose_skin_serial; snap.key[k].matrices = mb.pose_matrices;
        }
}

// CGPT_TEMPORAL_FOLLOW_POSES with a usable history that cgpt_scene_skin_mesh calls have happened since: the record of every object
// (ctx_internal.h: PoseRecord) in d->pose_records and, when an object is not in state 0, in dn.pose_table, with the history's matrices of
// the re-posed skins in dn.pose_matrices (asynchronous copies on the stream: the host vectors live on).  An object whose copy no pose
// has written since the history is in state 0 whatever its skin; one that was posed is in state 0 when the matrices equal the
// snapshot's bytewise (A -> B -> A), 1 when they differ, 2 when either side knows no pose or the skin is another installation (or, which
// a skin's presence rules out, the guides came without the triangle index: a state-1 record is the only reader of dn.guide_tri).
// `posed`: an object is not in state 0, so the call runs pose_carry_back and reprojects through temporal_merge<.., POSE = true>.
// With `follow_morphs` (CGPT_TEMPORAL_FOLLOW_MORPHS) the same for the accepted cgpt_scene_morph_mesh calls since the
// history, and for the copies that were posed through an object's morph targets by either call: such a copy's key is the targets'
// installation, the weights and -- if a skin took part -- that skin's installation and matrices (ctx_internal.h: MorphBuffers).  Equal
// keys bytewise: state 0; the same installations and counts with other weights or matrices: state 1, with the object's MorphRecord in
// d->morph_records / dn.morph_table and the history's active table -- ActiveTable of the history's weights -- in dn.morph_active;
// anything else, and any such copy without the flag: state 2.  `morphed`: an object with targets is in state 1, so the call runs
// morph_carry_back in pose_carry_back's place.
int PreparePoses(cgpt_ctx* ctx, cgpt_ctx* d, bool follow_morphs, bool& posed, bool& morphed)
{
    posed = morphed = false;
    const bool have_tri = d->guide_tri_valid;                                  // EnsureGuides ran: the index buffer belongs to this call's guides
    const size_t n = d->h_objects.size();
    const PoseSnapshot& snap = d->temporal_poses;
    const MorphSnapshot& msnap = d->temporal_morphs;
    std::vector<int32_t> owner, morph_owner;
    size_t changed = 0;
    try {
        PoseOwners(d, owner);
        MorphOwners(d, morph_owner);
        d->pose_records.assign(n, PoseRecord{});
        d->morph_records.assign(n, MorphRecord{});
        d->pose_matrices.clear();
        d->morph_active.clear();
        std::vector<int64_t> base(n, -1);                                      // where skin k's history matrices start, in joints
        std::vector<int64_t> active_base(n, -1), active_count(n, 0);           // ... and morph owner k's history active table, in entries
        for (size_t j = 0; j < n; ++j) {
            PoseRecord& r = d->pose_records[j];
            if (d->top_state.xform.size() == 12 * n) memcpy(r.xform, d->top_state.xform.data() + 12 * j, sizeof(r.xform));
            r.tri_base = d->h_objects[j].tri_base; r.smooth = d->h_objects[j].smooth; r.n_tris = d->refit_objects[j].tri_count;
            const bool posed_since = j < d->pose_stamp.size() && d->pose_stamp[j] > d->temporal_pose_generation;
            const bool morphed_since = j < d->morph_stamp.size() && d->morph_stamp[j] > d->temporal_morph_generation;
            if (!posed_since && !morphed_since) continue;                       // not posed since: state 0
            r.state = kMotionDrop;
            const int32_t mk = follow_morphs ? morph_owner[j] : -1;
            if (mk >= 0) {                                                     // the copy shows a pose made through mk's targets
                const MorphBuffers& mb = d->morphs[mk];
                const bool same = have_tri && j < msnap.owner.size() && msnap.owner[j] == mk && msnap.key[mk].serial == mb.serial &&
                                  msnap.key[mk].weights.size() == mb.weights.size() && mb.weights.size() == mb.n_targets &&
                                  msnap.key[mk].skin_serial == mb.pose_skin_serial && msnap.key[mk].matrices.size() == mb.pose_matrices.size();
                const bool skinned = mb.pose_skin_serial != 0;                 // ... and through mk's skin, which must still be the installation that took part
                const bool skin_there = !skinned || ((size_t)mk < d->skins.size() && d->skins[mk].serial == mb.pose_skin_serial &&
                                                     12 * (size_t)d->skins[mk].n_joints == mb.pose_matrices.size());
                if (same && skin_there) {
                    const MorphSnapshot::Key& hk = msnap.key[mk];
                    if (memcmp(hk.weights.data(), mb.weights.data(), mb.weights.size() * sizeof(float)) == 0 &&
                        (!skinned || memcmp(hk.matrices.data(), mb.pose_matrices.data(), mb.pose_matrices.size() * sizeof(float)) == 0)) r.state = kMotionUnmoved;
                    else {
                        if (active_base[mk] < 0) {
                            active_base[mk] = (int64_t)d->morph_active.size();
                            const std::vector<uint2> table = ActiveTable(hk.weights.data(), mb.n_targets);
                            d->morph_active.insert(d->morph_active.end(), table.begin(), table.end());
                            active_count[mk] = (int64_t)table.size();
                        }
                        MorphRecord& m = d->morph_records[j];
                        m.data = mb.data.p; m.slot_of_tri = mb.slot_of_tri.p;
                        m.active_base = (uint32_t)active_base[mk]; m.n_active = (uint32_t)active_count[mk];
                        m.flags = kMorphRecordMorph | (mb.leaf_order ? kMorphRecordLeaf : 0u) | (skinned ? kMorphRecordSkin : 0u);
                        r.state = kMotionMoved;
                        if (skinned) {
                            const SkinBuffers& sk = d->skins[mk];
                            if (base[mk] < 0) {                                // morph and skin owners are disjoint: base[] serves both
                                base[mk] = (int64_t)(d->pose_matrices.size() / 12);
                                d->pose_matrices.insert(d->pose_matrices.end(), hk.matrices.begin(), hk.matrices.end());
                            }
                            r.matrix_base = (uint32_t)base[mk];
                            r.joints = reinterpret_cast<const uint2*>(sk.joints.p);
                            r.weights = reinterpret_cast<const float4*>(sk.weights.p);
                        }
                        morphed = true;
                    }
                }
                if (r.state != kMotionUnmoved) ++changed;
                continue;
            }
            const int32_t k = owner[j];
            if (have_tri && k >= 0 && j < snap.owner.size() && snap.owner[j] == k && snap.serial[k] == d->skins[k].serial && snap.matrices[k].size() == d->skins[k].pose.size()) {
                const SkinBuffers& sk = d->skins[k];
                if (memcmp(snap.matrices[k].data(), sk.pose.data(), sk.pose.size() * sizeof(float)) == 0) r.state = kMotionUnmoved;
                else {
                    if (base[k] < 0) {
                        base[k] = (int64_t)(d->pose_matrices.size() / 12);
                        d->pose_matrices.insert(d->pose_matrices.end(), snap.matrices[k].begin(), snap.matrices[k].end());
                    }
                    r.state = kMotionMoved;
                    r.matrix_base = (uint32_t)base[k];
                    r.bind = reinterpret_cast<const float2*>(sk.bind.p);
                    r.joints = reinterpret_cast<const uint2*>(sk.joints.p);
                    r.weights = reinterpret_cast<const float4*>(sk.weights.p);
                    d->morph_records[j].flags = kMorphRecordSkin;              // read by morph_carry_back alone
                }
            }
            if (r.state != kMotionUnmoved) ++changed;
        }
    } catch (const std::exception& e) { return CtxFail(ctx, CGPT_ERR_INVALID, "out of host memory: %s", e.what()); }
    if (changed == 0) { morphed = false; return CGPT_OK; }
    static_assert(sizeof(PoseRecord) == 6 * sizeof(float4), "6 float4 per object");
    HIP_TRY(ctx, d->dn.pose_table.Grow(6 * n));                                // hipFree waits for the device
    HIP_TRY(ctx, hipMemcpyAsync(d->dn.pose_table.p, d->pose_records.data(), n * sizeof(PoseRecord), hipMemcpyHostToDevice, d->stream));
    if (!d->pose_matrices.empty()) {
        HIP_TRY(ctx, d->dn.pose_matrices.Grow(d->pose_matrices.size() / 4));
        HIP_TRY(ctx, hipMemcpyAsync(d->dn.pose_matrices.p, d->pose_matrices.data(), d->pose_matrices.size() * sizeof(float), hipMemcpyHostToDevice, d->stream));
    }
    if (morphed) {
        static_assert(sizeof(MorphRecord) == 2 * sizeof(float4), "2 float4 per object");
        HIP_TRY(ctx, d->dn.morph_table.Grow(2 * n));
        HIP_TRY(ctx, hipMemcpyAsync(d->dn.morph_table.p, d->morph_records.data(), n * sizeof(MorphRecord), hipMemcpyHostToDevice, d->stream));
        HIP_TRY(ctx, d->dn.morph_active.Grow(d->morph_active.size() + 1));       // never empty: a table of all-zero history weights has no entry
        if (!d->morph_active.empty())
            HIP_TRY(ctx, hipMemcpyAsync(d->dn.morph_active.p, d->morph_active.data(), d->morph_active.size() * sizeof(uint2), hipMemcpyHostToDevice, d->stream));
    }
    posed = true;
    return CGPT_OK;
}

// the arguments of the temporal stage of a frame: from dn.history[temporal_slot] (when `have`) into the other slot, on filter[0].
// `carried` (PrepareMotion, PreparePoses): hits are carried back through dn.motion or dn.previous_hits, so equal camera bytes do not mean
// equal hits -- the call reprojects.
void FillTemporalArgs(const Frame& f, const cgpt_camera* camera, const cgpt_temporal_params& t, uint32_t demodulate, bool have, bool carried, TemporalArgs& a)
{
    cgpt_ctx* d = f.dev;
    const uint32_t src = d->temporal_slot, dst = src ^ 1u;
    a.guides = d->dn.guides.p; a.demod = d->dn.guide_demod.p; a.materials = d->scene.materials;
    a.hist = d->dn.history[src].p; a.hist_guides = d->dn.history_guides[src].p;
    a.hist_out = d->dn.history[dst].p; a.hist_guides_out = d->dn.history_guides[dst].p;
    a.color = d->dn.filter[0].p; a.pixels = d->dn.filter_pixels.p;
    a.width = f.width; a.n_rows = f.n_rows; a.demodulate = demodulate;
    a.drop_view_dependent = (t.flags & CGPT_TEMPORAL_KEEP_VIEW_DEPENDENT) ? 0u : 1u;
    a.n_samples = (float)f.num_accumulated; a.max_history = t.max_history; a.normal_cos_min = t.normal_cos_min; a.plane_tolerance = t.plane_tolerance;
    a.height = (float)f.height; a.first_row = (float)f.first_row;
    a.mode = kNoHistory;
    if (have) {
        if (!carried && memcmp(&d->temporal_camera, camera, sizeof(cgpt_camera)) == 0) a.mode = kSameCamera;
        else if (InvertCamera(d->temporal_camera, a.minv)) {                   // a singular camera: no history
            memcpy(a.pos_prev, d->temporal_camera.pos, sizeof(a.pos_prev));
            a.mode = kReproject;
        }
    }
}

// what a successful temporal stage leaves: the history in the other slot, and what it was stored for (`xform`: the call's snapshot
// of top_state.xform, swapped in; `poses`, `morphs`: its snapshots of the poses, likewise)
void StoreTemporalKey(cgpt_ctx* d, const cgpt_camera* camera, const uint32_t key[4], uint32_t demodulate, std::vector<float>& xform, PoseSnapshot& poses,
                      MorphSnapshot& morphs)
{
    d->temporal_slot ^= 1u;
    d->temporal_demodulate = demodulate;
    d->temporal_generation = d->scene_generation;
    d->temporal_shape_generation = d->shape_generation;
    d->temporal_xform.swap(xform);
    d->temporal_pose_generation = d->pose_generation;
    std::swap(d->temporal_poses, poses);
    d->temporal_morph_generation = d->morph_generation;
    std::swap(d->temporal_morphs, morphs);
    memcpy(&d->temporal_camera, camera, sizeof(cgpt_camera));
    memcpy(d->temporal_frame, key, sizeof(d->temporal_frame));
    d->temporal_valid = true;
}

int CheckVarianceParams(cgpt_ctx* ctx, const cgpt_variance_params& v)
{
    if (!std::isfinite(v.sigma_luminance) || !(v.sigma_luminance > 0.0f)) return CtxFail(ctx, CGPT_ERR_INVALID, "sigma_luminance must be finite and > 0, got %g", v.sigma_luminance);
    if (v.min_history_frames == 0u) return CtxFail(ctx, CGPT_ERR_INVALID, "min_history_frames must be >= 1");
    if (v.flags & ~(uint32_t)CGPT_VARIANCE_TEMPORAL) return CtxFail(ctx, CGPT_ERR_INVALID, "unknown variance flags 0x%x", v.flags);
    return CGPT_OK;
}

int EnsureVarianceBuffers(cgpt_ctx* ctx, cgpt_ctx* d, size_t n, bool temporal)
{
    if (d->dn.variance.n != n) {
        d->variance_valid = false;
        HIP_TRY(ctx, d->dn.variance.Alloc(n));
    }
    if (temporal && d->dn.moments[1].n != n) {                                 // any other size: both anew (the second one's count is the key)
        d->moments_valid = false;
        ResetAll(d->dn.moments[0], d->dn.moments[1]);
        HIP_TRY(ctx, d->dn.moments[0].Alloc(n));
        HIP_TRY(ctx, d->dn.moments[1].Alloc(n));
    }
    return CGPT_OK;
}

// what runs in front of the passes: temporal_merge; variance_estimate, with variance_pass for atrous_pass
struct Stages { bool temporal, variance; };

// temporal_merge<FINAL, MOMENTS, MOTION, POSE> for a call in which an object moved (PrepareMotion) or was re-posed (PreparePoses)
template <bool FINAL, bool MOMENTS>
decltype(&temporal_merge<FINAL, MOMENTS>) PickMerge(bool moved, bool posed)
{
    if (posed) return moved ? temporal_merge<FINAL, MOMENTS, true, true> : temporal_merge<FINAL, MOMENTS, false, true>;
    return moved ? temporal_merge<FINAL, MOMENTS, true> : temporal_merge<FINAL, MOMENTS>;
}

// One filtering call's launches: denoise_prepare, the temporal merge, the variance estimate, the passes (or, iterations = 0, an
// identity), the read-back.
//
// The validity flags, T the temporal stage and V the variance stage of the call:
//                    cleared before the first launch    set after ReadBack succeeded
//   temporal_valid   T                                  T, with the temporal key (StoreTemporalKey)
//   moments_valid    T                                  T and V: cgpt_denoise_temporal moves the colour on without the moments
//   variance_valid   V                                  V, with variance_frame
//   guides_valid     EnsureGuides' own; FilterCall clears it when this function fails
// `have` and `have_moments` are sampled before the clearing.  Ensure*Buffers clear the flag of what they reallocate.  A group's failed
// gather (FilterCall) clears temporal_valid (T) and variance_valid (V) alone.  cgpt_denoise (neither stage) touches none of the three.
int RunStages(cgpt_ctx* ctx, const Frame& f, const cgpt_camera* camera, Stages st, const cgpt_denoise_params& p, const cgpt_temporal_params& t,
              const cgpt_variance_params& v, const float4* acc, float* dst_rgba, uint32_t* dst_pixels)
{
    cgpt_ctx* d = f.dev;
    const size_t n = (size_t)f.width * f.n_rows;
    const uint32_t key[4] = { f.width, f.height, f.first_row, f.n_rows };
    const uint32_t demodulate = (p.flags & CGPT_DENOISE_DEMODULATE_ALBEDO) ? 1u : 0u;
    const uint32_t blocks = (uint32_t)((n + 255u) / 256u), tiles = Tiles(f);
    const float n_samples = (float)f.num_accumulated;
    const float inv_normal = (float)(1.0 / ((double)p.sigma_normal * p.sigma_normal));
    const float inv_position = (float)(1.0 / ((double)p.sigma_position * p.sigma_position));
    const bool follow = (t.flags & CGPT_TEMPORAL_FOLLOW_TRANSFORMS) != 0u, follow_poses = (t.flags & CGPT_TEMPORAL_FOLLOW_POSES) != 0u;
    const bool follow_morphs = (t.flags & CGPT_TEMPORAL_FOLLOW_MORPHS) != 0u;
    const bool have = st.temporal && HistoryMatches(d, key, demodulate, follow, follow_poses, follow_morphs);
    const bool have_moments = have && d->moments_valid;
    bool wrote_previous_hits = false;                                          // this call launched pose_carry_back
    std::vector<float> xform;                                                  // the matrices this call's history is stored for
    PoseSnapshot poses;                                                        // ... and the poses
    MorphSnapshot morphs;                                                      // ... those made through morph targets
    if (st.temporal) {
        try {
            xform.resize(d->top_state.xform.size());
            SnapshotPoses(d, poses);
            SnapshotMorphs(d, morphs);
        } catch (const std::exception& e) { return CtxFail(ctx, CGPT_ERR_INVALID, "out of host memory: %s", e.what()); }
        SnapshotTransforms(d->top_state.xform.data(), xform.size() / 12, xform.data());
    }
    if (st.variance) d->variance_valid = false;                                // a call that fails from here on leaves no map
    if (st.temporal) d->temporal_valid = d->moments_valid = false;             // ... and no history
    int rc;
    HIP_TRY(ctx, hipSetDevice(d->device));
    if ((rc = EnsureFilterBuffers(ctx, d, n)) != CGPT_OK) return rc;
    if (st.temporal && (rc = EnsureHistoryBuffers(ctx, d, n)) != CGPT_OK) return rc;
    if (st.variance && (rc = EnsureVarianceBuffers(ctx, d, n, st.temporal)) != CGPT_OK) return rc;
    float4* const c0 = d->dn.filter[0].p;
    uint32_t* const pixels = d->dn.filter_pixels.p;
    if (st.temporal || st.variance || p.iterations != 0) {                     // cgpt_denoise with iterations = 0 needs no guides
        if ((rc = EnsureGuides(ctx, f, camera)) != CGPT_OK) return rc;
        hipLaunchKernelGGL(denoise_prepare, dim3(blocks), dim3(256), 0, d->stream, acc, d->dn.guide_demod.p, c0, n, n_samples, demodulate);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (st.temporal) {
        bool moved = false;                                                    // an object moved since the history was stored, and the call follows it
        bool posed = false;                                                    // ... was re-posed
        bool morphed = false;                                                  // ... through morph targets: morph_carry_back carries the frame's poses back
        if (have && follow && (rc = PrepareMotion(ctx, d, moved)) != CGPT_OK) return rc;
        const bool pose_edits = follow_poses && d->pose_generation != d->temporal_pose_generation;
        const bool morph_edits = follow_morphs && d->morph_generation != d->temporal_morph_generation;
        if (have && (pose_edits || morph_edits) && (rc = PreparePoses(ctx, d, follow_morphs, posed, morphed)) != CGPT_OK) return rc;
        TemporalArgs a{};
        FillTemporalArgs(f, camera, t, demodulate, have, moved || posed, a);
        moved = moved && a.mode == kReproject;                                 // a singular history camera: no history, the existing kernel
        posed = posed && a.mode == kReproject;
        a.motion = moved ? d->dn.motion.p : nullptr;
        if (posed) {
            if (d->dn.previous_hits.n != 2 * n) HIP_TRY(ctx, d->dn.previous_hits.Alloc(2 * n));
            d->previous_hits_valid = false;                                    // overwritten from here on
            PoseArgs pa{};
            pa.guides = d->dn.guides.p; pa.tri = d->guide_tri_valid ? d->dn.guide_tri.p : nullptr; pa.table = reinterpret_cast<const PoseRecord*>(d->dn.pose_table.p);
            pa.matrices = d->dn.pose_matrices.p; pa.out = d->dn.previous_hits.p; pa.width = f.width; pa.n_rows = f.n_rows;
            if (morphed) {
                MorphCarryArgs ma{};
                ma.pose = pa; ma.morph_table = reinterpret_cast<const MorphRecord*>(d->dn.morph_table.p); ma.active = d->dn.morph_active.p;
                hipLaunchKernelGGL(morph_carry_back, dim3(tiles), dim3(256), 0, d->stream, d->scene, ma);
            } else
                hipLaunchKernelGGL(pose_carry_back, dim3(tiles), dim3(256), 0, d->stream, d->scene, pa);
            HIP_TRY(ctx, hipGetLastError());
            a.pose = d->dn.previous_hits.p;
        }
        wrote_previous_hits = posed;
        if (st.variance) {
            a.moments = d->dn.moments[d->temporal_slot].p; a.moments_out = d->dn.moments[d->temporal_slot ^ 1u].p;
            a.variance = d->dn.variance.p;
            a.have_moments = have_moments ? 1u : 0u;
            a.min_history_n = (float)v.min_history_frames * n_samples;
            hipLaunchKernelGGL((PickMerge<false, true>(moved, posed)), dim3(tiles), dim3(256), 0, d->stream, a);
        } else if (p.iterations == 0) hipLaunchKernelGGL((PickMerge<true, false>(moved, posed)), dim3(tiles), dim3(256), 0, d->stream, a);
        else hipLaunchKernelGGL((PickMerge<false, false>(moved, posed)), dim3(tiles), dim3(256), 0, d->stream, a);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (st.variance) {
        VarianceArgs a{};
        a.color = c0; a.guides = d->dn.guides.p; a.variance = d->dn.variance.p;
        a.width = f.width; a.n_rows = f.n_rows; a.have_temporal = st.temporal ? 1u : 0u;
        a.inv_normal = inv_normal; a.inv_position = inv_position;
        hipLaunchKernelGGL(variance_estimate, dim3(tiles), dim3(256), 0, d->stream, a);
        HIP_TRY(ctx, hipGetLastError());
    }
    float4* out = c0;                                                          // iterations = 0 behind the temporal stage alone: temporal_merge<true>'s, in place
    if (p.iterations == 0 && (st.variance || !st.temporal)) {                  // the unfiltered image: the accumulator's, or the merged c
        if (st.variance) out = d->dn.filter[1].p;                              // filter[0] is variance_estimate's
        if (st.temporal) hipLaunchKernelGGL(variance_identity, dim3(blocks), dim3(256), 0, d->stream, c0, d->dn.guide_demod.p, out, pixels, n, demodulate);
        else hipLaunchKernelGGL(denoise_identity, dim3(blocks), dim3(256), 0, d->stream, acc, out, pixels, n, n_samples);
        HIP_TRY(ctx, hipGetLastError());
    }
    for (uint32_t it = 0; it < p.iterations; ++it) {                           // from filter[0], ping-pong
        PassArgs a;
        a.src = d->dn.filter[it & 1u].p;
        a.dst = out = d->dn.filter[(it + 1u) & 1u].p;
        a.pixels = pixels;
        a.guides = d->dn.guides.p; a.demod = d->dn.guide_demod.p;
        a.width = f.width; a.n_rows = f.n_rows; a.step = 1u << it; a.demodulate = demodulate;
        const double sc = (double)p.sigma_color / (double)(1u << it);       // sigma_c 2^-i
        a.color_scale = st.variance ? v.sigma_luminance : (float)(1.0 / (sc * sc));
        a.inv_normal = inv_normal; a.inv_position = inv_position;
        const bool last = it + 1u == p.iterations;
        if (st.variance) hipLaunchKernelGGL((last ? variance_pass<true> : variance_pass<false>), dim3(tiles), dim3(256), 0, d->stream, VarPassArgs{ a });
        else hipLaunchKernelGGL((last ? atrous_pass<true> : atrous_pass<false>), dim3(tiles), dim3(256), 0, d->stream, a);
        HIP_TRY(ctx, hipGetLastError());
    }
    if ((rc = ReadBack(ctx, d, n, out, dst_rgba, dst_pixels)) != CGPT_OK) return rc;
    d->denoised = out; d->denoised_n = n;                                      // CGPT_TONEMAP_DENOISED
    if (st.temporal) {
        StoreTemporalKey(d, camera, key, demodulate, xform, poses, morphs);
        d->moments_valid = st.variance;
        if (wrote_previous_hits) {
            memcpy(d->previous_hits_frame, key, sizeof(key));
            d->previous_hits_valid = true;
        }
    }
    if (st.variance) {
        memcpy(d->variance_frame, key, sizeof(key));
        d->variance_valid = true;
    }
    return CGPT_OK;
}

// The three filtering calls.  Refused, in this order: no context; the frame (ResolveFrame); `params`; with want.variance
// (cgpt_denoise_variance_guided) `variance`, whose CGPT_VARIANCE_TEMPORAL then decides the temporal stage; `temporal`, read only with
// that stage; the output buffers.  A NULL parameter block is its defaults.  Then a group's frame is gathered and the stages run.
int FilterCall(cgpt_ctx* ctx, const cgpt_camera* camera, const cgpt_denoise_params* params, const cgpt_temporal_params* temporal,
               const cgpt_variance_params* variance, Stages want, float* dst_rgba, size_t n_floats, uint32_t* dst_pixels, size_t n_pixels)
{
    if (!ctx) return CGPT_ERR_INVALID;
    (ctx->group ? GroupFirstMember(ctx) : ctx)->denoised = nullptr;            // CGPT_TONEMAP_DENOISED: only a call that succeeds leaves a result
    Frame f;
    int rc = ResolveFrame(ctx, true, camera, f);
    if (rc != CGPT_OK) return rc;
    const cgpt_denoise_params p = params ? *params : kDefaults;
    if ((rc = CheckParams(ctx, p)) != CGPT_OK) return rc;
    const cgpt_variance_params v = want.variance && variance ? *variance : kVarianceDefaults;
    if (want.variance && (rc = CheckVarianceParams(ctx, v)) != CGPT_OK) return rc;
    const Stages st = { want.variance ? (v.flags & CGPT_VARIANCE_TEMPORAL) != 0u : want.temporal, want.variance };
    const cgpt_temporal_params t = st.temporal && temporal ? *temporal : kTemporalDefaults;
    if ((rc = CheckTemporalParams(ctx, t)) != CGPT_OK) return rc;
    const size_t n = (size_t)f.width * f.n_rows;
    if (!dst_rgba && !dst_pixels) return CtxFail(ctx, CGPT_ERR_INVALID, "both outputs are null");
    if (dst_rgba && n_floats != 4 * n) return CtxFail(ctx, CGPT_ERR_INVALID, "expected a buffer of %zu floats (4 per pixel)", 4 * n);
    if (dst_pixels && n_pixels != n) return CtxFail(ctx, CGPT_ERR_INVALID, "expected a buffer of %zu pixels", n);
    const float4* acc = ctx->fb.accumulator.p;
    if (ctx->group && (rc = GroupGatherUncounted(ctx, &acc)) != CGPT_OK) {
        if (st.variance) f.dev->variance_valid = false;
        if (st.temporal) f.dev->temporal_valid = false;
        return rc;
    }
    if ((rc = RunStages(ctx, f, camera, st, p, t, v, acc, dst_rgba, dst_pixels)) != CGPT_OK) f.dev->guides_valid = false;
    return rc;
}

// set the device, copy, wait: the tail of the read-outs
int CopyToHost(cgpt_ctx* ctx, cgpt_ctx* d, void* dst, const void* src, size_t bytes)
{
    HIP_TRY(ctx, hipSetDevice(d->device));
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(ctx, hipStreamSynchronize(d->stream));
    return CGPT_OK;
}

}  // namespace

void DenoiseFree(cgpt_ctx* ctx)
{
    ctx->dn = DenoiseBuffers{};
    ctx->denoised = nullptr;
    ctx->guides_valid = false;
    ctx->temporal_valid = false;
    ctx->moments_valid = false;
    ctx->variance_valid = false;
    ctx->guide_tri_valid = false;
    ctx->previous_hits_valid = false;
}

}  // namespace cgpt

using namespace cgpt;

extern "C" {

int cgpt_read_guides(cgpt_ctx* ctx, const cgpt_camera* camera, float* dst, size_t n_floats)
{
    if (!ctx) return CGPT_ERR_INVALID;
    Frame f;
    int rc = ResolveFrame(ctx, false, camera, f);
    if (rc != CGPT_OK) return rc;
    const size_t n = (size_t)f.width * f.n_rows;
    if (!dst || n_floats != 12 * n) return CtxFail(ctx, CGPT_ERR_INVALID, "expected a buffer of %zu floats (12 per pixel)", 12 * n);
    cgpt_ctx* d = f.dev;
    HIP_TRY(ctx, hipSetDevice(d->device));
    if ((rc = EnsureGuides(ctx, f, camera)) == CGPT_OK) {
        hipError_t e = hipMemcpyAsync(dst, d->dn.guides.p, n * 3 * sizeof(float4), hipMemcpyDeviceToHost, d->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
        if (e != hipSuccess) rc = CtxFail(ctx, CGPT_ERR_HIP, "cgpt_read_guides: %s", hipGetErrorString(e));
    }
    if (rc != CGPT_OK) d->guides_valid = false;
    return rc;
}

int cgpt_denoise(cgpt_ctx* ctx, const cgpt_camera* camera, const cgpt_denoise_params* params, float* dst_rgba, size_t n_floats,
                 uint32_t* dst_pixels, size_t n_pixels)
{
    return FilterCall(ctx, camera, params, nullptr, nullptr, Stages{ false, false }, dst_rgba, n_floats, dst_pixels, n_pixels);
}

int cgpt_denoise_temporal(cgpt_ctx* ctx, const cgpt_camera* camera, const cgpt_denoise_params* params, const cgpt_temporal_params* temporal,
                          float* dst_rgba, size_t n_floats, uint32_t* dst_pixels, size_t n_pixels)
{
    return FilterCall(ctx, camera, params, temporal, nullptr, Stages{ true, false }, dst_rgba, n_floats, dst_pixels, n_pixels);
}

int cgpt_denoise_variance_guided(cgpt_ctx* ctx, const cgpt_camera* camera, const cgpt_denoise_params* params, const cgpt_temporal_params* temporal,
                                 const cgpt_variance_params* variance, float* dst_rgba, size_t n_floats, uint32_t* dst_pixels, size_t n_pixels)
{
    return FilterCall(ctx, camera, params, temporal, variance, Stages{ false, true }, dst_rgba, n_floats, dst_pixels, n_pixels);   // temporal: by the flag
}

int cgpt_read_variance(cgpt_ctx* ctx, float* dst, size_t n_floats)
{
    if (!ctx) return CGPT_ERR_INVALID;
    cgpt_ctx* const first = GroupFirstMemberOrNull(ctx);
    cgpt_ctx* const d = first ? first : ctx;
    uint32_t key[4] = { ctx->width, ctx->height, ctx->band_key[0], ctx->n_rows };       // the current band
    if (ctx->group) {
        uint32_t num_accumulated, debug;
        GroupFrameInfo(ctx, &key[0], &key[1], &num_accumulated, &debug);
        key[2] = 0; key[3] = key[1];
    }
    if (!d->variance_valid || memcmp(d->variance_frame, key, sizeof(key)) != 0)
        return CtxFail(ctx, CGPT_ERR_INVALID, "no variance map: no cgpt_denoise_variance_guided call succeeded for this band");
    const size_t n = (size_t)key[0] * key[3];
    if (!dst || n_floats != n) return CtxFail(ctx, CGPT_ERR_INVALID, "expected a buffer of %zu floats (1 per pixel)", n);
    return CopyToHost(ctx, d, dst, d->dn.variance.p, n * sizeof(float));
}

int cgpt_temporal_reset(cgpt_ctx* ctx)
{
    if (!ctx) return CGPT_ERR_INVALID;
    cgpt_ctx* const first = GroupFirstMemberOrNull(ctx);
    (first ? first : ctx)->temporal_valid = false;
    return CGPT_OK;
}

int cgpt_read_temporal_history(cgpt_ctx* ctx, float* dst, size_t n_floats)
{
    if (!ctx) return CGPT_ERR_INVALID;
    cgpt_ctx* const first = GroupFirstMemberOrNull(ctx);
    cgpt_ctx* const d = first ? first : ctx;
    if (!d->temporal_valid || d->temporal_generation != d->scene_generation) return CtxFail(ctx, CGPT_ERR_INVALID, "no temporal history");
    const size_t n = (size_t)d->temporal_frame[0] * d->temporal_frame[3];
    if (!dst || n_floats != 4 * n) return CtxFail(ctx, CGPT_ERR_INVALID, "expected a buffer of %zu floats (4 per pixel)", 4 * n);
    return CopyToHost(ctx, d, dst, d->dn.history[d->temporal_slot].p, n * sizeof(float4));
}

int cgpt_read_previous_hits(cgpt_ctx* ctx, float* dst, size_t n_floats)
{
    if (!ctx) return CGPT_ERR_INVALID;
    cgpt_ctx* const first = GroupFirstMemberOrNull(ctx);
    cgpt_ctx* const d = first ? first : ctx;
    if (!d->previous_hits_valid) return CtxFail(ctx, CGPT_ERR_INVALID, "no previous hits: no temporal call with CGPT_TEMPORAL_FOLLOW_POSES or CGPT_TEMPORAL_FOLLOW_MORPHS has carried a pose back");
    const size_t n = (size_t)d->previous_hits_frame[0] * d->previous_hits_frame[3];
    if (!dst || n_floats != 8 * n) return CtxFail(ctx, CGPT_ERR_INVALID, "expected a buffer of %zu floats (8 per pixel)", 8 * n);
    return CopyToHost(ctx, d, dst, d->dn.previous_hits.p, n * sizeof(float4) * 2);
}

}  // extern "C"
