// accumulate.hpp -- the accumulate + pack step shared by the wavefront pipeline and the persistent kernel (gfx950):
// adds the finished paths' radiance of one batch to the float4 accumulator IN SAMPLE ORDER (the reference adds one sample per
// Render(), ref: Source/Main.cpp:735-746; float addition is not associative, so the order is part of the result) and packs
// data.pixels (ref: Include/MathLib.h:144-152).
#pragma once
#include <hip/hip_runtime.h>

#include "device_scene.h"
#include "rt_device.hpp"
#include "shade_device.hpp"
#include "trace_steps.hpp"

namespace cgpt {
namespace dev {

static constexpr uint32_t kAccChunk = 8;                 // samples staged per pixel and pass in the pixel-major path

// A pixel whose primary ray left the scene gives every one of its paths the record {0, 0, 0, bits(depth 0)} (shade_bounce returns on
// a miss before it draws a number, ref: Main.cpp:415-416).  In the wavefront pipeline that record is not stored and not loaded: where this
// predicate holds, round 0 of wf_shade writes nothing to st_en for the pixel's paths and accumulate_batch<true> feeds add_sample the
// record itself, once per sample.  Both evaluate it on the same operands -- the launch arguments of the batch and the pixel's
// px_hit record, which the batch's own round-0 trace wrote before either kernel starts -- so the writer and the reader always agree
// (DESIGN.md 5.1).  False for the debug views (the ray-depth view reads the stored depth, the BVH-depth view colours the misses) and for
// TracePath pixels (they run brute_level).
__device__ __forceinline__ bool pixel_adds_nothing(const DevRenderArgs& args, float4 first_hit, uint32_t px)
{
    const DevSettings& st = args.settings;
    const bool trace_path = st.render_mode == 1u || (st.render_mode == 0u && px < args.width / 2u);   // ref: Main.cpp:719-729
    return __float_as_uint(first_hit.x) == kNoHit && st.debug_mode == 0u && !trace_path;
}

// All 256 threads of the block call it (ends in a block-level reduction).  One thread = one pixel, grid-stride over the band.
// st_en[path id] = {radiance.xyz, bits(final ray depth)}.  With pixel-major path ids a pixel's samples are one contiguous run: read
// directly, the 64 lanes of a wave would touch 64 different lines per load (measured: 9.3 ms instead of 1.3 per 256-spp frame),
// so the wave loads 64 pixels x kAccChunk samples in memory order (eight full 128-byte lines per load instruction) into LDS and
// every lane then reads its own pixel's samples from there, in order.
// SKIP (the wavefront pipeline): px_hit holds the band's first-hit records and the samples of a pixel that adds nothing are not read.
template <bool SKIP = false>
__device__ __forceinline__ void accumulate_batch(const DevRenderArgs& args, const float4* __restrict__ st_en, const PathGrid& g,
                                                 uint32_t batch_first, uint32_t batch_n, const float4* __restrict__ px_hit = nullptr)
{
    __shared__ float4 stage[4][64 * (kAccChunk + 1u)];                         // per wave: [pixel][sample], one float4 of padding per pixel
    const DevSettings& st = args.settings;
    const uint32_t lane = threadIdx.x & 63u;
    float4* const my_stage = stage[threadIdx.x >> 6];
    double energy_sum = 0.0;
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < g.n_pixels; p += gridDim.x * 256u) {     // grid-stride: a bounded number of blocks
        uint32_t px = 0, py = 0, local_row = 0;
        const bool is_pixel = pixel_of_index(args, g, p, px, py, local_row);
        const size_t local_index = (size_t)local_row * args.width + px;
        const bool brute = st.render_mode == 1u || (st.render_mode == 0u && px < args.width / 2u);   // TracePath has no ray-depth view (ref: Main.cpp:581-689)
        float4 acc = is_pixel ? args.accumulator[local_index] : float4{ 0.0f, 0.0f, 0.0f, 0.0f };
        V3 last = mk(0.0f);
        auto add_sample = [&](float4 e4) {
            PathState ps;
            ps.energy = mk(e4.x, e4.y, e4.z);
            ps.depth = __float_as_uint(e4.w) & 0xFFu;
            const V3 e = brute ? ps.energy : final_energy(st, ps);
            energy_sum += (double)(e.x + e.y + e.z) * 0.001;                  // ref: Main.cpp:735
            if (st.debug_mode == 0u) { acc.x += e.x; acc.y += e.y; acc.z += e.z; acc.w += 1.0f; }
            else last = e;
        };
        bool nothing = false;                                                 // SKIP: this pixel's samples are the zero record, unread
        if (SKIP && is_pixel) nothing = pixel_adds_nothing(args, px_hit[p], px);
        const float4 zero_record = float4{ 0.0f, 0.0f, 0.0f, __uint_as_float(0u) };   // {no energy, depth 0}
        if (g.order == kPixelMajor) {
            const uint32_t p_base = p - lane;                                 // the wave's 64 pixels: one 8x8 tile
            const unsigned long long unread = SKIP ? __builtin_amdgcn_ballot_w64(nothing) : 0ull;   // bit i: pixel p_base + i (the whole wave is in the loop)
            for (uint32_t s0 = 0; s0 < batch_n; s0 += kAccChunk) {
                const uint32_t cnt = min(kAccChunk, batch_n - s0);
#pragma unroll
                for (uint32_t k = 0; k < kAccChunk; ++k) {
                    const uint32_t e = k * 64u + lane, pix = e / kAccChunk, smp = e % kAccChunk;
                    if (smp < cnt && !(SKIP && ((unread >> pix) & 1ull))) my_stage[pix * (kAccChunk + 1u) + smp] = st_en[(size_t)(p_base + pix) * g.n_samples + s0 + smp];
                }
                __builtin_amdgcn_wave_barrier();
                if (is_pixel)
                    for (uint32_t j = 0; j < cnt; ++j) add_sample(SKIP && nothing ? zero_record : my_stage[lane * (kAccChunk + 1u) + j]);   // (its staged entries are stale)
                __builtin_amdgcn_wave_barrier();
            }
        } else if (is_pixel) {
            for (uint32_t s = 0; s < batch_n; ++s) add_sample(SKIP && nothing ? zero_record : ld_stream(&st_en[path_id(g, s, p)]));
        }
        if (is_pixel) {
            if (st.debug_mode == 0u) {
                args.accumulator[local_index] = acc;
                const float n = (float)(batch_first + batch_n);               // data.num_accumulated after this batch
                args.pixels[local_index] = vec4_to_uint(acc.x / n, acc.y / n, acc.z / n);
            } else {
                args.pixels[local_index] = vec4_to_uint(last.x, last.y, last.z);
            }
        }
    }
    block_add_f64(&args.counters->total_energy, energy_sum);
}

}  // namespace dev
}  // namespace cgpt
