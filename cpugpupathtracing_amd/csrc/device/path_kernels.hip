// path_kernels.hip -- the render kernels (gfx950).
//
// megakernel<COUNT>: one lane = one pixel, the sample loop inside the kernel, the whole TracePathAdvanced state machine
// (ref: Source/Main.cpp:396-579) in registers.  The loop is flattened so that every iteration traces exactly ONE ray per
// lane -- an extend ray or the NEE shadow ray -- and a lane whose path ended starts its next sample in the same
// iteration, so the 64 lanes of a wave stay in the traversal loop together instead of idling at bounce boundaries.
// Replaces: Render()'s tile loop + ThreadPool::Dispatch (ref: Main.cpp:699-754).
//
// intersect_rays_kernel: IntersectScene on a ray batch (the extend step alone), for bit-exact hit-record parity tests.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ctx_internal.h"
#include "device_scene.h"
#include "launch_common.h"
#include "rt_device.hpp"
#include "shade_device.hpp"

namespace cgpt {

using namespace dev;

extern __shared__ uint32_t lds_stack[];

// BRUTE: lanes whose pixel uses the brute-force integrator (RENDER_MODE_BRUTE_FORCE, or the left half of the image in
// RENDER_MODE_COMPARISON, ref: Main.cpp:719-729) run TracePath (ref: Main.cpp:581-689) instead; its per-level operations
// live in per-lane scratch, so the plain TracePathAdvanced instantiation carries no scratch at all.
// Block shape: 256 threads = a 16x16-pixel tile (the reference's job size, ref: Main.cpp:705-711), or -- one-sample calls -- 64 threads =
// one 8x8 tile per single-wave block: the wave's slot and its LDS are free the moment its own longest path ends instead of its block's,
// and the dispatcher places single waves (1080p, one sample: 1.71 -> 1.68 ms, profiles/r03/one_sample.md).
// LEVEL: the kernel level, kernel_variant.h.  RIS: shade_device.hpp, above shade_bounce.
template <bool COUNT, bool BRUTE, int LEVEL, bool RIS>
__global__ void __launch_bounds__(256) megakernel(const DevRenderArgs args)
{
    constexpr bool TREE = ThroughTree(LEVEL);
    constexpr int LOBES = LobeOf(LEVEL);
    const DevScene& sc = args.scene;
    uint32_t* const stack = lds_stack + threadIdx.x;
    const uint32_t stride = blockDim.x;

    const bool tile8 = blockDim.x == 64u;
    const uint32_t tiles_x = tile8 ? (args.width + 7u) / 8u : (args.width + 15u) / 16u;
    const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t px = tile8 ? tx * 8u + (lane & 7u) : tx * 16u + (wave & 1u) * 8u + (lane & 7u);
    const uint32_t local_row = tile8 ? ty * 8u + (lane >> 3) : ty * 16u + (wave >> 1) * 8u + (lane >> 3);
    const bool active = px < args.width && local_row < args.n_rows;
    const uint32_t py = GlobalRow(local_row, args.band_first, args.band_h, args.band_stride);

    Counters cnt = { 0, 0, 0, 0, 0, 0 };
    double energy_sum = 0.0;

    if (active) {
        const DevSettings& st = args.settings;
        const uint32_t pixel_index = py * args.width + px;                    // global index: RNG key, same for any tiling
        const size_t local_index = (size_t)local_row * args.width + px;
        const float screen_u = (float)px * (1.0f / (float)args.width);        // ref: Main.cpp:700,713-714
        const float screen_v = (float)py * (1.0f / (float)args.height);
        float4 acc = args.accumulator[local_index];
        V3 last_color = mk(0.0f);

        uint32_t s = args.first_sample;
        const uint32_t s_end = args.first_sample + args.n_samples;

        // path state (TracePathAdvanced locals, ref: Main.cpp:398-402)
        Ray ray = make_ray(mk(0.0f), mk(0.0f), 0.0f);
        PathState ps; ps.throughput = mk(1.0f); ps.energy = mk(0.0f); ps.rng = 0; ps.depth = 0; ps.is_specular = false;
        bool need_new = true, shadow_kind = false, dead = false;
        bool same_ray = false;                                                // shade_bounce left `ray` as it was (total internal reflection, SURVEY A-3)
        Ray sray = make_ray(mk(0.0f), mk(0.0f), 0.0f);                       // pending NEE connection
        V3 pending = mk(0.0f);
        const bool use_brute = BRUTE && (st.render_mode == 1u || (st.render_mode == 0u && px < args.width / 2u));
        BruteLevel levels[BRUTE ? kMaxBruteLevels : 1u];                      // the TracePath chain: level k at [k]

        for (;;) {
            if (need_new) {
                if (s == s_end) break;
                ps.rng = pcg_seed(pixel_index, s, args.seed);
                ray = camera_ray(args.camera, screen_u, screen_v);            // no jitter: SURVEY A-14
                ps.throughput = mk(1.0f); ps.energy = mk(0.0f);
                ps.depth = 0; ps.is_specular = false; need_new = false; shadow_kind = false; dead = false; same_ray = false;
            }

            // ---- one ray per iteration: the extend ray or the pending shadow ray ----
            // The same ray again: IntersectScene accepts only t < ray.t and ray.t is this ray's closest hit, so the call returns the hit it
            // starts from.  It is counted and not walked; the counting kernels walk it, as the oracle does.
            Ray cur = shadow_kind ? sray : ray;
            if (!COUNT && same_ray && !shadow_kind) { cnt.rays++; cnt.unwalked++; }
            else intersect_scene<COUNT, HonoursTransforms(LOBES), TREE>(sc, cur, stack, stride, cnt);

            bool finalize;
            if (BRUTE && use_brute) {
                ray.t = cur.t; ray.obj = cur.obj; ray.tri = cur.tri; ray.bvh_depth = cur.bvh_depth;
                finalize = brute_level<COUNT, LOBES>(sc, st, ray, ps.rng, ps.depth, [&](uint32_t k, const BruteLevel& lv) { levels[k] = lv; },
                                                      [&](uint32_t k) { return levels[k]; }, ps.energy, cnt);
            } else if (shadow_kind) {
                if (cur.obj == kNoHit) ps.energy = ps.energy + pending;       // ref: Main.cpp:454-463
                shadow_kind = false;
                finalize = dead;
            } else {
                ray.t = cur.t; ray.obj = cur.obj; ray.tri = cur.tri; ray.bvh_depth = cur.bvh_depth;
                const uint32_t flags = shade_bounce<COUNT, LOBES, RIS>(sc, st, ray, ps, sray, pending, cnt);
                dead = (flags & kBounceTerminate) != 0;
                shadow_kind = (flags & kBounceShadow) != 0;
                same_ray = !dead && ((flags >> kBounceChainShift) & 3u) == kChainTir;
                finalize = dead && !shadow_kind;
            }

            if (finalize) {
                const V3 e = (BRUTE && use_brute) ? ps.energy : final_energy(st, ps);
                energy_sum += (double)(e.x + e.y + e.z) * 0.001;              // ref: Main.cpp:735
                if (st.debug_mode == 0u) { acc.x += e.x; acc.y += e.y; acc.z += e.z; acc.w += 1.0f; }   // ref: Main.cpp:740
                else last_color = e;
                ++s;
                need_new = true;
            }
        }

        if (args.n_samples > 0) {
            if (st.debug_mode == 0u) {                                        // ref: Main.cpp:738-746
                args.accumulator[local_index] = acc;
                const float n = (float)s_end;                                 // data.num_accumulated after these frames
                args.pixels[local_index] = vec4_to_uint(acc.x / n, acc.y / n, acc.z / n);
            } else {
                args.pixels[local_index] = vec4_to_uint(last_color.x, last_color.y, last_color.z);
            }
        }
    }

    // one atomic per wave per counter
    wave_add_u64(&args.counters->traced_rays, cnt.rays);
    wave_add_f64(&args.counters->total_energy, energy_sum);
    if (!COUNT) wave_add_u64(&args.counters->retrace_unwalked, cnt.unwalked);
    if (COUNT) {
        wave_add_u64(&args.counters->inner_steps, cnt.inner);
        wave_add_u64(&args.counters->tri_tests, cnt.tris);
        wave_add_u64(&args.counters->bvh_depth_sum, cnt.depth);
        wave_add_u64(&args.counters->closest_hits, cnt.hits);
    }
}

// host-side launcher (the ABI translation unit calls plain C++ functions, kernels stay in this one)
// threads per block, for the launch and the occupancy query alike
static uint32_t MegakernelBlockThreads(const DevRenderArgs& args)
{
    return args.n_samples == 1u ? 64u : 256u;
}

// every instantiation, [RIS][COUNT][BRUTE][LEVEL]: the lobe levels, then the same through the top-level tree
#define CGPT_MEGAKERNELS(R) \
    { { { megakernel<false, false, 0, R>, megakernel<false, false, 1, R>, megakernel<false, false, 2, R>, megakernel<false, false, 3, R>, megakernel<false, false, 4, R>, megakernel<false, false, 5, R>, megakernel<false, false, 6, R>, megakernel<false, false, 7, R>, megakernel<false, false, 8, R>, megakernel<false, false, 9, R> },     \
        { megakernel<false, true, 0, R>, megakernel<false, true, 1, R>, megakernel<false, true, 2, R>, megakernel<false, true, 3, R>, megakernel<false, true, 4, R>, megakernel<false, true, 5, R>, megakernel<false, true, 6, R>, megakernel<false, true, 7, R>, megakernel<false, true, 8, R>, megakernel<false, true, 9, R> } },         \
      { { megakernel<true, false, 0, R>, megakernel<true, false, 1, R>, megakernel<true, false, 2, R>, megakernel<true, false, 3, R>, megakernel<true, false, 4, R>, megakernel<true, false, 5, R>, megakernel<true, false, 6, R>, megakernel<true, false, 7, R>, megakernel<true, false, 8, R>, megakernel<true, false, 9, R> },         \
        { megakernel<true, true, 0, R>, megakernel<true, true, 1, R>, megakernel<true, true, 2, R>, megakernel<true, true, 3, R>, megakernel<true, true, 4, R>, megakernel<true, true, 5, R>, megakernel<true, true, 6, R>, megakernel<true, true, 7, R>, megakernel<true, true, 8, R>, megakernel<true, true, 9, R> } } }
static decltype(&megakernel<false, false, 0, false>) const kMegakernels[2][2][2][kKernelLevels] = { CGPT_MEGAKERNELS(false), CGPT_MEGAKERNELS(true) };
#undef CGPT_MEGAKERNELS

hipError_t LaunchMegakernel(const DevRenderArgs& args, ShadeVariant v, hipStream_t stream)
{
    const bool brute = args.settings.render_mode != 2u;
    const uint32_t bt = MegakernelBlockThreads(args);
    const uint32_t edge = bt == 64u ? 8u : 16u;
    const uint32_t tiles_x = (args.width + edge - 1u) / edge, tiles_y = (args.n_rows + edge - 1u) / edge;
    const dim3 grid(tiles_x * tiles_y), block(bt);
    const size_t lds = (size_t)args.scene.stack_depth * bt * sizeof(uint32_t);
    hipLaunchKernelGGL(kMegakernels[v.ris][v.count][brute][KernelLevel(v)], grid, block, lds, stream, args);
    return hipGetLastError();
}

uint32_t MegakernelWavesPerSimd(const DevRenderArgs& args, ShadeVariant v)
{
    int b = 0;
    const uint32_t bt = MegakernelBlockThreads(args);
    const size_t lds = (size_t)args.scene.stack_depth * bt * sizeof(uint32_t);
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, kMegakernels[v.ris][0][args.settings.render_mode != 2u][KernelLevel(v)], (int)bt, lds);
    return e == hipSuccess && b > 0 ? std::max(1u, (uint32_t)b * bt / 256u) : 1u;    // blocks per CU -> waves per SIMD (4 SIMDs)
}

// data.pixels from data.accumulator / data.num_accumulated (ref: Main.cpp:741), for an accumulator restored from a checkpoint
__global__ void __launch_bounds__(256) pack_pixels_kernel(const float4* __restrict__ accumulator, uint32_t* __restrict__ pixels, size_t n_pixels, float n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_pixels) {
        const float4 a = accumulator[i];
        pixels[i] = vec4_to_uint(a.x / n, a.y / n, a.z / n);
    }
}

hipError_t LaunchPackPixels(const float4* accumulator, uint32_t* pixels, size_t n_pixels, uint32_t num_accumulated, hipStream_t stream)
{
    if (n_pixels == 0 || num_accumulated == 0) return hipSuccess;             // nothing accumulated: pixels stay as they are
    hipLaunchKernelGGL(pack_pixels_kernel, dim3((uint32_t)((n_pixels + 255u) / 256u)), dim3(256), 0, stream, accumulator, pixels, n_pixels, (float)num_accumulated);
    return hipGetLastError();
}

// IntersectScene on a batch of rays (ref: Main.cpp:299-316).  XFORM: the scene has a transformed object (rt_device.hpp: intersect_scene);
// the rays and the returned t are the world's either way
template <bool XFORM, bool TREE = false>
__global__ void __launch_bounds__(256) intersect_rays_kernel(const DevScene sc, const float* __restrict__ origins,
                                                             const float* __restrict__ dirs, const float* __restrict__ tmax,
                                                             uint32_t n, float* __restrict__ out_t, uint32_t* __restrict__ out_obj,
                                                             uint32_t* __restrict__ out_tri, uint32_t* __restrict__ out_depth,
                                                             DevCounters* counters)
{
    uint32_t* const stack = lds_stack + threadIdx.x;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    Counters cnt = { 0, 0, 0, 0, 0, 0 };
    if (i < n) {
        Ray ray = make_ray(mk(origins + 3 * (size_t)i), mk(dirs + 3 * (size_t)i), tmax ? tmax[i] : 1e34f);
        intersect_scene<true, XFORM, TREE>(sc, ray, stack, blockDim.x, cnt);
        out_t[i] = ray.t; out_obj[i] = ray.obj; out_tri[i] = ray.tri; out_depth[i] = ray.bvh_depth;
    }
    wave_add_u64(&counters->traced_rays, cnt.rays);
    wave_add_u64(&counters->inner_steps, cnt.inner);
    wave_add_u64(&counters->tri_tests, cnt.tris);
    wave_add_u64(&counters->bvh_depth_sum, cnt.depth);
}

hipError_t LaunchIntersectRays(const cgpt_ctx* ctx, const float* origins, const float* dirs, const float* tmax, uint32_t n, float* out_t,
                               uint32_t* out_obj, uint32_t* out_tri, uint32_t* out_depth)
{
    const size_t lds = (size_t)ctx->scene.stack_depth * 256 * sizeof(uint32_t);
    // a chain of this shape and no table: the order in which the three are first named is their order in the code object, which stays as it was
    const int level = ChooseIntersectLevel(ctx);
    const auto kernel = level == 2 ? intersect_rays_kernel<true, true> : (level == 1 ? intersect_rays_kernel<true> : intersect_rays_kernel<false>);
    hipLaunchKernelGGL(kernel, dim3((n + 255u) / 256u), dim3(256), lds, ctx->stream, ctx->scene, origins, dirs, tmax, n, out_t, out_obj,
                       out_tri, out_depth, ctx->counters.p);
    return hipGetLastError();
}

}  // namespace cgpt
