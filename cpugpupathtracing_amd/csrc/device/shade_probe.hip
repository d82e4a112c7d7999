// shade_probe.hip -- cgpt_shade_samples: shade_bounce on samples the host supplies (gfx950), the shade step's counterpart of
// cgpt_intersect_rays.  One thread loads one sample, calls shade_bounce<false, LOBES, RIS> once and stores what it left; nothing is traced.
// LOBES and RIS come from the function that chooses them for a render (ctx_internal.h: ChooseVariant), so the code a sample runs through is
// the code a render of this context inlines into its kernels.  tests/shade_ref.py states the bounce in numpy and is what the results are compared with.
#include <hip/hip_runtime.h>

#include <cmath>

#include "cpugpupt_abi.h"
#include "ctx_internal.h"
#include "device_scene.h"
#include "rt_device.hpp"
#include "shade_device.hpp"

namespace cgpt {

using namespace dev;

namespace {

constexpr uint32_t kMaxSamples = 65536;

static_assert(sizeof(cgpt_shade_sample) == 64 && sizeof(cgpt_shade_result) == 112, "the sample records are 16 and 28 words");

template <int LOBES, bool RIS>
__global__ void __launch_bounds__(256) shade_samples_kernel(const DevScene sc, const DevSettings st, const cgpt_shade_sample* __restrict__ samples,
                                                            uint32_t n, cgpt_shade_result* __restrict__ results)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const cgpt_shade_sample s = samples[i];
    Ray ray = make_ray(mk(s.o), mk(s.d), s.t);
    ray.obj = s.obj; ray.tri = s.tri; ray.bvh_depth = s.bvh_depth;
    PathState ps;
    ps.throughput = mk(s.throughput); ps.energy = mk(0.0f); ps.rng = s.rng; ps.depth = s.depth; ps.is_specular = s.is_specular != 0u;
    Ray shadow = make_ray(mk(0.0f), mk(0.0f), 0.0f);
    V3 pending = mk(0.0f);
    Counters cnt = { 0, 0, 0, 0, 0, 0 };
    const uint32_t flags = shade_bounce<false, LOBES, RIS>(sc, st, ray, ps, shadow, pending, cnt);
    if (!(flags & kBounceShadow)) { shadow = make_ray(mk(0.0f), mk(0.0f), 0.0f); pending = mk(0.0f); }
    cgpt_shade_result r;
    r.flags = flags;
    r.o[0] = ray.o.x; r.o[1] = ray.o.y; r.o[2] = ray.o.z; r.d[0] = ray.d.x; r.d[1] = ray.d.y; r.d[2] = ray.d.z;
    r.throughput[0] = ps.throughput.x; r.throughput[1] = ps.throughput.y; r.throughput[2] = ps.throughput.z;
    r.energy[0] = ps.energy.x; r.energy[1] = ps.energy.y; r.energy[2] = ps.energy.z;
    r.rng = ps.rng; r.depth = ps.depth; r.is_specular = ps.is_specular ? 1u : 0u;
    r.shadow_o[0] = shadow.o.x; r.shadow_o[1] = shadow.o.y; r.shadow_o[2] = shadow.o.z;
    r.shadow_d[0] = shadow.d.x; r.shadow_d[1] = shadow.d.y; r.shadow_d[2] = shadow.d.z;
    r.shadow_tmax = shadow.t;
    r.pending[0] = pending.x; r.pending[1] = pending.y; r.pending[2] = pending.z;
    r.unwalked = cnt.unwalked; r.reserved = 0u;
    results[i] = r;
}

// [RIS][lobe level]
#define CGPT_SHADE_PROBES(R) { shade_samples_kernel<0, R>, shade_samples_kernel<1, R>, shade_samples_kernel<2, R>, shade_samples_kernel<3, R>, shade_samples_kernel<4, R> }
decltype(&shade_samples_kernel<0, false>) const kShadeProbes[2][kLobeLevels] = { CGPT_SHADE_PROBES(false), CGPT_SHADE_PROBES(true) };
#undef CGPT_SHADE_PROBES

bool Finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

}  // namespace
}  // namespace cgpt

using namespace cgpt;

extern "C" int cgpt_shade_samples(cgpt_ctx* ctx, const cgpt_settings* settings, const cgpt_shade_sample* samples, uint32_t n, cgpt_shade_result* results)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return GroupForwarded(ctx, cgpt_shade_samples(GroupFirstMember(ctx), settings, samples, n, results));
    if (!ctx->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "cgpt_shade_samples before cgpt_scene_upload");
    if (!settings || !samples || !results) return CtxFail(ctx, CGPT_ERR_INVALID, "null argument");
    if (n == 0 || n > kMaxSamples) return CtxFail(ctx, CGPT_ERR_INVALID, "%u samples outside [1, %u]", n, kMaxSamples);
    DevSettings st{};
    const int rc = TranslateSettings(ctx, *settings, st);
    if (rc != CGPT_OK) return rc;
    // the kernel indexes objects[], the triangle records and (through objects[].mat_index, checked at upload) materials[] with these numbers
    for (uint32_t i = 0; i < n; ++i) {
        const cgpt_shade_sample& s = samples[i];
        if (s.depth > 255u) return CtxFail(ctx, CGPT_ERR_INVALID, "sample %u: depth %u above 255", i, s.depth);
        if (s.obj == kNoHit) continue;
        if (s.obj >= ctx->h_objects.size()) return CtxFail(ctx, CGPT_ERR_INVALID, "sample %u: object %u of %zu", i, s.obj, ctx->h_objects.size());
        const DevObject& obj = ctx->h_objects[s.obj];
        if (obj.kind == CGPT_OBJECT_MESH && s.tri >= obj.n_tris) return CtxFail(ctx, CGPT_ERR_INVALID, "sample %u: triangle %u of a mesh of %u", i, s.tri, obj.n_tris);
        if (!std::isfinite(s.t) || !Finite3(s.o) || !Finite3(s.d) || !Finite3(s.throughput))
            return CtxFail(ctx, CGPT_ERR_INVALID, "sample %u: t, o, d or throughput of a hit is not finite", i);
    }

    st.render_mode = CGPT_MODE_ADVANCED;                                       // the probe is shade_bounce, whatever the mode: RIS as an ADVANCED render has it
    const ShadeVariant v = ChooseVariant(ctx, st, 0u);

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf<cgpt_shade_sample> d_in;
    DevBuf<cgpt_shade_result> d_out;
    HIP_TRY(ctx, d_in.Alloc(n)); HIP_TRY(ctx, d_out.Alloc(n));
    HIP_TRY(ctx, hipMemcpyAsync(d_in.p, samples, sizeof(cgpt_shade_sample) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(kShadeProbes[v.ris][v.lobe_level], dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->scene, st, d_in.p, n, d_out.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(results, d_out.p, sizeof(cgpt_shade_result) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CGPT_OK;
}
