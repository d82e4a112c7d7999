// cgpt_abi.hip -- implementation of the C ABI in include/cpugpupt_abi.h on HIP (gfx950).
// Context management, the upload of a laid-out scene (scene_layout.h -> device_scene.h), kernel launches, statistics.
// There is no CPU fallback anywhere in this file: without a gfx950 device every entry point fails loudly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "cpugpupt_abi.h"
#include "device_scene.h"
#include "launch_common.h"
#include "scene_layout.h"

namespace cgpt {
hipError_t LaunchMegakernel(const DevRenderArgs& args, ShadeVariant v, hipStream_t stream);                                  // path_kernels.hip
hipError_t LaunchIntersectRays(const struct ::cgpt_ctx* ctx, const float* origins, const float* dirs, const float* tmax, uint32_t n, float* out_t,
                               uint32_t* out_obj, uint32_t* out_tri, uint32_t* out_depth);
int LaunchWavefront(struct ::cgpt_ctx* ctx, const DevRenderArgs& args, ShadeVariant v);                                     // wavefront_kernels.hip
void WavefrontFree(void* state);
void WavefrontCollectTiming(void* state, double* trace_ms, uint32_t* trace_launches, double* round0_ms, uint32_t* round0_launches);
int WavefrontSetTuning(struct ::cgpt_ctx* ctx, const char* name, uint32_t value);
uint32_t WavefrontTraceWavesPerSimd(void* state);
int LaunchPersistent(struct ::cgpt_ctx* ctx, const DevRenderArgs& args, ShadeVariant v);                                    // persistent_kernel.hip
void PersistentFree(void* state);
void PersistentCollectTiming(void* state, ShadeVariant v, double* ms, uint32_t* launches, uint32_t* waves_per_simd);
int PersistentSetTuning(struct ::cgpt_ctx* ctx, const char* name, uint32_t value, bool* known);
uint32_t MegakernelWavesPerSimd(const DevRenderArgs& args, ShadeVariant v);                                                  // path_kernels.hip
}  // namespace cgpt

using namespace cgpt;

namespace {
std::string g_create_error = "";
}

#include "ctx_internal.h"

namespace cgpt {
// accessors for the other translation units
hipStream_t CtxStream(cgpt_ctx* ctx) { return ctx->stream; }
int CtxDevice(cgpt_ctx* ctx) { return ctx->device; }
void** CtxWavefrontSlot(cgpt_ctx* ctx) { return &ctx->wavefront_state; }
void** CtxPersistentSlot(cgpt_ctx* ctx) { return &ctx->persistent_state; }
// the launchers of the multi-launch kernels record the render's start event themselves, after their one-time host setup
// (allocations, occupancy queries), so that cgpt_stats.kernel_ms of a first call is device time
hipEvent_t CtxStartEvent(cgpt_ctx* ctx) { return ctx->ev_start.e; }
int CtxFail(cgpt_ctx* ctx, int code, const char* fmt, ...)                   // ctx null: cgpt_ctx_create failed, and there is no context to hold the text
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    if (ctx) ctx->error = buf; else g_create_error = buf;
    return code;
}
}  // namespace cgpt

namespace {

template <typename T>
int UploadArray(cgpt_ctx* ctx, DevBuf<T>& dst, const std::vector<T>& src)   // an empty vector still gets one element: no kernel argument is null
{
    HIP_TRY(ctx, dst.Alloc(src.empty() ? 1 : src.size()));
    if (!src.empty()) HIP_TRY(ctx, hipMemcpy(dst.p, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
    return CGPT_OK;
}

void FreeScene(cgpt_ctx* ctx)
{
    ctx->sb = SceneBuffers{};
    ctx->skins.clear(); ctx->pose_stamp.clear();                               // an upload drops every skin
    ctx->morphs.clear(); ctx->morph_stamp.clear();                             // ... and every object's morph targets
    ctx->h_objects.clear(); ctx->refit_objects.clear(); ctx->record_perm.clear(); ctx->mesh_group.clear();
    ctx->footprint = cgpt_scene_footprint{};
    ctx->h_roughness.clear(); ctx->h_transmission_roughness.clear(); ctx->h_materials.clear(); ctx->h_lights.clear();
    ctx->features = SceneFeatures{};
    ctx->top_state = TopLevelState{};
    ctx->has_scene = false;
}

void FreeFramebuffer(cgpt_ctx* ctx) { ctx->fb = FrameBuffers{}; ctx->denoised = nullptr; }   // ... and no denoised result of the old frame (CGPT_TONEMAP_DENOISED)

int EnsureFramebuffer(cgpt_ctx* ctx, uint32_t W, uint32_t H, uint32_t n_rows, const uint32_t key[5])
{
    if (ctx->fb.accumulator.p && ctx->width == W && ctx->height == H && memcmp(ctx->band_key, key, sizeof(ctx->band_key)) == 0) return CGPT_OK;
    FreeFramebuffer(ctx);
    const size_t n = (size_t)W * n_rows;
    HIP_TRY(ctx, ctx->fb.accumulator.Alloc(n));
    HIP_TRY(ctx, ctx->fb.pixels.Alloc(n));
    HIP_TRY(ctx, hipMemsetAsync(ctx->fb.accumulator.p, 0, n * sizeof(float4), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->fb.pixels.p, 0, n * sizeof(uint32_t), ctx->stream));
    ctx->width = W; ctx->height = H; ctx->n_rows = n_rows; memcpy(ctx->band_key, key, sizeof(ctx->band_key));
    ctx->num_accumulated = 0;
    return CGPT_OK;
}

// rows of a context: a contiguous band, or interleaved bands of interleave_rows rows (multi-GPU load balance)
struct Band { uint32_t n_rows, first, h, stride; uint32_t key[5]; };
int ResolveBand(cgpt_ctx* ctx, const cgpt_render_params& p, Band& b)
{
    if (p.width == 0 || p.height == 0 || p.row_begin >= p.row_end || p.row_end > p.height)
        return CtxFail(ctx, CGPT_ERR_INVALID, "bad framebuffer/rows: %ux%u rows [%u,%u)", p.width, p.height, p.row_begin, p.row_end);
    if ((uint64_t)p.width * p.height > 0xFFFFFFFFull) return CtxFail(ctx, CGPT_ERR_INVALID, "framebuffer too large");
    if (p.interleave_rows == 0 && p.interleave_count == 0) {
        b.n_rows = p.row_end - p.row_begin; b.first = p.row_begin; b.h = b.n_rows; b.stride = 0;
    } else {
        const uint32_t h = p.interleave_rows, R = p.interleave_count, r = p.interleave_index;
        if (h == 0 || R == 0 || r >= R || p.row_begin != 0 || p.row_end != p.height)
            return CtxFail(ctx, CGPT_ERR_INVALID, "bad interleave: rows %u count %u index %u (row_begin/row_end must be 0/height)", h, R, r);
        b.first = r * h; b.h = h; b.stride = R * h;
        b.n_rows = 0;
        for (uint64_t first = b.first; first < p.height; first += b.stride) b.n_rows += std::min<uint32_t>(h, p.height - (uint32_t)first);
        if (b.n_rows == 0) return CtxFail(ctx, CGPT_ERR_INVALID, "interleave index %u owns no rows of a %u-row image", r, p.height);
    }
    const uint32_t key[5] = { p.row_begin, p.row_end, p.interleave_rows, p.interleave_count, p.interleave_index };
    memcpy(b.key, key, sizeof(key));
    return CGPT_OK;
}

// cgpt_scene_update_roughness (transmission false: PackMaterial's alpha, materials[4i+3].z) and cgpt_scene_update_transmission_roughness
// (true: alpha_t, .w) of a one-device context.  Everything is refused before the device write; the other lobe's values are kept.
int UpdateRoughnessWord(cgpt_ctx* ctx, const float* roughness, uint32_t n_materials, bool transmission)
{
    const char* const what = transmission ? "transmission roughness" : "roughness";
    if (!ctx->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "no scene uploaded");
    if (!roughness || n_materials != ctx->n_materials) return CtxFail(ctx, CGPT_ERR_INVALID, "expected %u %s values", ctx->n_materials, what);
    for (uint32_t i = 0; i < n_materials; ++i)
        if (!(roughness[i] >= 0.0f && roughness[i] <= 1.0f)) return CtxFail(ctx, CGPT_ERR_INVALID, "material %u: %s %g outside [0, 1]", i, what, (double)roughness[i]);
    std::vector<float4> mats;
    std::vector<float> values;
    try { mats = ctx->h_materials; values.assign(roughness, roughness + n_materials); } catch (const std::exception& e) { return CtxFail(ctx, CGPT_ERR_INVALID, "out of host memory: %s", e.what()); }
    for (uint32_t i = 0; i < n_materials; ++i) (transmission ? mats[4 * (size_t)i + 3].w : mats[4 * (size_t)i + 3].z) = roughness[i] * roughness[i];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // first hits and albedo do not depend on either roughness: the denoiser's guides stay valid (scene_generation is left as it is)
    const hipError_t e = hipMemcpy(ctx->sb.materials.p, mats.data(), mats.size() * sizeof(float4), hipMemcpyHostToDevice);
    if (e != hipSuccess) {                                                     // the records may be half written: drop the scene (refit.hip: SceneLost)
        ctx->has_scene = false;
        return CtxFail(ctx, CGPT_ERR_HIP, "hipMemcpy of the material records failed: %s (the device scene is dropped; upload it again)", hipGetErrorString(e));
    }
    ctx->h_materials.swap(mats);
    (transmission ? ctx->features.rough_dielectric : ctx->features.rough_specular) = std::any_of(values.begin(), values.end(), [](float v) { return v > 0.0f; });
    (transmission ? ctx->h_transmission_roughness : ctx->h_roughness).swap(values);
    return CGPT_OK;
}

// cgpt_scene_update_smooth_normals of a one-device context: DevObject.smooth of every object.  Everything is refused before the device write.
int UpdateSmoothNormals(cgpt_ctx* ctx, const uint32_t* smooth, uint32_t n_objects)
{
    if (!ctx->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "no scene uploaded");
    if (!smooth || n_objects != ctx->h_objects.size()) return CtxFail(ctx, CGPT_ERR_INVALID, "expected %zu smooth-normal flags", ctx->h_objects.size());
    bool any = false;
    for (uint32_t i = 0; i < n_objects; ++i) {
        if (smooth[i] > 1u) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u: smooth-normal flag %u is neither 0 nor 1", i, smooth[i]);
        any = any || smooth[i] != 0u;
    }
    for (const uint32_t li : ctx->h_lights)
        if (smooth[li] != 0u) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u is a light: its sampled normal is v0.normal, so it cannot shade with smooth normals", li);
    std::vector<DevObject> objects;
    try { objects = ctx->h_objects; } catch (const std::exception& e) { return CtxFail(ctx, CGPT_ERR_INVALID, "out of host memory: %s", e.what()); }
    for (uint32_t i = 0; i < n_objects; ++i) objects[i].smooth = smooth[i];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->scene_generation++; ctx->shape_generation++;                          // the denoiser's guides hold the normal (denoise.hip)
    const hipError_t e = hipMemcpy(ctx->sb.objects.p, objects.data(), objects.size() * sizeof(DevObject), hipMemcpyHostToDevice);
    if (e != hipSuccess) {                                                     // the records may be half written: drop the scene (refit.hip: SceneLost)
        ctx->has_scene = false;
        return CtxFail(ctx, CGPT_ERR_HIP, "hipMemcpy of the object records failed: %s (the device scene is dropped; upload it again)", hipGetErrorString(e));
    }
    ctx->h_objects.swap(objects);
    ctx->features.smooth_normals = any;
    return CGPT_OK;
}

// cgpt_scene_update_transforms of a one-device context: the flag in every object's obj_trace record and the transform records behind them,
// one write.  Everything is refused before it (scene_layout.h: LayoutTransforms).
int UpdateTransforms(cgpt_ctx* ctx, const float* object_to_world, uint32_t n_objects)
{
    if (!ctx->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "no scene uploaded");
    std::vector<float4> trace;                                                 // obj_trace's 2 n records, then the 3 n transform records, then (mode 1) the tree
    bool any = false;
    TopLevelState top;
    const int rc = Guarded(ctx, "transform update", [&] {
        std::vector<float4> records;
        std::vector<uint32_t> flags;
        const int rl = LayoutTransforms(object_to_world, n_objects, ctx->h_objects, ctx->h_lights, records, flags, ctx->error);
        if (rl != CGPT_OK) return rl;
        trace.resize(5 * (size_t)n_objects);
        for (uint32_t i = 0; i < n_objects; ++i) {
            any = any || flags[i] != 0u;
            PackObjTrace(ctx->h_objects[i], trace[2 * (size_t)i], trace[2 * (size_t)i + 1], flags[i]);
        }
        std::copy(records.begin(), records.end(), trace.begin() + 2 * (size_t)n_objects);
        top = ctx->top_state;                                                  // the boxes follow the matrices (in mode 0 too: the mode may be turned on later)
        top.xform.assign(object_to_world, object_to_world + 12 * (size_t)n_objects);
        if (ctx->top_level) {                                                  // still one copy: the tree sits right behind
            const std::vector<float4> tree = PackTopLevel(ctx->h_objects, top);
            trace.insert(trace.end(), tree.begin(), tree.end());
        }
        return (int)CGPT_OK;
    });
    if (rc != CGPT_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->scene_generation++;                                                   // the denoiser's guides hold position and normal (denoise.hip); shape_generation
                                                                               // stays: a temporal call may follow the matrices (CGPT_TEMPORAL_FOLLOW_TRANSFORMS)
    const hipError_t e = trace.empty() ? hipSuccess : hipMemcpy(ctx->sb.obj_trace.p, trace.data(), trace.size() * sizeof(float4), hipMemcpyHostToDevice);
    if (e != hipSuccess) {                                                     // the records may be half written: drop the scene (refit.hip: SceneLost)
        ctx->has_scene = false;
        return CtxFail(ctx, CGPT_ERR_HIP, "hipMemcpy of the transform records failed: %s (the device scene is dropped; upload it again)", hipGetErrorString(e));
    }
    ctx->features.transforms = any;
    ctx->top_state.xform.swap(top.xform);
    return CGPT_OK;
}

}  // namespace

namespace cgpt {
hipError_t WriteTopLevel(cgpt_ctx* ctx, const std::vector<DevObject>& objects, const TopLevelState& st)
{
    if (!ctx->top_level || objects.empty()) return hipSuccess;
    const std::vector<float4> tree = PackTopLevel(objects, st);
    return hipMemcpy(ctx->sb.obj_trace.p + 5 * objects.size(), tree.data(), tree.size() * sizeof(float4), hipMemcpyHostToDevice);
}
}  // namespace cgpt

extern "C" {

uint32_t cgpt_abi_version(void) { return CGPT_ABI_VERSION; }

const char* cgpt_last_error(const cgpt_ctx* ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

int cgpt_ctx_create(const int* device_ids, int n_devices, uint32_t flags, cgpt_ctx** out)
{
    if (!out) return CtxFail(nullptr, CGPT_ERR_INVALID, "out is null");
    *out = nullptr;
    if (n_devices < 1 || n_devices > 8) return CtxFail(nullptr, CGPT_ERR_INVALID, "n_devices %d outside [1, 8] (one node)", n_devices);
    if (n_devices > 1 || (flags & CGPT_CTX_FORCE_COLLECTIVE)) {
        return Guarded(nullptr, "cgpt_ctx_create", [&] { return GroupCreate(device_ids, n_devices, flags, out); });
    }
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
        return CtxFail(nullptr, CGPT_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU path", e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    const int dev = device_ids ? device_ids[0] : 0;
    if (dev < 0 || dev >= count) return CtxFail(nullptr, CGPT_ERR_INVALID, "device id %d out of range (%d devices)", dev, count);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, dev)) != hipSuccess) return CtxFail(nullptr, CGPT_ERR_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return CtxFail(nullptr, CGPT_ERR_NO_DEVICE, "device %d is %s; the kernels are built for gfx950 (MI355X) only", dev, prop.gcnArchName);

    cgpt_ctx* ctx = new (std::nothrow) cgpt_ctx;
    if (!ctx) return CtxFail(nullptr, CGPT_ERR_INVALID, "out of host memory");
    ctx->device = dev;
    if ((e = hipSetDevice(dev)) != hipSuccess || (e = ctx->own_stream.Create(hipStreamNonBlocking)) != hipSuccess ||
        (e = ctx->ev_start.Create()) != hipSuccess || (e = ctx->ev_stop.Create()) != hipSuccess ||
        (e = ctx->counters.Alloc(1)) != hipSuccess ||
        (e = hipMemset(ctx->counters.p, 0, sizeof(DevCounters))) != hipSuccess) {
        delete ctx;                                                            // gives back whatever the earlier steps created
        return CtxFail(nullptr, CGPT_ERR_HIP, "context setup failed: %s", hipGetErrorString(e));
    }
    ctx->stream = ctx->own_stream.s;
    *out = ctx;
    return CGPT_OK;
}

int cgpt_ctx_destroy(cgpt_ctx* ctx)
{
    if (!ctx) return CGPT_OK;
    if (ctx->group) { GroupDestroy(ctx); delete ctx; return CGPT_OK; }
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    FreeScene(ctx);
    FreeFramebuffer(ctx);
    ctx->counters.Reset();
    WavefrontFree(ctx->wavefront_state);
    PersistentFree(ctx->persistent_state);
    DenoiseFree(ctx);
    delete ctx;                                                                // the events, then the stream
    return CGPT_OK;
}

int cgpt_set_stream(cgpt_ctx* ctx, void* hip_stream)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return CtxFail(ctx, CGPT_ERR_UNSUPPORTED, "cgpt_set_stream: a multi-device context owns its streams");
    // the renders fork onto pool streams and join back through event waits on this stream: that needs a stream object
    if ((hipStream_t)hip_stream == hipStreamLegacy || (hipStream_t)hip_stream == hipStreamPerThread)
        return CtxFail(ctx, CGPT_ERR_UNSUPPORTED, "cgpt_set_stream: %s names a default stream; use a non-default stream (hipStreamCreate)",
                       (hipStream_t)hip_stream == hipStreamLegacy ? "hipStreamLegacy" : "hipStreamPerThread");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream.s;
    return CGPT_OK;
}

int cgpt_set_nee_candidates(cgpt_ctx* ctx, uint32_t candidates)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (candidates < 1u || candidates > 32u) return CtxFail(ctx, CGPT_ERR_INVALID, "nee candidates %u outside [1, 32]", candidates);
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupSetNeeCandidates(ctx, candidates); });
    ctx->nee_candidates = candidates;                                          // read by the next render; first hits do not depend on it: the guides stay
    return CGPT_OK;
}

int cgpt_set_top_level(cgpt_ctx* ctx, uint32_t mode)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (mode > 1u) return CtxFail(ctx, CGPT_ERR_INVALID, "top-level mode %u is neither 0 (object list) nor 1 (tree)", mode);
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupSetTopLevel(ctx, mode); });
    if (mode == ctx->top_level) return CGPT_OK;
    if (mode == 1u && ctx->has_scene) {                                        // the tree becomes active: write it (the edits kept its source current)
        return Guarded(ctx, __func__, [&] {
            HIP_TRY(ctx, hipSetDevice(ctx->device));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            ctx->top_level = 1u;
            const hipError_t e = WriteTopLevel(ctx, ctx->h_objects, ctx->top_state);
            if (e != hipSuccess) {                                             // the records may be half written: drop the scene (refit.hip: SceneLost)
                ctx->has_scene = false;
                return CtxFail(ctx, CGPT_ERR_HIP, "hipMemcpy of the top-level tree failed: %s (the device scene is dropped; upload it again)", hipGetErrorString(e));
            }
            return (int)CGPT_OK;
        });
    }
    ctx->top_level = mode;                                                     // read by the next render; the image does not depend on it: accumulator and guides stay
    return CGPT_OK;
}

// cgpt_scene_upload (instanced false: every object laid out) and cgpt_scene_upload_instanced (true: one copy per mesh group): one body, so
// the two validate, refuse, reset and keep alike
static int SceneUpload(cgpt_ctx* ctx, const cgpt_scene_desc* scene, bool instanced, const char* func)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, func, [&] { return GroupSceneUpload(ctx, scene, instanced); });
    if (!scene) return CtxFail(ctx, CGPT_ERR_INVALID, "scene is null");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->scene_generation++; ctx->shape_generation++;                          // the denoiser's guides are stale (denoise.hip)
    return Guarded(ctx, "scene upload", [&] {                                  // the re-layout allocates host vectors
        SceneLayout layout;
        const int rc = LayoutScene(*scene, layout, ctx->error, instanced);
        return rc != CGPT_OK ? rc : SceneInstall(ctx, layout);
    });
}

int cgpt_scene_upload(cgpt_ctx* ctx, const cgpt_scene_desc* scene) { return SceneUpload(ctx, scene, false, __func__); }

int cgpt_scene_upload_instanced(cgpt_ctx* ctx, const cgpt_scene_desc* scene) { return SceneUpload(ctx, scene, true, __func__); }

int cgpt_get_scene_footprint(cgpt_ctx* ctx, cgpt_scene_footprint* out)
{
    if (!ctx || !out) return CGPT_ERR_INVALID;
    if (ctx->group) return GroupForwarded(ctx, cgpt_get_scene_footprint(GroupFirstMember(ctx), out));   // every device holds the same arrays
    if (!ctx->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "no scene uploaded");
    *out = ctx->footprint;
    return CGPT_OK;
}

int cgpt_scene_update_materials(cgpt_ctx* ctx, const cgpt_material* materials, uint32_t n_materials)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupUpdateMaterials(ctx, materials, n_materials); });
    if (!ctx->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "no scene uploaded");
    if (!materials || n_materials != ctx->n_materials) return CtxFail(ctx, CGPT_ERR_INVALID, "expected %u materials", ctx->n_materials);
    std::vector<float4> mats;
    try { mats.resize(4 * (size_t)n_materials); } catch (const std::exception& e) { return CtxFail(ctx, CGPT_ERR_INVALID, "out of host memory: %s", e.what()); }
    for (uint32_t i = 0; i < n_materials; ++i) PackMaterial(materials[i], ctx->h_roughness[i], ctx->h_transmission_roughness[i], mats.data() + 4 * (size_t)i);   // both roughnesses are kept
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->scene_generation++; ctx->shape_generation++;
    HIP_TRY(ctx, hipMemcpy(ctx->sb.materials.p, mats.data(), mats.size() * sizeof(float4), hipMemcpyHostToDevice));
    ctx->h_materials.swap(mats);
    return CGPT_OK;
}

int cgpt_scene_update_roughness(cgpt_ctx* ctx, const float* roughness, uint32_t n_materials)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupUpdateRoughness(ctx, roughness, n_materials); });
    return UpdateRoughnessWord(ctx, roughness, n_materials, false);
}

int cgpt_scene_update_transmission_roughness(cgpt_ctx* ctx, const float* roughness, uint32_t n_materials)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupUpdateTransmissionRoughness(ctx, roughness, n_materials); });
    return UpdateRoughnessWord(ctx, roughness, n_materials, true);
}

int cgpt_scene_update_smooth_normals(cgpt_ctx* ctx, const uint32_t* smooth, uint32_t n_objects)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupUpdateSmoothNormals(ctx, smooth, n_objects); });
    return UpdateSmoothNormals(ctx, smooth, n_objects);
}

int cgpt_scene_update_transforms(cgpt_ctx* ctx, const float* object_to_world, uint32_t n_objects)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupUpdateTransforms(ctx, object_to_world, n_objects); });
    return UpdateTransforms(ctx, object_to_world, n_objects);
}

int cgpt_camera_from_view(const float pos[3], const float view_dir[3], float fov_deg, float aspect, cgpt_camera* out)
{
    if (!pos || !view_dir || !out) return CGPT_ERR_INVALID;
    const float fov = fov_deg * 3.14159265f / 180.0f;                         // Deg2Rad, ref: MathLib.h:9-12
    float center[3];
    for (int i = 0; i < 3; ++i) center[i] = pos[i] + fov * view_dir[i];       // ref: Main.cpp:145
    for (int i = 0; i < 3; ++i) out->pos[i] = pos[i];
    out->top_left[0] = center[0] + -aspect; out->top_left[1] = center[1] + 1.0f; out->top_left[2] = center[2] + 0.0f;
    out->top_right[0] = center[0] + aspect; out->top_right[1] = center[1] + 1.0f; out->top_right[2] = center[2] + 0.0f;
    out->bottom_left[0] = center[0] + -aspect; out->bottom_left[1] = center[1] + -1.0f; out->bottom_left[2] = center[2] + 0.0f;
    return CGPT_OK;
}

}  // extern "C"

namespace cgpt {

// The device half of a scene upload: replaces the context's scene by the arrays of `layout` (scene_layout.h).  Only called with a
// layout that LayoutScene accepted, so a refused scene leaves the previous one installed.
int SceneInstall(cgpt_ctx* ctx, const SceneLayout& layout)
{
    FreeScene(ctx);
    int rc;
    if ((rc = UploadArray(ctx, ctx->sb.node_pairs, layout.node_pairs)) != CGPT_OK) return rc;
    if ((rc = UploadArray(ctx, ctx->sb.tri_leaf, layout.tri_leaf)) != CGPT_OK) return rc;
    if ((rc = UploadArray(ctx, ctx->sb.tri_orig, layout.tri_orig)) != CGPT_OK) return rc;
    // tri_normal: the n0 records, then the {n1, n2} pairs (device_scene.h)
    const size_t n_tris_total = layout.tri_normal.size();
    if (layout.tri_normal12.size() != 2 * n_tris_total) return CtxFail(ctx, CGPT_ERR_INVALID, "layout: %zu normal pairs for %zu triangles", layout.tri_normal12.size() / 2, n_tris_total);
    HIP_TRY(ctx, ctx->sb.tri_normal.Alloc(n_tris_total ? 3 * n_tris_total : 1));
    if (n_tris_total) {
        HIP_TRY(ctx, hipMemcpy(ctx->sb.tri_normal.p, layout.tri_normal.data(), sizeof(float4) * n_tris_total, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(ctx->sb.tri_normal.p + n_tris_total, layout.tri_normal12.data(), sizeof(float4) * 2 * n_tris_total, hipMemcpyHostToDevice));
    }
    if ((rc = UploadArray(ctx, ctx->sb.materials, layout.materials)) != CGPT_OK) return rc;
    if ((rc = UploadArray(ctx, ctx->sb.objects, layout.objects)) != CGPT_OK) return rc;
    // obj_trace: the 2 n trace records, then the 3 n transform records (device_scene.h)
    const size_t n_obj = layout.objects.size();
    if (layout.obj_trace.size() != 2 * n_obj || layout.obj_xform.size() != 3 * n_obj) return CtxFail(ctx, CGPT_ERR_INVALID, "layout: %zu trace and %zu transform records for %zu objects", layout.obj_trace.size(), layout.obj_xform.size(), n_obj);
    if (layout.mesh_group.size() != n_obj) return CtxFail(ctx, CGPT_ERR_INVALID, "layout: mesh groups of %zu objects", layout.mesh_group.size());
    if (layout.top_state.local_box.size() != 6 * n_obj || layout.top_state.xform.size() != 12 * n_obj) return CtxFail(ctx, CGPT_ERR_INVALID, "layout: top-level state of %zu objects", layout.top_state.local_box.size() / 6);
    HIP_TRY(ctx, ctx->sb.obj_trace.Alloc(n_obj ? 5 * n_obj + TopLevelFloat4s(n_obj) : 1));   // ... then the top-level tree (written while cgpt_set_top_level is 1)
    if (n_obj) {
        HIP_TRY(ctx, hipMemcpy(ctx->sb.obj_trace.p, layout.obj_trace.data(), sizeof(float4) * 2 * n_obj, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(ctx->sb.obj_trace.p + 2 * n_obj, layout.obj_xform.data(), sizeof(float4) * 3 * n_obj, hipMemcpyHostToDevice));
    }
    if ((rc = UploadArray(ctx, ctx->sb.lights, layout.lights)) != CGPT_OK) return rc;
    if ((rc = UploadArray(ctx, ctx->sb.refit_levels, layout.refit_levels)) != CGPT_OK) return rc;
    ctx->h_objects = layout.objects; ctx->refit_objects = layout.refit_objects; ctx->record_perm = layout.record_perm;
    ctx->h_roughness.assign(layout.n_materials, 0.0f); ctx->h_transmission_roughness.assign(layout.n_materials, 0.0f); ctx->h_materials = layout.materials;
    ctx->h_lights = layout.lights;                                             // FreeScene cleared the features: an upload resets every roughness, smooth-normal flag and transform (LayoutScene writes 0 and the identity)
    ctx->top_state = layout.top_state;
    ctx->mesh_group = layout.mesh_group;
    ctx->n_refit_levels = (uint32_t)layout.refit_levels.size();
    HIP_TRY(ctx, WriteTopLevel(ctx, ctx->h_objects, ctx->top_state));          // the mode is context state: an upload keeps it

    cgpt_scene_footprint& fp = ctx->footprint;
    const SceneBuffers& sb = ctx->sb;
    fp = cgpt_scene_footprint{};
    fp.device_bytes = sizeof(float4) * (uint64_t)(sb.node_pairs.n + sb.tri_leaf.n + sb.tri_orig.n + sb.tri_normal.n + sb.materials.n + sb.obj_trace.n) +
                      sizeof(DevObject) * (uint64_t)sb.objects.n + sizeof(uint32_t) * (uint64_t)(sb.lights.n + sb.refit_levels.n);
    fp.n_objects = (uint32_t)n_obj;
    for (size_t i = 0; i < n_obj; ++i)
        if (layout.objects[i].kind == CGPT_OBJECT_MESH) { fp.n_mesh_objects++; if (layout.mesh_group[i] == i) fp.n_mesh_copies++; }
    fp.n_leaf_records = (uint32_t)(layout.tri_leaf.size() / 3); fp.n_pair_records = layout.n_pair_records; fp.n_orig_triangles = (uint32_t)n_tris_total;

    ctx->scene.node_pairs = ctx->sb.node_pairs.p; ctx->scene.tri_leaf = ctx->sb.tri_leaf.p; ctx->scene.tri_orig = ctx->sb.tri_orig.p; ctx->scene.tri_normal = ctx->sb.tri_normal.p;
    ctx->scene.materials = ctx->sb.materials.p; ctx->scene.objects = ctx->sb.objects.p; ctx->scene.obj_trace = ctx->sb.obj_trace.p; ctx->scene.lights = ctx->sb.lights.p;
    ctx->scene.n_objects = (uint32_t)layout.objects.size(); ctx->scene.n_lights = (uint32_t)layout.lights.size(); ctx->scene.stack_depth = layout.stack_depth;
    ctx->scene.n_top_records = layout.n_top_records; ctx->scene.n_tris_total = (uint32_t)n_tris_total; ctx->scene.n_small_tris = layout.n_small_tris;
    ctx->n_materials = layout.n_materials;
    ctx->has_scene = true;
    return CGPT_OK;
}

int TranslateSettings(cgpt_ctx* ctx, const cgpt_settings& settings, DevSettings& st)
{
    if (settings.max_ray_depth < 0 || settings.max_ray_depth > 254)
        return CtxFail(ctx, CGPT_ERR_INVALID, "max_ray_depth %d outside [0,254] (ray_depth is a uint8_t in the reference, Main.cpp:401)", settings.max_ray_depth);
    if (settings.render_mode > CGPT_MODE_ADVANCED || settings.debug_render_mode > CGPT_DEBUG_BVH_DEPTH)
        return CtxFail(ctx, CGPT_ERR_INVALID, "bad render_mode/debug_render_mode");
    st.max_ray_depth = settings.max_ray_depth;
    st.nee = settings.next_event_estimation_enabled;
    st.cosine = settings.cosine_weighted_diffuse_reflection_enabled;
    st.rr = settings.russian_roulette_enabled;
    st.render_mode = settings.render_mode;
    st.debug_mode = settings.debug_render_mode;
    return CGPT_OK;
}

int RenderEnqueue(cgpt_ctx* ctx, const cgpt_camera* camera, const cgpt_settings* settings, const cgpt_render_params* p)
{
    ctx->pending_kernel = 0;
    ctx->denoised = nullptr;                                                   // CGPT_TONEMAP_DENOISED: the last filter call's result is of an older frame
    if (!camera || !settings || !p) return CtxFail(ctx, CGPT_ERR_INVALID, "null argument");
    if (!ctx->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "cgpt_render before cgpt_scene_upload");
    DevRenderArgs args{};
    int rc = TranslateSettings(ctx, *settings, args.settings);
    if (rc != CGPT_OK) return rc;
    if (settings->render_mode != CGPT_MODE_ADVANCED) {
        // TracePath (brute force) keeps its per-level operations in HBM in the persistent kernel (per lane) and in the wavefront
        // pipeline (per path), any depth; the megakernel keeps them in per-lane scratch of 32 levels
        if (p->kernel == CGPT_KERNEL_MEGAKERNEL && settings->max_ray_depth + 1 > 32)
            return CtxFail(ctx, CGPT_ERR_UNSUPPORTED, "brute-force / comparison modes in the megakernel support max_ray_depth <= 31 (got %d)", settings->max_ray_depth);
    }
    if ((uint64_t)p->first_sample + p->n_samples > 0xFFFFFFFFull) return CtxFail(ctx, CGPT_ERR_INVALID, "sample index overflow");

    Band band;
    rc = ResolveBand(ctx, *p, band);
    if (rc != CGPT_OK) return rc;
    const uint32_t n_rows = band.n_rows, band_first = band.first, band_h = band.h, band_stride = band.stride;

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = EnsureFramebuffer(ctx, p->width, p->height, n_rows, band.key);
    if (rc != CGPT_OK) return rc;
    if (p->n_samples == 0) return CGPT_OK;

    args.scene = ctx->scene;
    memcpy(&args.camera, camera, sizeof(DevCamera));
    args.width = p->width; args.height = p->height;
    args.n_rows = n_rows; args.band_first = band_first; args.band_h = band_h; args.band_stride = band_stride;
    args.first_sample = p->first_sample; args.n_samples = p->n_samples; args.seed = p->seed;
    args.accumulator = ctx->fb.accumulator.p; args.pixels = ctx->fb.pixels.p; args.counters = ctx->counters.p;

    const ShadeVariant variant = ChooseVariant(ctx, args.settings, p->flags);
    // AUTO: all three kernels give bit-identical images, so the choice is speed alone.  MI355X, glass scene, ms per call
    // (profiles/r03/small_calls_table.txt; 16 samples and more: profiles/r02/frame_time_after.txt):
    //                 64x64  1 / 2 / 8 samples     960x540  1 / 2 / 8        1920x1080  1 / 2 / 4 / 8 / 16 / 32 / 64 / 128
    //   megakernel    0.62 / 1.32 / 5.12           1.26 / 2.53 / 9.91        1.68 / 3.17 / 6.06 / 11.9 / 23.1 / ...   one thread walks a pixel's samples: time ~ samples
    //   persistent    0.79 / 0.70 / 0.77           1.68 / 1.82 / 2.35        2.13 / 2.36 / 3.01 / 5.02 / 8.25 / 14.9 / 27.9 / 53.9
    //   wavefront     1.45 / 1.54 / 1.66           2.21 / 2.44 / 2.76        2.48 / 2.98 / 3.57 / 5.13 / 8.35 / 14.7 / 26.7 / 51.1      (256 samples: 93 vs 106 ms)
    // A call cannot finish before its longest path does (~1.2 ms in the megakernel, ~2 ms in the voted kernels on this scene), which
    // is what a one-sample call pays: the megakernel wins every one-sample call, at every frame size; with two or more samples per call
    // the voted kernels win, the persistent kernel (two launches) up to ~16 M paths, the wavefront pipeline beyond -- TracePath /
    // COMPARISON (the reference's default mode) included: 256-spp 1080p COMPARISON 88.6 ms in the pipeline against 95.3 in the
    // persistent kernel, BRUTE_FORCE 71.4 against 73.1 (profiles/r03).
    const uint64_t n_paths = (uint64_t)p->width * n_rows * p->n_samples;
    uint32_t kernel = p->kernel;
    if (kernel == CGPT_KERNEL_AUTO) {
        const bool advanced = settings->render_mode == CGPT_MODE_ADVANCED;
        if (p->n_samples == 1u && n_paths < 3000000ull && (advanced || settings->max_ray_depth + 1 <= 32)) kernel = CGPT_KERNEL_MEGAKERNEL;
        else if (n_paths < 16000000ull) kernel = CGPT_KERNEL_PERSISTENT;   // (40 M until the end of round 3: 1080p x 8 / 16 samples now 4.77 / 7.59 ms in the pipeline, 4.90 / 8.10 here)
        // Beyond that the pipeline, whatever the size of the tree.  (Rounds 2-3 sent trees of more than 800 K child pairs -- 84 MB + 63 MB of
        // leaf triangles at 1.31 M triangles, far beyond the L2 -- to the persistent kernel, then 5 % faster there.  With the ray lists ordered
        // by image band the pipeline leads: rank shares of the 1080p x 1024 / 4K x 4096 spp configurations 34.4-34.6 vs 36.6-36.8 ms and
        // 510 vs 556 ms, the whole 1080p x 1024 frame 260 vs 280 ms; profiles/r03/image_bands.md.)
        else kernel = CGPT_KERNEL_WAVEFRONT;
    }

    if (kernel == CGPT_KERNEL_MEGAKERNEL) {
        HIP_TRY(ctx, hipEventRecord(ctx->ev_start.e, ctx->stream));
        HIP_TRY(ctx, LaunchMegakernel(args, variant, ctx->stream));
        ctx->kernel_launches += 1;
    } else if (kernel == CGPT_KERNEL_WAVEFRONT) {
        rc = LaunchWavefront(ctx, args, variant);
        if (rc < 0) return ctx->error.empty() ? CtxFail(ctx, CGPT_ERR_HIP, "wavefront launch failed") : CGPT_ERR_HIP;
        ctx->kernel_launches += (uint32_t)rc;
    } else if (kernel == CGPT_KERNEL_PERSISTENT) {
        rc = LaunchPersistent(ctx, args, variant);
        if (rc < 0) return ctx->error.empty() ? CtxFail(ctx, CGPT_ERR_HIP, "persistent kernel launch failed") : CGPT_ERR_HIP;
        ctx->kernel_launches += (uint32_t)rc;
    } else {
        return CtxFail(ctx, CGPT_ERR_INVALID, "unknown kernel %u", p->kernel);
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_stop.e, ctx->stream));
    ctx->pending_kernel = kernel; ctx->pending_args = args; ctx->pending_num_accumulated = p->first_sample + p->n_samples; ctx->pending_variant = variant;
    ctx->last_debug_mode = settings->debug_render_mode;
    ctx->last_kernel = kernel;
    return CGPT_OK;
}

int RenderFinish(cgpt_ctx* ctx)
{
    const uint32_t kernel = ctx->pending_kernel;
    if (kernel == 0) return CGPT_OK;                                           // nothing was enqueued (n_samples == 0)
    ctx->pending_kernel = 0;
    const DevRenderArgs& args = ctx->pending_args;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev_stop.e));
    float ms = 0.0f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev_start.e, ctx->ev_stop.e));
    ctx->kernel_ms += ms;
    if (kernel == CGPT_KERNEL_MEGAKERNEL) { ctx->dominant_ms += ms; ctx->dominant_launches += 1; ctx->dominant_waves_per_simd = MegakernelWavesPerSimd(args, ctx->pending_variant); }
    else if (kernel == CGPT_KERNEL_PERSISTENT) {
        double tms = 0.0; uint32_t tl = 0, w = 0;
        PersistentCollectTiming(ctx->persistent_state, ctx->pending_variant, &tms, &tl, &w);
        ctx->dominant_ms += tms; ctx->dominant_launches += tl; ctx->dominant_waves_per_simd = w;
    } else {
        ctx->dominant_waves_per_simd = WavefrontTraceWavesPerSimd(ctx->wavefront_state);
        double tms = 0.0, r0ms = 0.0; uint32_t tl = 0, r0l = 0;
        WavefrontCollectTiming(ctx->wavefront_state, &tms, &tl, &r0ms, &r0l);
        ctx->dominant_ms += tms; ctx->dominant_launches += tl;
        ctx->dominant_round0_ms += r0ms; ctx->dominant_round0_launches += r0l;
    }
    ctx->num_accumulated = ctx->pending_num_accumulated;
    return CGPT_OK;
}

}  // namespace cgpt

extern "C" {

int cgpt_render(cgpt_ctx* ctx, const cgpt_camera* camera, const cgpt_settings* settings, const cgpt_render_params* p)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupRender(ctx, camera, settings, p); });
    const int rc = RenderEnqueue(ctx, camera, settings, p);
    return rc != CGPT_OK ? rc : RenderFinish(ctx);
}

int cgpt_reset_accumulator(cgpt_ctx* ctx)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupResetAccumulator(ctx); });
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->num_accumulated = 0;                                                  // ref: Main.cpp:240-242
    ctx->denoised = nullptr;
    if (ctx->fb.accumulator.p) {
        const size_t n = (size_t)ctx->width * ctx->n_rows;
        HIP_TRY(ctx, hipMemsetAsync(ctx->fb.accumulator.p, 0, n * sizeof(float4), ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    double zero = 0.0;
    HIP_TRY(ctx, hipMemcpy(&ctx->counters.p->total_energy, &zero, sizeof(double), hipMemcpyHostToDevice));
    return CGPT_OK;
}

int cgpt_read_accumulator(cgpt_ctx* ctx, float* dst, size_t n_floats)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupReadAccumulator(ctx, dst, n_floats); });
    if (!ctx->fb.accumulator.p) return CtxFail(ctx, CGPT_ERR_INVALID, "nothing rendered yet");
    const size_t n = (size_t)ctx->width * ctx->n_rows * 4;
    if (!dst || n_floats != n) return CtxFail(ctx, CGPT_ERR_INVALID, "expected a buffer of %zu floats", n);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(dst, ctx->fb.accumulator.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return CGPT_OK;
}

int cgpt_read_pixels(cgpt_ctx* ctx, uint32_t* dst, size_t n_pixels)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupReadPixels(ctx, dst, n_pixels); });
    if (!ctx->fb.pixels.p) return CtxFail(ctx, CGPT_ERR_INVALID, "nothing rendered yet");
    const size_t n = (size_t)ctx->width * ctx->n_rows;
    if (!dst || n_pixels != n) return CtxFail(ctx, CGPT_ERR_INVALID, "expected a buffer of %zu pixels", n);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(dst, ctx->fb.pixels.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return CGPT_OK;
}

int cgpt_write_accumulator(cgpt_ctx* ctx, const cgpt_render_params* p, const float* src, size_t n_floats, uint32_t num_accumulated)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupWriteAccumulator(ctx, p, src, n_floats, num_accumulated); });
    ctx->denoised = nullptr;
    if (!p || !src) return CtxFail(ctx, CGPT_ERR_INVALID, "null argument");
    Band band;
    int rc = ResolveBand(ctx, *p, band);
    if (rc != CGPT_OK) return rc;
    const size_t n = (size_t)p->width * band.n_rows;
    if (n_floats != 4 * n) return CtxFail(ctx, CGPT_ERR_INVALID, "expected %zu floats for %u rows of %u pixels, got %zu", 4 * n, band.n_rows, p->width, n_floats);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = EnsureFramebuffer(ctx, p->width, p->height, band.n_rows, band.key)) != CGPT_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->fb.accumulator.p, src, n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, LaunchPackPixels(ctx->fb.accumulator.p, ctx->fb.pixels.p, n, num_accumulated, ctx->stream));   // data.pixels, ref: Main.cpp:741
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->num_accumulated = num_accumulated;                                    // ref: Main.cpp:205
    ctx->last_debug_mode = 0;                                                  // data.pixels are the packed sums again
    return CGPT_OK;
}

int cgpt_set_tuning(cgpt_ctx* ctx, const char* name, uint32_t value)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupSetTuning(ctx, name, value); });
    if (!name) return CtxFail(ctx, CGPT_ERR_INVALID, "null knob name");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (strcmp(name, "skin_joints_lds") == 0) {                                // cgpt_scene_skin_mesh: where the kernel reads the joint matrices
        if (value > 1u) return CtxFail(ctx, CGPT_ERR_INVALID, "skin_joints_lds %u is neither 0 (vector cache) nor 1 (LDS)", value);
        ctx->skin_joints_lds = value;
        return CGPT_OK;
    }
    if (strcmp(name, "morph_leaf_order") == 0) {                               // cgpt_scene_set_morph_targets: how the next set stores the targets
        if (value > 1u) return CtxFail(ctx, CGPT_ERR_INVALID, "morph_leaf_order %u is neither 0 (as given) nor 1 (leaf-slot order)", value);
        ctx->morph_leaf_order = value;
        return CGPT_OK;
    }
    if (strcmp(name, "morph_max_blocks") == 0) {                               // cgpt_scene_morph_mesh: the cap of the kernel's grid
        if (value < 1u || value > 1024u) return CtxFail(ctx, CGPT_ERR_INVALID, "morph_max_blocks %u outside [1, 1024]", value);
        ctx->morph_max_blocks = value;
        return CGPT_OK;
    }
    bool known = false;
    const int rc = PersistentSetTuning(ctx, name, value, &known);              // "pt_*" knobs
    if (known) return rc;
    return WavefrontSetTuning(ctx, name, value);
}

int cgpt_accumulator_device_ptr(cgpt_ctx* ctx, void** ptr, size_t* n_bytes)
{
    if (!ctx || !ptr || !n_bytes) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupDevicePtr(ctx, false, ptr, n_bytes); });
    if (!ctx->fb.accumulator.p) return CtxFail(ctx, CGPT_ERR_INVALID, "nothing rendered yet");
    *ptr = ctx->fb.accumulator.p;
    *n_bytes = (size_t)ctx->width * ctx->n_rows * sizeof(float4);
    return CGPT_OK;
}

int cgpt_pixels_device_ptr(cgpt_ctx* ctx, void** ptr, size_t* n_bytes)
{
    if (!ctx || !ptr || !n_bytes) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupDevicePtr(ctx, true, ptr, n_bytes); });
    if (!ctx->fb.pixels.p) return CtxFail(ctx, CGPT_ERR_INVALID, "nothing rendered yet");
    *ptr = ctx->fb.pixels.p;
    *n_bytes = (size_t)ctx->width * ctx->n_rows * sizeof(uint32_t);
    return CGPT_OK;
}

int cgpt_get_stats(cgpt_ctx* ctx, cgpt_stats* out)
{
    if (!ctx || !out) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupGetStats(ctx, out); });
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    DevCounters c;
    HIP_TRY(ctx, hipMemcpy(&c, ctx->counters.p, sizeof(c), hipMemcpyDeviceToHost));
    out->traced_rays = c.traced_rays; out->inner_steps = c.inner_steps; out->tri_tests = c.tri_tests;
    out->bvh_depth_sum = c.bvh_depth_sum; out->closest_hits = c.closest_hits; out->total_energy_received = c.total_energy;
    out->num_accumulated = ctx->num_accumulated; out->kernel_launches = ctx->kernel_launches; out->kernel_ms = ctx->kernel_ms;
    out->dominant_launches = ctx->dominant_launches; out->dominant_waves_per_simd = ctx->dominant_waves_per_simd; out->dominant_ms = ctx->dominant_ms;
    out->gather_ms = 0.0; out->gathers = 0; out->n_devices = 1; out->rccl_ranks = 0; out->last_kernel = ctx->last_kernel;
    memset(out->device_ms, 0, sizeof(out->device_ms)); out->device_ms[0] = ctx->kernel_ms;
    out->dominant_round0_ms = ctx->dominant_round0_ms; out->dominant_round0_launches = ctx->dominant_round0_launches; out->chain_followers = (uint32_t)std::min<unsigned long long>(c.chain_followers, 0xFFFFFFFFull);
    out->probe_resolved = c.probe_resolved;
    return CGPT_OK;
}

int cgpt_get_retrace_unwalked(cgpt_ctx* ctx, uint64_t* out)
{
    if (!ctx || !out) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupGetRetraceUnwalked(ctx, out); });
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    unsigned long long v = 0;
    HIP_TRY(ctx, hipMemcpy(&v, &ctx->counters.p->retrace_unwalked, sizeof(v), hipMemcpyDeviceToHost));
    *out = v;
    return CGPT_OK;
}

int cgpt_reset_stats(cgpt_ctx* ctx)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupResetStats(ctx); });
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemset(ctx->counters.p, 0, sizeof(DevCounters)));
    ctx->kernel_launches = 0; ctx->kernel_ms = 0.0; ctx->dominant_launches = 0; ctx->dominant_ms = 0.0;
    ctx->dominant_round0_launches = 0; ctx->dominant_round0_ms = 0.0;
    return CGPT_OK;
}

int cgpt_intersect_rays(cgpt_ctx* ctx, const float* origins, const float* dirs, const float* tmax, uint32_t n,
                        float* out_t, uint32_t* out_obj, uint32_t* out_tri, uint32_t* out_depth)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return GroupForwarded(ctx, cgpt_intersect_rays(GroupFirstMember(ctx), origins, dirs, tmax, n, out_t, out_obj, out_tri, out_depth));
    if (!ctx->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "cgpt_intersect_rays before cgpt_scene_upload");
    if (n == 0) return CGPT_OK;
    if (!origins || !dirs || !out_t || !out_obj || !out_tri || !out_depth) return CtxFail(ctx, CGPT_ERR_INVALID, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n3 = 3 * (size_t)n;
    DevBuf<float> d_o, d_d, d_tm, d_t;
    DevBuf<uint32_t> d_obj, d_tri, d_dep;
    HIP_TRY(ctx, d_o.Alloc(n3)); HIP_TRY(ctx, d_d.Alloc(n3));
    if (tmax) HIP_TRY(ctx, d_tm.Alloc(n));
    HIP_TRY(ctx, d_t.Alloc(n)); HIP_TRY(ctx, d_obj.Alloc(n));
    HIP_TRY(ctx, d_tri.Alloc(n)); HIP_TRY(ctx, d_dep.Alloc(n));
    HIP_TRY(ctx, hipMemcpyAsync(d_o.p, origins, 12 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_d.p, dirs, 12 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if (tmax) HIP_TRY(ctx, hipMemcpyAsync(d_tm.p, tmax, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, LaunchIntersectRays(ctx, d_o.p, d_d.p, d_tm.p, n, d_t.p, d_obj.p, d_tri.p, d_dep.p));
    HIP_TRY(ctx, hipMemcpyAsync(out_t, d_t.p, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(out_obj, d_obj.p, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(out_tri, d_tri.p, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(out_depth, d_dep.p, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CGPT_OK;
}

uint64_t cgpt_debug_live_device_bytes(void) { return Ledger().live.load(); }

int cgpt_synchronize(cgpt_ctx* ctx)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupSynchronize(ctx); });
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CGPT_OK;
}

}  // extern "C"
