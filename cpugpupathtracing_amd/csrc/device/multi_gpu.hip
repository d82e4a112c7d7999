// multi_gpu.hip -- one host process, up to 8 MI355X: the multi-device context behind cgpt_ctx_create(device_ids, n_devices > 1).
//
// The reference is ONE C++ process whose main loop calls Render() and then hands data.pixels to the presenter
// (ref: Source/Main.cpp:773 ThreadPool::Init, :753-754 Dispatch / WaitAll, :834-836, :935 CopyToBackBuffer).  A maintainer who
// follows INTEGRATION.md keeps that shape: one context, one cgpt_render per frame, one cgpt_read_pixels -- and the context
// spreads the frame over the GPUs of the node:
//   * the image is cut into bands of `band_rows` rows dealt round-robin over the devices (cgpt_render_params.interleave_*:
//     every GPU gets the same mix of sky, mesh and ground rows); the scene is replicated by cgpt_scene_upload;
//   * cgpt_render enqueues every device's kernels without waiting in between, then waits for all of them;
//   * cgpt_read_accumulator / cgpt_read_pixels run ONE grouped RCCL exchange -- every device ncclSend()s its float4 band,
//     device 0 ncclRecv()s them (a gather with per-rank counts; the bands differ by up to band_rows rows) -- over xGMI, then a
//     row-reorder kernel on device 0 puts the bands back into image order.  Nothing is exchanged during tracing.
// RNG streams are keyed by the global pixel index, so the gathered image is bit-identical to a one-GPU render.
// bench.py --gpus N (launched as a plain command) runs through this context; under torch.distributed.run it keeps one process per
// GPU instead (cpugpupathtracing_amd/distributed.py).
// Host threads: the context owns one persistent worker per device beyond the first (started by cgpt_ctx_create, joined by
// cgpt_ctx_destroy); cgpt_render hands every worker its device's enqueue and does device 0's itself, so a one-sample-per-call
// host (the reference's own main loop, ref: Main.cpp:825-942) pays a condition-variable wake per frame, not a thread spawn.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <exception>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "cpugpupt_abi.h"
#include "ctx_internal.h"

namespace cgpt {

static constexpr uint32_t kMaxRanks = 8;

// Persistent per-device host workers: rank r >= 1 runs `job(arg, r)` on its own thread, the caller runs rank 0's share.
struct WorkerPool {
    std::vector<std::thread> threads;
    std::mutex m;
    std::condition_variable cv_job, cv_done;
    uint64_t generation = 0;
    uint32_t pending = 0;
    bool exit = false;
    void (*job)(void*, uint32_t) = nullptr;
    void* arg = nullptr;

    void Start(uint32_t n_ranks)                                              // may throw (std::system_error): only called under cgpt_ctx_create's try
    {
        for (uint32_t r = 1; r < n_ranks; ++r) threads.emplace_back([this, r]() { Loop(r); });
    }
    void Loop(uint32_t r)
    {
        uint64_t seen = 0;
        for (;;) {
            void (*fn)(void*, uint32_t); void* a;
            {
                std::unique_lock<std::mutex> lk(m);
                cv_job.wait(lk, [&]() { return exit || generation != seen; });
                if (exit) return;
                seen = generation; fn = job; a = arg;
            }
            fn(a, r);                                                         // jobs do not throw (they catch and record a status)
            {
                std::lock_guard<std::mutex> lk(m);
                if (--pending == 0) cv_done.notify_one();
            }
        }
    }
    void Run(void (*fn)(void*, uint32_t), void* a)                            // all ranks; returns when every rank's job has returned
    {
        const uint32_t n_workers = (uint32_t)threads.size();
        if (n_workers) {
            std::lock_guard<std::mutex> lk(m);
            job = fn; arg = a; pending = n_workers; ++generation;
        }
        if (n_workers) cv_job.notify_all();
        fn(a, 0);
        if (n_workers) {
            std::unique_lock<std::mutex> lk(m);
            cv_done.wait(lk, [&]() { return pending == 0; });
        }
    }
    void Stop()
    {
        { std::lock_guard<std::mutex> lk(m); exit = true; }
        cv_job.notify_all();
        for (std::thread& t : threads) if (t.joinable()) t.join();
        threads.clear();
    }
};

struct DeviceGroup {
    std::vector<cgpt_ctx*> members;        // one-device contexts, rank order
    std::vector<ncclComm_t> comms;         // empty with CGPT_CTX_GATHER_PEER_COPY
    WorkerPool workers;
    bool peer_copy = false;
    uint32_t band_rows_cfg = 4;            // configured band height (cgpt_set_tuning "band_rows")
    uint32_t band_rows = 4;                // effective band height of the current frame: the configured one, halved until every device owns rows
    // framebuffer of the last render
    uint32_t width = 0, height = 0;
    std::vector<uint32_t> n_rows;          // rows of each member's band
    uint32_t num_accumulated = 0;
    uint32_t last_debug_mode = 0;
    uint32_t last_kernel = 0;
    // device 0: staging (all bands, rank after rank) and the gathered full frame
    DevBuf<float4> staging, full; DevBuf<uint32_t> pix_staging, full_pixels;
    DevBuf<uint32_t> rank_base;            // first staging row of every rank (8 words)
    bool gathered = false, pixels_valid = false;
    uint32_t gathers = 0;
    double gather_ms = 0.0;                // summed duration of the exchanges (hipEvents on device 0's stream)
    DevEvent ev_gather0, ev_gather1;
};

namespace {

// band-ordered rows of all ranks (rank after rank, each in its own compact order) -> image order
__global__ void __launch_bounds__(256) reorder_rows_f4(const float4* __restrict__ staging, float4* __restrict__ full, uint32_t width, uint32_t height,
                                                        uint32_t band_rows, uint32_t n_ranks, const uint32_t* __restrict__ rank_base_rows)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (size_t)width * height) return;
    const uint32_t y = (uint32_t)(i / width), x = (uint32_t)(i - (size_t)y * width);
    const uint32_t band = y / band_rows, r = band % n_ranks;
    const uint32_t local_row = (band / n_ranks) * band_rows + y % band_rows;   // same enumeration as cgpt_render_params.interleave_*
    full[i] = staging[((size_t)rank_base_rows[r] + local_row) * width + x];
}
__global__ void __launch_bounds__(256) reorder_rows_u32(const uint32_t* __restrict__ staging, uint32_t* __restrict__ full, uint32_t width, uint32_t height,
                                                         uint32_t band_rows, uint32_t n_ranks, const uint32_t* __restrict__ rank_base_rows)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (size_t)width * height) return;
    const uint32_t y = (uint32_t)(i / width), x = (uint32_t)(i - (size_t)y * width);
    const uint32_t band = y / band_rows, r = band % n_ranks;
    const uint32_t local_row = (band / n_ranks) * band_rows + y % band_rows;
    full[i] = staging[((size_t)rank_base_rows[r] + local_row) * width + x];
}

uint32_t RowsOfRank(uint32_t height, uint32_t band_rows, uint32_t n, uint32_t r)
{
    uint32_t rows = 0;
    for (uint64_t first = (uint64_t)r * band_rows; first < height; first += (uint64_t)n * band_rows) rows += std::min<uint32_t>(band_rows, height - (uint32_t)first);
    return rows;
}

// band height of a frame: the configured one, halved until every device owns rows
uint32_t EffectiveBandRows(uint32_t cfg, uint32_t n, uint32_t height)
{
    uint32_t band_rows = cfg;
    while (band_rows > 1 && (uint64_t)n * band_rows > height) band_rows /= 2;
    return band_rows;
}

// (re)derives the tiling of a width x height frame from the configured band height
void SetTiling(DeviceGroup* g, uint32_t width, uint32_t height)
{
    const uint32_t n = (uint32_t)g->members.size();
    g->band_rows = EffectiveBandRows(g->band_rows_cfg, n, height);
    g->width = width; g->height = height;
    for (uint32_t r = 0; r < n; ++r) g->n_rows[r] = RowsOfRank(height, g->band_rows, n, r);
}

// copies the members' message (if any) into the group context and returns rc
int Propagate(cgpt_ctx* ctx, cgpt_ctx* member, int rc)
{
    if (rc != CGPT_OK) ctx->error = std::string("device ") + std::to_string(member->device) + ": " + member->error;
    return rc;
}

// The one collective: every rank's band to device 0, then image order.  `pixels`: gather the RGBA8 band as well (debug views,
// where data.pixels is not a function of the accumulator).
int Gather(cgpt_ctx* ctx, bool pixels)
{
    DeviceGroup* g = ctx->group;
    const uint32_t n = (uint32_t)g->members.size();
    if (g->width == 0) return CtxFail(ctx, CGPT_ERR_INVALID, "nothing rendered yet");
    if (g->gathered && (!pixels || g->pixels_valid)) return CGPT_OK;
    cgpt_ctx* root = g->members[0];
    const size_t n_px = (size_t)g->width * g->height;
    HIP_TRY(ctx, hipSetDevice(root->device));
    HIP_TRY(ctx, g->staging.Grow(n_px)); HIP_TRY(ctx, g->full.Grow(n_px));   // grow-only, each on its own count
    HIP_TRY(ctx, g->pix_staging.Grow(n_px)); HIP_TRY(ctx, g->full_pixels.Grow(n_px));
    HIP_TRY(ctx, g->rank_base.Grow(kMaxRanks));
    uint32_t base[kMaxRanks] = { 0 };
    for (uint32_t r = 1; r < n; ++r) base[r] = base[r - 1] + g->n_rows[r - 1];

    HIP_TRY(ctx, hipEventRecord(g->ev_gather0.e, root->stream));
    if (g->peer_copy) {
        for (uint32_t r = 0; r < n; ++r) {
            cgpt_ctx* m = g->members[r];
            const size_t count = (size_t)g->n_rows[r] * g->width;
            HIP_TRY(ctx, hipMemcpyPeerAsync(g->staging.p + (size_t)base[r] * g->width, root->device, m->fb.accumulator.p, m->device, count * sizeof(float4), root->stream));
            if (pixels) HIP_TRY(ctx, hipMemcpyPeerAsync(g->pix_staging.p + (size_t)base[r] * g->width, root->device, m->fb.pixels.p, m->device, count * sizeof(uint32_t), root->stream));
        }
    } else {
        // one grouped exchange: rank r sends on its own stream, rank 0 receives all of them (its own band included) on its stream.
        // A group that was opened is always closed: the first failure is kept and reported after ncclGroupEnd.
        ncclResult_t first = ncclGroupStart();
        const char* what = "ncclGroupStart";
        if (first == ncclSuccess) {
            auto keep = [&](ncclResult_t r, const char* w) { if (first == ncclSuccess && r != ncclSuccess) { first = r; what = w; } };
            for (uint32_t r = 0; r < n && first == ncclSuccess; ++r) {
                cgpt_ctx* m = g->members[r];
                const size_t count = (size_t)g->n_rows[r] * g->width;
                keep(ncclSend(m->fb.accumulator.p, count * 4, ncclFloat, 0, g->comms[r], m->stream), "ncclSend");
                keep(ncclRecv(g->staging.p + (size_t)base[r] * g->width, count * 4, ncclFloat, (int)r, g->comms[0], root->stream), "ncclRecv");
                if (pixels) {
                    keep(ncclSend(m->fb.pixels.p, count, ncclUint32, 0, g->comms[r], m->stream), "ncclSend");
                    keep(ncclRecv(g->pix_staging.p + (size_t)base[r] * g->width, count, ncclUint32, (int)r, g->comms[0], root->stream), "ncclRecv");
                }
            }
            keep(ncclGroupEnd(), "ncclGroupEnd");
        }
        if (first != ncclSuccess) return CtxFail(ctx, CGPT_ERR_HIP, "%s failed: %s", what, ncclGetErrorString(first));
    }
    HIP_TRY(ctx, hipSetDevice(root->device));
    uint32_t* const d_base = g->rank_base.p;
    HIP_TRY(ctx, hipMemcpyAsync(d_base, base, n * sizeof(uint32_t), hipMemcpyHostToDevice, root->stream));
    const dim3 grid((uint32_t)((n_px + 255u) / 256u)), block(256);
    hipLaunchKernelGGL(reorder_rows_f4, grid, block, 0, root->stream, (const float4*)g->staging.p, g->full.p, g->width, g->height, g->band_rows, n, (const uint32_t*)d_base);
    if (pixels) hipLaunchKernelGGL(reorder_rows_u32, grid, block, 0, root->stream, (const uint32_t*)g->pix_staging.p, g->full_pixels.p, g->width, g->height, g->band_rows, n, (const uint32_t*)d_base);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(g->ev_gather1.e, root->stream));
    for (uint32_t r = 0; r < n; ++r) {                                         // the senders' streams too: their bands are free again
        HIP_TRY(ctx, hipSetDevice(g->members[r]->device));
        HIP_TRY(ctx, hipStreamSynchronize(g->members[r]->stream));
    }
    HIP_TRY(ctx, hipSetDevice(root->device));
    HIP_TRY(ctx, hipStreamSynchronize(root->stream));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, g->ev_gather0.e, g->ev_gather1.e) == hipSuccess) g->gather_ms += ms;
    g->gathered = true; g->pixels_valid = pixels;
    g->gathers++;
    return CGPT_OK;
}

struct EnqueueJob {
    DeviceGroup* g;
    const cgpt_camera* camera; const cgpt_settings* settings; const cgpt_render_params* p;
    int rcs[kMaxRanks];
};
void EnqueueRank(void* arg, uint32_t r)                                       // every thread touches its own member context only
{
    EnqueueJob* j = static_cast<EnqueueJob*>(arg);
    cgpt_ctx* m = j->g->members[r];
    j->rcs[r] = Guarded(m, "render enqueue", [&] {
        cgpt_render_params q = *j->p;
        q.interleave_rows = j->g->band_rows; q.interleave_count = (uint32_t)j->g->members.size(); q.interleave_index = r;
        return RenderEnqueue(m, j->camera, j->settings, &q);
    });
}

}  // namespace

cgpt_ctx* GroupFirstMember(cgpt_ctx* ctx) { return ctx->group->members[0]; }
cgpt_ctx* GroupFirstMemberOrNull(cgpt_ctx* ctx) { return ctx && ctx->group ? ctx->group->members[0] : nullptr; }
int GroupForwarded(cgpt_ctx* ctx, int rc) { return Propagate(ctx, ctx->group->members[0], rc); }

int GroupCreate(const int* device_ids, int n_devices, uint32_t flags, cgpt_ctx** out)
{
    cgpt_ctx* ctx = new (std::nothrow) cgpt_ctx;
    DeviceGroup* g = new (std::nothrow) DeviceGroup;
    if (!ctx || !g) { delete ctx; delete g; return CtxFail(nullptr, CGPT_ERR_INVALID, "out of host memory"); }
    ctx->group = g;
    g->peer_copy = (flags & CGPT_CTX_GATHER_PEER_COPY) != 0;
    auto fail = [&](int rc) { GroupDestroy(ctx); delete ctx; return rc; };
    try {
        std::vector<int> devs(n_devices);
        for (int i = 0; i < n_devices; ++i) devs[i] = device_ids ? device_ids[i] : i;
        if (!g->peer_copy)                                                      // RCCL wants one rank per GPU
            for (int i = 0; i < n_devices; ++i)
                for (int j = 0; j < i; ++j)
                    if (devs[i] == devs[j])
                        return fail(CtxFail(nullptr, CGPT_ERR_INVALID, "device %d listed twice (only a CGPT_CTX_GATHER_PEER_COPY context may share a device between ranks)", devs[i]));
        g->members.reserve(n_devices);
        g->n_rows.assign(n_devices, 0);
        for (int i = 0; i < n_devices; ++i) {
            cgpt_ctx* m = nullptr;
            const int rc = cgpt_ctx_create(&devs[i], 1, 0, &m);                 // its failure text is the create error already
            if (rc != CGPT_OK) return fail(rc);
            g->members.push_back(m);
        }
        hipError_t e = hipSetDevice(g->members[0]->device);
        if (e == hipSuccess) e = g->ev_gather0.Create();
        if (e == hipSuccess) e = g->ev_gather1.Create();
        if (e != hipSuccess) return fail(CtxFail(nullptr, CGPT_ERR_HIP, "multi-device context events: %s", hipGetErrorString(e)));
        if (!g->peer_copy) {
            g->comms.assign(n_devices, nullptr);
            const ncclResult_t r = ncclCommInitAll(g->comms.data(), n_devices, devs.data());
            if (r != ncclSuccess) {
                g->comms.clear();
                return fail(CtxFail(nullptr, CGPT_ERR_HIP, "ncclCommInitAll over %d devices failed: %s", n_devices, ncclGetErrorString(r)));
            }
        }
        g->workers.Start((uint32_t)n_devices);
    } catch (const std::exception& e) {
        return fail(CtxFail(nullptr, CGPT_ERR_INVALID, "cgpt_ctx_create: %s", e.what()));
    }
    *out = ctx;
    return CGPT_OK;
}

void GroupDestroy(cgpt_ctx* ctx)
{
    DeviceGroup* g = ctx->group;
    if (!g) return;
    g->workers.Stop();
    for (cgpt_ctx* m : g->members) { (void)hipSetDevice(m->device); (void)hipStreamSynchronize(m->stream); }
    for (ncclComm_t c : g->comms) if (c) (void)ncclCommDestroy(c);
    std::vector<cgpt_ctx*> members;
    members.swap(g->members);
    if (!members.empty()) (void)hipSetDevice(members[0]->device);
    delete g;                                                                  // the gathered frame and its events, before the contexts they live on
    for (cgpt_ctx* m : members) (void)cgpt_ctx_destroy(m);
    ctx->group = nullptr;
}

int GroupSceneUpload(cgpt_ctx* ctx, const cgpt_scene_desc* scene, bool instanced)
{
    // laid out once (a refusal touches no member's scene), installed on every member in rank order as its cgpt_scene_upload would
    cgpt_ctx* first = ctx->group->members[0];
    if (!scene) return Propagate(ctx, first, CtxFail(first, CGPT_ERR_INVALID, "scene is null"));
    SceneLayout layout;
    int rc = LayoutScene(*scene, layout, first->error, instanced);
    if (rc != CGPT_OK) return Propagate(ctx, first, rc);
    for (cgpt_ctx* m : ctx->group->members) {
        if ((rc = cgpt_synchronize(m)) != CGPT_OK) return Propagate(ctx, m, rc);   // selects the member's device and drains its stream
        m->scene_generation++; m->shape_generation++;
        if ((rc = SceneInstall(m, layout)) != CGPT_OK) return Propagate(ctx, m, rc);
    }
    ctx->has_scene = true;
    return CGPT_OK;
}

int GroupUpdateMaterials(cgpt_ctx* ctx, const cgpt_material* materials, uint32_t n)
{
    for (cgpt_ctx* m : ctx->group->members) { const int rc = cgpt_scene_update_materials(m, materials, n); if (rc != CGPT_OK) return Propagate(ctx, m, rc); }
    return CGPT_OK;
}

// In-place scene edits run on every member.  A member validates before its first device write and all hold the same scene, so only the
// first member can refuse the call; any later failure (or a first member that dropped its scene) leaves the members with different
// geometry, and the whole group's scene is dropped: the next render returns CGPT_ERR_NO_SCENE.
template <class F>
int GroupEdit(cgpt_ctx* ctx, F&& edit)
{
    std::vector<cgpt_ctx*>& ms = ctx->group->members;
    for (size_t r = 0; r < ms.size(); ++r) {
        const int rc = edit(ms[r], r == 0);
        if (rc == CGPT_OK) continue;
        if (r > 0 || !ms[0]->has_scene) {
            for (cgpt_ctx* m : ms) m->has_scene = false;
            ctx->has_scene = false;
        }
        return Propagate(ctx, ms[r], rc);
    }
    return CGPT_OK;
}

int GroupRefitMesh(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_triangle* triangles, uint32_t n_tris, float* total_area_out)
{
    return GroupEdit(ctx, [&](cgpt_ctx* m, bool first) { return cgpt_scene_refit_mesh(m, obj_index, triangles, n_tris, first ? total_area_out : nullptr); });
}

int GroupUpdatePrimitive(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_object* obj)
{
    return GroupEdit(ctx, [&](cgpt_ctx* m, bool) { return cgpt_scene_update_primitive(m, obj_index, obj); });
}

// every member keeps its own skin buffers and poses its own copy
int GroupSetSkin(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_triangle* bind_triangles, const uint16_t* joints, const float* weights, uint32_t n_tris, uint32_t n_joints)
{
    return GroupEdit(ctx, [&](cgpt_ctx* m, bool) { return cgpt_scene_set_skin(m, obj_index, bind_triangles, joints, weights, n_tris, n_joints); });
}

int GroupSkinMesh(cgpt_ctx* ctx, uint32_t obj_index, const float* joint_matrices, uint32_t n_joints)
{
    return GroupEdit(ctx, [&](cgpt_ctx* m, bool) { return cgpt_scene_skin_mesh(m, obj_index, joint_matrices, n_joints); });
}

int GroupClearSkin(cgpt_ctx* ctx, uint32_t obj_index)
{
    return GroupEdit(ctx, [&](cgpt_ctx* m, bool) { return cgpt_scene_clear_skin(m, obj_index); });
}

// ... and its own morph targets
int GroupSetMorphTargets(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_triangle* base_triangles, const cgpt_triangle* target_deltas, uint32_t n_tris, uint32_t n_targets)
{
    return GroupEdit(ctx, [&](cgpt_ctx* m, bool) { return cgpt_scene_set_morph_targets(m, obj_index, base_triangles, target_deltas, n_tris, n_targets); });
}

int GroupMorphMesh(cgpt_ctx* ctx, uint32_t obj_index, const float* weights, uint32_t n_targets)
{
    return GroupEdit(ctx, [&](cgpt_ctx* m, bool) { return cgpt_scene_morph_mesh(m, obj_index, weights, n_targets); });
}

int GroupClearMorphTargets(cgpt_ctx* ctx, uint32_t obj_index)
{
    return GroupEdit(ctx, [&](cgpt_ctx* m, bool) { return cgpt_scene_clear_morph_targets(m, obj_index); });
}

// ... and a batch of poses: every member plans and runs it on its own copy
int GroupPoseObjects(cgpt_ctx* ctx, const cgpt_pose* poses, uint32_t n_poses)
{
    return GroupEdit(ctx, [&](cgpt_ctx* m, bool) { return cgpt_scene_pose_objects(m, poses, n_poses); });
}

// ... and a batch of animated poses: every member evaluates the matrices on its own device from its own copy of the clip and skeleton
int GroupSetSkeleton(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_skeleton_desc* skeleton)
{
    return GroupEdit(ctx, [&](cgpt_ctx* m, bool) { return cgpt_scene_set_skeleton(m, obj_index, skeleton); });
}

int GroupAnimateObjects(cgpt_ctx* ctx, const cgpt_animation* entries, uint32_t n_entries)
{
    return GroupEdit(ctx, [&](cgpt_ctx* m, bool) { return cgpt_scene_animate_objects(m, entries, n_entries); });
}

int GroupAnimateLayers(cgpt_ctx* ctx, const cgpt_layered_animation* entries, uint32_t n_entries)
{
    return GroupEdit(ctx, [&](cgpt_ctx* m, bool) { return cgpt_scene_animate_layers(m, entries, n_entries); });
}

// a clip is no part of the scene: every member holds a copy under the same handle (the members' handles advance in step), and a member
// that cannot take it leaves the others without it
int GroupClipCreate(cgpt_ctx* ctx, const cgpt_clip_desc* clip, uint32_t* clip_out)
{
    std::vector<cgpt_ctx*>& ms = ctx->group->members;
    uint32_t handle = 0;
    for (size_t r = 0; r < ms.size(); ++r) {
        uint32_t h = 0;
        int rc = cgpt_clip_create(ms[r], clip, &h);
        if (rc == CGPT_OK && r > 0 && h != handle) { (void)cgpt_clip_destroy(ms[r], h); rc = CtxFail(ms[r], CGPT_ERR_INVALID, "the members' clip handles differ (%u, %u)", handle, h); }
        if (rc != CGPT_OK) {
            for (size_t q = 0; q < r; ++q) (void)cgpt_clip_destroy(ms[q], handle);
            return Propagate(ctx, ms[r], rc);
        }
        handle = h;
    }
    if (clip_out) *clip_out = handle;
    return CGPT_OK;
}

int GroupClipDestroy(cgpt_ctx* ctx, uint32_t clip)
{
    for (cgpt_ctx* m : ctx->group->members) { const int rc = cgpt_clip_destroy(m, clip); if (rc != CGPT_OK) return Propagate(ctx, m, rc); }
    return CGPT_OK;
}

// every member rebuilds its own copy: the builder is deterministic, so the trees stay equal (the record names may differ, and are no one's business)
int GroupRebuildMesh(cgpt_ctx* ctx, uint32_t obj_index, uint32_t build_option, uint32_t* n_nodes_out, uint32_t* max_depth_out)
{
    return GroupEdit(ctx, [&](cgpt_ctx* m, bool first) { return cgpt_scene_rebuild_mesh(m, obj_index, build_option, first ? n_nodes_out : nullptr, first ? max_depth_out : nullptr); });
}

// every member sums its own copy and all must report the same bits (tree_cost.hip: the sums' order is fixed); the first member's are returned.
// A read: a refusal or a disagreement drops no scene
int GroupTreeCosts(cgpt_ctx* ctx, const uint32_t* obj_indices, uint32_t n, double c_inner, double c_tri, cgpt_tree_cost* out)
{
    std::vector<cgpt_ctx*>& ms = ctx->group->members;
    std::vector<cgpt_tree_cost> first(n), other(n);
    for (size_t r = 0; r < ms.size(); ++r) {
        const int rc = cgpt_scene_tree_costs(ms[r], obj_indices, n, c_inner, c_tri, n && out ? (r == 0 ? first.data() : other.data()) : out);
        if (rc != CGPT_OK) return Propagate(ctx, ms[r], rc);
        if (r > 0 && n && memcmp(first.data(), other.data(), sizeof(cgpt_tree_cost) * n) != 0)
            return Propagate(ctx, ms[r], CtxFail(ms[r], CGPT_ERR_HIP, "cgpt_scene_tree_costs: this device's costs differ from device %d's: the copies of the scene are no longer equal", ms[0]->device));
    }
    if (n && out) memcpy(out, first.data(), sizeof(cgpt_tree_cost) * n);
    return CGPT_OK;
}

int GroupUpdateRoughness(cgpt_ctx* ctx, const float* roughness, uint32_t n)
{
    return GroupEdit(ctx, [&](cgpt_ctx* m, bool) { return cgpt_scene_update_roughness(m, roughness, n); });
}

int GroupUpdateTransmissionRoughness(cgpt_ctx* ctx, const float* roughness, uint32_t n)
{
    return GroupEdit(ctx, [&](cgpt_ctx* m, bool) { return cgpt_scene_update_transmission_roughness(m, roughness, n); });
}

int GroupUpdateSmoothNormals(cgpt_ctx* ctx, const uint32_t* smooth, uint32_t n)
{
    return GroupEdit(ctx, [&](cgpt_ctx* m, bool) { return cgpt_scene_update_smooth_normals(m, smooth, n); });
}

int GroupUpdateTransforms(cgpt_ctx* ctx, const float* object_to_world, uint32_t n)
{
    return GroupEdit(ctx, [&](cgpt_ctx* m, bool) { return cgpt_scene_update_transforms(m, object_to_world, n); });
}

int GroupSetNeeCandidates(cgpt_ctx* ctx, uint32_t candidates)              // the range was checked: no member can refuse, none is left behind
{
    for (cgpt_ctx* m : ctx->group->members) { const int rc = cgpt_set_nee_candidates(m, candidates); if (rc != CGPT_OK) return Propagate(ctx, m, rc); }
    ctx->nee_candidates = candidates;
    return CGPT_OK;
}

int GroupSetTopLevel(cgpt_ctx* ctx, uint32_t mode)                          // the value was checked; a member fails only on a HIP error, which drops its scene
{
    for (cgpt_ctx* m : ctx->group->members) { const int rc = cgpt_set_top_level(m, mode); if (rc != CGPT_OK) return Propagate(ctx, m, rc); }
    ctx->top_level = mode;
    return CGPT_OK;
}

int GroupRender(cgpt_ctx* ctx, const cgpt_camera* camera, const cgpt_settings* settings, const cgpt_render_params* p)
{
    DeviceGroup* g = ctx->group;
    if (!camera || !settings || !p) return CtxFail(ctx, CGPT_ERR_INVALID, "null argument");
    if (p->row_begin != 0 || p->row_end != p->height || p->interleave_rows || p->interleave_count || p->interleave_index)
        return CtxFail(ctx, CGPT_ERR_INVALID, "a multi-device context tiles the image itself: pass row_begin = 0, row_end = height and no interleave");
    const uint32_t n = (uint32_t)g->members.size();
    if (p->height < n) return CtxFail(ctx, CGPT_ERR_INVALID, "image of %u rows is too small for %u devices", p->height, n);
    if (g->width != p->width || g->height != p->height || g->band_rows != EffectiveBandRows(g->band_rows_cfg, n, p->height)) SetTiling(g, p->width, p->height);
    g->gathered = false; g->pixels_valid = false;
    // Enqueue everywhere, then wait everywhere: the devices render side by side.  One host thread per device does the enqueueing
    // (the wavefront pipeline is ~60 launches per batch: enqueued one device after the other, the eighth GPU would start several
    // milliseconds after the first).
    EnqueueJob job{ g, camera, settings, p, { 0 } };
    g->workers.Run(EnqueueRank, &job);
    int first_error = CGPT_OK;
    for (uint32_t r = 0; r < n; ++r)
        if (job.rcs[r] != CGPT_OK && first_error == CGPT_OK) first_error = Propagate(ctx, g->members[r], job.rcs[r]);
    for (uint32_t r = 0; r < n; ++r) {                                         // also after a failed enqueue elsewhere: nothing stays pending
        const int rc = RenderFinish(g->members[r]);
        if (rc != CGPT_OK && first_error == CGPT_OK) first_error = Propagate(ctx, g->members[r], rc);
    }
    if (first_error != CGPT_OK) return first_error;
    g->num_accumulated = p->n_samples ? p->first_sample + p->n_samples : g->num_accumulated;
    g->last_debug_mode = settings->debug_render_mode;
    g->last_kernel = g->members[0]->last_kernel;
    return CGPT_OK;
}

int GroupResetAccumulator(cgpt_ctx* ctx)
{
    for (cgpt_ctx* m : ctx->group->members) { const int rc = cgpt_reset_accumulator(m); if (rc != CGPT_OK) return Propagate(ctx, m, rc); }
    ctx->group->num_accumulated = 0; ctx->group->gathered = false;
    return CGPT_OK;
}

int GroupReadAccumulator(cgpt_ctx* ctx, float* dst, size_t n_floats)
{
    DeviceGroup* g = ctx->group;
    const size_t n = (size_t)g->width * g->height * 4;
    if (g->width == 0) return CtxFail(ctx, CGPT_ERR_INVALID, "nothing rendered yet");
    if (!dst || n_floats != n) return CtxFail(ctx, CGPT_ERR_INVALID, "expected a buffer of %zu floats", n);
    const int rc = Gather(ctx, false);
    if (rc != CGPT_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(g->members[0]->device));
    HIP_TRY(ctx, hipMemcpy(dst, g->full.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return CGPT_OK;
}

int GroupReadPixels(cgpt_ctx* ctx, uint32_t* dst, size_t n_pixels)
{
    DeviceGroup* g = ctx->group;
    const size_t n = (size_t)g->width * g->height;
    if (g->width == 0) return CtxFail(ctx, CGPT_ERR_INVALID, "nothing rendered yet");
    if (!dst || n_pixels != n) return CtxFail(ctx, CGPT_ERR_INVALID, "expected a buffer of %zu pixels", n);
    // data.pixels = Vec4ToUint(accumulator / num_accumulated) (ref: Main.cpp:741): packed on device 0 from the gathered sums, so the
    // float4 framebuffer is the only thing that crosses xGMI; the debug views' pixels are not a function of the sums and are gathered
    const bool debug = g->last_debug_mode != 0u;
    const int rc = Gather(ctx, debug);
    if (rc != CGPT_OK) return rc;
    cgpt_ctx* root = g->members[0];
    HIP_TRY(ctx, hipSetDevice(root->device));
    if (!debug) {
        HIP_TRY(ctx, LaunchPackPixels(g->full.p, g->full_pixels.p, n, g->num_accumulated, root->stream));
        HIP_TRY(ctx, hipStreamSynchronize(root->stream));
    }
    HIP_TRY(ctx, hipMemcpy(dst, g->full_pixels.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return CGPT_OK;
}

void GroupFrameInfo(cgpt_ctx* ctx, uint32_t* width, uint32_t* height, uint32_t* num_accumulated, uint32_t* last_debug_mode)
{
    const DeviceGroup* g = ctx->group;
    *width = g->width; *height = g->height; *num_accumulated = g->num_accumulated; *last_debug_mode = g->last_debug_mode;
}

// cgpt_denoise reads the frame without being a read-back: cgpt_stats (gathers, gather_ms) does not grow, and a frame that was not
// gathered before counts as not gathered afterwards, so the next read-back gathers and counts as it would have without this call
int GroupGatherUncounted(cgpt_ctx* ctx, const float4** frame)
{
    DeviceGroup* g = ctx->group;
    const bool gathered = g->gathered, pixels_valid = g->pixels_valid;
    const uint32_t gathers = g->gathers;
    const double gather_ms = g->gather_ms;
    const int rc = Gather(ctx, false);
    g->gathers = gathers; g->gather_ms = gather_ms;
    if (rc != CGPT_OK) { g->gathered = false; g->pixels_valid = false; return rc; }
    g->gathered = gathered; g->pixels_valid = gathered && pixels_valid;
    *frame = g->full.p;
    return CGPT_OK;
}

int GroupWriteAccumulator(cgpt_ctx* ctx, const cgpt_render_params* p, const float* src, size_t n_floats, uint32_t num_accumulated)
{
    DeviceGroup* g = ctx->group;
    if (!p || !src) return CtxFail(ctx, CGPT_ERR_INVALID, "null argument");
    if (p->row_begin != 0 || p->row_end != p->height || p->interleave_rows || p->interleave_count || p->interleave_index || p->width == 0 || p->height == 0)
        return CtxFail(ctx, CGPT_ERR_INVALID, "a multi-device context restores whole frames: pass row_begin = 0, row_end = height and no interleave");
    if (n_floats != (size_t)p->width * p->height * 4) return CtxFail(ctx, CGPT_ERR_INVALID, "expected %zu floats", (size_t)p->width * p->height * 4);
    const uint32_t n = (uint32_t)g->members.size();
    if (p->height < n) return CtxFail(ctx, CGPT_ERR_INVALID, "image of %u rows is too small for %u devices", p->height, n);
    SetTiling(g, p->width, p->height);
    const uint32_t band_rows = g->band_rows;
    std::vector<float> band;
    for (uint32_t r = 0; r < n; ++r) {
        band.resize((size_t)g->n_rows[r] * p->width * 4);
        size_t out_row = 0;
        for (uint64_t first = (uint64_t)r * band_rows; first < p->height; first += (uint64_t)n * band_rows)
            for (uint32_t j = 0; j < band_rows && first + j < p->height; ++j, ++out_row)
                memcpy(band.data() + out_row * p->width * 4, src + (first + j) * (size_t)p->width * 4, (size_t)p->width * 16);
        cgpt_render_params q = *p;
        q.interleave_rows = band_rows; q.interleave_count = n; q.interleave_index = r;
        const int rc = cgpt_write_accumulator(g->members[r], &q, band.data(), band.size(), num_accumulated);
        if (rc != CGPT_OK) return Propagate(ctx, g->members[r], rc);
    }
    g->num_accumulated = num_accumulated; g->last_debug_mode = 0; g->gathered = false; g->pixels_valid = false;
    return CGPT_OK;
}

int GroupDevicePtr(cgpt_ctx* ctx, bool pixels, void** ptr, size_t* n_bytes)
{
    DeviceGroup* g = ctx->group;
    int rc = Gather(ctx, pixels && g->last_debug_mode != 0u);
    if (rc != CGPT_OK) return rc;
    const size_t n = (size_t)g->width * g->height;
    if (pixels && g->last_debug_mode == 0u) {
        cgpt_ctx* root = g->members[0];
        HIP_TRY(ctx, hipSetDevice(root->device));
        HIP_TRY(ctx, LaunchPackPixels(g->full.p, g->full_pixels.p, n, g->num_accumulated, root->stream));
        HIP_TRY(ctx, hipStreamSynchronize(root->stream));
    }
    *ptr = pixels ? (void*)g->full_pixels.p : (void*)g->full.p;               // on device_ids[0]
    *n_bytes = n * (pixels ? sizeof(uint32_t) : sizeof(float4));
    return CGPT_OK;
}

int GroupGetStats(cgpt_ctx* ctx, cgpt_stats* out)
{
    DeviceGroup* g = ctx->group;
    memset(out, 0, sizeof(*out));
    uint32_t r = 0;
    for (cgpt_ctx* m : g->members) {
        cgpt_stats s;
        const int rc = cgpt_get_stats(m, &s);
        if (rc != CGPT_OK) return Propagate(ctx, m, rc);
        out->traced_rays += s.traced_rays; out->inner_steps += s.inner_steps; out->tri_tests += s.tri_tests;
        out->bvh_depth_sum += s.bvh_depth_sum; out->closest_hits += s.closest_hits; out->total_energy_received += s.total_energy_received;
        out->kernel_launches += s.kernel_launches;
        out->kernel_ms = std::max(out->kernel_ms, s.kernel_ms);                // the devices run side by side: the frame takes as long as the slowest
        out->dominant_launches += s.dominant_launches; out->dominant_ms += s.dominant_ms;
        out->dominant_waves_per_simd = s.dominant_waves_per_simd;
        out->dominant_round0_ms += s.dominant_round0_ms; out->dominant_round0_launches += s.dominant_round0_launches;
        out->chain_followers = (uint32_t)std::min<uint64_t>(0xFFFFFFFFull, (uint64_t)out->chain_followers + s.chain_followers);
        out->probe_resolved += s.probe_resolved;
        out->device_ms[r++] = s.kernel_ms;
    }
    out->num_accumulated = g->num_accumulated;
    out->gather_ms = g->gather_ms; out->gathers = g->gathers;
    out->n_devices = (uint32_t)g->members.size(); out->rccl_ranks = (uint32_t)g->comms.size();
    out->last_kernel = g->last_kernel;
    return CGPT_OK;
}

int GroupGetRetraceUnwalked(cgpt_ctx* ctx, uint64_t* out)
{
    *out = 0;
    for (cgpt_ctx* m : ctx->group->members) {
        uint64_t v = 0;
        const int rc = cgpt_get_retrace_unwalked(m, &v);
        if (rc != CGPT_OK) return Propagate(ctx, m, rc);
        *out += v;
    }
    return CGPT_OK;
}

int GroupResetStats(cgpt_ctx* ctx)
{
    for (cgpt_ctx* m : ctx->group->members) { const int rc = cgpt_reset_stats(m); if (rc != CGPT_OK) return Propagate(ctx, m, rc); }
    ctx->group->gather_ms = 0.0; ctx->group->gathers = 0;
    return CGPT_OK;
}

int GroupSetTuning(cgpt_ctx* ctx, const char* name, uint32_t value)
{
    DeviceGroup* g = ctx->group;
    if (name && strcmp(name, "band_rows") == 0) {
        if (value == 0 || value > 1024) return CtxFail(ctx, CGPT_ERR_INVALID, "band_rows %u outside [1, 1024]", value);
        if (value == g->band_rows_cfg) return CGPT_OK;
        const uint32_t n = (uint32_t)g->members.size();
        if (g->width == 0 || EffectiveBandRows(value, n, g->height) == g->band_rows) { g->band_rows_cfg = value; return CGPT_OK; }   // nothing to move
        // A frame is being accumulated under the old tiling: results never depend on a knob, so the sums move with the tiling --
        // gathered under the old bands, scattered under the new ones (the checkpoint path); data.pixels is re-packed from them.
        std::vector<float> frame((size_t)g->width * g->height * 4);
        int rc = GroupReadAccumulator(ctx, frame.data(), frame.size());
        if (rc != CGPT_OK) return rc;
        const uint32_t old_cfg = g->band_rows_cfg;
        g->band_rows_cfg = value;
        cgpt_render_params p{};
        p.width = g->width; p.height = g->height; p.row_begin = 0; p.row_end = g->height;
        rc = GroupWriteAccumulator(ctx, &p, frame.data(), frame.size(), g->num_accumulated);
        if (rc != CGPT_OK) g->band_rows_cfg = old_cfg;
        return rc;
    }
    for (cgpt_ctx* m : g->members) { const int rc = cgpt_set_tuning(m, name, value); if (rc != CGPT_OK) return Propagate(ctx, m, rc); }
    return CGPT_OK;
}

int GroupSynchronize(cgpt_ctx* ctx)
{
    for (cgpt_ctx* m : ctx->group->members) { const int rc = cgpt_synchronize(m); if (rc != CGPT_OK) return Propagate(ctx, m, rc); }
    return CGPT_OK;
}

}  // namespace cgpt
