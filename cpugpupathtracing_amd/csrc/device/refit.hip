// refit.hip -- in-place edits of an uploaded scene: new triangle positions for a mesh with its tree kept (a BVH refit), the tree
// read back, and new sphere / plane parameters.  No render kernel changes: they read the edited arrays as they read an upload.
//
// Refit contract (tests/test_host_refit.py, tests/test_gpu_refit.py; host statement: MeshBVH::Refit): the tree keeps its nodes,
// left_first / prim_count and tri_indices; every node's bounds become BVH::CalculateNodeBounds (ref: BVH.cpp:188-202) over its
// CURRENT leaf-order range of the new triangles -- 1e30 / -1e30 folded with TriangleBounds (ref: Primitives.cpp:232-243) in range
// order by std::min / std::max.  For an inner node that equals min_std(left, right) / max_std(left, right) of its children in every
// bit (signed zeros, NaN, values beyond 1e30 included): the left range comes first and a tie keeps the first operand.  So:
//   * triangle pass (refit_triangles): one thread per leaf slot of the object.  Its tri_leaf record names the triangle (tri_idx),
//     which the thread gathers from the staging copy of the host triangles; it rewrites v0 / e1 / e2 (scene_layout.h: PackLeafTri's subtraction),
//     keeps tri_idx, last_in_leaf and the pad word, and writes the original-order record (tri_orig) and tri_normal (n0 and the {n1, n2} pair);
//   * bound pass (refit_level): the object's child-pair records grouped by depth at upload (scene_layout.hip: LayoutScene), one launch per level,
//     deepest first, a thread per record.  A leaf side folds its triangles' positions from tri_orig (v0 + e1 is not v1 in floating
//     point); an inner side is the union of the child record's two sides, written by the previous launch (stream order is the only
//     synchronisation).  The codes float4 is not written.
// total_area is the sequential float sum of GetTriangleArea in original order (ref: BVH.cpp:22), summed on the host while the input is
// read, and written into the object's DevObject (mesh-light sampling reads it).
// After cgpt_scene_upload_instanced the objects of a mesh group share the one copy these passes edit: the refit goes through any member's
// RefitObject (they are equal), and the area and the top-level box, which are per object, are written for every member.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <exception>
#include <vector>

#include "cpugpupt_abi.h"
#include "ctx_internal.h"
#include "device_scene.h"
#include "minmax_std.h"
#include "scene_layout.h"

namespace cgpt {

float HostTriangleArea(const cgpt_triangle& t);                               // bvh_build.hip

namespace {

constexpr uint32_t kRefitThreads = 256;

__global__ __launch_bounds__(kRefitThreads) void refit_triangles(const float* __restrict__ staging, float4* __restrict__ tri_leaf,
                                                                 float4* __restrict__ tri_orig, float4* __restrict__ tri_normal,
                                                                 uint32_t leaf_base, uint32_t tri_base, uint32_t n, uint32_t n_tris_total)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4* leaf = tri_leaf + 3 * (size_t)(leaf_base + i);
    const float4 keep = leaf[2];                                              // {pad, e2.z, tri_idx, last_in_leaf}
    const uint32_t t = __float_as_uint(keep.z);
    if (t >= n) return;                                                       // validated at upload
    const float* tr = staging + 18 * (size_t)t;                               // cgpt_triangle: v0 {pos, normal}, v1, v2 (72 B, 8-byte aligned)
    const float p0x = tr[0], p0y = tr[1], p0z = tr[2], n0x = tr[3], n0y = tr[4], n0z = tr[5];
    const float p1x = tr[6], p1y = tr[7], p1z = tr[8], n1x = tr[9], n1y = tr[10], n1z = tr[11];
    const float p2x = tr[12], p2y = tr[13], p2z = tr[14], n2x = tr[15], n2y = tr[16], n2z = tr[17];
    const float e1x = p1x - p0x, e1y = p1y - p0y, e1z = p1z - p0z;            // ref: Primitives.cpp:9 (PackLeafTri)
    const float e2x = p2x - p0x, e2y = p2y - p0y, e2z = p2z - p0z;            // ref: Primitives.cpp:10
    leaf[0] = make_float4(p0x, p0y, p0z, e1x);
    leaf[1] = make_float4(e1y, e1z, e2x, e2y);
    leaf[2] = make_float4(keep.x, e2z, keep.z, keep.w);
    float4* orig = tri_orig + 3 * (size_t)(tri_base + t);                     // PackOrigTri
    orig[0] = make_float4(p0x, p0y, p0z, n0x);
    orig[1] = make_float4(p1x, p1y, p1z, n0y);
    orig[2] = make_float4(p2x, p2y, p2z, n0z);
    tri_normal[tri_base + t] = make_float4(n0x, n0y, n0z, 0.0f);              // TriangleNormal, ref: Primitives.cpp:148-151
    float4* pair = tri_normal + n_tris_total + 2 * (size_t)(tri_base + t);    // PackNormalPair (device_scene.h: tri_normal)
    pair[0] = make_float4(n1x, n1y, n1z, 0.0f);
    pair[1] = make_float4(n2x, n2y, n2z, 0.0f);
}

struct Box { float lo[3], hi[3]; };

// CalculateNodeBounds of a leaf (ref: BVH.cpp:188-202): its slots in order, each triangle's TriangleBounds (v0, then v1, then v2)
__device__ inline Box fold_leaf(const float4* __restrict__ tri_leaf, const float4* __restrict__ tri_orig, uint32_t tri_base, uint32_t slot)
{
    Box b;
    for (int k = 0; k < 3; ++k) { b.lo[k] = 1e30f; b.hi[k] = -1e30f; }
    for (;;) {
        const float4 r2 = tri_leaf[3 * (size_t)slot + 2];
        const float4* o = tri_orig + 3 * (size_t)(tri_base + __float_as_uint(r2.z));
        const float4 a = o[0], c = o[1], e = o[2];
        b.lo[0] = min_std(b.lo[0], min_std(min_std(a.x, c.x), e.x)); b.hi[0] = max_std(b.hi[0], max_std(max_std(a.x, c.x), e.x));
        b.lo[1] = min_std(b.lo[1], min_std(min_std(a.y, c.y), e.y)); b.hi[1] = max_std(b.hi[1], max_std(max_std(a.y, c.y), e.y));
        b.lo[2] = min_std(b.lo[2], min_std(min_std(a.z, c.z), e.z)); b.hi[2] = max_std(b.hi[2], max_std(max_std(a.z, c.z), e.z));
        if (__float_as_uint(r2.w) != 0u) break;                               // last_in_leaf
        ++slot;
    }
    return b;
}

__device__ inline Box side_bounds(const float4* __restrict__ node_pairs, const float4* __restrict__ tri_leaf, const float4* __restrict__ tri_orig,
                                  uint32_t tri_base, uint32_t code)
{
    if (code & kLeafBit) return fold_leaf(tri_leaf, tri_orig, tri_base, code & ~kLeafBit);
    const float4* c = node_pairs + 4 * (size_t)code;                          // the child's record, refitted by the previous launch
    const float4 q0 = c[0], q1 = c[1], q2 = c[2];
    Box b;
    b.lo[0] = min_std(q0.x, q0.y); b.lo[1] = min_std(q0.z, q0.w); b.lo[2] = min_std(q1.x, q1.y);
    b.hi[0] = max_std(q1.z, q1.w); b.hi[1] = max_std(q2.x, q2.y); b.hi[2] = max_std(q2.z, q2.w);
    return b;
}

__global__ __launch_bounds__(kRefitThreads) void refit_level(float4* node_pairs, const float4* __restrict__ tri_leaf, const float4* __restrict__ tri_orig,
                                                             const uint32_t* __restrict__ records, uint32_t n, uint32_t tri_base)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4* rec = node_pairs + 4 * (size_t)records[i];
    const float4 codes = rec[3];
    const Box l = side_bounds(node_pairs, tri_leaf, tri_orig, tri_base, __float_as_uint(codes.z));
    const Box r = side_bounds(node_pairs, tri_leaf, tri_orig, tri_base, __float_as_uint(codes.w));
    rec[0] = make_float4(l.lo[0], r.lo[0], l.lo[1], r.lo[1]);                 // device_scene.h: node_pairs
    rec[1] = make_float4(l.lo[2], r.lo[2], l.hi[0], r.hi[0]);
    rec[2] = make_float4(l.hi[1], r.hi[1], l.hi[2], r.hi[2]);
}

const char* KindName(uint32_t kind)
{
    return kind == CGPT_OBJECT_MESH ? "mesh" : kind == CGPT_OBJECT_SPHERE ? "sphere" : kind == CGPT_OBJECT_PLANE ? "plane" : "triangle object";
}

int CheckObject(cgpt_ctx* ctx, uint32_t obj_index)
{
    if (!ctx->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "no scene uploaded");
    if (obj_index >= ctx->h_objects.size()) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u out of range (%zu objects)", obj_index, ctx->h_objects.size());
    return CGPT_OK;
}

// a HIP call failed after the device scene began to change: drop the scene rather than render a half-edited one
int SceneLost(cgpt_ctx* ctx, const char* what, hipError_t e)
{
    ctx->has_scene = false;
    return CtxFail(ctx, CGPT_ERR_HIP, "%s failed: %s (the device scene is dropped; upload it again)", what, hipGetErrorString(e));
}

// HIP_TRY once the device scene has begun to change
#define REFIT_HIP_WRITING(ctx, expr)                                                                                    \
    do {                                                                                                                \
        hipError_t e_ = (expr);                                                                                         \
        if (e_ != hipSuccess) return SceneLost((ctx), #expr, e_);                                                       \
    } while (0)

int RefitMesh(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_triangle* triangles, uint32_t n_tris, float* total_area_out)
{
    int rc = CheckObject(ctx, obj_index);
    if (rc != CGPT_OK) return rc;
    DevObject& d = ctx->h_objects[obj_index];
    const RefitObject& ro = ctx->refit_objects[obj_index];
    if (d.kind != CGPT_OBJECT_MESH && d.kind != CGPT_OBJECT_TRIANGLE)
        return CtxFail(ctx, CGPT_ERR_INVALID, "object %u is a %s: it has no triangles (cgpt_scene_update_primitive edits it)", obj_index, KindName(d.kind));
    if (!triangles) return CtxFail(ctx, CGPT_ERR_INVALID, "triangles is null");
    if (n_tris != ro.tri_count) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u has %u triangles, got %u (a refit keeps the topology)", obj_index, ro.tri_count, n_tris);

    // BVH::m_total_area (ref: BVH.cpp:22): a sequential sum in original order.  A triangle object has none (it cannot be a light).
    float area = 0.0f;
    if (d.kind == CGPT_OBJECT_MESH)
        for (uint32_t i = 0; i < n_tris; ++i) area += HostTriangleArea(triangles[i]);

    // the top-level tree's box of this object: the min / max of the new vertex positions, which is what the refit's root bounds come to;
    // every object of its mesh group moves with it (ctx->mesh_group: obj_index alone after a plain upload)
    TopLevelState top = ctx->top_state;
    std::vector<uint32_t> members;
    for (uint32_t j = 0; j < ctx->mesh_group.size(); ++j)
        if (ctx->mesh_group[j] == ctx->mesh_group[obj_index]) members.push_back(j);
    TriangleBounds(triangles, n_tris, top.local_box.data() + 6 * (size_t)obj_index);
    for (const uint32_t j : members)
        if (j != obj_index) memcpy(top.local_box.data() + 6 * (size_t)j, top.local_box.data() + 6 * (size_t)obj_index, 24);

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, ctx->sb.refit_staging.Grow(n_tris));                          // the stream was just drained: nothing uses the old one
    HIP_TRY(ctx, hipMemcpyAsync(ctx->sb.refit_staging.p, triangles, sizeof(cgpt_triangle) * (size_t)n_tris, hipMemcpyHostToDevice, ctx->stream));

    // from here on the scene changes
    const uint32_t tri_base = d.tri_base;
    hipLaunchKernelGGL(refit_triangles, dim3((n_tris + kRefitThreads - 1) / kRefitThreads), dim3(kRefitThreads), 0, ctx->stream,
                       reinterpret_cast<const float*>(ctx->sb.refit_staging.p), ctx->sb.tri_leaf.p, ctx->sb.tri_orig.p, ctx->sb.tri_normal.p, ro.leaf_base, tri_base, n_tris, ctx->scene.n_tris_total);
    REFIT_HIP_WRITING(ctx, hipGetLastError());
    for (size_t level = ro.level_offsets.empty() ? 0 : ro.level_offsets.size() - 1; level-- > 0;) {
        const uint32_t first = ro.level_offsets[level], n = ro.level_offsets[level + 1] - first;
        if (n == 0) continue;
        hipLaunchKernelGGL(refit_level, dim3((n + kRefitThreads - 1) / kRefitThreads), dim3(kRefitThreads), 0, ctx->stream,
                           ctx->sb.node_pairs.p, ctx->sb.tri_leaf.p, ctx->sb.tri_orig.p, ctx->sb.refit_levels.p + ro.level_begin + first, n, tri_base);
        REFIT_HIP_WRITING(ctx, hipGetLastError());
    }
    if (d.kind == CGPT_OBJECT_MESH) {
        for (const uint32_t j : members) {
            ctx->h_objects[j].total_area = area;
            REFIT_HIP_WRITING(ctx, hipMemcpyAsync(&ctx->sb.objects.p[j].total_area, &ctx->h_objects[j].total_area, sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        }
    }
    REFIT_HIP_WRITING(ctx, hipStreamSynchronize(ctx->stream));
    REFIT_HIP_WRITING(ctx, WriteTopLevel(ctx, ctx->h_objects, top));
    ctx->top_state.local_box.swap(top.local_box);
    if (total_area_out) *total_area_out = area;
    return CGPT_OK;
}

int ExportBvh(cgpt_ctx* ctx, uint32_t obj_index, cgpt_bvh_node* nodes_out, uint32_t n_nodes)
{
    int rc = CheckObject(ctx, obj_index);
    if (rc != CGPT_OK) return rc;
    const DevObject& d = ctx->h_objects[obj_index];
    const RefitObject& ro = ctx->refit_objects[obj_index];
    if (d.kind != CGPT_OBJECT_MESH) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u is a %s: it has no BVH", obj_index, KindName(d.kind));
    if (!nodes_out) return CtxFail(ctx, CGPT_ERR_INVALID, "nodes_out is null");
    if (n_nodes != ro.node_count) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u has %u nodes, got room for %u", obj_index, ro.node_count, n_nodes);
    const uint32_t n_pairs = ro.node_count / 2, n_tris = ro.tri_count;

    // where the records are now: the renumbering put the top ones at the front, the rest keep their depth-first order
    std::vector<uint32_t> stored(n_pairs);
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    for (uint32_t k = 0; k < n_pairs; ++k) {
        const uint32_t r = ro.pair_base + k;
        stored[k] = ctx->record_perm[r];
        lo = std::min(lo, stored[k]); hi = std::max(hi, stored[k]);
    }
    std::vector<float4> span(n_pairs ? 4 * (size_t)(hi - lo + 1) : 0);
    std::vector<float4> leaf_tail(n_tris);                                    // {pad, e2.z, tri_idx, last_in_leaf} of every leaf slot
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (n_pairs) HIP_TRY(ctx, hipMemcpy(span.data(), ctx->sb.node_pairs.p + 4 * (size_t)lo, span.size() * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy2D(leaf_tail.data(), sizeof(float4), ctx->sb.tri_leaf.p + 3 * (size_t)ro.leaf_base + 2, 3 * sizeof(float4),
                               sizeof(float4), n_tris, hipMemcpyDeviceToHost));

    std::vector<uint32_t> pair_of(n_pairs ? hi - lo + 1 : 0, 0xFFFFFFFFu);    // stored record -> depth-first pair index k (nodes 2k+1, 2k+2)
    for (uint32_t k = 0; k < n_pairs; ++k) pair_of[stored[k] - lo] = k;
    auto bits = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
    auto words = [&](uint32_t code, cgpt_bvh_node& out) -> bool {            // {left_first, prim_count} behind a traversal code
        if (code & kLeafBit) {
            const uint32_t first = (code & ~kLeafBit) - ro.leaf_base;
            if (first >= n_tris) return false;
            uint32_t last = first;
            while (bits(leaf_tail[last].w) == 0u) if (++last >= n_tris) return false;
            out.left_first = first; out.prim_count = last - first + 1;
            return true;
        }
        if (code < lo || code > hi || pair_of[code - lo] == 0xFFFFFFFFu) return false;
        out.left_first = 2 * pair_of[code - lo] + 1; out.prim_count = 0;
        return true;
    };
    auto set_bounds = [](cgpt_bvh_node& n, float x0, float y0, float z0, float x1, float y1, float z1) {
        n.aabb_min[0] = x0; n.aabb_min[1] = y0; n.aabb_min[2] = z0; n.aabb_max[0] = x1; n.aabb_max[1] = y1; n.aabb_max[2] = z1;
    };
    for (uint32_t k = 0; k < n_pairs; ++k) {
        const float4* rec = span.data() + 4 * (size_t)(stored[k] - lo);
        cgpt_bvh_node& l = nodes_out[2 * k + 1];
        cgpt_bvh_node& r = nodes_out[2 * k + 2];
        set_bounds(l, rec[0].x, rec[0].z, rec[1].x, rec[1].z, rec[2].x, rec[2].z);
        set_bounds(r, rec[0].y, rec[0].w, rec[1].y, rec[1].w, rec[2].y, rec[2].w);
        if (!words(bits(rec[3].z), l) || !words(bits(rec[3].w), r)) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u: record of nodes %u, %u is malformed", obj_index, 2 * k + 1, 2 * k + 2);
    }
    cgpt_bvh_node& root = nodes_out[0];
    if (!words(d.root_code, root)) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u: malformed root", obj_index);
    if (d.root_code & kLeafBit) {                                             // a leaf-rooted mesh: CalculateNodeBounds over every slot
        std::vector<float4> orig(3 * (size_t)n_tris);
        HIP_TRY(ctx, hipMemcpy(orig.data(), ctx->sb.tri_orig.p + 3 * (size_t)d.tri_base, orig.size() * sizeof(float4), hipMemcpyDeviceToHost));
        float b[6] = { 1e30f, 1e30f, 1e30f, -1e30f, -1e30f, -1e30f };
        for (uint32_t s = 0; s < n_tris; ++s) {
            const uint32_t t = bits(leaf_tail[s].z);
            if (t >= n_tris) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u: leaf slot %u names triangle %u", obj_index, s, t);
            const float4 a = orig[3 * (size_t)t], c = orig[3 * (size_t)t + 1], e = orig[3 * (size_t)t + 2];
            b[0] = min_std(b[0], min_std(min_std(a.x, c.x), e.x)); b[3] = max_std(b[3], max_std(max_std(a.x, c.x), e.x));
            b[1] = min_std(b[1], min_std(min_std(a.y, c.y), e.y)); b[4] = max_std(b[4], max_std(max_std(a.y, c.y), e.y));
            b[2] = min_std(b[2], min_std(min_std(a.z, c.z), e.z)); b[5] = max_std(b[5], max_std(max_std(a.z, c.z), e.z));
        }
        set_bounds(root, b[0], b[1], b[2], b[3], b[4], b[5]);
    } else {                                                                  // the union of the root record's two sides
        const float4* rec = span.data() + 4 * (size_t)(d.root_code - lo);
        set_bounds(root, min_std(rec[0].x, rec[0].y), min_std(rec[0].z, rec[0].w), min_std(rec[1].x, rec[1].y),
                   max_std(rec[1].z, rec[1].w), max_std(rec[2].x, rec[2].y), max_std(rec[2].z, rec[2].w));
    }
    return CGPT_OK;
}

int UpdatePrimitive(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_object* obj)
{
    int rc = CheckObject(ctx, obj_index);
    if (rc != CGPT_OK) return rc;
    DevObject& d = ctx->h_objects[obj_index];
    if (!obj) return CtxFail(ctx, CGPT_ERR_INVALID, "obj is null");
    if (d.kind != CGPT_OBJECT_SPHERE && d.kind != CGPT_OBJECT_PLANE)
        return CtxFail(ctx, CGPT_ERR_INVALID, "object %u is a %s: cgpt_scene_refit_mesh edits it", obj_index, KindName(d.kind));
    if (obj->kind != d.kind) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u is a %s, got kind %u", obj_index, KindName(d.kind), obj->kind);
    if (obj->mat_index != d.mat_index) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u has material %u, got %u (materials are not changed here)", obj_index, d.mat_index, obj->mat_index);
    DevObject nd = d;
    if (d.kind == CGPT_OBJECT_SPHERE) {
        memcpy(nd.sphere_center, obj->sphere_center, 12);
        nd.sphere_radius = obj->sphere_radius;
        nd.sphere_radius_sq = obj->sphere_radius * obj->sphere_radius;        // Sphere ctor, ref: Primitives.h:38-39 (as at upload)
    } else {
        memcpy(nd.plane_normal, obj->plane_normal, 12);
        memcpy(nd.plane_point, obj->plane_point, 12);
    }
    float4 q[2];
    PackObjTrace(nd, q[0], q[1]);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    REFIT_HIP_WRITING(ctx, hipMemcpyAsync(ctx->sb.objects.p + obj_index, &nd, sizeof(DevObject), hipMemcpyHostToDevice, ctx->stream));
    REFIT_HIP_WRITING(ctx, hipMemcpyAsync(ctx->sb.obj_trace.p + 2 * (size_t)obj_index, q, sizeof(q), hipMemcpyHostToDevice, ctx->stream));
    REFIT_HIP_WRITING(ctx, hipStreamSynchronize(ctx->stream));
    d = nd;
    REFIT_HIP_WRITING(ctx, WriteTopLevel(ctx, ctx->h_objects, ctx->top_state));   // a sphere's or plane's box is read from its DevObject
    return CGPT_OK;
}

}  // namespace
}  // namespace cgpt

using namespace cgpt;

extern "C" {

int cgpt_scene_refit_mesh(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_triangle* triangles, uint32_t n_tris, float* total_area_out)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupRefitMesh(ctx, obj_index, triangles, n_tris, total_area_out); });
    ctx->scene_generation++; ctx->shape_generation++;                          // the denoiser's guides are stale (denoise.hip)
    return Guarded(ctx, __func__, [&] { return RefitMesh(ctx, obj_index, triangles, n_tris, total_area_out); });
}

int cgpt_scene_export_bvh(cgpt_ctx* ctx, uint32_t obj_index, cgpt_bvh_node* nodes_out, uint32_t n_nodes)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return GroupForwarded(ctx, cgpt_scene_export_bvh(GroupFirstMember(ctx), obj_index, nodes_out, n_nodes));
    return Guarded(ctx, __func__, [&] { return ExportBvh(ctx, obj_index, nodes_out, n_nodes); });
}

int cgpt_scene_update_primitive(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_object* obj)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupUpdatePrimitive(ctx, obj_index, obj); });
    ctx->scene_generation++; ctx->shape_generation++;
    return Guarded(ctx, __func__, [&] { return UpdatePrimitive(ctx, obj_index, obj); });
}

}  // extern "C"
