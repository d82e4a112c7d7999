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
// Skinning (cgpt_scene_set_skin / cgpt_scene_skin_mesh): the same refit with the triangle pass fed from a bind pose, joint
// indices and weights that stay on the device (skin_triangles poses each triangle by the arithmetic of csrc/host/skinning.h and writes the
// records through the function refit_triangles writes them with), then the same bound pass.  No staging copy and no per-triangle host work:
// the top-level box comes back from the refitted root record (or a one-block fold), and total_area is left as uploaded.  A skin remembers
// the matrices of its last pose on the host (SkinBuffers::pose): what a temporal call with CGPT_TEMPORAL_FOLLOW_POSES compares (denoise.hip).
// Morph targets (cgpt_scene_set_morph_targets / cgpt_scene_morph_mesh): the base triangles and the targets' displacements
// stay on the device too, in leaf-slot order; morph_triangles blends them by the arithmetic of csrc/host/morph.h and, for an object that also
// has a posed skin, hands each morphed corner to SkinCorner in registers.  Either call poses through PoseObject.
// Many objects in one call (cgpt_scene_pose_objects): the same poses for any number of objects with launches that do not
// grow with their count -- pose_plan.h plans the batch on the host, PoseObjects runs it through batched shells of the kernels above.
// Animation clips (cgpt_scene_animate_objects): that batch with every entry's joint matrices evaluated on the device first, by
// the arithmetic of csrc/host/animation.h, from a resident skeleton and clip (animate_joints_batch); PoseObjects then reads them where
// the kernel wrote them.  cgpt_scene_animate_layers is the same call with each joint's T / R / S blended from up to four
// clips at wrapped times before the hierarchy walk (animate_layers_batch).
// After cgpt_scene_upload_instanced the objects of a mesh group share the one copy these passes edit: the refit goes through any member's
// RefitObject (they are equal), and the area and the top-level box, which are per object, are written for every member.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <exception>
#include <vector>

#include "animation.h"
#include "cpugpupt_abi.h"
#include "ctx_internal.h"
#include "device_scene.h"
#include "minmax_std.h"
#include "morph.h"
#include "pose_plan.h"
#include "scene_layout.h"
#include "skinning.h"

namespace cgpt {

float HostTriangleArea(const cgpt_triangle& t);                               // bvh_build.hip

// the active targets of a pose's weights, {target, bits(weight)} in ascending order: a zero weight of either sign is skipped (morph.h).
// Declared in ctx_internal.h: denoise.hip compacts a history's weights by the same rule.
std::vector<uint2> ActiveTable(const float* weights, uint32_t n_targets)
{
    std::vector<uint2> table;
    for (uint32_t k = 0; k < n_targets; ++k)
        if (weights[k] != 0.0f) { uint32_t w; memcpy(&w, &weights[k], 4); table.push_back(make_uint2(k, w)); }
    return table;
}

namespace {

constexpr uint32_t kRefitThreads = 256;
static_assert(kRefitThreads == kPoseThreads, "pose_plan.h deals blocks of this size");

// The records of one triangle, stated once for the refit's and the skin's triangle pass: tr is the cgpt_triangle (v0 {pos, normal}, v1, v2),
// `leaf` its tri_leaf record with `keep` = leaf[2] as it was ({pad, e2.z, tri_idx, last_in_leaf}: pad, tri_idx and last_in_leaf stay), t = tri_idx
__device__ __forceinline__ void write_triangle_records(const float (&tr)[18], float4* __restrict__ leaf, const float4 keep, float4* __restrict__ tri_orig,
                                                       float4* __restrict__ tri_normal, uint32_t tri_base, uint32_t t, uint32_t n_tris_total)
{
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
    const float* src = staging + 18 * (size_t)t;                              // cgpt_triangle: v0 {pos, normal}, v1, v2 (72 B, 8-byte aligned)
    float tr[18];
    for (int k = 0; k < 18; ++k) tr[k] = src[k];
    write_triangle_records(tr, leaf, keep, tri_orig, tri_normal, tri_base, t, n_tris_total);
}

// The skin's triangle pass (cgpt_scene_skin_mesh; skinning.h states the arithmetic): refit_triangles with the posed triangle computed
// here from the resident bind pose instead of gathered from a staging copy.  A thread per leaf slot, blocks striding over the slots so
// that a block stages the joint matrices once: LDS true keeps the n_joints x 3 float4 rows in LDS (dynamic, 48 n_joints bytes: 48 KB at
// the 1024-joint limit), false reads them through the vector cache.  The joint indices are per lane and were validated by
// cgpt_scene_set_skin.  *range_flag is set when a posed position is not finite or lies beyond 1e30, where the refitted root bounds (a
// fold from +-1e30) no longer give the top-level box.
// (the cap of its grid, kSkinMaxBlocks, is stated in pose_plan.h: the batch planner applies it per entry)
// the 12 blended entries of corner c of triangle t (skinning.h: SkinBlend), for the skin's and the morph's triangle pass
__device__ __forceinline__ void blend_corner_joints(const float4* mat, const uint2* __restrict__ joints, const float4* __restrict__ weights, uint32_t t, int c, float (&m)[12])
{
    const uint2 jw = joints[3 * (size_t)t + c];                               // four uint16_t: the corner's joints
    const float4 w = weights[3 * (size_t)t + c];
    const uint32_t j0 = jw.x & 0xFFFFu, j1 = jw.x >> 16, j2 = jw.y & 0xFFFFu, j3 = jw.y >> 16;
    for (int r = 0; r < 3; ++r) {
        const float4 a0 = mat[3 * j0 + r], a1 = mat[3 * j1 + r], a2 = mat[3 * j2 + r], a3 = mat[3 * j3 + r];
        m[4 * r] = SkinBlend(w.x, a0.x, w.y, a1.x, w.z, a2.x, w.w, a3.x);
        m[4 * r + 1] = SkinBlend(w.x, a0.y, w.y, a1.y, w.z, a2.y, w.w, a3.y);
        m[4 * r + 2] = SkinBlend(w.x, a0.z, w.y, a1.z, w.z, a2.z, w.w, a3.z);
        m[4 * r + 3] = SkinBlend(w.x, a0.w, w.y, a1.w, w.z, a2.w, w.w, a3.w);
    }
}
template <bool LDS>
__global__ __launch_bounds__(kRefitThreads) void skin_triangles(const float2* __restrict__ bind, const uint2* __restrict__ joints, const float4* __restrict__ weights,
                                                                const float4* __restrict__ matrices, uint32_t n_joints, float4* __restrict__ tri_leaf,
                                                                float4* __restrict__ tri_orig, float4* __restrict__ tri_normal, uint32_t* __restrict__ range_flag,
                                                                uint32_t leaf_base, uint32_t tri_base, uint32_t n, uint32_t n_tris_total)
{
    extern __shared__ float4 s_matrices[];
    const float4* mat = matrices;
    if (LDS) {
        for (uint32_t k = threadIdx.x; k < 3 * n_joints; k += blockDim.x) s_matrices[k] = matrices[k];
        __syncthreads();
        mat = s_matrices;
    }
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float4* leaf = tri_leaf + 3 * (size_t)(leaf_base + i);
        const float4 keep = leaf[2];                                          // {pad, e2.z, tri_idx, last_in_leaf}
        const uint32_t t = __float_as_uint(keep.z);
        if (t >= n) continue;                                                 // validated at upload
        float tr[18];
        bool in_range = true;
        for (int c = 0; c < 3; ++c) {
            float m[12];
            blend_corner_joints(mat, joints, weights, t, c, m);
            const float2 b0 = bind[9 * (size_t)t + 3 * c], b1 = bind[9 * (size_t)t + 3 * c + 1], b2 = bind[9 * (size_t)t + 3 * c + 2];
            const float pn[6] = { b0.x, b0.y, b1.x, b1.y, b2.x, b2.y };
            SkinCorner(m, pn, tr + 6 * c);
            in_range = in_range && fabsf(tr[6 * c]) <= 1e30f && fabsf(tr[6 * c + 1]) <= 1e30f && fabsf(tr[6 * c + 2]) <= 1e30f;   // false for a NaN too
        }
        write_triangle_records(tr, leaf, keep, tri_orig, tri_normal, tri_base, t, n_tris_total);
        if (!in_range) atomicOr(range_flag, 1u);
    }
}

// The morph's triangle pass (cgpt_scene_morph_mesh, and cgpt_scene_skin_mesh on an object with targets; morph.h states the arithmetic):
// skin_triangles with the bind corner computed here -- the base record plus the active targets' records, which stay in registers and are
// the pn of SkinCorner when SKIN is set (no intermediate triangle exists), or the written triangle when it is not.  A thread per leaf
// slot i, striding.  LEAF: `data` holds component planes in leaf-slot order -- float2 plane p of set s at data[(9 s + p) n + i], so the
// lanes of a wave read consecutive 8-byte pieces (512 B an instruction); otherwise records as given, triangle t's at data[9 (s n + t)],
// a 72-byte gather per lane as skin_triangles' bind read is.  `active` holds the pose's n_active nonzero weights in ascending target
// order, {target, bits(weight)}: uniform reads.  The skin's joints and weights are in original order (by t) either way.
template <bool SKIN, bool LDS, bool LEAF>
__global__ __launch_bounds__(kRefitThreads) void morph_triangles(const float2* __restrict__ data, const uint2* __restrict__ active, uint32_t n_active,
                                                                 const uint2* __restrict__ joints, const float4* __restrict__ weights,
                                                                 const float4* __restrict__ matrices, uint32_t n_joints, float4* __restrict__ tri_leaf,
                                                                 float4* __restrict__ tri_orig, float4* __restrict__ tri_normal, uint32_t* __restrict__ range_flag,
                                                                 uint32_t leaf_base, uint32_t tri_base, uint32_t n, uint32_t n_tris_total)
{
    extern __shared__ float4 s_matrices[];
    const float4* mat = matrices;
    if (SKIN && LDS) {
        for (uint32_t k = threadIdx.x; k < 3 * n_joints; k += blockDim.x) s_matrices[k] = matrices[k];
        __syncthreads();
        mat = s_matrices;
    }
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float4* leaf = tri_leaf + 3 * (size_t)(leaf_base + i);
        const float4 keep = leaf[2];                                          // {pad, e2.z, tri_idx, last_in_leaf}
        const uint32_t t = __float_as_uint(keep.z);
        if (t >= n) continue;                                                 // validated at upload
        const auto record = [&](uint32_t set, float (&out)[18]) {
            for (int p = 0; p < 9; ++p) {
                const float2 v = LEAF ? data[(9 * (size_t)set + p) * n + i] : data[9 * ((size_t)set * n + t) + p];
                out[2 * p] = v.x; out[2 * p + 1] = v.y;
            }
        };
        float base[18], x[18];
        record(0u, base);
        for (int j = 0; j < 18; ++j) x[j] = base[j];
        for (uint32_t a = 0; a < n_active; ++a) {
            const uint2 kw = active[a];
            float d[18];
            record(1u + kw.x, d);
            MorphAccumulate(x, __uint_as_float(kw.y), d);
        }
        if (n_active != 0u) MorphNormalise(base, x);
        float tr[18];
        if (SKIN) {
            for (int c = 0; c < 3; ++c) {
                float m[12];
                blend_corner_joints(mat, joints, weights, t, c, m);
                SkinCorner(m, x + 6 * c, tr + 6 * c);
            }
        } else {
            for (int j = 0; j < 18; ++j) tr[j] = x[j];
        }
        bool in_range = true;
        for (int c = 0; c < 3; ++c)
            in_range = in_range && fabsf(tr[6 * c]) <= 1e30f && fabsf(tr[6 * c + 1]) <= 1e30f && fabsf(tr[6 * c + 2]) <= 1e30f;   // false for a NaN too
        write_triangle_records(tr, leaf, keep, tri_orig, tri_normal, tri_base, t, n_tris_total);
        if (!in_range) atomicOr(range_flag, 1u);
    }
}

// TriangleBounds (scene_layout.hip) of an object's n triangles as tri_orig holds them: words 1..6 of `out` get min / max of the vertex
// positions by < and >, word 7 is 1 where a position is not finite.  One block: the top-level box of a leaf-rooted mesh or a triangle
// object, which has no root record to read, and of a pose that set the range flag.
constexpr uint32_t kSkinScratchWords = 8;                                     // {range flag, lo.xyz, hi.xyz, not finite}
__global__ __launch_bounds__(kRefitThreads) void fold_object_box(const float4* __restrict__ tri_orig, uint32_t tri_base, uint32_t n, uint32_t* __restrict__ out)
{
    __shared__ float s_box[kRefitThreads][6];
    __shared__ uint32_t s_bad[kRefitThreads];
    float box[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
    uint32_t bad = 0u;
    for (uint32_t t = threadIdx.x; t < n; t += blockDim.x) {
        const float4* o = tri_orig + 3 * (size_t)(tri_base + t);
        for (int v = 0; v < 3; ++v) {
            const float4 q = o[v];
            const float x[3] = { q.x, q.y, q.z };
            for (int a = 0; a < 3; ++a) {
                if (!(fabsf(x[a]) < INFINITY)) bad = 1u;
                if (x[a] < box[a]) box[a] = x[a];
                if (x[a] > box[3 + a]) box[3 + a] = x[a];
            }
        }
    }
    for (int a = 0; a < 6; ++a) s_box[threadIdx.x][a] = box[a];
    s_bad[threadIdx.x] = bad;
    __syncthreads();
    for (uint32_t stride = blockDim.x / 2; stride > 0; stride /= 2) {
        if (threadIdx.x < stride) {
            for (int a = 0; a < 3; ++a) {
                if (s_box[threadIdx.x + stride][a] < s_box[threadIdx.x][a]) s_box[threadIdx.x][a] = s_box[threadIdx.x + stride][a];
                if (s_box[threadIdx.x + stride][3 + a] > s_box[threadIdx.x][3 + a]) s_box[threadIdx.x][3 + a] = s_box[threadIdx.x + stride][3 + a];
            }
            s_bad[threadIdx.x] |= s_bad[threadIdx.x + stride];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        for (int a = 0; a < 6; ++a) out[1 + a] = __float_as_uint(s_box[0][a]);
        out[7] = s_bad[0];
    }
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

// ---- the kernels of a batch (cgpt_scene_pose_objects; pose_plan.h plans it) --------------------------------------------
// The shells above once more, with what was a kernel argument of one object read from a table: a block belongs to one entry (or one
// entry's records of the launch's depth), found from blockIdx.x through the ascending first_block words, so everything it reads of the
// table is block-uniform and comes through scalar loads.  The arithmetic is the shared device functions'.
// One entry as the triangle pass and the box kernel read it: 72 bytes
struct PoseEntryRecord {
    const float2* data;                                                       // MORPH: MorphBuffers::data; otherwise the skin's bind pose
    const uint2* joints;                                                      // SKIN: the skin's joints and weights
    const float4* weights;
    uint32_t leaf_base, tri_base, n_tris, n_joints;
    uint32_t matrix_base, active_base, n_active, first_block;                 // PosePlanEntry's
    uint32_t blocks, root_code, leaf_root, pad;
};
// per entry {range flag, lo.xyz, hi.xyz, not finite} as kSkinScratchWords, then the 12 floats of the refitted root record's bounds
constexpr uint32_t kPoseScratchWords = 20;

// the last of table[0 .. n) whose first_block is not after `block` (first_block ascends from 0)
template <class T>
__device__ __forceinline__ uint32_t last_not_after(const T* __restrict__ table, uint32_t n, uint32_t block)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) / 2u;
        if (table[mid].first_block <= block) lo = mid; else hi = mid;
    }
    return lo;
}

// skin_triangles<LDS> (MORPH false: SKIN is set and LEAF is not) and morph_triangles<SKIN, LDS, LEAF> over the entries of one
// instantiation.  `entries` and `scratch` start at the launch's first entry; an entry's blocks stride over its leaf slots by its own
// block count, stage its own joint matrices (dynamic LDS: 48 B x the launch's largest joint count) and flag its own scratch.
template <bool MORPH, bool SKIN, bool LDS, bool LEAF>
__global__ __launch_bounds__(kRefitThreads) void pose_triangles_batch(const PoseEntryRecord* __restrict__ entries, uint32_t n_entries, const uint2* __restrict__ active_tables,
                                                                      const float4* __restrict__ matrices, float4* __restrict__ tri_leaf, float4* __restrict__ tri_orig,
                                                                      float4* __restrict__ tri_normal, uint32_t* __restrict__ scratch, uint32_t n_tris_total)
{
    extern __shared__ float4 s_matrices[];
    const uint32_t k = last_not_after(entries, n_entries, blockIdx.x);
    const PoseEntryRecord e = entries[k];
    const float4* mat = matrices + 3 * (size_t)e.matrix_base;
    if (SKIN && LDS) {
        for (uint32_t j = threadIdx.x; j < 3 * e.n_joints; j += blockDim.x) s_matrices[j] = mat[j];
        __syncthreads();
        mat = s_matrices;
    }
    const float2* __restrict__ data = e.data;
    const uint2* __restrict__ active = active_tables + e.active_base;
    uint32_t* range_flag = scratch + kPoseScratchWords * (size_t)k;
    const uint32_t n = e.n_tris;
    for (uint32_t i = (blockIdx.x - e.first_block) * blockDim.x + threadIdx.x; i < n; i += e.blocks * blockDim.x) {
        float4* leaf = tri_leaf + 3 * (size_t)(e.leaf_base + i);
        const float4 keep = leaf[2];                                          // {pad, e2.z, tri_idx, last_in_leaf}
        const uint32_t t = __float_as_uint(keep.z);
        if (t >= n) continue;                                                 // validated at upload
        const auto record = [&](uint32_t set, float (&out)[18]) {
            for (int p = 0; p < 9; ++p) {
                const float2 v = LEAF ? data[(9 * (size_t)set + p) * n + i] : data[9 * ((size_t)set * n + t) + p];
                out[2 * p] = v.x; out[2 * p + 1] = v.y;
            }
        };
        float base[18], x[18];
        record(0u, base);                                                     // the skin's bind record where nothing is morphed
        for (int j = 0; j < 18; ++j) x[j] = base[j];
        if (MORPH) {
            for (uint32_t a = 0; a < e.n_active; ++a) {
                const uint2 kw = active[a];
                float d[18];
                record(1u + kw.x, d);
                MorphAccumulate(x, __uint_as_float(kw.y), d);
            }
            if (e.n_active != 0u) MorphNormalise(base, x);
        }
        float tr[18];
        if (SKIN) {
            for (int c = 0; c < 3; ++c) {
                float m[12];
                blend_corner_joints(mat, e.joints, e.weights, t, c, m);
                SkinCorner(m, x + 6 * c, tr + 6 * c);
            }
        } else {
            for (int j = 0; j < 18; ++j) tr[j] = x[j];
        }
        bool in_range = true;
        for (int c = 0; c < 3; ++c)
            in_range = in_range && fabsf(tr[6 * c]) <= 1e30f && fabsf(tr[6 * c + 1]) <= 1e30f && fabsf(tr[6 * c + 2]) <= 1e30f;   // false for a NaN too
        write_triangle_records(tr, leaf, keep, tri_orig, tri_normal, e.tri_base, t, n_tris_total);
        if (!in_range) atomicOr(range_flag, 1u);
    }
}

// refit_level over the records of one depth of every entry whose tree reaches it: a segment takes whole blocks, a thread a record
__global__ __launch_bounds__(kRefitThreads) void refit_level_batch(float4* node_pairs, const float4* __restrict__ tri_leaf, const float4* __restrict__ tri_orig,
                                                                   const uint32_t* __restrict__ refit_levels, const PosePlanSegment* __restrict__ segments, uint32_t n_segments)
{
    const PosePlanSegment s = segments[last_not_after(segments, n_segments, blockIdx.x)];
    const uint32_t i = (blockIdx.x - s.first_block) * blockDim.x + threadIdx.x;
    if (i >= s.count) return;
    float4* rec = node_pairs + 4 * (size_t)refit_levels[s.records_begin + i];
    const float4 codes = rec[3];
    const Box l = side_bounds(node_pairs, tri_leaf, tri_orig, s.tri_base, __float_as_uint(codes.z));
    const Box r = side_bounds(node_pairs, tri_leaf, tri_orig, s.tri_base, __float_as_uint(codes.w));
    rec[0] = make_float4(l.lo[0], r.lo[0], l.lo[1], r.lo[1]);                 // device_scene.h: node_pairs
    rec[1] = make_float4(l.lo[2], r.lo[2], l.hi[0], r.hi[0]);
    rec[2] = make_float4(l.hi[1], r.hi[1], l.hi[2], r.hi[2]);
}

// What the host reads back of every entry, a block an entry: the refitted root record's bounds behind the entry's scratch words, and
// fold_object_box's fold into them for an entry without a root record or with its range flag set.  (The fold is that kernel's body once
// more: called from here as a function it compiles to another instruction stream there, and the single calls keep theirs.)
__global__ __launch_bounds__(kRefitThreads) void pose_boxes_batch(const PoseEntryRecord* __restrict__ entries, const float4* __restrict__ node_pairs,
                                                                  const float4* __restrict__ tri_orig, uint32_t* scratch)
{
    __shared__ float s_box[kRefitThreads][6];
    __shared__ uint32_t s_bad[kRefitThreads];
    const PoseEntryRecord e = entries[blockIdx.x];
    uint32_t* out = scratch + kPoseScratchWords * (size_t)blockIdx.x;
    if (e.leaf_root == 0u) {
        if (threadIdx.x < 12u) out[kSkinScratchWords + threadIdx.x] = reinterpret_cast<const uint32_t*>(node_pairs + 4 * (size_t)e.root_code)[threadIdx.x];
        if (out[0] == 0u) return;                                             // block-uniform: the triangle pass finished before this launch
    }
    float box[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
    uint32_t bad = 0u;
    for (uint32_t t = threadIdx.x; t < e.n_tris; t += blockDim.x) {
        const float4* o = tri_orig + 3 * (size_t)(e.tri_base + t);
        for (int v = 0; v < 3; ++v) {
            const float4 q = o[v];
            const float x[3] = { q.x, q.y, q.z };
            for (int a = 0; a < 3; ++a) {
                if (!(fabsf(x[a]) < INFINITY)) bad = 1u;
                if (x[a] < box[a]) box[a] = x[a];
                if (x[a] > box[3 + a]) box[3 + a] = x[a];
            }
        }
    }
    for (int a = 0; a < 6; ++a) s_box[threadIdx.x][a] = box[a];
    s_bad[threadIdx.x] = bad;
    __syncthreads();
    for (uint32_t stride = blockDim.x / 2; stride > 0; stride /= 2) {
        if (threadIdx.x < stride) {
            for (int a = 0; a < 3; ++a) {
                if (s_box[threadIdx.x + stride][a] < s_box[threadIdx.x][a]) s_box[threadIdx.x][a] = s_box[threadIdx.x + stride][a];
                if (s_box[threadIdx.x + stride][3 + a] > s_box[threadIdx.x][3 + a]) s_box[threadIdx.x][3 + a] = s_box[threadIdx.x + stride][3 + a];
            }
            s_bad[threadIdx.x] |= s_bad[threadIdx.x + stride];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        for (int a = 0; a < 6; ++a) out[1 + a] = __float_as_uint(s_box[0][a]);
        out[7] = s_bad[0];
    }
}

// ---- joint matrices from a clip (cgpt_scene_animate_objects; animation.h states the arithmetic) -----------------------
// One entry as animate_joints_batch reads it: 80 bytes, block-uniform, so it comes through scalar loads
struct AnimEntryRecord {
    const int32_t* parents;                                                   // the skin's skeleton (SkinBuffers)
    const float* inverse_bind;
    const float* rest;
    const float* root;                                                        // null: no root multiply
    const uint32_t* map;                                                      // the clip (ClipBuffers)
    const AnimChannel* channels;
    const float* times;
    const float* values;
    uint32_t n_joints, matrix_base;                                           // the entry's matrices start at float4 3 * matrix_base of `matrices`
    float time;
    uint32_t pad;
};
// A block an entry, a lane the joints tid, tid + 256, ...: it samples T, R and S and writes L_j to LDS (dynamic, 48 B a joint, sized to
// the launch's largest joint count: 48 KB at the 1024-joint limit); after one barrier it walks its joint's ancestors through LDS
// (the parents were validated by cgpt_scene_set_skeleton: in range, no cycle) and writes M_j as three float4.  flags[entry] is set when
// a matrix entry is not finite.  Nothing else is written: the scene is not touched.
// The 48-byte records are three 16-byte stores a lane, 12 dwords apart: the eight lanes a store is served in cover dwords 0, 12, 24,
// 36 = 4, 16, 28, 8, 20 (mod 32) + 0..3, every bank once; a wave that walks a chain (parents[j] = j - 1) reads sixteen records 12 dwords
// apart a group, sixteen different 16-byte slots of the 64 banks: neither conflicts, so the records stay whole.
__global__ __launch_bounds__(kRefitThreads) void animate_joints_batch(const AnimEntryRecord* __restrict__ entries, float4* __restrict__ matrices, uint32_t* __restrict__ flags)
{
    extern __shared__ float4 s_locals[];
    const AnimEntryRecord e = entries[blockIdx.x];
    for (uint32_t j = threadIdx.x; j < e.n_joints; j += blockDim.x) {
        float L[12];
        AnimLocalMatrix(e.map, e.channels, e.times, e.values, e.rest, j, e.time, L);
        s_locals[3 * j] = make_float4(L[0], L[1], L[2], L[3]);
        s_locals[3 * j + 1] = make_float4(L[4], L[5], L[6], L[7]);
        s_locals[3 * j + 2] = make_float4(L[8], L[9], L[10], L[11]);
    }
    __syncthreads();
    float4* out = matrices + 3 * (size_t)e.matrix_base;
    bool finite = true;
    for (uint32_t j = threadIdx.x; j < e.n_joints; j += blockDim.x) {
        float M[12];
        AnimJointMatrix(reinterpret_cast<const float*>(s_locals), e.parents, e.inverse_bind, e.root, j, M);
        for (int i = 0; i < 12; ++i) finite = finite && fabsf(M[i]) < INFINITY;   // false for a NaN too
        out[3 * j] = make_float4(M[0], M[1], M[2], M[3]);
        out[3 * j + 1] = make_float4(M[4], M[5], M[6], M[7]);
        out[3 * j + 2] = make_float4(M[8], M[9], M[10], M[11]);
    }
    if (!finite) atomicOr(flags + blockIdx.x, 1u);
}

// ---- ... from a blend of clips (cgpt_scene_animate_layers) -------------------------------------------------------------
// One entry as animate_layers_batch reads it: 208 bytes, block-uniform.  The host has compacted the active layers (weight > 0), wrapped
// their times and normalised their weights (animation.h: ResolveLayers), so layers[0 .. n_layers) are all sampled
struct AnimLayersEntryRecord {
    const int32_t* parents;
    const float* inverse_bind;
    const float* rest;
    const float* root;                                                        // null: no root multiply
    AnimLayer layers[CGPT_ANIM_MAX_LAYERS];
    uint32_t n_joints, matrix_base, n_layers, pad;
};
// animate_joints_batch with each lane's T, q, S blended from the entry's layers in registers (animation.h: AnimBlendJoint) before L_j
// goes to the same 48-byte LDS records; the layer loop's bound and every layer's record are block-uniform (scalar loads), so a launch
// mixes one-layer and four-layer entries freely.  The walk, the output and the flag word are animate_joints_batch's.
__global__ __launch_bounds__(kRefitThreads) void animate_layers_batch(const AnimLayersEntryRecord* __restrict__ entries, float4* __restrict__ matrices, uint32_t* __restrict__ flags)
{
    extern __shared__ float4 s_locals[];
    const AnimLayersEntryRecord* __restrict__ e = entries + blockIdx.x;
    const uint32_t n_joints = e->n_joints, n_layers = e->n_layers;
    const float* rest = e->rest;
    for (uint32_t j = threadIdx.x; j < n_joints; j += blockDim.x) {
        float T[3], q[4], S[3], L[12];
        AnimBlendJoint(e->layers, n_layers, rest, j, T, q, S);
        AnimComposeLocal(T, q, S, L);
        s_locals[3 * j] = make_float4(L[0], L[1], L[2], L[3]);
        s_locals[3 * j + 1] = make_float4(L[4], L[5], L[6], L[7]);
        s_locals[3 * j + 2] = make_float4(L[8], L[9], L[10], L[11]);
    }
    __syncthreads();
    float4* out = matrices + 3 * (size_t)e->matrix_base;
    const int32_t* parents = e->parents;
    const float* inverse_bind = e->inverse_bind;
    const float* root = e->root;
    bool finite = true;
    for (uint32_t j = threadIdx.x; j < n_joints; j += blockDim.x) {
        float M[12];
        AnimJointMatrix(reinterpret_cast<const float*>(s_locals), parents, inverse_bind, root, j, M);
        for (int i = 0; i < 12; ++i) finite = finite && fabsf(M[i]) < INFINITY;   // false for a NaN too
        out[3 * j] = make_float4(M[0], M[1], M[2], M[3]);
        out[3 * j + 1] = make_float4(M[4], M[5], M[6], M[7]);
        out[3 * j + 2] = make_float4(M[8], M[9], M[10], M[11]);
    }
    if (!finite) atomicOr(flags + blockIdx.x, 1u);
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

// the bound pass behind either triangle pass: one launch per level of the object's tree, deepest first, in stream order
hipError_t LaunchRefitLevels(cgpt_ctx* ctx, const RefitObject& ro, uint32_t tri_base)
{
    for (size_t level = ro.level_offsets.empty() ? 0 : ro.level_offsets.size() - 1; level-- > 0;) {
        const uint32_t first = ro.level_offsets[level], n = ro.level_offsets[level + 1] - first;
        if (n == 0) continue;
        hipLaunchKernelGGL(refit_level, dim3((n + kRefitThreads - 1) / kRefitThreads), dim3(kRefitThreads), 0, ctx->stream,
                           ctx->sb.node_pairs.p, ctx->sb.tri_leaf.p, ctx->sb.tri_orig.p, ctx->sb.refit_levels.p + ro.level_begin + first, n, tri_base);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

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
    for (const uint32_t j : members) {                                         // the copy is no pose of any skin or targets now (CGPT_TEMPORAL_FOLLOW_POSES, _MORPHS: "no pose known")
        if (j < ctx->skins.size()) ctx->skins[j].pose_known = false;
        if (j < ctx->morphs.size()) ctx->morphs[j].pose_known = false;
    }
    const uint32_t tri_base = d.tri_base;
    hipLaunchKernelGGL(refit_triangles, dim3((n_tris + kRefitThreads - 1) / kRefitThreads), dim3(kRefitThreads), 0, ctx->stream,
                       reinterpret_cast<const float*>(ctx->sb.refit_staging.p), ctx->sb.tri_leaf.p, ctx->sb.tri_orig.p, ctx->sb.tri_normal.p, ro.leaf_base, tri_base, n_tris, ctx->scene.n_tris_total);
    REFIT_HIP_WRITING(ctx, hipGetLastError());
    REFIT_HIP_WRITING(ctx, LaunchRefitLevels(ctx, ro, tri_base));
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

// ---- skinning (cgpt_scene_set_skin / cgpt_scene_skin_mesh / cgpt_scene_clear_skin) -----------------------------------
int SetSkin(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_triangle* bind, const uint16_t* joints, const float* weights, uint32_t n_tris, uint32_t n_joints)
{
    int rc = CheckObject(ctx, obj_index);
    if (rc != CGPT_OK) return rc;
    const DevObject& d = ctx->h_objects[obj_index];
    const RefitObject& ro = ctx->refit_objects[obj_index];
    if (d.kind != CGPT_OBJECT_MESH && d.kind != CGPT_OBJECT_TRIANGLE)
        return CtxFail(ctx, CGPT_ERR_INVALID, "object %u is a %s: it has no triangles to skin", obj_index, KindName(d.kind));
    for (const uint32_t li : ctx->h_lights)
        if (li == obj_index) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u is a light: a pose does not recompute the area its sampling reads, so it takes no skin", obj_index);
    if (!bind || !joints || !weights) return CtxFail(ctx, CGPT_ERR_INVALID, "%s is null", !bind ? "bind_triangles" : !joints ? "joints" : "weights");
    if (n_tris != ro.tri_count) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u has %u triangles, got %u (a skin keeps the topology)", obj_index, ro.tri_count, n_tris);
    std::string why;
    if (!CheckSkin(bind, joints, weights, n_tris, n_joints, why)) return CtxFail(ctx, CGPT_ERR_INVALID, "%s", why.c_str());

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                           // nothing uses the skin this one replaces
    SkinBuffers sk;                                                            // installed whole, or not at all
    HIP_TRY(ctx, sk.bind.Alloc(n_tris));
    HIP_TRY(ctx, sk.joints.Alloc(12 * (size_t)n_tris));
    HIP_TRY(ctx, sk.weights.Alloc(12 * (size_t)n_tris));
    HIP_TRY(ctx, sk.matrices.Alloc(12 * (size_t)n_joints));
    HIP_TRY(ctx, ctx->sb.skin_scratch.Grow(kSkinScratchWords));
    HIP_TRY(ctx, hipMemcpy(sk.bind.p, bind, sizeof(cgpt_triangle) * (size_t)n_tris, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(sk.joints.p, joints, sizeof(uint16_t) * 12 * (size_t)n_tris, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(sk.weights.p, weights, sizeof(float) * 12 * (size_t)n_tris, hipMemcpyHostToDevice));
    sk.n_joints = n_joints;
    sk.serial = ++ctx->skin_serial;                                            // no pose known yet
    if (ctx->skins.size() != ctx->h_objects.size()) ctx->skins.resize(ctx->h_objects.size());
    ctx->skins[obj_index] = std::move(sk);
    return CGPT_OK;
}

bool HasMorphTargets(const cgpt_ctx* ctx, uint32_t obj_index) { return obj_index < ctx->morphs.size() && ctx->morphs[obj_index].n_targets != 0u; }

// Every pose writes both small inputs its kernel reads -- the active table and, with a skin, the joint matrices -- from the host values
// it poses with, never trusting what an earlier call left on the device: a call that failed between its upload and its first scene write
// keeps the scene and its committed weights / matrices, and the next pose through either call must use those.
hipError_t UploadActiveTable(cgpt_ctx* ctx, const MorphBuffers& mb, const std::vector<uint2>& table)
{
    return table.empty() ? hipSuccess : hipMemcpyAsync(mb.active.p, table.data(), sizeof(uint2) * table.size(), hipMemcpyHostToDevice, ctx->stream);
}

// A device pose of object obj_index, shared by cgpt_scene_skin_mesh and cgpt_scene_morph_mesh: the triangle pass -- skin_triangles for an
// object without morph targets, else morph_triangles over the n_active entries of its active table, through the skin's joints when
// `skinned` -- the refit's bound pass and the top-level box.  The caller has validated; `upload` queues its own small copy (the joint
// matrices or the active table) once nothing before the first write can fail any more.
template <class Upload>
int PoseObject(cgpt_ctx* ctx, uint32_t obj_index, bool skinned, uint32_t n_active, Upload&& upload)
{
    const DevObject& d = ctx->h_objects[obj_index];
    const RefitObject& ro = ctx->refit_objects[obj_index];
    const uint32_t n_tris = ro.tri_count, tri_base = d.tri_base;
    const bool morphed = HasMorphTargets(ctx, obj_index);
    TopLevelState top = ctx->top_state;                                        // may throw: before the first write
    if (ctx->pose_stamp.size() != ctx->h_objects.size()) ctx->pose_stamp.resize(ctx->h_objects.size(), 0);

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, upload());
    HIP_TRY(ctx, hipMemsetAsync(ctx->sb.skin_scratch.p, 0, sizeof(uint32_t) * kSkinScratchWords, ctx->stream));

    // from here on the scene changes
    for (uint32_t j = 0; j < ctx->mesh_group.size(); ++j)                      // every placement of the copy: posed now, and by no other skin or targets
        if (ctx->mesh_group[j] == ctx->mesh_group[obj_index]) {
            ctx->pose_stamp[j] = ctx->pose_generation;
            if (j < ctx->skins.size()) ctx->skins[j].pose_known = false;
            if (j < ctx->morphs.size()) ctx->morphs[j].pose_known = false;
        }
    const SkinBuffers none;
    const SkinBuffers& sk = skinned ? ctx->skins[obj_index] : none;
    const uint32_t n_joints = sk.n_joints;
    const uint32_t blocks = (n_tris + kRefitThreads - 1) / kRefitThreads;
    const dim3 block(kRefitThreads);
    const size_t lds_bytes = skinned && ctx->skin_joints_lds ? 3 * sizeof(float4) * (size_t)n_joints : 0;
    if (!morphed) {
        const dim3 grid(std::min(blocks, kSkinMaxBlocks));
        const auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, lds_bytes, ctx->stream, reinterpret_cast<const float2*>(sk.bind.p), reinterpret_cast<const uint2*>(sk.joints.p),
                               reinterpret_cast<const float4*>(sk.weights.p), reinterpret_cast<const float4*>(sk.matrices.p), n_joints, ctx->sb.tri_leaf.p,
                               ctx->sb.tri_orig.p, ctx->sb.tri_normal.p, ctx->sb.skin_scratch.p, ro.leaf_base, tri_base, n_tris, ctx->scene.n_tris_total);
        };
        if (ctx->skin_joints_lds) launch(skin_triangles<true>);
        else launch(skin_triangles<false>);
    } else {
        const MorphBuffers& mb = ctx->morphs[obj_index];
        const dim3 grid(std::min(blocks, ctx->morph_max_blocks));
        const auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, lds_bytes, ctx->stream, mb.data.p, mb.active.p, n_active, reinterpret_cast<const uint2*>(sk.joints.p),
                               reinterpret_cast<const float4*>(sk.weights.p), reinterpret_cast<const float4*>(sk.matrices.p), n_joints, ctx->sb.tri_leaf.p,
                               ctx->sb.tri_orig.p, ctx->sb.tri_normal.p, ctx->sb.skin_scratch.p, ro.leaf_base, tri_base, n_tris, ctx->scene.n_tris_total);
        };
        const bool leaf = mb.leaf_order != 0u;
        if (!skinned) { if (leaf) launch(morph_triangles<false, false, true>); else launch(morph_triangles<false, false, false>); }
        else if (ctx->skin_joints_lds) { if (leaf) launch(morph_triangles<true, true, true>); else launch(morph_triangles<true, true, false>); }
        else { if (leaf) launch(morph_triangles<true, false, true>); else launch(morph_triangles<true, false, false>); }
    }
    REFIT_HIP_WRITING(ctx, hipGetLastError());
    REFIT_HIP_WRITING(ctx, LaunchRefitLevels(ctx, ro, tri_base));

    // The top-level tree's box of the object, TriangleBounds of the pose (what RefitMesh computes on the host): the refitted root record's two
    // sides where the object has one and every position lies within the +-1e30 its fold starts from, else a fold of tri_orig on the device
    uint32_t scratch[kSkinScratchWords];
    float4 root[3];
    const bool leaf_root = (d.root_code & kLeafBit) != 0u;
    const auto fold = [&]() -> hipError_t {
        hipLaunchKernelGGL(fold_object_box, dim3(1), dim3(kRefitThreads), 0, ctx->stream, ctx->sb.tri_orig.p, tri_base, n_tris, ctx->sb.skin_scratch.p);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipMemcpy(scratch, ctx->sb.skin_scratch.p, sizeof(scratch), hipMemcpyDeviceToHost);
        return e;
    };
    if (leaf_root) {
        REFIT_HIP_WRITING(ctx, fold());
    } else {
        REFIT_HIP_WRITING(ctx, hipStreamSynchronize(ctx->stream));
        REFIT_HIP_WRITING(ctx, hipMemcpy(scratch, ctx->sb.skin_scratch.p, sizeof(scratch), hipMemcpyDeviceToHost));
        if (scratch[0] != 0u) REFIT_HIP_WRITING(ctx, fold());
        else REFIT_HIP_WRITING(ctx, hipMemcpy(root, ctx->sb.node_pairs.p + 4 * (size_t)d.root_code, sizeof(root), hipMemcpyDeviceToHost));
    }
    float* box = top.local_box.data() + 6 * (size_t)obj_index;
    if (leaf_root || scratch[0] != 0u) {
        if (scratch[7] != 0u) UnboundedBox(box);
        else memcpy(box, scratch + 1, 24);
    } else {
        box[0] = min_std(root[0].x, root[0].y); box[1] = min_std(root[0].z, root[0].w); box[2] = min_std(root[1].x, root[1].y);
        box[3] = max_std(root[1].z, root[1].w); box[4] = max_std(root[2].x, root[2].y); box[5] = max_std(root[2].z, root[2].w);
    }
    for (uint32_t j = 0; j < ctx->mesh_group.size(); ++j)                      // every placement of the group moves (RefitMesh)
        if (j != obj_index && ctx->mesh_group[j] == ctx->mesh_group[obj_index]) memcpy(top.local_box.data() + 6 * (size_t)j, box, 24);
    REFIT_HIP_WRITING(ctx, WriteTopLevel(ctx, ctx->h_objects, top));
    ctx->top_state.local_box.swap(top.local_box);
    return CGPT_OK;
}

// what cgpt_scene_skin_mesh refuses, for it and for an entry of cgpt_scene_pose_objects: of the object and its skin (all an entry of
// cgpt_scene_animate_objects can be refused for: its matrices do not exist yet), and of the matrices
int CheckSkinJoints(cgpt_ctx* ctx, uint32_t obj_index, uint32_t n_joints)
{
    int rc = CheckObject(ctx, obj_index);
    if (rc != CGPT_OK) return rc;
    if (obj_index >= ctx->skins.size() || ctx->skins[obj_index].n_joints == 0u)
        return CtxFail(ctx, CGPT_ERR_INVALID, "object %u has no skin (cgpt_scene_set_skin installs one)", obj_index);
    const SkinBuffers& sk = ctx->skins[obj_index];
    if (n_joints != sk.n_joints) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u's skin has %u joints, got %u", obj_index, sk.n_joints, n_joints);
    return CGPT_OK;
}

int CheckSkinPose(cgpt_ctx* ctx, uint32_t obj_index, const float* joint_matrices, uint32_t n_joints)
{
    int rc = CheckSkinJoints(ctx, obj_index, n_joints);
    if (rc != CGPT_OK) return rc;
    std::string why;
    if (!CheckJointMatrices(joint_matrices, n_joints, why)) return CtxFail(ctx, CGPT_ERR_INVALID, "%s", why.c_str());
    return CGPT_OK;
}

int SkinMesh(cgpt_ctx* ctx, uint32_t obj_index, const float* joint_matrices, uint32_t n_joints)
{
    int rc = CheckSkinPose(ctx, obj_index, joint_matrices, n_joints);
    if (rc != CGPT_OK) return rc;
    SkinBuffers& sk = ctx->skins[obj_index];
    std::vector<float> pose(joint_matrices, joint_matrices + 12 * (size_t)n_joints);   // what a temporal call that follows poses compares (denoise.hip)
    const bool morphed = HasMorphTargets(ctx, obj_index);                      // the morphed base is the bind pose then: one kernel does both
    std::vector<uint2> table;                                                  // ... of the last weights given, written again: see UploadActiveTable
    if (morphed) table = ActiveTable(ctx->morphs[obj_index].weights.data(), ctx->morphs[obj_index].n_targets);
    rc = PoseObject(ctx, obj_index, true, (uint32_t)table.size(), [&] {
        const hipError_t e = hipMemcpyAsync(sk.matrices.p, joint_matrices, sizeof(float) * 12 * (size_t)n_joints, hipMemcpyHostToDevice, ctx->stream);
        return e != hipSuccess || !morphed ? e : UploadActiveTable(ctx, ctx->morphs[obj_index], table);
    });
    if (rc != CGPT_OK) return rc;
    sk.pose.swap(pose);
    sk.pose_known = !morphed;                                                  // the matrices alone do not tell a morphed pose: "no pose known"
    if (morphed) {                                                             // ... the targets' state does (CGPT_TEMPORAL_FOLLOW_MORPHS): the last weights through this skin
        MorphBuffers& mb = ctx->morphs[obj_index];
        mb.pose_matrices = sk.pose;
        mb.pose_skin_serial = sk.serial;
        mb.pose_known = true;
    }
    return CGPT_OK;
}

int ClearSkin(cgpt_ctx* ctx, uint32_t obj_index)
{
    if (obj_index >= ctx->skins.size() || ctx->skins[obj_index].n_joints == 0u) return CGPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->skins[obj_index] = SkinBuffers{};
    return CGPT_OK;
}

// ---- morph targets (cgpt_scene_set_morph_targets / cgpt_scene_morph_mesh / cgpt_scene_clear_morph_targets) ------------
int SetMorphTargets(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_triangle* base, const cgpt_triangle* deltas, uint32_t n_tris, uint32_t n_targets)
{
    int rc = CheckObject(ctx, obj_index);
    if (rc != CGPT_OK) return rc;
    const DevObject& d = ctx->h_objects[obj_index];
    const RefitObject& ro = ctx->refit_objects[obj_index];
    if (d.kind != CGPT_OBJECT_MESH && d.kind != CGPT_OBJECT_TRIANGLE)
        return CtxFail(ctx, CGPT_ERR_INVALID, "object %u is a %s: it has no triangles to morph", obj_index, KindName(d.kind));
    for (const uint32_t li : ctx->h_lights)
        if (li == obj_index) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u is a light: a pose does not recompute the area its sampling reads, so it takes no morph targets", obj_index);
    if (!base || !deltas) return CtxFail(ctx, CGPT_ERR_INVALID, "%s is null", !base ? "base_triangles" : "target_deltas");
    if (n_tris != ro.tri_count) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u has %u triangles, got %u (a morph keeps the topology)", obj_index, ro.tri_count, n_tris);
    std::string why;
    if (!CheckMorphTargets(base, deltas, n_tris, n_targets, why)) return CtxFail(ctx, CGPT_ERR_INVALID, "%s", why.c_str());

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                           // nothing uses the targets this set replaces
    const size_t n = n_tris, per_set = 9 * n;                                  // float2 a set
    MorphBuffers mb;                                                           // installed whole, or not at all
    mb.leaf_order = ctx->morph_leaf_order;
    mb.weights.assign(n_targets, 0.0f);
    HIP_TRY(ctx, mb.data.Alloc(per_set * ((size_t)n_targets + 1)));
    HIP_TRY(ctx, mb.active.Alloc(n_targets));
    HIP_TRY(ctx, ctx->sb.skin_scratch.Grow(kSkinScratchWords));
    if (mb.leaf_order) {
        // The slot -> triangle map is fixed while the targets live (an upload drops them, a refit keeps the tree): every set goes up as nine
        // float2 planes in leaf-slot order, permuted here, one set at a time
        std::vector<float4> leaf_tail(n);                                      // {pad, e2.z, tri_idx, last_in_leaf} of every leaf slot
        HIP_TRY(ctx, hipMemcpy2D(leaf_tail.data(), sizeof(float4), ctx->sb.tri_leaf.p + 3 * (size_t)ro.leaf_base + 2, 3 * sizeof(float4),
                                   sizeof(float4), n, hipMemcpyDeviceToHost));
        std::vector<uint32_t> slot_tri(n);
        for (size_t i = 0; i < n; ++i) {
            memcpy(&slot_tri[i], &leaf_tail[i].z, 4);
            if (slot_tri[i] >= n_tris) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u: leaf slot %zu names triangle %u", obj_index, i, slot_tri[i]);
        }
        std::vector<uint32_t> slot_of_tri(n, 0u);                              // the inverse: where CGPT_TEMPORAL_FOLLOW_MORPHS finds a triangle's planes
        for (size_t i = 0; i < n; ++i) slot_of_tri[slot_tri[i]] = (uint32_t)i;
        HIP_TRY(ctx, mb.slot_of_tri.Alloc(n));
        HIP_TRY(ctx, hipMemcpy(mb.slot_of_tri.p, slot_of_tri.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
        std::vector<float2> planes(per_set);
        for (uint32_t s = 0; s <= n_targets; ++s) {
            const float* src = reinterpret_cast<const float*>(s == 0 ? base : deltas + (size_t)(s - 1) * n);
            for (size_t i = 0; i < n; ++i) {
                const float* rec = src + 18 * (size_t)slot_tri[i];
                for (int p = 0; p < 9; ++p) planes[p * n + i] = make_float2(rec[2 * p], rec[2 * p + 1]);
            }
            HIP_TRY(ctx, hipMemcpy(mb.data.p + per_set * s, planes.data(), sizeof(float2) * per_set, hipMemcpyHostToDevice));
        }
    } else {
        HIP_TRY(ctx, hipMemcpy(mb.data.p, base, sizeof(cgpt_triangle) * n, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(mb.data.p + per_set, deltas, sizeof(cgpt_triangle) * n * n_targets, hipMemcpyHostToDevice));
    }
    mb.n_targets = n_targets;
    mb.serial = ++ctx->morph_serial;                                           // no pose known yet: the scene holds the uploaded triangles, which need not be the base
    if (ctx->morphs.size() != ctx->h_objects.size()) ctx->morphs.resize(ctx->h_objects.size());
    ctx->morphs[obj_index] = std::move(mb);
    return CGPT_OK;
}

// what cgpt_scene_morph_mesh refuses, for it and for an entry of cgpt_scene_pose_objects
int CheckMorphPose(cgpt_ctx* ctx, uint32_t obj_index, const float* weights, uint32_t n_targets)
{
    int rc = CheckObject(ctx, obj_index);
    if (rc != CGPT_OK) return rc;
    if (!HasMorphTargets(ctx, obj_index))
        return CtxFail(ctx, CGPT_ERR_INVALID, "object %u has no morph targets (cgpt_scene_set_morph_targets installs them)", obj_index);
    const MorphBuffers& mb = ctx->morphs[obj_index];
    if (n_targets != mb.n_targets) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u has %u morph targets, got %u", obj_index, mb.n_targets, n_targets);
    std::string why;
    if (!CheckMorphWeights(weights, n_targets, why)) return CtxFail(ctx, CGPT_ERR_INVALID, "%s", why.c_str());
    return CGPT_OK;
}

int MorphMesh(cgpt_ctx* ctx, uint32_t obj_index, const float* weights, uint32_t n_targets)
{
    int rc = CheckMorphPose(ctx, obj_index, weights, n_targets);
    if (rc != CGPT_OK) return rc;
    MorphBuffers& mb = ctx->morphs[obj_index];
    std::vector<float> kept(weights, weights + n_targets);
    const std::vector<uint2> table = ActiveTable(weights, n_targets);
    // a skin that has been posed since it was installed takes part with the matrices of its last pose (sk.pose, written again: see UploadActiveTable)
    const bool skinned = obj_index < ctx->skins.size() && ctx->skins[obj_index].n_joints != 0u && !ctx->skins[obj_index].pose.empty();
    if (ctx->morph_stamp.size() != ctx->h_objects.size()) ctx->morph_stamp.resize(ctx->h_objects.size(), 0);
    std::vector<float> pose_matrices;                                          // the skin part of this pose's key
    if (skinned) pose_matrices = ctx->skins[obj_index].pose;
    ctx->scene_generation++; ctx->shape_generation++; ctx->morph_generation++;   // accepted -- as a refit: guides and temporal history are stale, CGPT_TEMPORAL_FOLLOW_POSES
                                                                               // included (a call with CGPT_TEMPORAL_FOLLOW_MORPHS keeps the history: morph_generation tells a morph from a refit)
    rc = PoseObject(ctx, obj_index, skinned, (uint32_t)table.size(), [&] {
        const hipError_t e = UploadActiveTable(ctx, mb, table);
        if (e != hipSuccess || !skinned) return e;
        const SkinBuffers& sk = ctx->skins[obj_index];
        return hipMemcpyAsync(sk.matrices.p, sk.pose.data(), sizeof(float) * sk.pose.size(), hipMemcpyHostToDevice, ctx->stream);
    });
    if (rc != CGPT_OK) return rc;
    mb.weights.swap(kept);
    for (uint32_t j = 0; j < ctx->mesh_group.size(); ++j)                      // every placement of the copy: morphed now
        if (ctx->mesh_group[j] == ctx->mesh_group[obj_index]) ctx->morph_stamp[j] = ctx->morph_generation;
    mb.pose_matrices.swap(pose_matrices);
    mb.pose_skin_serial = skinned ? ctx->skins[obj_index].serial : 0;
    mb.pose_known = true;
    return CGPT_OK;
}

int ClearMorphTargets(cgpt_ctx* ctx, uint32_t obj_index)
{
    if (!HasMorphTargets(ctx, obj_index)) return CGPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->morphs[obj_index] = MorphBuffers{};
    return CGPT_OK;
}

// ---- many objects in one call (cgpt_scene_pose_objects) ---------------------------------------------------------------
// What the single calls would do entry by entry -- MorphMesh for an entry with weights, then SkinMesh for one with matrices -- with the
// launches of PlanPoseBatch: one triangle launch an instantiation in use, one bound launch a depth, one box launch; one upload (the
// zeroed scratch, the entry table, the segments, every entry's matrices and active table in one piece), one synchronise, one readback
// and one WriteTopLevel.  The per-skin `matrices` and per-object `active` buffers are not written: only the single calls' kernels read
// them, and those calls upload them again themselves.
// `anim` (cgpt_scene_animate_objects): entry i's joint_matrices is null and its matrices are those of anim[i], evaluated on the device
// between the upload and the first write (AnimateEntries) and read by the triangle pass where they were written.
// n_layers != 0 (cgpt_scene_animate_layers): the entry's active layers instead, compacted, times wrapped, weights normalised; a batch is
// all of one kind
struct AnimResolved {
    const SkinBuffers* skin; const ClipBuffers* clip; float time;
    uint32_t n_layers = 0;
    const ClipBuffers* layer_clip[CGPT_ANIM_MAX_LAYERS] = {};
    float layer_time[CGPT_ANIM_MAX_LAYERS] = {}, layer_weight[CGPT_ANIM_MAX_LAYERS] = {};
};
int AnimateEntries(cgpt_ctx* ctx, const AnimResolved* anim, const cgpt_pose* poses, uint32_t n_poses, const PosePlan& plan, float* d_matrices,
                   std::vector<std::vector<float>>& kept_matrices);

int PoseObjects(cgpt_ctx* ctx, const cgpt_pose* poses, uint32_t n_poses, const AnimResolved* anim = nullptr)
{
    if (n_poses == 0u) return CGPT_OK;
    if (!ctx->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "no scene uploaded");
    if (!poses) return CtxFail(ctx, CGPT_ERR_INVALID, "poses is null");

    // the single calls' refusals, entry by entry, and what each entry poses with: its own arrays, or what the object's last pose left
    struct Resolved { const float* matrices = nullptr; const float* weights = nullptr; bool morphed = false, skinned = false; std::vector<uint2> table; };
    std::vector<Resolved> resolved(n_poses);
    std::vector<PosePlanInput> in(n_poses);
    for (uint32_t i = 0; i < n_poses; ++i) {
        const cgpt_pose& p = poses[i];
        const uint32_t o = p.obj_index;
        int rc = CheckObject(ctx, o);
        if (rc == CGPT_OK && p.n_joints == 0u && p.n_targets == 0u) rc = CtxFail(ctx, CGPT_ERR_INVALID, "object %u: neither joint matrices nor morph weights are given", o);
        if (rc == CGPT_OK && p.n_targets != 0u) rc = CheckMorphPose(ctx, o, p.weights, p.n_targets);
        if (rc == CGPT_OK && p.n_joints != 0u) rc = anim ? CheckSkinJoints(ctx, o, p.n_joints) : CheckSkinPose(ctx, o, p.joint_matrices, p.n_joints);
        if (rc != CGPT_OK) { ctx->error = "entry " + std::to_string(i) + ": " + ctx->error; return rc; }
        Resolved& r = resolved[i];
        r.morphed = HasMorphTargets(ctx, o);
        const bool posed_skin = o < ctx->skins.size() && ctx->skins[o].n_joints != 0u && !ctx->skins[o].pose.empty();   // MorphMesh: takes part with its last matrices
        r.matrices = p.n_joints != 0u ? p.joint_matrices : posed_skin ? ctx->skins[o].pose.data() : nullptr;
        r.skinned = r.matrices != nullptr || (anim && p.n_joints != 0u);
        if (r.morphed) {
            const MorphBuffers& mb = ctx->morphs[o];
            r.weights = p.n_targets != 0u ? p.weights : mb.weights.data();    // SkinMesh: the last weights given
            r.table = ActiveTable(r.weights, mb.n_targets);
        }
        in[i] = { o, r.skinned ? ctx->skins[o].n_joints : 0u, r.morphed ? 1u : 0u, r.morphed ? ctx->morphs[o].leaf_order : 0u, (uint32_t)r.table.size() };
    }
    PosePlan plan;
    std::string why;
    const int planned = PlanPoseBatch(ctx->h_objects, ctx->refit_objects, ctx->mesh_group, in.data(), n_poses, ctx->skin_joints_lds, ctx->morph_max_blocks, plan, why);
    if (planned != CGPT_OK) return CtxFail(ctx, planned, "%s", why.c_str());

    // the upload, in 32-bit words, every part at a multiple of 16 bytes: scratch | entries | segments | matrices | active tables
    static_assert(sizeof(PoseEntryRecord) == 72 && sizeof(PosePlanSegment) == 16, "the upload's parts");
    const auto round4 = [](size_t words) { return (words + 3) / 4 * 4; };
    const size_t n = plan.entries.size();
    const size_t entries_at = round4(kPoseScratchWords * n), segments_at = entries_at + round4(sizeof(PoseEntryRecord) / 4 * n);
    const size_t matrices_at = segments_at + 4 * plan.segments.size(), active_at = matrices_at + 12 * (size_t)plan.n_matrix_joints;
    const size_t total = active_at + round4(2 * (size_t)plan.n_active) + 4;   // never empty
    std::vector<uint32_t> blob(total, 0u);
    for (size_t k = 0; k < n; ++k) {
        const PosePlanEntry& e = plan.entries[k];
        const Resolved& r = resolved[e.source];
        PoseEntryRecord rec{};
        if (r.skinned) {
            const SkinBuffers& sk = ctx->skins[e.obj_index];
            rec.joints = reinterpret_cast<const uint2*>(sk.joints.p); rec.weights = reinterpret_cast<const float4*>(sk.weights.p);
            if (!r.morphed) rec.data = reinterpret_cast<const float2*>(sk.bind.p);
            if (r.matrices) memcpy(blob.data() + matrices_at + 12 * (size_t)e.matrix_base, r.matrices, sizeof(float) * 12 * (size_t)e.n_joints);
        }
        if (r.morphed) rec.data = ctx->morphs[e.obj_index].data.p;
        if (!r.table.empty()) memcpy(blob.data() + active_at + 2 * (size_t)e.active_base, r.table.data(), sizeof(uint2) * r.table.size());
        rec.leaf_base = e.leaf_base; rec.tri_base = e.tri_base; rec.n_tris = e.n_tris; rec.n_joints = e.n_joints;
        rec.matrix_base = e.matrix_base; rec.active_base = e.active_base; rec.n_active = e.n_active; rec.first_block = e.first_block;
        rec.blocks = e.blocks; rec.root_code = e.root_code; rec.leaf_root = e.leaf_root;
        memcpy(blob.data() + entries_at + sizeof(PoseEntryRecord) / 4 * k, &rec, sizeof(rec));
    }
    if (!plan.segments.empty()) memcpy(blob.data() + segments_at, plan.segments.data(), sizeof(PosePlanSegment) * plan.segments.size());
    std::vector<uint32_t> back(kPoseScratchWords * n);
    TopLevelState top = ctx->top_state;                                        // may throw: before the first write
    if (ctx->pose_stamp.size() != ctx->h_objects.size()) ctx->pose_stamp.resize(ctx->h_objects.size(), 0);
    if (ctx->morph_stamp.size() != ctx->h_objects.size()) ctx->morph_stamp.resize(ctx->h_objects.size(), 0);
    std::vector<std::vector<float>> kept_matrices(n_poses), kept_weights(n_poses);   // what the commit below installs: allocated while a refusal is still possible
    for (uint32_t i = 0; i < n_poses; ++i) {
        if (poses[i].n_joints != 0u && !anim) kept_matrices[i].assign(poses[i].joint_matrices, poses[i].joint_matrices + 12 * (size_t)poses[i].n_joints);
        if (poses[i].n_targets != 0u) kept_weights[i].assign(poses[i].weights, poses[i].weights + poses[i].n_targets);
    }

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, ctx->sb.pose_batch.Grow(total));                              // the stream was just drained: nothing uses the old one
    HIP_TRY(ctx, hipMemcpyAsync(ctx->sb.pose_batch.p, blob.data(), sizeof(uint32_t) * total, hipMemcpyHostToDevice, ctx->stream));
    if (anim) {                                                                // the matrices: computed where the triangle pass reads them, and kept as the caller's would be
        const int rc = AnimateEntries(ctx, anim, poses, n_poses, plan, reinterpret_cast<float*>(ctx->sb.pose_batch.p + matrices_at), kept_matrices);
        if (rc != CGPT_OK) return rc;
    }

    // from here on the scene changes.  The generations and stamps move as the single calls move them, entry by entry: an accepted morph
    // counts one scene, shape and morph edit, a pose one scene, shape and pose edit (denoise.hip: HistoryMatches)
    const auto each_placement = [&](uint32_t obj, auto&& f) {
        for (uint32_t j = 0; j < ctx->mesh_group.size(); ++j)
            if (ctx->mesh_group[j] == ctx->mesh_group[obj]) f(j);
    };
    for (uint32_t i = 0; i < n_poses; ++i) {
        const uint32_t o = poses[i].obj_index;
        if (poses[i].n_targets != 0u) {
            ctx->scene_generation++; ctx->shape_generation++; ctx->morph_generation++;
            each_placement(o, [&](uint32_t j) { ctx->pose_stamp[j] = ctx->pose_generation; ctx->morph_stamp[j] = ctx->morph_generation; });
        }
        if (poses[i].n_joints != 0u) {
            ctx->scene_generation++; ctx->shape_generation++; ctx->pose_generation++;
            each_placement(o, [&](uint32_t j) { ctx->pose_stamp[j] = ctx->pose_generation; });
        }
        each_placement(o, [&](uint32_t j) {                                    // posed now, and by no other skin or targets
            if (j < ctx->skins.size()) ctx->skins[j].pose_known = false;
            if (j < ctx->morphs.size()) ctx->morphs[j].pose_known = false;
        });
    }

    uint32_t* const dev = ctx->sb.pose_batch.p;
    const PoseEntryRecord* const d_entries = reinterpret_cast<const PoseEntryRecord*>(dev + entries_at);
    const PosePlanSegment* const d_segments = reinterpret_cast<const PosePlanSegment*>(dev + segments_at);
    const float4* const d_matrices = reinterpret_cast<const float4*>(dev + matrices_at);
    const uint2* const d_active = reinterpret_cast<const uint2*>(dev + active_at);
    const dim3 block(kRefitThreads);
    for (const PosePlanLaunch& l : plan.launches) {
        const bool lds = l.kernel == kPoseSkinLds || l.kernel == kPoseMorphSkinLds || l.kernel == kPoseMorphSkinLdsLeaf;
        const size_t lds_bytes = lds ? 3 * sizeof(float4) * (size_t)l.max_joints : 0;
        const auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(l.n_blocks), block, lds_bytes, ctx->stream, d_entries + l.first_entry, l.n_entries, d_active, d_matrices, ctx->sb.tri_leaf.p,
                               ctx->sb.tri_orig.p, ctx->sb.tri_normal.p, dev + kPoseScratchWords * (size_t)l.first_entry, ctx->scene.n_tris_total);
        };
        switch (l.kernel) {
        case kPoseSkin: launch(pose_triangles_batch<false, true, false, false>); break;
        case kPoseSkinLds: launch(pose_triangles_batch<false, true, true, false>); break;
        case kPoseMorph: launch(pose_triangles_batch<true, false, false, false>); break;
        case kPoseMorphLeaf: launch(pose_triangles_batch<true, false, false, true>); break;
        case kPoseMorphSkin: launch(pose_triangles_batch<true, true, false, false>); break;
        case kPoseMorphSkinLeaf: launch(pose_triangles_batch<true, true, false, true>); break;
        case kPoseMorphSkinLds: launch(pose_triangles_batch<true, true, true, false>); break;
        default: launch(pose_triangles_batch<true, true, true, true>); break;
        }
        REFIT_HIP_WRITING(ctx, hipGetLastError());
    }
    for (const PosePlanLevel& lv : plan.levels) {
        hipLaunchKernelGGL(refit_level_batch, dim3(lv.n_blocks), block, 0, ctx->stream, ctx->sb.node_pairs.p, ctx->sb.tri_leaf.p, ctx->sb.tri_orig.p,
                           ctx->sb.refit_levels.p, d_segments + lv.first_segment, lv.n_segments);
        REFIT_HIP_WRITING(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(pose_boxes_batch, dim3((uint32_t)n), block, 0, ctx->stream, d_entries, ctx->sb.node_pairs.p, ctx->sb.tri_orig.p, dev);
    REFIT_HIP_WRITING(ctx, hipGetLastError());
    REFIT_HIP_WRITING(ctx, hipStreamSynchronize(ctx->stream));
    REFIT_HIP_WRITING(ctx, hipMemcpy(back.data(), dev, sizeof(uint32_t) * back.size(), hipMemcpyDeviceToHost));

    // the top-level boxes, as PoseObject reads them: the fold where there is no root record or the range flag is set, else the root record's two sides
    for (size_t k = 0; k < n; ++k) {
        const PosePlanEntry& e = plan.entries[k];
        const uint32_t* scratch = back.data() + kPoseScratchWords * k;
        float* box = top.local_box.data() + 6 * (size_t)e.obj_index;
        if (e.leaf_root != 0u || scratch[0] != 0u) {
            if (scratch[7] != 0u) UnboundedBox(box);
            else memcpy(box, scratch + 1, 24);
        } else {
            float4 root[3];
            memcpy(root, scratch + kSkinScratchWords, sizeof(root));
            box[0] = min_std(root[0].x, root[0].y); box[1] = min_std(root[0].z, root[0].w); box[2] = min_std(root[1].x, root[1].y);
            box[3] = max_std(root[1].z, root[1].w); box[4] = max_std(root[2].x, root[2].y); box[5] = max_std(root[2].z, root[2].w);
        }
        each_placement(e.obj_index, [&](uint32_t j) { if (j != e.obj_index) memcpy(top.local_box.data() + 6 * (size_t)j, box, 24); });
    }
    REFIT_HIP_WRITING(ctx, WriteTopLevel(ctx, ctx->h_objects, top));
    ctx->top_state.local_box.swap(top.local_box);

    // what a temporal call that follows poses or morphs compares, as MorphMesh and then SkinMesh leave it
    for (uint32_t i = 0; i < n_poses; ++i) {
        const uint32_t o = poses[i].obj_index;
        const bool morphed = resolved[i].morphed;
        if (poses[i].n_targets != 0u) {
            MorphBuffers& mb = ctx->morphs[o];
            const bool skinned = o < ctx->skins.size() && ctx->skins[o].n_joints != 0u && !ctx->skins[o].pose.empty();
            mb.weights.swap(kept_weights[i]);
            if (skinned) mb.pose_matrices = ctx->skins[o].pose; else mb.pose_matrices.clear();
            mb.pose_skin_serial = skinned ? ctx->skins[o].serial : 0;
            mb.pose_known = true;
        }
        if (poses[i].n_joints != 0u) {
            SkinBuffers& sk = ctx->skins[o];
            sk.pose.swap(kept_matrices[i]);
            sk.pose_known = !morphed;
            if (morphed) {
                MorphBuffers& mb = ctx->morphs[o];
                mb.pose_matrices = sk.pose;
                mb.pose_skin_serial = sk.serial;
                mb.pose_known = true;
            }
        }
    }
    return CGPT_OK;
}

// ---- animation clips (cgpt_scene_set_skeleton / cgpt_clip_create / cgpt_scene_animate_objects) -----------------------
// Phase 1 of cgpt_scene_animate_objects, behind the batch's upload: the entry records go up, animate_joints_batch writes every entry's
// matrices at its matrix_base of the batch's matrix array, and after one synchronise the matrices and the flags come back.  A flagged
// entry refuses the call; nothing of the scene has been written yet.
int AnimateEntries(cgpt_ctx* ctx, const AnimResolved* anim, const cgpt_pose* poses, uint32_t n_poses, const PosePlan& plan, float* d_matrices,
                   std::vector<std::vector<float>>& kept_matrices)
{
    static_assert(sizeof(AnimEntryRecord) == 80 && sizeof(AnimChannel) == 16, "the entry table's parts");
    static_assert(sizeof(AnimLayer) == 40 && sizeof(AnimLayersEntryRecord) == 208, "the layered entry table's parts");
    const size_t n = plan.entries.size();
    const bool layered = n_poses != 0u && anim[0].n_layers != 0u;             // cgpt_scene_animate_layers: its own record and kernel
    const size_t record_words = (layered ? sizeof(AnimLayersEntryRecord) : sizeof(AnimEntryRecord)) / 4;
    const size_t records_at = (n + 3) / 4 * 4, total = records_at + record_words * n;
    std::vector<uint32_t> blob(total, 0u);                                     // flags | records
    uint32_t max_joints = 0;
    for (size_t k = 0; k < n; ++k) {
        const PosePlanEntry& e = plan.entries[k];
        const AnimResolved& a = anim[e.source];
        if (layered) {
            AnimLayersEntryRecord rec{};
            rec.parents = a.skin->parents.p; rec.inverse_bind = a.skin->inverse_bind.p; rec.rest = a.skin->rest.p;
            rec.root = a.skin->has_root ? a.skin->root.p : nullptr;
            for (uint32_t l = 0; l < a.n_layers; ++l) {
                const ClipBuffers& c = *a.layer_clip[l];
                rec.layers[l] = { c.map.p, reinterpret_cast<const AnimChannel*>(c.channels.p), c.times.p, c.values.p, a.layer_time[l], a.layer_weight[l] };
            }
            rec.n_joints = e.n_joints; rec.matrix_base = e.matrix_base; rec.n_layers = a.n_layers;
            memcpy(blob.data() + records_at + record_words * k, &rec, sizeof(rec));
        } else {
            AnimEntryRecord rec{};
            rec.parents = a.skin->parents.p; rec.inverse_bind = a.skin->inverse_bind.p; rec.rest = a.skin->rest.p;
            rec.root = a.skin->has_root ? a.skin->root.p : nullptr;
            rec.map = a.clip->map.p; rec.channels = reinterpret_cast<const AnimChannel*>(a.clip->channels.p); rec.times = a.clip->times.p; rec.values = a.clip->values.p;
            rec.n_joints = e.n_joints; rec.matrix_base = e.matrix_base; rec.time = a.time;
            memcpy(blob.data() + records_at + record_words * k, &rec, sizeof(rec));
        }
        max_joints = std::max(max_joints, e.n_joints);
    }
    std::vector<float> back(12 * (size_t)plan.n_matrix_joints);
    std::vector<uint32_t> flags(n);
    HIP_TRY(ctx, ctx->sb.anim_batch.Grow(total));                              // the caller drained the stream: nothing uses the old one
    HIP_TRY(ctx, hipMemcpyAsync(ctx->sb.anim_batch.p, blob.data(), sizeof(uint32_t) * total, hipMemcpyHostToDevice, ctx->stream));
    if (layered)
        hipLaunchKernelGGL(animate_layers_batch, dim3((uint32_t)n), dim3(kRefitThreads), 3 * sizeof(float4) * (size_t)max_joints, ctx->stream,
                           reinterpret_cast<const AnimLayersEntryRecord*>(ctx->sb.anim_batch.p + records_at), reinterpret_cast<float4*>(d_matrices), ctx->sb.anim_batch.p);
    else
        hipLaunchKernelGGL(animate_joints_batch, dim3((uint32_t)n), dim3(kRefitThreads), 3 * sizeof(float4) * (size_t)max_joints, ctx->stream,
                           reinterpret_cast<const AnimEntryRecord*>(ctx->sb.anim_batch.p + records_at), reinterpret_cast<float4*>(d_matrices), ctx->sb.anim_batch.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(back.data(), d_matrices, sizeof(float) * back.size(), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(flags.data(), ctx->sb.anim_batch.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    uint32_t refused = n_poses;                                                // the first flagged entry in the caller's order
    for (size_t k = 0; k < n; ++k)
        if (flags[k] != 0u) refused = std::min(refused, plan.entries[k].source);
    if (refused != n_poses)
        return layered ? CtxFail(ctx, CGPT_ERR_INVALID, "entry %u: object %u: a joint matrix of the blended layers is not finite", refused, poses[refused].obj_index)
                       : CtxFail(ctx, CGPT_ERR_INVALID, "entry %u: object %u: a joint matrix of the clip at time %g is not finite", refused, poses[refused].obj_index, (double)anim[refused].time);
    for (size_t k = 0; k < n; ++k) {
        const PosePlanEntry& e = plan.entries[k];
        const float* m = back.data() + 12 * (size_t)e.matrix_base;
        kept_matrices[e.source].assign(m, m + 12 * (size_t)e.n_joints);
    }
    return CGPT_OK;
}

int SetSkeleton(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_skeleton_desc* s)
{
    int rc = CheckObject(ctx, obj_index);
    if (rc != CGPT_OK) return rc;
    if (obj_index >= ctx->skins.size() || ctx->skins[obj_index].n_joints == 0u)
        return CtxFail(ctx, CGPT_ERR_INVALID, "object %u has no skin (cgpt_scene_set_skin installs one)", obj_index);
    std::string why;
    if (!CheckSkeleton(s, why)) return CtxFail(ctx, CGPT_ERR_INVALID, "%s", why.c_str());
    SkinBuffers& sk = ctx->skins[obj_index];
    if (s->n_joints != sk.n_joints) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u's skin has %u joints, the skeleton %u", obj_index, sk.n_joints, s->n_joints);

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                           // nothing uses the skeleton this one replaces
    const size_t n = s->n_joints;
    DevBuf<int32_t> parents;                                                   // installed whole, or not at all
    DevBuf<float> inverse_bind, rest, root;
    HIP_TRY(ctx, parents.Alloc(n));
    HIP_TRY(ctx, inverse_bind.Alloc(12 * n));
    HIP_TRY(ctx, rest.Alloc(10 * n));
    HIP_TRY(ctx, root.Alloc(12));
    HIP_TRY(ctx, hipMemcpy(parents.p, s->parents, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(inverse_bind.p, s->inverse_bind, sizeof(float) * 12 * n, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(rest.p, s->rest, sizeof(float) * 10 * n, hipMemcpyHostToDevice));
    if (s->root) HIP_TRY(ctx, hipMemcpy(root.p, s->root, sizeof(float) * 12, hipMemcpyHostToDevice));
    sk.parents = std::move(parents); sk.inverse_bind = std::move(inverse_bind); sk.rest = std::move(rest); sk.root = std::move(root);
    sk.has_root = s->root != nullptr;
    sk.has_skeleton = true;
    return CGPT_OK;
}

int ClipCreate(cgpt_ctx* ctx, const cgpt_clip_desc* desc, uint32_t* clip_out)
{
    if (!clip_out) return CtxFail(ctx, CGPT_ERR_INVALID, "clip_out is null");
    ClipTable table;
    std::string why;
    bool unsupported = false;
    if (!CheckClip(desc, table, why, unsupported)) return CtxFail(ctx, unsupported ? CGPT_ERR_UNSUPPORTED : CGPT_ERR_INVALID, "%s", why.c_str());
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ClipBuffers cb;                                                            // one element of room where an array is empty: no kernel argument is null
    const auto up = [&](auto& buf, const void* src, size_t count, size_t elem) -> hipError_t {
        const hipError_t e = buf.Alloc(std::max<size_t>(count, 1));
        return e != hipSuccess || count == 0 ? e : hipMemcpy(buf.p, src, count * elem, hipMemcpyHostToDevice);
    };
    HIP_TRY(ctx, up(cb.map, table.map.data(), table.map.size(), sizeof(uint32_t)));
    HIP_TRY(ctx, up(cb.channels, table.channels.data(), 4 * table.channels.size(), sizeof(uint32_t)));
    HIP_TRY(ctx, up(cb.times, table.times.data(), table.times.size(), sizeof(float)));
    HIP_TRY(ctx, up(cb.values, table.values.data(), table.values.size(), sizeof(float)));
    cb.n_joints = table.n_joints;
    cb.begin = table.begin; cb.end = table.end;
    ctx->clips.push_back(std::move(cb));                                       // a handle is never given twice
    *clip_out = (uint32_t)ctx->clips.size();
    return CGPT_OK;
}

const ClipBuffers* FindClip(const cgpt_ctx* ctx, uint32_t clip)
{
    return clip == 0u || clip > ctx->clips.size() || ctx->clips[clip - 1].n_joints == 0u ? nullptr : &ctx->clips[clip - 1];
}

int ClipDestroy(cgpt_ctx* ctx, uint32_t clip)
{
    if (!FindClip(ctx, clip)) return CtxFail(ctx, CGPT_ERR_INVALID, "clip %u is unknown or destroyed", clip);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->clips[clip - 1] = ClipBuffers{};
    return CGPT_OK;
}

int AnimateObjects(cgpt_ctx* ctx, const cgpt_animation* entries, uint32_t n)
{
    if (n == 0u) return CGPT_OK;
    if (!ctx->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "no scene uploaded");
    if (!entries) return CtxFail(ctx, CGPT_ERR_INVALID, "entries is null");
    std::vector<cgpt_pose> poses(n);
    std::vector<AnimResolved> anim(n);
    for (uint32_t i = 0; i < n; ++i) {
        const cgpt_animation& a = entries[i];
        const uint32_t o = a.obj_index;
        int rc = CheckObject(ctx, o);
        if (rc == CGPT_OK && (o >= ctx->skins.size() || ctx->skins[o].n_joints == 0u || !ctx->skins[o].has_skeleton))
            rc = CtxFail(ctx, CGPT_ERR_INVALID, "object %u has no skeleton (cgpt_scene_set_skeleton installs one on its skin)", o);
        const ClipBuffers* clip = FindClip(ctx, a.clip);
        if (rc == CGPT_OK && !clip) rc = CtxFail(ctx, CGPT_ERR_INVALID, "clip %u is unknown or destroyed", a.clip);
        if (rc == CGPT_OK && clip->n_joints != ctx->skins[o].n_joints)
            rc = CtxFail(ctx, CGPT_ERR_INVALID, "clip %u animates %u joints, object %u's skeleton has %u", a.clip, clip->n_joints, o, ctx->skins[o].n_joints);
        if (rc == CGPT_OK && !std::isfinite(a.time)) rc = CtxFail(ctx, CGPT_ERR_INVALID, "time is not finite");
        if (rc != CGPT_OK) { ctx->error = "entry " + std::to_string(i) + ": " + ctx->error; return rc; }
        poses[i] = cgpt_pose{ o, ctx->skins[o].n_joints, nullptr, a.n_targets, a.weights };
        anim[i] = { &ctx->skins[o], clip, a.time };
    }
    return PoseObjects(ctx, poses.data(), n, anim.data());
}

// cgpt_scene_animate_layers: AnimateObjects with every entry's layers checked, their times wrapped and their weights normalised here
// (animation.h: ResolveLayers), so the kernel receives plain times as animate_joints_batch does
int AnimateLayers(cgpt_ctx* ctx, const cgpt_layered_animation* entries, uint32_t n)
{
    if (n == 0u) return CGPT_OK;
    if (!ctx->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "no scene uploaded");
    if (!entries) return CtxFail(ctx, CGPT_ERR_INVALID, "entries is null");
    std::vector<cgpt_pose> poses(n);
    std::vector<AnimResolved> anim(n);
    for (uint32_t i = 0; i < n; ++i) {
        const cgpt_layered_animation& a = entries[i];
        const uint32_t o = a.obj_index;
        const ClipBuffers* clips[CGPT_ANIM_MAX_LAYERS] = {};
        float ranges[CGPT_ANIM_MAX_LAYERS][2] = {};
        int rc = CheckObject(ctx, o);
        if (rc == CGPT_OK && (o >= ctx->skins.size() || ctx->skins[o].n_joints == 0u || !ctx->skins[o].has_skeleton))
            rc = CtxFail(ctx, CGPT_ERR_INVALID, "object %u has no skeleton (cgpt_scene_set_skeleton installs one on its skin)", o);
        if (rc == CGPT_OK && !a.layers) rc = CtxFail(ctx, CGPT_ERR_INVALID, "layers is null");
        if (rc == CGPT_OK && (a.n_layers == 0u || a.n_layers > CGPT_ANIM_MAX_LAYERS)) rc = CtxFail(ctx, CGPT_ERR_INVALID, "n_layers %u outside [1, %u]", a.n_layers, CGPT_ANIM_MAX_LAYERS);
        for (uint32_t l = 0; rc == CGPT_OK && l < a.n_layers; ++l) {           // every layer's clip, inactive ones included
            const uint32_t handle = a.layers[l].clip;
            clips[l] = FindClip(ctx, handle);
            if (!clips[l]) rc = CtxFail(ctx, CGPT_ERR_INVALID, "layer %u: clip %u is unknown or destroyed", l, handle);
            else if (clips[l]->n_joints != ctx->skins[o].n_joints)
                rc = CtxFail(ctx, CGPT_ERR_INVALID, "layer %u: clip %u animates %u joints, object %u's skeleton has %u", l, handle, clips[l]->n_joints, o, ctx->skins[o].n_joints);
            else { ranges[l][0] = clips[l]->begin; ranges[l][1] = clips[l]->end; }
        }
        AnimActiveLayers active;
        std::string why;
        if (rc == CGPT_OK && !ResolveLayers(a.layers, a.n_layers, ranges, active, why)) rc = CtxFail(ctx, CGPT_ERR_INVALID, "%s", why.c_str());
        if (rc != CGPT_OK) { ctx->error = "entry " + std::to_string(i) + ": " + ctx->error; return rc; }
        poses[i] = cgpt_pose{ o, ctx->skins[o].n_joints, nullptr, a.n_targets, a.weights };
        AnimResolved& r = anim[i];
        r.skin = &ctx->skins[o]; r.clip = nullptr; r.time = 0.0f; r.n_layers = active.n;
        for (uint32_t k = 0; k < active.n; ++k) { r.layer_clip[k] = clips[active.index[k]]; r.layer_time[k] = active.time[k]; r.layer_weight[k] = active.weight[k]; }
    }
    return PoseObjects(ctx, poses.data(), n, anim.data());
}

int ClipGetRange(cgpt_ctx* ctx, uint32_t clip, float* begin, float* end)
{
    const ClipBuffers* c = FindClip(ctx, clip);
    if (!c) return CtxFail(ctx, CGPT_ERR_INVALID, "clip %u is unknown or destroyed", clip);
    if (begin) *begin = c->begin;
    if (end) *end = c->end;
    return CGPT_OK;
}

int GetJointMatrices(cgpt_ctx* ctx, uint32_t obj_index, float* out, uint32_t n_joints)
{
    int rc = CheckSkinJoints(ctx, obj_index, n_joints);
    if (rc != CGPT_OK) return rc;
    if (!out) return CtxFail(ctx, CGPT_ERR_INVALID, "out is null");
    const SkinBuffers& sk = ctx->skins[obj_index];
    if (sk.pose.empty()) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u's skin has not been posed", obj_index);
    memcpy(out, sk.pose.data(), sizeof(float) * sk.pose.size());
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

    // where the records are now: the renumbering put the top ones at the front, the rest keep their depth-first order -- or, after a
    // cgpt_scene_rebuild_mesh, sit in the mesh's span at the end of the array.  Two ranges are read: the mesh's names below n_top_records
    // and its others, so that a rebuilt mesh's export does not copy every record that lies between the two
    std::vector<uint32_t> stored(n_pairs);
    struct Range { uint32_t lo = 0xFFFFFFFFu, hi = 0; std::vector<float4> rec; std::vector<uint32_t> pair_of; };
    Range range[2];                                                           // [0] names below n_top_records, [1] the others
    const uint32_t n_top = ctx->scene.n_top_records;
    for (uint32_t k = 0; k < n_pairs; ++k) {
        stored[k] = ctx->record_perm[ro.pair_base + k];
        Range& g = range[stored[k] < n_top ? 0 : 1];
        g.lo = std::min(g.lo, stored[k]); g.hi = std::max(g.hi, stored[k]);
    }
    for (Range& g : range)
        if (g.lo <= g.hi) { g.rec.resize(4 * (size_t)(g.hi - g.lo + 1)); g.pair_of.assign(g.hi - g.lo + 1, 0xFFFFFFFFu); }   // stored record -> depth-first pair index k (nodes 2k+1, 2k+2)
    for (uint32_t k = 0; k < n_pairs; ++k) { Range& g = range[stored[k] < n_top ? 0 : 1]; g.pair_of[stored[k] - g.lo] = k; }
    std::vector<float4> leaf_tail(n_tris);                                    // {pad, e2.z, tri_idx, last_in_leaf} of every leaf slot
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (Range& g : range)
        if (!g.rec.empty()) HIP_TRY(ctx, hipMemcpy(g.rec.data(), ctx->sb.node_pairs.p + 4 * (size_t)g.lo, g.rec.size() * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy2D(leaf_tail.data(), sizeof(float4), ctx->sb.tri_leaf.p + 3 * (size_t)ro.leaf_base + 2, 3 * sizeof(float4),
                               sizeof(float4), n_tris, hipMemcpyDeviceToHost));
    const auto record_of = [&](uint32_t name) -> const float4* {             // a stored record's copy, null for a name outside both ranges
        const Range& g = range[name < n_top ? 0 : 1];
        return g.rec.empty() || name < g.lo || name > g.hi ? nullptr : g.rec.data() + 4 * (size_t)(name - g.lo);
    };
    const auto pair_index = [&](uint32_t name) -> uint32_t {
        const Range& g = range[name < n_top ? 0 : 1];
        return g.rec.empty() || name < g.lo || name > g.hi ? 0xFFFFFFFFu : g.pair_of[name - g.lo];
    };

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
        if (pair_index(code) == 0xFFFFFFFFu) return false;
        out.left_first = 2 * pair_index(code) + 1; out.prim_count = 0;
        return true;
    };
    auto set_bounds = [](cgpt_bvh_node& n, float x0, float y0, float z0, float x1, float y1, float z1) {
        n.aabb_min[0] = x0; n.aabb_min[1] = y0; n.aabb_min[2] = z0; n.aabb_max[0] = x1; n.aabb_max[1] = y1; n.aabb_max[2] = z1;
    };
    for (uint32_t k = 0; k < n_pairs; ++k) {
        const float4* rec = record_of(stored[k]);
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
        const float4* rec = record_of(d.root_code);                            // words() accepted the root: the name lies in a range
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

hipError_t FoldObjectBoxToHost(cgpt_ctx* ctx, uint32_t tri_base, uint32_t n_tris, uint32_t out[8])
{
    hipError_t e = hipStreamSynchronize(ctx->stream);                          // before the scratch may be replaced
    if (e == hipSuccess) e = ctx->sb.skin_scratch.Grow(kSkinScratchWords);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fold_object_box, dim3(1), dim3(kRefitThreads), 0, ctx->stream, ctx->sb.tri_orig.p, tri_base, n_tris, ctx->sb.skin_scratch.p);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(out, ctx->sb.skin_scratch.p, sizeof(uint32_t) * kSkinScratchWords, hipMemcpyDeviceToHost);
    return e;
}

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

int cgpt_scene_set_skin(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_triangle* bind_triangles, const uint16_t* joints, const float* weights,
                        uint32_t n_tris, uint32_t n_joints)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupSetSkin(ctx, obj_index, bind_triangles, joints, weights, n_tris, n_joints); });
    return Guarded(ctx, __func__, [&] { return SetSkin(ctx, obj_index, bind_triangles, joints, weights, n_tris, n_joints); });   // the scene does not change
}

int cgpt_scene_skin_mesh(cgpt_ctx* ctx, uint32_t obj_index, const float* joint_matrices, uint32_t n_joints)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupSkinMesh(ctx, obj_index, joint_matrices, n_joints); });
    ctx->scene_generation++; ctx->shape_generation++; ctx->pose_generation++;   // as a refit: guides and temporal history are stale (a call with
                                                                               // CGPT_TEMPORAL_FOLLOW_POSES keeps the history: pose_generation tells a pose from a refit)
    return Guarded(ctx, __func__, [&] { return SkinMesh(ctx, obj_index, joint_matrices, n_joints); });
}

int cgpt_scene_clear_skin(cgpt_ctx* ctx, uint32_t obj_index)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupClearSkin(ctx, obj_index); });
    return Guarded(ctx, __func__, [&] { return ClearSkin(ctx, obj_index); });
}

int cgpt_scene_set_morph_targets(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_triangle* base_triangles, const cgpt_triangle* target_deltas,
                                 uint32_t n_tris, uint32_t n_targets)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupSetMorphTargets(ctx, obj_index, base_triangles, target_deltas, n_tris, n_targets); });
    return Guarded(ctx, __func__, [&] { return SetMorphTargets(ctx, obj_index, base_triangles, target_deltas, n_tris, n_targets); });   // the scene does not change
}

int cgpt_scene_morph_mesh(cgpt_ctx* ctx, uint32_t obj_index, const float* weights, uint32_t n_targets)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupMorphMesh(ctx, obj_index, weights, n_targets); });
    return Guarded(ctx, __func__, [&] { return MorphMesh(ctx, obj_index, weights, n_targets); });   // bumps the generations once the call is accepted
}

int cgpt_scene_clear_morph_targets(cgpt_ctx* ctx, uint32_t obj_index)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupClearMorphTargets(ctx, obj_index); });
    return Guarded(ctx, __func__, [&] { return ClearMorphTargets(ctx, obj_index); });
}

int cgpt_scene_pose_objects(cgpt_ctx* ctx, const cgpt_pose* poses, uint32_t n_poses)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupPoseObjects(ctx, poses, n_poses); });
    return Guarded(ctx, __func__, [&] { return PoseObjects(ctx, poses, n_poses); });   // bumps the generations once the batch is accepted
}

int cgpt_scene_set_skeleton(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_skeleton_desc* skeleton)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupSetSkeleton(ctx, obj_index, skeleton); });
    return Guarded(ctx, __func__, [&] { return SetSkeleton(ctx, obj_index, skeleton); });   // the scene does not change
}

int cgpt_clip_create(cgpt_ctx* ctx, const cgpt_clip_desc* clip, uint32_t* clip_out)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupClipCreate(ctx, clip, clip_out); });
    return Guarded(ctx, __func__, [&] { return ClipCreate(ctx, clip, clip_out); });
}

int cgpt_clip_destroy(cgpt_ctx* ctx, uint32_t clip)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupClipDestroy(ctx, clip); });
    return Guarded(ctx, __func__, [&] { return ClipDestroy(ctx, clip); });
}

int cgpt_scene_animate_objects(cgpt_ctx* ctx, const cgpt_animation* entries, uint32_t n_entries)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupAnimateObjects(ctx, entries, n_entries); });
    return Guarded(ctx, __func__, [&] { return AnimateObjects(ctx, entries, n_entries); });   // bumps the generations once the batch is accepted
}

int cgpt_scene_animate_layers(cgpt_ctx* ctx, const cgpt_layered_animation* entries, uint32_t n_entries)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupAnimateLayers(ctx, entries, n_entries); });
    return Guarded(ctx, __func__, [&] { return AnimateLayers(ctx, entries, n_entries); });
}

int cgpt_clip_get_range(cgpt_ctx* ctx, uint32_t clip, float* begin, float* end)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return GroupForwarded(ctx, cgpt_clip_get_range(GroupFirstMember(ctx), clip, begin, end));
    return Guarded(ctx, __func__, [&] { return ClipGetRange(ctx, clip, begin, end); });
}

int cgpt_scene_get_joint_matrices(cgpt_ctx* ctx, uint32_t obj_index, float* out, uint32_t n_joints)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return GroupForwarded(ctx, cgpt_scene_get_joint_matrices(GroupFirstMember(ctx), obj_index, out, n_joints));
    return Guarded(ctx, __func__, [&] { return GetJointMatrices(ctx, obj_index, out, n_joints); });
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
