// tree_cost.hip -- cgpt_scene_tree_costs and cgpt_scene_rebuild_degraded: the surface-area cost of uploaded meshes' trees
// (csrc/host/tree_cost.h states the metric), summed on the device over the child-pair records as they are now -- after an upload, a refit,
// a pose or a rebuild -- and the policy on top of it that rebuilds the meshes whose cost has grown past a ratio of a reference.
// No other kernel changes, and the cost call writes nothing of the scene.
//
// One call, any number of entries, two launches:
//   * tree_cost_batch: a thread per record of an entry's slice of refit_levels (the slice names every record of the mesh, wherever it
//     lies: among the top slots, in the upload's depth-first run, in the span a rebuild gave the mesh).  Blocks of 256 threads are dealt
//     to the entries as pose_plan.h deals them: block b belongs to the last entry with first_block <= b, so what it reads of the entry
//     table -- and the root record, whose box every term is taken relative to -- is block-uniform.  A thread loads its record with four
//     16-byte loads, forms the two children's half areas (tree_cost.h: TreeCostHalfArea; a leaf child's triangle count is a walk over
//     tri_leaf to last_in_leaf, as fold_leaf walks) and adds them to exact integer sums (below); the block folds them in LDS and its
//     partial goes to scratch.
//   * tree_cost_finish: a block per entry folds the entry's partials and writes the entry's result.
// No atomic of either kind.  The sums are exact integers, so an entry's bits depend on its own tree alone -- not on where its records
// lie, not on the batch or its position in it, not on the device.  A name or a leaf slot outside the mesh's tables is never followed: it
// raises the entry's flag word and the host refuses the call.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "cpugpupt_abi.h"
#include "ctx_internal.h"
#include "device_scene.h"
#include "scene_layout.h"
#include "tree_cost.h"

namespace cgpt {
namespace {

constexpr uint32_t kCostThreads = 256;

// One entry as the kernels read it: 32 bytes
struct TreeCostEntry {
    uint32_t records_begin, n_records;          // refit_levels[records_begin .. records_begin + n_records): the mesh's records
    uint32_t root_code;                         // DevObject::root_code: the root's record
    uint32_t leaf_base, n_tris;                 // the mesh's slots of tri_leaf
    uint32_t first_block, blocks;               // its blocks of tree_cost_batch = where its partials lie
    uint32_t pad;
};
// The sums are exact, so that their order cannot matter: a rebuild on the device numbers the records of one depth in the order its
// level kernels allocated them, which is not the same from run to run, and a double sum in record order would differ in its last bit
// between two contexts that hold the same tree.  Every term is taken relative to the root box, q = H(c) / H(root) -- one correctly
// rounded division, the same bits wherever the record lies; a child box lies inside the root box, so q <= 1 -- and split into an
// integer part and four 32-bit limbs of fraction (128 bits: every bit of a q >= 2^-75, a smaller one cut at 2^-128).  Limbs are
// summed as 64-bit integers: a limb is below 2^32, a leaf's is multiplied by its triangle count, and a mesh has fewer than 2^26
// triangles and records, so no sum passes 2^58.  Integer addition is associative: any order, any block shape, the same bits.
constexpr int kCostLimbs = 5;                   // the integer part, then 2^-32, 2^-64, 2^-96, 2^-128
constexpr double kCostLimbMax = 4294967296.0;   // 2^32: a q at or above it is reported as not finite (no nested tree has one)
struct TreeCostPartial {                        // a block's partial, and an entry's sums: 96 bytes
    uint64_t inner[kCostLimbs], leaf[kCostLimbs];   // sum of q over inner children; sum of q n_l over leaf children
    uint32_t n_inner_children, n_leaves, max_leaf_tris;
    uint32_t bad;                               // 1: a name or a slot outside the mesh's tables; 2: a term that is not finite (or no root area)
};
static_assert(sizeof(TreeCostEntry) == 32 && sizeof(TreeCostPartial) == 96 && sizeof(cgpt_tree_cost) == 32, "the scratch is laid out in 32-byte units");
enum : uint32_t { kCostBadName = 1u, kCostNotFinite = 2u };

__device__ __forceinline__ uint32_t entry_of_block(const TreeCostEntry* __restrict__ entries, uint32_t n, uint32_t block)
{
    uint32_t lo = 0, hi = n;                    // the last entry whose first_block is not after `block` (first_block ascends from 0)
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) / 2u;
        if (entries[mid].first_block <= block) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void zero_partial(TreeCostPartial& p)
{
    for (int k = 0; k < kCostLimbs; ++k) { p.inner[k] = 0u; p.leaf[k] = 0u; }
    p.n_inner_children = 0u; p.n_leaves = 0u; p.max_leaf_tris = 0u; p.bad = 0u;
}

__device__ __forceinline__ void add_partial(TreeCostPartial& a, const TreeCostPartial& b)
{
    for (int k = 0; k < kCostLimbs; ++k) { a.inner[k] += b.inner[k]; a.leaf[k] += b.leaf[k]; }
    a.n_inner_children += b.n_inner_children; a.n_leaves += b.n_leaves;
    a.max_leaf_tris = b.max_leaf_tris > a.max_leaf_tris ? b.max_leaf_tris : a.max_leaf_tris;
    a.bad |= b.bad;
}

// q, 0 <= q < 2^32, times `times` into the limbs; every step is exact in double
__device__ __forceinline__ void add_term(uint64_t (&limbs)[kCostLimbs], double q, uint32_t times)
{
    double f = q;
    for (int k = 0; k < kCostLimbs; ++k) {
        const double whole = floor(f);
        limbs[k] += (uint64_t)whole * times;
        f = (f - whole) * kCostLimbMax;
    }
}

// the limbs as a double: from the least significant up, so that what the small limbs hold is not lost to the large ones' rounding
__device__ __forceinline__ double limbs_value(const uint64_t (&limbs)[kCostLimbs])
{
    double v = 0.0;
    for (int k = kCostLimbs - 1; k >= 0; --k) v = v / kCostLimbMax + (double)limbs[k];
    return v;
}

// the fold of a block: every thread's TreeCostPartial into thread 0's
__device__ __forceinline__ TreeCostPartial fold_block(const TreeCostPartial& mine)
{
    __shared__ TreeCostPartial s_part[kCostThreads];
    const uint32_t t = threadIdx.x;
    s_part[t] = mine;
    __syncthreads();
    for (uint32_t stride = kCostThreads / 2u; stride > 0u; stride /= 2u) {
        if (t < stride) add_partial(s_part[t], s_part[t + stride]);
        __syncthreads();
    }
    return s_part[0];
}

// the triangles of the leaf that starts at `slot`: the walk to last_in_leaf, kept inside the mesh's slots (0: the walk left them)
__device__ __forceinline__ uint32_t leaf_triangles(const float4* __restrict__ tri_leaf, uint32_t leaf_base, uint32_t n_tris, uint32_t slot)
{
    if (slot < leaf_base || slot - leaf_base >= n_tris) return 0u;
    const uint32_t end = leaf_base + n_tris;
    uint32_t count = 0u;
    for (;;) {
        ++count;
        const uint32_t last = __float_as_uint(reinterpret_cast<const float*>(tri_leaf + 3 * (size_t)slot + 2)[3]);
        if (last != 0u) return count;
        if (++slot >= end) return 0u;
    }
}

// H of the root box from the root's record (tree_cost.h: TreeCostRootHalfArea); the caller has checked the name
__device__ __forceinline__ double root_half_area(const float4* __restrict__ node_pairs, uint32_t root_code)
{
    const float4* rec = node_pairs + 4 * (size_t)root_code;
    const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2];
    const float l_lo[3] = { q0.x, q0.z, q1.x }, l_hi[3] = { q1.z, q2.x, q2.z }, r_lo[3] = { q0.y, q0.w, q1.y }, r_hi[3] = { q1.w, q2.y, q2.w };
    return TreeCostRootHalfArea(l_lo, l_hi, r_lo, r_hi);
}

__global__ __launch_bounds__(kCostThreads) void tree_cost_batch(const TreeCostEntry* __restrict__ entries, uint32_t n_entries, const float4* __restrict__ node_pairs,
                                                                uint32_t n_pair_records, const float4* __restrict__ tri_leaf,
                                                                const uint32_t* __restrict__ refit_levels, TreeCostPartial* __restrict__ partials)
{
    const TreeCostEntry e = entries[entry_of_block(entries, n_entries, blockIdx.x)];
    const uint32_t i = (blockIdx.x - e.first_block) * kCostThreads + threadIdx.x;
    TreeCostPartial mine;
    zero_partial(mine);
    const bool root_ok = e.root_code < n_pair_records;
    const double h_root = root_ok ? root_half_area(node_pairs, e.root_code) : 0.0;   // block-uniform: scalar loads
    if (!root_ok) mine.bad |= kCostBadName;
    else if (!(h_root > 0.0) || !(h_root < INFINITY)) mine.bad |= kCostNotFinite;
    if (mine.bad == 0u && i < e.n_records) {
        const uint32_t name = refit_levels[e.records_begin + i];
        if (name < n_pair_records) {
            const float4* rec = node_pairs + 4 * (size_t)name;                 // device_scene.h: node_pairs
            const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3];
            const uint32_t code[2] = { __float_as_uint(q3.z), __float_as_uint(q3.w) };
            const double h[2] = { TreeCostHalfArea(q0.x, q0.z, q1.x, q1.z, q2.x, q2.z), TreeCostHalfArea(q0.y, q0.w, q1.y, q1.w, q2.y, q2.w) };
            for (int side = 0; side < 2; ++side) {
                const double q = h[side] / h_root;
                if (!(q >= 0.0) || !(q < kCostLimbMax)) { mine.bad |= kCostNotFinite; continue; }
                if (code[side] & kLeafBit) {
                    const uint32_t leaf_tris = leaf_triangles(tri_leaf, e.leaf_base, e.n_tris, code[side] & ~kLeafBit);
                    if (leaf_tris == 0u) { mine.bad |= kCostBadName; continue; }
                    add_term(mine.leaf, q, leaf_tris);
                    mine.n_leaves += 1u;
                    mine.max_leaf_tris = leaf_tris > mine.max_leaf_tris ? leaf_tris : mine.max_leaf_tris;
                } else {
                    add_term(mine.inner, q, 1u);
                    mine.n_inner_children += 1u;
                }
            }
        } else {
            mine.bad |= kCostBadName;
        }
    }
    const TreeCostPartial sum = fold_block(mine);
    if (threadIdx.x == 0u) partials[blockIdx.x] = sum;
}

// cost = c_inner (1 + sum of q over inner children) + c_tri sum of q n_l over leaf children: tree_cost.h's quotient with the division
// by H(root) taken into every term.  results[k].reserved carries the entry's flag word to the host, which clears it
__global__ __launch_bounds__(kCostThreads) void tree_cost_finish(const TreeCostEntry* __restrict__ entries, const TreeCostPartial* __restrict__ partials,
                                                                 const float4* __restrict__ node_pairs, uint32_t n_pair_records, double c_inner, double c_tri,
                                                                 cgpt_tree_cost* __restrict__ results)
{
    const TreeCostEntry e = entries[blockIdx.x];
    TreeCostPartial mine;
    zero_partial(mine);
    for (uint32_t b = threadIdx.x; b < e.blocks; b += kCostThreads) add_partial(mine, partials[e.first_block + b]);
    const TreeCostPartial sum = fold_block(mine);
    if (threadIdx.x != 0u) return;
    cgpt_tree_cost out;
    out.cost = 0.0; out.root_half_area = 0.0;
    out.n_inner = sum.n_inner_children + 1u; out.n_leaves = sum.n_leaves; out.max_leaf_tris = sum.max_leaf_tris;
    out.reserved = sum.bad;
    if (e.root_code < n_pair_records) out.root_half_area = root_half_area(node_pairs, e.root_code);
    if (sum.bad == 0u) {
        out.cost = c_inner * (1.0 + limbs_value(sum.inner)) + c_tri * limbs_value(sum.leaf);
        if (out.n_inner != e.n_records) out.reserved = kCostBadName;          // every record but the root's is some record's inner child
    }
    results[blockIdx.x] = out;
}

int CheckCostConstants(cgpt_ctx* ctx, const char* call, double c_inner, double c_tri)
{
    if (!TreeCostConstantOk(c_inner)) return CtxFail(ctx, CGPT_ERR_INVALID, "%s: c_inner must be finite and > 0, got %g", call, c_inner);
    if (!TreeCostConstantOk(c_tri)) return CtxFail(ctx, CGPT_ERR_INVALID, "%s: c_tri must be finite and > 0, got %g", call, c_tri);
    return CGPT_OK;
}

// what cgpt_scene_tree_costs refuses of one entry of a context's scene
int CheckCostObject(cgpt_ctx* ctx, const cgpt_ctx* scene, uint32_t entry, uint32_t obj)
{
    if (obj >= scene->h_objects.size()) return CtxFail(ctx, CGPT_ERR_INVALID, "entry %u: object %u out of range (%zu objects)", entry, obj, scene->h_objects.size());
    if (scene->h_objects[obj].kind != CGPT_OBJECT_MESH) return CtxFail(ctx, CGPT_ERR_INVALID, "entry %u: object %u is no mesh: only a mesh has a tree", entry, obj);
    return CGPT_OK;
}

int TreeCosts(cgpt_ctx* ctx, const uint32_t* obj_indices, uint32_t n, double c_inner, double c_tri, cgpt_tree_cost* out)
{
    if (!ctx->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "no scene uploaded");
    int rc = CheckCostConstants(ctx, "cgpt_scene_tree_costs", c_inner, c_tri);
    if (rc != CGPT_OK) return rc;
    if (n == 0u) return CGPT_OK;
    if (!obj_indices) return CtxFail(ctx, CGPT_ERR_INVALID, "obj_indices is null");
    if (!out) return CtxFail(ctx, CGPT_ERR_INVALID, "out is null");

    std::vector<cgpt_tree_cost> results(n);
    std::vector<TreeCostEntry> entries;
    std::vector<uint32_t> source;                                              // the caller's index of every device entry
    uint32_t total_blocks = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t o = obj_indices[i];
        if ((rc = CheckCostObject(ctx, ctx, i, o)) != CGPT_OK) return rc;
        const DevObject& d = ctx->h_objects[o];
        const RefitObject& ro = ctx->refit_objects[o];
        if (ro.tri_count == 0u || ro.tri_count != d.n_tris) return CtxFail(ctx, CGPT_ERR_INVALID, "entry %u: object %u: the layout's triangle counts disagree", i, o);
        if (d.root_code & kLeafBit) {                                          // a root that never split: no record, no device work
            results[i] = { c_tri * (double)ro.tri_count, 0.0, 0u, 1u, ro.tri_count, 0u };
            continue;
        }
        const uint32_t n_records = ro.level_offsets.empty() ? 0u : ro.level_offsets.back();
        if (n_records == 0u || n_records != ro.node_count / 2u || (uint64_t)ro.level_begin + n_records > ctx->n_refit_levels)
            return CtxFail(ctx, CGPT_ERR_INVALID, "entry %u: object %u: the layout's record slice is inconsistent", i, o);
        const uint32_t blocks = (n_records + kCostThreads - 1u) / kCostThreads;
        entries.push_back({ ro.level_begin, n_records, d.root_code, ro.leaf_base, ro.tri_count, total_blocks, blocks, 0u });
        source.push_back(i);
        total_blocks += blocks;
    }
    const size_t m = entries.size();
    if (m != 0u) {
        // the scratch, in 32-bit words: results | entries | partials
        const size_t words = 8 * (2 * m) + sizeof(TreeCostPartial) / 4 * (size_t)total_blocks;
        std::vector<cgpt_tree_cost> back(m);
        hipStream_t stream = ctx->stream;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipStreamSynchronize(stream));
        HIP_TRY(ctx, ctx->sb.tree_cost.Grow(words));                           // the stream was just drained: nothing uses the old one
        cgpt_tree_cost* const d_results = reinterpret_cast<cgpt_tree_cost*>(ctx->sb.tree_cost.p);
        TreeCostEntry* const d_entries = reinterpret_cast<TreeCostEntry*>(ctx->sb.tree_cost.p + 8 * m);
        TreeCostPartial* const d_partials = reinterpret_cast<TreeCostPartial*>(ctx->sb.tree_cost.p + 16 * m);
        HIP_TRY(ctx, hipMemcpyAsync(d_entries, entries.data(), sizeof(TreeCostEntry) * m, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(tree_cost_batch, dim3(total_blocks), dim3(kCostThreads), 0, stream, d_entries, (uint32_t)m, ctx->sb.node_pairs.p, ctx->footprint.n_pair_records,
                           ctx->sb.tri_leaf.p, ctx->sb.refit_levels.p, d_partials);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(tree_cost_finish, dim3((uint32_t)m), dim3(kCostThreads), 0, stream, d_entries, d_partials, ctx->sb.node_pairs.p, ctx->footprint.n_pair_records,
                           c_inner, c_tri, d_results);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(back.data(), d_results, sizeof(cgpt_tree_cost) * m, hipMemcpyDeviceToHost, stream));   // the one readback
        HIP_TRY(ctx, hipStreamSynchronize(stream));
        for (size_t k = 0; k < m; ++k) {
            if (back[k].reserved & kCostBadName)
                return CtxFail(ctx, CGPT_ERR_HIP, "entry %u: object %u: a record or a leaf of the tree names something outside the mesh", source[k], obj_indices[source[k]]);
            results[source[k]] = back[k];
            if (back[k].reserved & kCostNotFinite) results[source[k]].cost = NAN;   // reported below, in the caller's order
            results[source[k]].reserved = 0u;
        }
    }
    for (uint32_t i = 0; i < n; ++i)
        if (!std::isfinite(results[i].cost) || !std::isfinite(results[i].root_half_area))
            return CtxFail(ctx, CGPT_ERR_INVALID, "entry %u: object %u: the cost is not finite (a bound that is not finite, or a root box without area)", i, obj_indices[i]);
    memcpy(out, results.data(), sizeof(cgpt_tree_cost) * n);
    return CGPT_OK;
}

int RebuildDegraded(cgpt_ctx* ctx, const cgpt_rebuild_candidate* entries, uint32_t n, double ratio, uint32_t build_option, double c_inner, double c_tri,
                    cgpt_rebuild_result* results)
{
    const cgpt_ctx* scene = ctx->group ? GroupFirstMember(ctx) : ctx;          // every member holds the same objects
    if (!ctx->has_scene || !scene->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "no scene uploaded");
    int rc = CheckCostConstants(ctx, "cgpt_scene_rebuild_degraded", c_inner, c_tri);
    if (rc != CGPT_OK) return rc;
    if (!TreeCostConstantOk(ratio)) return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_scene_rebuild_degraded: ratio must be finite and > 0, got %g", ratio);
    if (build_option > CGPT_BUILD_SAH_BINNED) return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_scene_rebuild_degraded: unknown build option %u", build_option);
    if (build_option == CGPT_BUILD_SAH_SPLIT_PRIMITIVES)
        return CtxFail(ctx, CGPT_ERR_UNSUPPORTED, "cgpt_scene_rebuild_degraded: SAH-split-primitives never splits (SURVEY A-5): nothing to rebuild with");
    if (n == 0u) return CGPT_OK;
    if (!entries) return CtxFail(ctx, CGPT_ERR_INVALID, "entries is null");
    if (!results) return CtxFail(ctx, CGPT_ERR_INVALID, "results is null");

    // what cgpt_scene_rebuild_mesh refuses without a launch, for every entry, before anything is rebuilt
    std::vector<uint32_t> objs(n);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t o = objs[i] = entries[i].obj_index;
        if ((rc = CheckCostObject(ctx, scene, i, o)) != CGPT_OK) return rc;
        if (!TreeCostConstantOk(entries[i].reference_cost))
            return CtxFail(ctx, CGPT_ERR_INVALID, "entry %u: reference_cost must be finite and > 0, got %g", i, entries[i].reference_cost);
        const RefitObject& ro = scene->refit_objects[o];
        if (ro.tri_count == 0u || ro.tri_count != scene->h_objects[o].n_tris) return CtxFail(ctx, CGPT_ERR_INVALID, "entry %u: object %u: the layout's triangle counts disagree", i, o);
        if (ro.span_base == kNoSpan && (uint64_t)scene->footprint.n_pair_records + (ro.tri_count - 1u) >= (1u << 26))
            return CtxFail(ctx, CGPT_ERR_INVALID, "entry %u: object %u: scene too large: a rebuild's record span would pass 2^26 records", i, o);
    }

    std::vector<cgpt_tree_cost> before(n);
    if ((rc = cgpt_scene_tree_costs(ctx, objs.data(), n, c_inner, c_tri, before.data())) != CGPT_OK) return rc;

    // the decision, once, from these numbers (a group's: its first member's); a copy that several entries reach is rebuilt once
    std::vector<uint32_t> rebuilt_groups, rebuild_through;
    const auto group_rebuilt = [&](uint32_t o) {
        for (const uint32_t g : rebuilt_groups) if (g == scene->mesh_group[o]) return true;
        return false;
    };
    for (uint32_t i = 0; i < n; ++i)
        if (before[i].cost > ratio * entries[i].reference_cost && !group_rebuilt(objs[i])) { rebuilt_groups.push_back(scene->mesh_group[objs[i]]); rebuild_through.push_back(i); }
    for (const uint32_t i : rebuild_through) {
        rc = cgpt_scene_rebuild_mesh(ctx, objs[i], build_option, nullptr, nullptr);
        if (rc != CGPT_OK) { ctx->error = "entry " + std::to_string(i) + ": " + ctx->error; return rc; }
    }
    std::vector<uint32_t> again, again_objs;
    for (uint32_t i = 0; i < n; ++i)
        if (group_rebuilt(objs[i])) { again.push_back(i); again_objs.push_back(objs[i]); }
    std::vector<cgpt_tree_cost> after(again.size());
    if (!again.empty() && (rc = cgpt_scene_tree_costs(ctx, again_objs.data(), (uint32_t)again.size(), c_inner, c_tri, after.data())) != CGPT_OK) return rc;
    for (uint32_t i = 0; i < n; ++i) results[i] = { before[i].cost, before[i].cost, 0u, 0u };
    for (size_t k = 0; k < again.size(); ++k) { results[again[k]].cost_after = after[k].cost; results[again[k]].rebuilt = 1u; }
    return CGPT_OK;
}

}  // namespace
}  // namespace cgpt

using namespace cgpt;

extern "C" int cgpt_scene_tree_costs(cgpt_ctx* ctx, const uint32_t* obj_indices, uint32_t n, double c_inner, double c_tri, cgpt_tree_cost* out)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupTreeCosts(ctx, obj_indices, n, c_inner, c_tri, out); });
    return Guarded(ctx, __func__, [&] { return TreeCosts(ctx, obj_indices, n, c_inner, c_tri, out); });
}

extern "C" int cgpt_scene_rebuild_degraded(cgpt_ctx* ctx, const cgpt_rebuild_candidate* entries, uint32_t n, double ratio, uint32_t build_option,
                                           double c_inner, double c_tri, cgpt_rebuild_result* results)
{
    if (!ctx) return CGPT_ERR_INVALID;
    return Guarded(ctx, __func__, [&] { return RebuildDegraded(ctx, entries, n, ratio, build_option, c_inner, c_tri, results); });
}
