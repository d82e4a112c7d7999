// scene_layout.hip -- LayoutScene: the reference's AoS scene validated and re-laid into the device layout of device_scene.h.
// Host code only (no kernel, no HIP runtime call, no context); a .hip file because device_scene.h needs the HIP headers for float4.
#include "scene_layout.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <exception>
#include <map>
#include <tuple>

#include "cpugpupt_host.h"

namespace cgpt {
void HostSetError(const char* msg);                                           // host_capi.cpp: the text behind cgpth_last_error()

namespace {

int Refuse(std::string& error, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    error = buf;
    return code;
}

uint32_t LeafRecords(const cgpt_object& o)                                    // a triangle object has one leaf record, like a one-triangle mesh
{
    return o.kind == CGPT_OBJECT_MESH ? o.tri_count : (o.kind == CGPT_OBJECT_TRIANGLE ? 1u : 0u);
}

// The mesh groups of an instanced layout (cgpt_scene_upload_instanced): mesh objects whose four slice words are all equal share one copy,
// laid out from the first of them.  group[oi] is that first object, oi itself for every object that shares with nobody -- which is every
// object of the plain layout.  Slices that overlap only in part are different keys: separate meshes.
std::vector<uint32_t> MeshGroups(const cgpt_scene_desc& sd, bool instanced)
{
    std::vector<uint32_t> group(sd.n_objects);
    std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>, uint32_t> first;
    for (uint32_t oi = 0; oi < sd.n_objects; ++oi) {
        const cgpt_object& o = sd.objects[oi];
        group[oi] = oi;
        if (instanced && o.kind == CGPT_OBJECT_MESH) group[oi] = first.emplace(std::make_tuple(o.node_offset, o.node_count, o.tri_offset, o.tri_count), oi).first->second;
    }
    return group;
}

// leaf-record order (device_scene.h): the triangles of the small meshes first, then the rest in object order; a mesh group counts once,
// at its first member.  Returns the first tri_leaf record of every object, sets n_small_tris and returns the number of records in `total`.
std::vector<uint32_t> LeafRecordOrder(const cgpt_scene_desc& sd, const std::vector<uint32_t>& group, uint32_t& n_small_tris, uint64_t& total)
{
    std::vector<uint32_t> leaf_base_of(sd.n_objects, 0);
    std::vector<uint8_t> small(sd.n_objects, 0);
    n_small_tris = 0; total = 0;
    for (uint32_t oi = 0; oi < sd.n_objects; ++oi) {
        if (group[oi] != oi) continue;
        const uint32_t n = LeafRecords(sd.objects[oi]);
        total += n;
        if (n > 0 && n <= kSmallMeshTris && n_small_tris + n <= kLdsTrisMax) { small[oi] = 1; leaf_base_of[oi] = n_small_tris; n_small_tris += n; }
    }
    uint32_t next = n_small_tris;
    for (uint32_t oi = 0; oi < sd.n_objects; ++oi)
        if (group[oi] == oi && !small[oi]) { leaf_base_of[oi] = next; next += LeafRecords(sd.objects[oi]); }
    for (uint32_t oi = 0; oi < sd.n_objects; ++oi) leaf_base_of[oi] = leaf_base_of[group[oi]];
    return leaf_base_of;
}

// The records of mesh object oi: its slices validated, leaf-ordered and original-order triangles, child-pair records in the
// reference's node order (RenumberRecords moves them), each record's depth in rec_depth (0xFF: not reached), the deepest node in
// max_tree_depth.  out.tri_leaf is sized by the caller.
int LayoutMesh(const cgpt_scene_desc& sd, uint32_t oi, uint32_t leaf_base, SceneLayout& out, std::vector<uint8_t>& rec_depth,
               uint32_t& max_tree_depth, std::string& error)
{
    const cgpt_object& o = sd.objects[oi];
    DevObject& d = out.objects[oi];
    if (!sd.nodes || !sd.triangles || !sd.tri_indices) return Refuse(error, CGPT_ERR_INVALID, "mesh object %u but nodes/triangles/tri_indices is null", oi);
    if (o.node_count == 0 || (uint64_t)o.node_offset + o.node_count > sd.n_nodes) return Refuse(error, CGPT_ERR_INVALID, "object %u: node slice out of range", oi);
    if (o.tri_count == 0 || (uint64_t)o.tri_offset + o.tri_count > sd.n_triangles) return Refuse(error, CGPT_ERR_INVALID, "object %u: triangle slice out of range", oi);
    if ((o.node_count & 1u) == 0) return Refuse(error, CGPT_ERR_INVALID, "object %u: a binary BVH has an odd node count, got %u", oi, o.node_count);
    const cgpt_bvh_node* nodes = sd.nodes + o.node_offset;
    const cgpt_triangle* tris = sd.triangles + o.tri_offset;
    const uint32_t* tidx = sd.tri_indices + o.tri_offset;

    std::vector<float4>& pairs = out.node_pairs;
    const uint32_t pair_base = (uint32_t)(pairs.size() / 4);
    const uint32_t orig_base = (uint32_t)(out.tri_orig.size() / 3);
    // record byte offsets are computed in 32 bits on the device (64-byte pairs, 48-byte leaf triangles)
    if ((uint64_t)leaf_base + o.tri_count >= (1u << 26) || (uint64_t)pair_base + o.node_count / 2 >= (1u << 26))
        return Refuse(error, CGPT_ERR_INVALID, "scene too large: more than 2^26 triangles or inner nodes");

    auto code_of = [&](uint32_t node_index, uint32_t& code) -> bool {
        const cgpt_bvh_node& n = nodes[node_index];
        if (n.prim_count > 0) {
            if ((uint64_t)n.left_first + n.prim_count > o.tri_count) return false;
            code = kLeafBit | (leaf_base + n.left_first);
            return true;
        }
        // children were allocated as a pair after the parent: odd index, both in range, both beyond the parent
        if ((n.left_first & 1u) == 0 || n.left_first <= node_index || (uint64_t)n.left_first + 1 >= o.node_count) return false;
        code = pair_base + (n.left_first - 1) / 2;
        return true;
    };

    uint32_t root_code;
    if (!code_of(0, root_code)) return Refuse(error, CGPT_ERR_INVALID, "object %u: malformed BVH root", oi);
    d.root_code = root_code; d.tri_base = orig_base; d.n_tris = o.tri_count; d.total_area = o.total_area;
    RefitObject& ro = out.refit_objects[oi];
    ro.node_count = o.node_count; ro.tri_count = o.tri_count; ro.leaf_base = leaf_base; ro.pair_base = pair_base;

    // leaf-ordered triangle records
    float4* leaf = out.tri_leaf.data() + 3 * (size_t)leaf_base;
    for (uint32_t i = 0; i < o.tri_count; ++i) {
        const uint32_t t = tidx[i];
        if (t >= o.tri_count) return Refuse(error, CGPT_ERR_INVALID, "object %u: tri_indices[%u] = %u out of range", oi, i, t);
        PackLeafTri(tris[t], t, leaf + 3 * (size_t)i);
    }
    // original-order records for GetTriangle users
    out.tri_orig.resize(out.tri_orig.size() + 3 * (size_t)o.tri_count);
    float4* orig = out.tri_orig.data() + 3 * (size_t)orig_base;
    for (uint32_t t = 0; t < o.tri_count; ++t) {
        const cgpt_triangle& tr = tris[t];
        PackOrigTri(tr, orig + 3 * (size_t)t);
        out.tri_normal.push_back(make_float4(tr.v0.normal[0], tr.v0.normal[1], tr.v0.normal[2], 0.0f));   // TriangleNormal, ref: Primitives.cpp:148-151
        float4 pair[2];
        PackNormalPair(tr, pair);
        out.tri_normal12.push_back(pair[0]); out.tri_normal12.push_back(pair[1]);
    }

    // child-pair records + leaf terminators; iterative DFS from the root also measures the real depth
    pairs.resize(pairs.size() + 4 * (size_t)(o.node_count / 2), make_float4(0, 0, 0, 0));
    rec_depth.resize(pairs.size() / 4, 0xFF);
    float4* pr = pairs.data() + 4 * (size_t)pair_base;
    std::vector<uint8_t> covered(o.tri_count, 0);
    struct Item { uint32_t node, depth; };
    std::vector<Item> todo;
    todo.push_back({ 0, 0 });
    uint32_t visited = 0;
    while (!todo.empty()) {
        const Item it = todo.back(); todo.pop_back();
        if (++visited > o.node_count) return Refuse(error, CGPT_ERR_INVALID, "object %u: BVH is not a tree", oi);
        if (it.depth > max_tree_depth) max_tree_depth = it.depth;
        const cgpt_bvh_node& n = nodes[it.node];
        if (n.prim_count > 0) {
            if ((uint64_t)n.left_first + n.prim_count > o.tri_count) return Refuse(error, CGPT_ERR_INVALID, "object %u: leaf %u out of range", oi, it.node);
            for (uint32_t i = n.left_first; i < n.left_first + n.prim_count; ++i) {
                if (covered[i]) return Refuse(error, CGPT_ERR_INVALID, "object %u: triangle slot %u is in two leaves", oi, i);
                covered[i] = 1;
            }
            leaf[3 * (size_t)(n.left_first + n.prim_count - 1) + 2].w = AsFloat(1u);     // last_in_leaf
            continue;
        }
        uint32_t lc, rc, dummy;
        if (!code_of(it.node, dummy)) return Refuse(error, CGPT_ERR_INVALID, "object %u: malformed inner node %u", oi, it.node);
        const uint32_t L = n.left_first;
        if (!code_of(L, lc) || !code_of(L + 1, rc)) return Refuse(error, CGPT_ERR_INVALID, "object %u: malformed children of node %u", oi, it.node);
        float4* rec = pr + 4 * (size_t)((L - 1) / 2);
        rec_depth[pair_base + (L - 1) / 2] = (uint8_t)std::min<uint32_t>(it.depth, 0xFEu);   // > 63 is refused by the caller
        const cgpt_bvh_node& l = nodes[L]; const cgpt_bvh_node& r = nodes[L + 1];
        // left / right interleaved per component: one packed-f32 instruction handles both children (device_scene.h)
        rec[0] = make_float4(l.aabb_min[0], r.aabb_min[0], l.aabb_min[1], r.aabb_min[1]);
        rec[1] = make_float4(l.aabb_min[2], r.aabb_min[2], l.aabb_max[0], r.aabb_max[0]);
        rec[2] = make_float4(l.aabb_max[1], r.aabb_max[1], l.aabb_max[2], r.aabb_max[2]);
        rec[3] = make_float4(0.0f, 0.0f, AsFloat(lc), AsFloat(rc));
        todo.push_back({ L + 1, it.depth + 1 });
        todo.push_back({ L, it.depth + 1 });
    }
    return CGPT_OK;
}

bool HasRecords(const DevObject& d) { return d.kind == CGPT_OBJECT_MESH && (d.root_code & kLeafBit) == 0u; }

// record order (device_scene.h: "record order").  The reference allocates nodes depth-first; a record's index is only a name here
// (codes are rewritten), so the records are renumbered: the first kTopRecords in breadth-first order over all meshes (the top of
// every tree, which every ray walks: the trace kernel mirrors records [0, n_top_records) in LDS), the rest in the reference's order.
// The breadth-first queue starts with one root per mesh group: the members of a group hold the same root, and a record is queued once.
void RenumberRecords(SceneLayout& out)
{
    std::vector<float4>& pairs = out.node_pairs;
    const uint32_t n_records = (uint32_t)(pairs.size() / 4);
    std::vector<uint32_t>& perm = out.record_perm;
    perm.assign(n_records, 0xFFFFFFFFu);
    std::vector<uint32_t> bfs; bfs.reserve(n_records);
    for (size_t oi = 0; oi < out.objects.size(); ++oi)
        if (out.mesh_group[oi] == oi && HasRecords(out.objects[oi])) bfs.push_back(out.objects[oi].root_code);
    const size_t bfs_limit = std::min<size_t>(n_records, kTopRecords);
    for (size_t head = 0; head < bfs.size() && bfs.size() < n_records; ++head) {
        if (bfs.size() >= bfs_limit + 2 * kTopRecords) break;                  // enough: only the first bfs_limit are used
        const float4& cc = pairs[4 * (size_t)bfs[head] + 3];
        uint32_t lc, rc; memcpy(&lc, &cc.z, 4); memcpy(&rc, &cc.w, 4);
        if ((lc & kLeafBit) == 0u) bfs.push_back(lc);
        if ((rc & kLeafBit) == 0u) bfs.push_back(rc);
    }
    uint32_t next = 0;
    for (size_t i = 0; i < bfs.size() && i < bfs_limit; ++i) perm[bfs[i]] = next++;
    for (uint32_t r = 0; r < n_records; ++r) if (perm[r] == 0xFFFFFFFFu) perm[r] = next++;
    std::vector<float4> moved(pairs.size());
    for (uint32_t r = 0; r < n_records; ++r) {
        float4* dst = moved.data() + 4 * (size_t)perm[r];
        const float4* src = pairs.data() + 4 * (size_t)r;
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
        uint32_t lc, rc; memcpy(&lc, &src[3].z, 4); memcpy(&rc, &src[3].w, 4);
        if ((lc & kLeafBit) == 0u) lc = perm[lc];
        if ((rc & kLeafBit) == 0u) rc = perm[rc];
        dst[3].z = AsFloat(lc); dst[3].w = AsFloat(rc);
    }
    pairs.swap(moved);
    for (DevObject& d : out.objects)
        if (HasRecords(d)) d.root_code = perm[d.root_code];
    out.n_pair_records = n_records;
    out.n_top_records = (uint32_t)std::min(bfs.size(), bfs_limit);
}

// each mesh's child-pair records grouped by depth, in their final numbering: the refit's bound pass runs one level after the other,
// deepest first (refit.hip).  Once per mesh group: every member carries the group's bases and levels, so a refit through any of them
// runs over the one copy.
void GroupRecordsByDepth(SceneLayout& out, const std::vector<uint8_t>& rec_depth)
{
    std::vector<uint32_t>& levels = out.refit_levels;
    levels.reserve(out.n_pair_records);
    for (size_t oi = 0; oi < out.objects.size(); ++oi) {
        RefitObject& ro = out.refit_objects[oi];
        if (out.mesh_group[oi] != oi || out.objects[oi].kind != CGPT_OBJECT_MESH || ro.node_count < 3) continue;   // a leaf-rooted mesh has no records
        uint32_t count[66] = { 0 };
        uint32_t n_levels = 0;
        const uint32_t r0 = ro.pair_base, r1 = ro.pair_base + ro.node_count / 2;
        for (uint32_t r = r0; r < r1; ++r)
            if (rec_depth[r] != 0xFF) { ++count[rec_depth[r] + 1]; n_levels = std::max<uint32_t>(n_levels, rec_depth[r] + 1u); }
        for (uint32_t d = 0; d < n_levels; ++d) count[d + 1] += count[d];
        ro.level_begin = (uint32_t)levels.size();
        ro.level_offsets.assign(count, count + n_levels + 1);
        levels.resize(levels.size() + count[n_levels]);
        uint32_t* dst = levels.data() + ro.level_begin;
        for (uint32_t r = r0; r < r1; ++r)
            if (rec_depth[r] != 0xFF) dst[count[rec_depth[r]]++] = out.record_perm[r];
    }
    for (size_t oi = 0; oi < out.objects.size(); ++oi)
        if (out.mesh_group[oi] != oi) out.refit_objects[oi] = out.refit_objects[out.mesh_group[oi]];
}

}  // namespace

int LayoutScene(const cgpt_scene_desc& sd, SceneLayout& out, std::string& error, bool instanced)
{
    out = SceneLayout();
    if (sd.n_objects == 0 || !sd.objects) return Refuse(error, CGPT_ERR_INVALID, "scene has no objects");
    if (sd.n_materials == 0 || !sd.materials) return Refuse(error, CGPT_ERR_INVALID, "scene has no materials");
    if (sd.n_lights && !sd.light_indices) return Refuse(error, CGPT_ERR_INVALID, "light_indices is null");

    out.mesh_group = MeshGroups(sd, instanced);
    uint64_t n_leaf_records = 0;                                              // laid-out records: a mesh group counts once
    const std::vector<uint32_t> leaf_base_of = LeafRecordOrder(sd, out.mesh_group, out.n_small_tris, n_leaf_records);
    if (n_leaf_records >= (1u << 26)) return Refuse(error, CGPT_ERR_INVALID, "scene too large: more than 2^26 triangles or inner nodes");
    out.tri_leaf.resize(3 * (size_t)n_leaf_records);
    out.tri_normal12.reserve(2 * (size_t)n_leaf_records);                      // one {n1, n2} pair per leaf record: no regrowth while the objects are laid out

    out.objects.resize(sd.n_objects);
    out.refit_objects.resize(sd.n_objects);
    out.top_state.local_box.assign(6 * (size_t)sd.n_objects, 0.0f);
    out.top_state.xform.resize(12 * (size_t)sd.n_objects);
    for (uint32_t oi = 0; oi < sd.n_objects; ++oi) {
        static const float kIdentity[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
        memcpy(out.top_state.xform.data() + 12 * (size_t)oi, kIdentity, sizeof(kIdentity));
    }
    uint32_t max_tree_depth = 0;
    std::vector<uint8_t> rec_depth;                                           // depth of every child-pair record (0xFF: not reached)
    for (uint32_t oi = 0; oi < sd.n_objects; ++oi) {
        const cgpt_object& o = sd.objects[oi];
        DevObject& d = out.objects[oi];
        memset(&d, 0, sizeof(d));
        d.kind = o.kind; d.mat_index = o.mat_index;
        if (o.mat_index >= sd.n_materials) return Refuse(error, CGPT_ERR_INVALID, "object %u: mat_index %u out of range", oi, o.mat_index);
        if (o.kind == CGPT_OBJECT_SPHERE) {
            memcpy(d.sphere_center, o.sphere_center, 12);
            d.sphere_radius = o.sphere_radius;
            d.sphere_radius_sq = o.sphere_radius * o.sphere_radius;                  // Sphere ctor, ref: Primitives.h:38-39
        } else if (o.kind == CGPT_OBJECT_PLANE) {
            memcpy(d.plane_normal, o.plane_normal, 12);
            memcpy(d.plane_point, o.plane_point, 12);
        } else if (o.kind == CGPT_OBJECT_TRIANGLE) {
            // Primitive(const Triangle&) (ref: Primitives.h:84-89): one leaf record as the root, so the trace kernels test it with
            // their leaf step -- IntersectTriangle (ref: Primitives.cpp:292-305) -- and its shading normal is v0.normal (:308-321)
            if (!sd.triangles) return Refuse(error, CGPT_ERR_INVALID, "triangle object %u but triangles is null", oi);
            if (o.tri_count != 1 || o.node_count != 0)
                return Refuse(error, CGPT_ERR_INVALID, "object %u: a triangle object has tri_count 1 and node_count 0, got %u and %u", oi, o.tri_count, o.node_count);
            if (o.tri_offset >= sd.n_triangles) return Refuse(error, CGPT_ERR_INVALID, "object %u: triangle %u out of range", oi, o.tri_offset);
            const cgpt_triangle& tr = sd.triangles[o.tri_offset];
            const uint32_t leaf_base = leaf_base_of[oi];
            const uint32_t orig_base = (uint32_t)(out.tri_orig.size() / 3);
            float4* leaf = out.tri_leaf.data() + 3 * (size_t)leaf_base;
            PackLeafTri(tr, 0u, leaf);
            leaf[2].w = AsFloat(1u);                                          // last_in_leaf
            out.tri_orig.resize(out.tri_orig.size() + 3);
            PackOrigTri(tr, out.tri_orig.data() + 3 * (size_t)orig_base);
            out.tri_normal.push_back(make_float4(tr.v0.normal[0], tr.v0.normal[1], tr.v0.normal[2], 0.0f));   // TriangleNormal, ref: Primitives.cpp:148-151
            float4 pair[2];
            PackNormalPair(tr, pair);
            out.tri_normal12.push_back(pair[0]); out.tri_normal12.push_back(pair[1]);
            d.root_code = kLeafBit | leaf_base; d.tri_base = orig_base; d.n_tris = 1;
            TriangleBounds(&tr, 1, out.top_state.local_box.data() + 6 * (size_t)oi);
            out.refit_objects[oi].tri_count = 1; out.refit_objects[oi].leaf_base = leaf_base;
        } else if (o.kind == CGPT_OBJECT_MESH && out.mesh_group[oi] != oi) {
            // an instance: the copy its group's first member laid out (the same four slice words, so the same validation passed)
            const uint32_t first = out.mesh_group[oi];
            d.root_code = out.objects[first].root_code; d.tri_base = out.objects[first].tri_base; d.n_tris = out.objects[first].n_tris;
            d.total_area = o.total_area;
            out.refit_objects[oi] = out.refit_objects[first];                  // the levels follow in GroupRecordsByDepth
            memcpy(out.top_state.local_box.data() + 6 * (size_t)oi, out.top_state.local_box.data() + 6 * (size_t)first, 24);
        } else if (o.kind == CGPT_OBJECT_MESH) {
            const int rc = LayoutMesh(sd, oi, leaf_base_of[oi], out, rec_depth, max_tree_depth, error);
            if (rc != CGPT_OK) return rc;
            float* box = out.top_state.local_box.data() + 6 * (size_t)oi;      // the root node's bounds; a leaf root: its triangles'
            const cgpt_bvh_node& root = sd.nodes[o.node_offset];
            if (root.prim_count > 0) TriangleBounds(sd.triangles + o.tri_offset, o.tri_count, box);
            else { memcpy(box, root.aabb_min, 12); memcpy(box + 3, root.aabb_max, 12); }
        } else {
            return Refuse(error, CGPT_ERR_UNSUPPORTED, "object %u: primitive kind %u has no intersector (the reference EXCEPTs on AABB too, Primitives.cpp:302-305)", oi, o.kind);
        }
    }

    for (uint32_t i = 0; i < sd.n_lights; ++i) {
        const uint32_t li = sd.light_indices[i];
        if (li >= sd.n_objects) return Refuse(error, CGPT_ERR_INVALID, "light_indices[%u] = %u out of range", i, li);
        if (sd.objects[li].kind != CGPT_OBJECT_MESH && sd.objects[li].kind != CGPT_OBJECT_SPHERE)   // planes and triangle objects
            return Refuse(error, CGPT_ERR_UNSUPPORTED, "light %u (object %u, kind %u): only mesh and sphere lights can be sampled (the reference EXCEPTs, Main.cpp:383)",
                          i, li, sd.objects[li].kind);
    }

    out.stack_depth = max_tree_depth + 1;
    if (out.stack_depth > 64) return Refuse(error, CGPT_ERR_UNSUPPORTED, "BVH depth %u exceeds the traversal stack of 64 (ref: BVH.cpp:66)", max_tree_depth);

    out.n_materials = sd.n_materials;
    out.materials.resize(4 * (size_t)sd.n_materials);
    for (uint32_t i = 0; i < sd.n_materials; ++i) PackMaterial(sd.materials[i], 0.0f, 0.0f, out.materials.data() + 4 * (size_t)i);   // an upload resets both roughnesses
    out.lights.assign(sd.light_indices, sd.light_indices + sd.n_lights);

    RenumberRecords(out);
    GroupRecordsByDepth(out, rec_depth);

    // per-object records for the trace kernel's object phase (device_scene.h: obj_trace)
    out.obj_trace.resize(2 * (size_t)sd.n_objects);
    for (uint32_t oi = 0; oi < sd.n_objects; ++oi) PackObjTrace(out.objects[oi], out.obj_trace[2 * (size_t)oi], out.obj_trace[2 * (size_t)oi + 1]);
    out.obj_xform.resize(3 * (size_t)sd.n_objects);                            // an upload resets every transform to the identity
    for (uint32_t oi = 0; oi < sd.n_objects; ++oi) IdentityTransformRecords(out.obj_xform.data() + 3 * (size_t)oi);
    return CGPT_OK;
}

void TriangleBounds(const cgpt_triangle* triangles, size_t n, float box[6])
{
    for (int a = 0; a < 3; ++a) { box[a] = INFINITY; box[3 + a] = -INFINITY; }
    bool finite = n > 0;
    for (size_t i = 0; i < n; ++i) {
        const float* const p[3] = { triangles[i].v0.pos, triangles[i].v1.pos, triangles[i].v2.pos };
        for (int v = 0; v < 3; ++v)
            for (int a = 0; a < 3; ++a) {
                const float x = p[v][a];
                finite = finite && std::isfinite(x);
                if (x < box[a]) box[a] = x;
                if (x > box[3 + a]) box[3 + a] = x;
            }
    }
    if (!finite) UnboundedBox(box);                                           // a NaN would slip through the comparisons
}

void TopLevelLeafBox(const DevObject& d, const float local_box[6], const float xform[12], float box[6])
{
    if (d.kind == CGPT_OBJECT_SPHERE) {
        for (int a = 0; a < 3; ++a) { box[a] = d.sphere_center[a] - d.sphere_radius; box[3 + a] = d.sphere_center[a] + d.sphere_radius; }
        for (int a = 0; a < 3; ++a)
            if (!(box[a] <= box[3 + a])) { UnboundedBox(box); break; }        // a negative or NaN radius: no box to trust
    } else if (d.kind == CGPT_OBJECT_PLANE) {
        UnboundedBox(box);
    } else {
        memcpy(box, local_box, 24);
        if (!IsFiniteBox(box)) UnboundedBox(box);
        else if (!IsIdentityTransform(xform)) TransformBox(xform, local_box, box);
    }
    PadBox(box);
}

namespace {
struct TopLevelBuilder {
    const std::vector<float>& leaf;                                           // 6 per object
    std::vector<float4>& nodes;
    std::vector<uint32_t>& entry;
    void Build(uint32_t i, uint32_t j, float box[6])
    {
        const size_t k = nodes.size() / 2;
        nodes.resize(nodes.size() + 2);
        if (entry[i] == 0xFFFFFFFFu) entry[i] = (uint32_t)k;                  // preorder: the first node that starts at i is the highest
        uint32_t object = 0xFFFFFFFFu;
        if (j - i == 1) { memcpy(box, leaf.data() + 6 * (size_t)i, 24); object = i; }
        else {
            const uint32_t m = i + (j - i + 1) / 2;
            float right[6];
            Build(i, m, box);
            Build(m, j, right);
            for (int a = 0; a < 3; ++a) { if (right[a] < box[a]) box[a] = right[a]; if (right[3 + a] > box[3 + a]) box[3 + a] = right[3 + a]; }
        }
        nodes[2 * k] = make_float4(box[0], box[1], box[2], AsFloat((uint32_t)(nodes.size() / 2)));   // skip: the first node behind this subtree
        nodes[2 * k + 1] = make_float4(box[3], box[4], box[5], AsFloat(object));
    }
};
}  // namespace

void LayoutTopLevel(const std::vector<DevObject>& objects, const TopLevelState& st, std::vector<float4>& nodes, std::vector<uint32_t>& entry)
{
    const uint32_t n = (uint32_t)objects.size();
    nodes.clear(); entry.assign((size_t)n + 1, 0xFFFFFFFFu);
    if (n == 0) { entry[0] = 0; return; }
    std::vector<float> leaf(6 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) TopLevelLeafBox(objects[i], st.local_box.data() + 6 * (size_t)i, st.xform.data() + 12 * (size_t)i, leaf.data() + 6 * (size_t)i);
    nodes.reserve(2 * (2 * (size_t)n - 1));
    TopLevelBuilder b{ leaf, nodes, entry };
    float box[6];
    b.Build(0, n, box);
    entry[n] = 2 * n - 1;
}

std::vector<float4> PackTopLevel(const std::vector<DevObject>& objects, const TopLevelState& st)
{
    std::vector<float4> nodes;
    std::vector<uint32_t> entry;
    LayoutTopLevel(objects, st, nodes, entry);
    std::vector<float4> blob(TopLevelFloat4s(objects.size()), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    if (!nodes.empty()) memcpy(blob.data(), nodes.data(), nodes.size() * sizeof(float4));
    if (!blob.empty()) memcpy(blob.data() + nodes.size(), entry.data(), entry.size() * sizeof(uint32_t));
    return blob;
}

int LayoutTransforms(const float* object_to_world, uint32_t n_objects, const std::vector<DevObject>& objects, const std::vector<uint32_t>& lights,
                     std::vector<float4>& records, std::vector<uint32_t>& flags, std::string& error)
{
    if (!object_to_world || n_objects != objects.size()) return Refuse(error, CGPT_ERR_INVALID, "expected %zu object-to-world matrices of 12 floats", objects.size());
    records.resize(3 * (size_t)n_objects);
    flags.assign(n_objects, 0u);
    for (uint32_t i = 0; i < n_objects; ++i) {
        const float* m = object_to_world + 12 * (size_t)i;
        float4* rec = records.data() + 3 * (size_t)i;
        if (IsIdentityTransform(m)) { IdentityTransformRecords(rec); continue; }
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(m[k])) return Refuse(error, CGPT_ERR_INVALID, "object %u: transform entry %d is not finite", i, k);
        if (objects[i].kind != CGPT_OBJECT_MESH && objects[i].kind != CGPT_OBJECT_TRIANGLE)
            return Refuse(error, CGPT_ERR_INVALID, "object %u is a %s: it takes no transform (cgpt_scene_update_primitive moves it)", i,
                          objects[i].kind == CGPT_OBJECT_SPHERE ? "sphere" : "plane");
        for (const uint32_t li : lights)
            if (li == i) return Refuse(error, CGPT_ERR_INVALID, "object %u is a light: mesh-light sampling reads its object-space triangles and area, so it takes no transform", i);
        float inv[12];
        const bool ok = InvertTransform(m, inv);
        if (ok) for (int r = 0; r < 3; ++r) rec[r] = make_float4(inv[4 * r], inv[4 * r + 1], inv[4 * r + 2], inv[4 * r + 3]);
        if (!ok) return Refuse(error, CGPT_ERR_INVALID, "object %u: the transform cannot be inverted in float range", i);
        flags[i] = 1u;
    }
    return CGPT_OK;
}

}  // namespace cgpt

using namespace cgpt;

static int SceneLayoutView(const cgpt_scene_desc* scene, const float* object_to_world, uint32_t n_objects, bool instanced, cgpth_scene_layout_view* view)
{
    // what the view points into: this thread's last layout and the per-object bookkeeping flattened
    struct Storage { SceneLayout layout; std::vector<uint32_t> leaf_base, pair_base, level_begin, level_offsets, level_offsets_start; };
    thread_local Storage st;
    try {
        if (!scene || !view) { HostSetError("null argument"); return CGPT_ERR_INVALID; }
        std::string error;
        const int rc = LayoutScene(*scene, st.layout, error, instanced);
        if (rc != CGPT_OK) { HostSetError(error.c_str()); return rc; }
        if (object_to_world || n_objects) {                                    // what cgpt_scene_update_transforms would install after this upload
            std::vector<uint32_t> flags;
            const int rt = LayoutTransforms(object_to_world, n_objects, st.layout.objects, st.layout.lights, st.layout.obj_xform, flags, error);
            if (rt != CGPT_OK) { HostSetError(error.c_str()); return rt; }
            for (uint32_t i = 0; i < n_objects; ++i) {
                PackObjTrace(st.layout.objects[i], st.layout.obj_trace[2 * (size_t)i], st.layout.obj_trace[2 * (size_t)i + 1], flags[i]);
            }
        }
        const SceneLayout& l = st.layout;
        st.leaf_base.clear(); st.pair_base.clear(); st.level_begin.clear(); st.level_offsets.clear(); st.level_offsets_start.assign(1, 0u);
        for (const RefitObject& ro : l.refit_objects) {
            st.leaf_base.push_back(ro.leaf_base); st.pair_base.push_back(ro.pair_base); st.level_begin.push_back(ro.level_begin);
            st.level_offsets.insert(st.level_offsets.end(), ro.level_offsets.begin(), ro.level_offsets.end());
            st.level_offsets_start.push_back((uint32_t)st.level_offsets.size());
        }
        auto f4 = [](const std::vector<float4>& v) { return reinterpret_cast<const float*>(v.data()); };
        view->node_pairs = f4(l.node_pairs); view->n_node_pairs = l.node_pairs.size();
        view->tri_leaf = f4(l.tri_leaf); view->n_tri_leaf = l.tri_leaf.size();
        view->tri_orig = f4(l.tri_orig); view->n_tri_orig = l.tri_orig.size();
        view->tri_normal = f4(l.tri_normal); view->n_tri_normal = l.tri_normal.size();
        view->materials = f4(l.materials); view->n_materials = l.materials.size();
        view->obj_trace = f4(l.obj_trace); view->n_obj_trace = l.obj_trace.size();
        view->objects = l.objects.data(); view->n_objects = l.objects.size(); view->object_size = sizeof(DevObject);
        view->lights = l.lights.data(); view->n_lights = l.lights.size();
        view->refit_levels = l.refit_levels.data(); view->n_refit_levels = l.refit_levels.size();
        view->record_perm = l.record_perm.data(); view->n_record_perm = l.record_perm.size();
        view->stack_depth = l.stack_depth; view->n_top_records = l.n_top_records; view->n_pair_records = l.n_pair_records; view->n_small_tris = l.n_small_tris;
        view->leaf_base = st.leaf_base.data(); view->pair_base = st.pair_base.data(); view->level_begin = st.level_begin.data();
        view->level_offsets = st.level_offsets.data(); view->level_offsets_start = st.level_offsets_start.data();
        view->tri_normal12 = f4(l.tri_normal12); view->n_tri_normal12 = l.tri_normal12.size();
        view->obj_xform = f4(l.obj_xform); view->n_obj_xform = l.obj_xform.size();
        return CGPT_OK;
    } catch (const std::exception& e) {
        HostSetError(e.what());
        return CGPT_ERR_INVALID;
    }
}

// ---- the top-level tree on the host: the upload's tree, then the edits the context applies to it (cgpt_abi.hip, refit.hip call the same
// functions on the same state) ----
namespace {
struct TopLevelStorage { std::vector<DevObject> objects; std::vector<uint32_t> lights; TopLevelState state; std::vector<float4> nodes; std::vector<uint32_t> entry; bool valid = false; };
TopLevelStorage& TopStorage() { thread_local TopLevelStorage st; return st; }
int TopLevelShow(TopLevelStorage& st, cgpth_top_level_view* view)
{
    LayoutTopLevel(st.objects, st.state, st.nodes, st.entry);
    view->nodes = reinterpret_cast<const float*>(st.nodes.data()); view->n_nodes = st.nodes.size() / 2;
    view->entry = st.entry.data(); view->n_entry = st.entry.size();
    return CGPT_OK;
}
template <class F> int TopLevelCall(cgpth_top_level_view* view, bool fresh, F&& f)
{
    try {
        TopLevelStorage& st = TopStorage();
        if (!view) { HostSetError("null argument"); return CGPT_ERR_INVALID; }
        if (!fresh && !st.valid) { HostSetError("no cgpth_top_level on this thread yet"); return CGPT_ERR_NO_SCENE; }
        std::string error;
        const int rc = f(st, error);
        if (rc != CGPT_OK) { HostSetError(error.c_str()); return rc; }
        return TopLevelShow(st, view);
    } catch (const std::exception& e) {
        HostSetError(e.what());
        return CGPT_ERR_INVALID;
    }
}
}  // namespace

extern "C" int cgpth_top_level(const cgpt_scene_desc* scene, cgpth_top_level_view* view)
{
    return TopLevelCall(view, true, [&](TopLevelStorage& st, std::string& error) {
        st.valid = false;
        if (!scene) return Refuse(error, CGPT_ERR_INVALID, "null argument");
        // the instanced layout: the boxes are per object and the same under either upload, and a scene whose copies would pass the record
        // limit (uploaded with cgpt_scene_upload_instanced) still shows its tree
        SceneLayout layout;
        const int rc = LayoutScene(*scene, layout, error, true);
        if (rc != CGPT_OK) return rc;
        st.objects = layout.objects; st.lights = layout.lights; st.state = layout.top_state; st.valid = true;
        return (int)CGPT_OK;
    });
}

extern "C" int cgpth_top_level_transforms(const float* object_to_world, uint32_t n_objects, cgpth_top_level_view* view)
{
    return TopLevelCall(view, false, [&](TopLevelStorage& st, std::string& error) {
        std::vector<float4> records; std::vector<uint32_t> flags;
        const int rc = LayoutTransforms(object_to_world, n_objects, st.objects, st.lights, records, flags, error);
        if (rc != CGPT_OK) return rc;
        st.state.xform.assign(object_to_world, object_to_world + 12 * (size_t)n_objects);
        return (int)CGPT_OK;
    });
}

extern "C" int cgpth_top_level_refit(uint32_t obj_index, const cgpt_triangle* triangles, uint32_t n_tris, cgpth_top_level_view* view)
{
    return TopLevelCall(view, false, [&](TopLevelStorage& st, std::string& error) {
        if (obj_index >= st.objects.size() || !triangles || n_tris != st.objects[obj_index].n_tris ||
            (st.objects[obj_index].kind != CGPT_OBJECT_MESH && st.objects[obj_index].kind != CGPT_OBJECT_TRIANGLE))
            return Refuse(error, CGPT_ERR_INVALID, "object %u: not a mesh or triangle object of %u triangles", obj_index, n_tris);
        TriangleBounds(triangles, n_tris, st.state.local_box.data() + 6 * (size_t)obj_index);
        return (int)CGPT_OK;
    });
}

extern "C" int cgpth_top_level_primitive(uint32_t obj_index, const cgpt_object* obj, cgpth_top_level_view* view)
{
    return TopLevelCall(view, false, [&](TopLevelStorage& st, std::string& error) {
        if (obj_index >= st.objects.size() || !obj || obj->kind != st.objects[obj_index].kind || (obj->kind != CGPT_OBJECT_SPHERE && obj->kind != CGPT_OBJECT_PLANE))
            return Refuse(error, CGPT_ERR_INVALID, "object %u: not a sphere or plane of that kind", obj_index);
        DevObject& d = st.objects[obj_index];
        memcpy(d.sphere_center, obj->sphere_center, 12); d.sphere_radius = obj->sphere_radius; d.sphere_radius_sq = obj->sphere_radius * obj->sphere_radius;
        memcpy(d.plane_normal, obj->plane_normal, 12); memcpy(d.plane_point, obj->plane_point, 12);
        return (int)CGPT_OK;
    });
}

extern "C" int cgpth_scene_layout_transformed(const cgpt_scene_desc* scene, const float* object_to_world, uint32_t n_objects, cgpth_scene_layout_view* view)
{
    return SceneLayoutView(scene, object_to_world, n_objects, false, view);
}

extern "C" int cgpth_scene_layout(const cgpt_scene_desc* scene, cgpth_scene_layout_view* view)
{
    return SceneLayoutView(scene, nullptr, 0u, false, view);
}

extern "C" int cgpth_scene_layout_instanced(const cgpt_scene_desc* scene, cgpth_scene_layout_view* view)
{
    return SceneLayoutView(scene, nullptr, 0u, true, view);
}
