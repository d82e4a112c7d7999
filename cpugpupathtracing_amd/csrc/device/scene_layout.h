// scene_layout.h -- the host half of a scene upload: the reference's AoS scene (cgpt_scene_desc) validated and re-laid into the
// device layout of device_scene.h, as plain host vectors.  No HIP runtime call and no context: cgpt_abi.hip (SceneInstall) and
// multi_gpu.hip copy the result to their devices, cgpth_scene_layout (cpugpupt_host.h) shows it to the CPU tests.
// The record packers are here too: the in-place edits (material and roughness updates, refit.hip) write the same records.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "cpugpupt_abi.h"
#include "device_scene.h"
#include "transform_math.h"

namespace cgpt {

// what an in-place edit of the uploaded scene needs of one object (LayoutScene fills it, refit.hip reads it)
struct RefitObject {
    uint32_t node_count = 0, tri_count = 0;   // as uploaded (a triangle object: 0 and 1)
    uint32_t leaf_base = 0;                    // first tri_leaf record of the object
    uint32_t pair_base = 0;                    // first child-pair record of the object before the renumbering (index into record_perm)
    uint32_t level_begin = 0;                  // first entry of the object's records in refit_levels ...
    std::vector<uint32_t> level_offsets;       // ... records of depth d at [level_begin + level_offsets[d], level_begin + level_offsets[d + 1])
    // cgpt_scene_rebuild_mesh (rebuild_layout.h): the first record of the span the mesh's first rebuild gave it at the end of node_pairs,
    // with room for tri_count - 1 records (as have its slices of refit_levels and record_perm from then on); kNoSpan: as uploaded
    uint32_t span_base = 0xFFFFFFFFu;
};
static constexpr uint32_t kNoSpan = 0xFFFFFFFFu;

// What the boxes of the top-level tree (cgpt_set_top_level) are computed from, kept current on the host by every edit
// that moves a box: per object the object-space box of a mesh or triangle object (the root node's bounds; the min / max of the vertex
// positions for a leaf root, a triangle object and after a refit) and its object-to-world matrix.  Spheres and planes are read from
// their DevObject.
struct TopLevelState {
    std::vector<float> local_box;              // 6 per object {lo.xyz, hi.xyz}
    std::vector<float> xform;                  // 12 per object, the rows of [A | b]; the identity after an upload
};

struct SceneLayout {
    // the arrays of device_scene.h, and each mesh's child-pair records grouped by depth (refit.hip's bound pass)
    std::vector<float4> node_pairs, tri_leaf, tri_orig, tri_normal, materials;
    std::vector<float4> tri_normal12;          // {n1.xyz, -}, {n2.xyz, -} per triangle, original order: installed behind tri_normal's n0 records
    std::vector<DevObject> objects;
    std::vector<float4> obj_trace;
    std::vector<float4> obj_xform;             // {Ainv row r, binv_r}, 3 per object: installed behind obj_trace's 2 n records.  LayoutScene writes the identity
    std::vector<uint32_t> lights;
    std::vector<uint32_t> refit_levels;
    TopLevelState top_state;                   // the source of the top-level tree's boxes (LayoutTopLevel)
    // host bookkeeping of the in-place edits
    std::vector<RefitObject> refit_objects;
    std::vector<uint32_t> record_perm;         // record index in the reference's depth-first order -> index in node_pairs
    // mesh instancing (cgpt_scene_upload_instanced): per object the first object laid out with the same four slice words,
    // the object itself where it shares with nobody -- every object of the plain layout.  The members of a group hold equal root_code,
    // tri_base, n_tris and RefitObject; everything else of an object is its own
    std::vector<uint32_t> mesh_group;
    uint32_t stack_depth = 0, n_top_records = 0, n_pair_records = 0, n_small_tris = 0, n_materials = 0;
};

// Validates everything a kernel will index with (a malformed tree must fail here, not fault on the GPU) and fills `out`.
// CGPT_OK, or CGPT_ERR_INVALID / CGPT_ERR_UNSUPPORTED with the reason in `error`; `out` is only meaningful on CGPT_OK.
// instanced: mesh objects that name the same node and triangle slices are laid out once (SceneLayout::mesh_group); false lays out every
// object, as cgpt_scene_upload always has.
int LayoutScene(const cgpt_scene_desc& sd, SceneLayout& out, std::string& error, bool instanced = false);

inline float AsFloat(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// roughness: the specular lobe's (cgpt_scene_update_roughness); transmission_roughness: the dielectric lobe's
// (cgpt_scene_update_transmission_roughness); the record holds alpha = roughness^2 of each, formed here once
inline void PackMaterial(const cgpt_material& m, float roughness, float transmission_roughness, float4 out[4])
{
    out[0] = make_float4(m.albedo[0], m.albedo[1], m.albedo[2], m.specular);
    out[1] = make_float4(m.refractivity, m.absorption[0], m.absorption[1], m.absorption[2]);
    out[2] = make_float4(m.ior, m.emissive[0], m.emissive[1], m.emissive[2]);
    out[3] = make_float4(m.intensity, AsFloat(m.is_light ? 1u : 0u), roughness * roughness, transmission_roughness * transmission_roughness);
}

// leaf-ordered triangle record (device_scene.h: tri_leaf) and original-order record (tri_orig) of one triangle
inline void PackLeafTri(const cgpt_triangle& tr, uint32_t tri_idx, float4 rec[3])
{
    const float e1[3] = { tr.v1.pos[0] - tr.v0.pos[0], tr.v1.pos[1] - tr.v0.pos[1], tr.v1.pos[2] - tr.v0.pos[2] };   // ref: Primitives.cpp:9
    const float e2[3] = { tr.v2.pos[0] - tr.v0.pos[0], tr.v2.pos[1] - tr.v0.pos[1], tr.v2.pos[2] - tr.v0.pos[2] };   // ref: Primitives.cpp:10
    rec[0] = make_float4(tr.v0.pos[0], tr.v0.pos[1], tr.v0.pos[2], e1[0]);
    rec[1] = make_float4(e1[1], e1[2], e2[0], e2[1]);
    rec[2] = make_float4(0.0f, e2[2], AsFloat(tri_idx), AsFloat(0u));                               // last_in_leaf set by the caller
}
inline void PackOrigTri(const cgpt_triangle& tr, float4 rec[3])
{
    rec[0] = make_float4(tr.v0.pos[0], tr.v0.pos[1], tr.v0.pos[2], tr.v0.normal[0]);
    rec[1] = make_float4(tr.v1.pos[0], tr.v1.pos[1], tr.v1.pos[2], tr.v0.normal[1]);
    rec[2] = make_float4(tr.v2.pos[0], tr.v2.pos[1], tr.v2.pos[2], tr.v0.normal[2]);
}

// the other two vertex normals of a triangle (device_scene.h: tri_normal, the pairs behind the n0 records)
inline void PackNormalPair(const cgpt_triangle& tr, float4 rec[2])
{
    rec[0] = make_float4(tr.v1.normal[0], tr.v1.normal[1], tr.v1.normal[2], 0.0f);
    rec[1] = make_float4(tr.v2.normal[0], tr.v2.normal[1], tr.v2.normal[2], 0.0f);
}

// obj_trace entry of an object (device_scene.h): what IntersectScene's object loop reads; upload and cgpt_scene_update_primitive
// xform: the object has a transform (cgpt_scene_update_transforms); meshes and triangle objects only
inline void PackObjTrace(const DevObject& d, float4& q0, float4& q1, uint32_t xform = 0u)
{
    q0 = make_float4(AsFloat(d.kind), 0.0f, 0.0f, 0.0f); q1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (d.kind == CGPT_OBJECT_MESH || d.kind == CGPT_OBJECT_TRIANGLE) { q0.x = AsFloat(CGPT_OBJECT_MESH); q0.y = AsFloat(d.root_code); q0.z = AsFloat(xform); }   // a triangle: a leaf-rooted mesh
    else if (d.kind == CGPT_OBJECT_SPHERE) { q0.y = d.sphere_center[0]; q0.z = d.sphere_center[1]; q0.w = d.sphere_center[2]; q1.x = d.sphere_radius_sq; }
    else { q0.y = d.plane_normal[0]; q0.z = d.plane_normal[1]; q0.w = d.plane_normal[2]; q1.x = d.plane_point[0]; q1.y = d.plane_point[1]; q1.z = d.plane_point[2]; }
}

// ---- per-object transforms (cgpt_scene_update_transforms; tests/transform_ref.py states the same arithmetic in numpy) ----------------
// An object-to-world matrix is 12 floats, the rows of [A | b]: world = A p + b.  The inverse and the identity test: transform_math.h.
inline void IdentityTransformRecords(float4 rec[3])
{
    rec[0] = make_float4(1.0f, 0.0f, 0.0f, 0.0f); rec[1] = make_float4(0.0f, 1.0f, 0.0f, 0.0f); rec[2] = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
}
// The validation of cgpt_scene_update_transforms against the uploaded objects and lights, and the records it installs: `records` gets the
// 3 n transform records, `flags` each object's transform flag (obj_trace; 0 for a bitwise identity).  CGPT_OK, or CGPT_ERR_INVALID with the reason
// in `error` and the outputs meaningless.  (scene_layout.hip)
int LayoutTransforms(const float* object_to_world, uint32_t n_objects, const std::vector<DevObject>& objects, const std::vector<uint32_t>& lights,
                     std::vector<float4>& records, std::vector<uint32_t>& flags, std::string& error);


// ---- the top-level tree (cgpt_set_top_level; tests/tlas_ref.py is the specification) ---------------------------------
// min / max of the vertex positions of n triangles (what CalculateNodeBounds yields for a node that holds them all)
void TriangleBounds(const cgpt_triangle* triangles, size_t n, float box[6]);
// The padded world box of object i.
void TopLevelLeafBox(const DevObject& d, const float local_box[6], const float xform[12], float box[6]);
// The balanced tree over the object index ranges in preorder, 2 n - 1 nodes of two float4s {lo.xyz, bits(skip) | hi.xyz, bits(object or
// 0xFFFFFFFF)}, and the table entry[j] = the highest node whose range starts at object j, entry[n] = 2 n - 1.  Host only, O(n).
void LayoutTopLevel(const std::vector<DevObject>& objects, const TopLevelState& st, std::vector<float4>& nodes, std::vector<uint32_t>& entry);
// float4s of the tree behind obj_trace's 5 n records: the nodes, then the entry table padded to whole float4s
inline size_t TopLevelFloat4s(size_t n) { return n ? 2 * (2 * n - 1) + (n + 1 + 3) / 4 : 0; }
// nodes and entry table as they are copied to the device, in one piece
std::vector<float4> PackTopLevel(const std::vector<DevObject>& objects, const TopLevelState& st);

}  // namespace cgpt
