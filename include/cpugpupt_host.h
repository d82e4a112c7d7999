/*
 * cpugpupt_host.h -- C entry points of the host-side mirror (scene structs, BVH build, glTF load path,
 * synthetic meshes, framebuffer dump).  Pure CPU code, no HIP calls: this is the part of the reference that
 * "stays host C++" (ref: Source/Main.cpp:51-275,775-819; Source/BVH.cpp:11-59,188-366; Source/GLTFLoader.cpp),
 * exported with a C ABI so non-C++ hosts (the Python tests and bench) can build scenes and hand the
 * flattened cgpt_scene_desc to cgpt_scene_upload() in cpugpupt_abi.h.
 *
 * Status convention as in cpugpupt_abi.h: 0 = ok, message from cgpth_last_error() (thread-local).
 */
#ifndef CPUGPUPT_HOST_H
#define CPUGPUPT_HOST_H

#include "cpugpupt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ref: Include/BVH.h:7-13 */
enum cgpth_build_option { CGPTH_BUILD_NAIVE = 0, CGPTH_BUILD_SAH_INTERVALS = 1, CGPTH_BUILD_SAH_PRIMITIVES = 2,
                          CGPTH_BUILD_SAH_BINNED = 3 /* CGPT_BUILD_SAH_BINNED: not in the reference; positions must be finite, |x| <= 1e30 */ };

typedef struct cgpth_mesh cgpth_mesh;    /* ref: Include/Primitives.h:24-28 (Mesh) */
typedef struct cgpth_scene cgpth_scene;  /* ref: Source/Main.cpp:200-236 (the parts of `data` Render() reads) */

typedef struct cgpth_bvh_info {
    uint32_t num_triangles, nodes_used, num_leaves, max_leaf_size, max_depth;
    float total_area;
} cgpth_bvh_info;

const char* cgpth_last_error(void);

/* ---- meshes ---- */
/* GLTFLoader::Load (ref: Source/GLTFLoader.cpp:19-89); NULL + error on failure */
cgpth_mesh* cgpth_mesh_load_gltf(const char* path);
cgpth_mesh* cgpth_mesh_from_arrays(const cgpt_vertex* vertices, uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices);
/* synthetic dragon stand-in: icosphere `level` -> 20*4^level triangles inside the dragon's AABB */
cgpth_mesh* cgpth_mesh_dragon_standin(uint32_t level);
cgpth_mesh* cgpth_mesh_bumpy_icosphere(uint32_t level, const float center[3], const float radii[3], float bump);
int cgpth_mesh_save_gltf(const cgpth_mesh* mesh, const char* gltf_path);
uint32_t cgpth_mesh_num_vertices(const cgpth_mesh* mesh);
uint32_t cgpth_mesh_num_indices(const cgpth_mesh* mesh);
const cgpt_vertex* cgpth_mesh_vertices(const cgpth_mesh* mesh);
const uint32_t* cgpth_mesh_indices(const cgpth_mesh* mesh);
void cgpth_mesh_free(cgpth_mesh* mesh);

/* ---- scene ---- */
cgpth_scene* cgpth_scene_new(void);
void cgpth_scene_free(cgpth_scene* scene);
/* the shipped scene (ref: Main.cpp:777-819) with `mesh` in place of the dragon and material `mesh_material` on it */
cgpth_scene* cgpth_scene_reference_layout(const cgpth_mesh* mesh, uint32_t mesh_material, float aspect, int build_option);
int cgpth_scene_add_material(cgpth_scene* scene, const cgpt_material* material);            /* returns index */
int cgpth_scene_set_material(cgpth_scene* scene, uint32_t index, const cgpt_material* material);   /* keeps the material's roughness and transmission roughness */
/* the specular lobe's roughness of material `index` (cgpt_scene_update_roughness holds the meaning and the validation: finite, in [0, 1]);
 * a new material has 0.  It is not part of cgpt_scene_desc: a host uploads the scene, then hands get_roughness's values to the device */
int cgpth_scene_set_roughness(cgpth_scene* scene, uint32_t index, float roughness);
/* out: n values, n == the scene's material count */
int cgpth_scene_get_roughness(const cgpth_scene* scene, float* out, uint32_t n);
/* the dielectric lobe's transmission roughness of material `index` (cgpt_scene_update_transmission_roughness holds the meaning and the
 * validation: finite, in [0, 1]); a new material has 0; handed to the device after the upload, as the roughness is */
int cgpth_scene_set_transmission_roughness(cgpth_scene* scene, uint32_t index, float transmission_roughness);
int cgpth_scene_get_transmission_roughness(const cgpth_scene* scene, float* out, uint32_t n);
int cgpth_scene_add_mesh(cgpth_scene* scene, const cgpth_mesh* mesh, uint32_t mat_index, int build_option);  /* Object ctor, ref: Main.cpp:247-251; returns object index */
/* same result as cgpth_scene_add_mesh(..., CGPTH_BUILD_SAH_INTERVALS) with the tree built on the GPU by cgpt_bvh_build
 * (bit-identical tree; the host keeps validating and owning it) */
/* an instance of mesh object `of_obj_index` (mesh instancing, cgpt_scene_upload_instanced): a new mesh object that SHARES that object's
 * triangles and BVH and has its own material, smooth flag and transform; returns its index.  An instance of an instance shares the same
 * mesh.  cgpth_scene_flatten emits the shared slices once and names them from every sharer, so cgpt_scene_upload_instanced keeps one
 * device copy (cgpt_scene_upload copies per object, as it does for any scene).  cgpth_scene_refit_mesh and the rebuilds through any sharer
 * act on the one tree.  Refused (negative): a bad index, or a sphere, a plane or a triangle object */
int cgpth_scene_add_instance(cgpth_scene* scene, uint32_t of_obj_index, uint32_t mat_index);
int cgpth_scene_add_mesh_device_built(cgpth_scene* scene, const cgpth_mesh* mesh, uint32_t mat_index, cgpt_ctx* ctx);
/* any BuildOption on the GPU (cgpt_bvh_build_ex; ref: BVH.cpp:208-297) */
int cgpth_scene_add_mesh_device_built_ex(cgpth_scene* scene, const cgpth_mesh* mesh, uint32_t mat_index, cgpt_ctx* ctx, int build_option);
int cgpth_scene_add_sphere(cgpth_scene* scene, const float center[3], float radius, uint32_t mat_index);
int cgpth_scene_add_plane(cgpth_scene* scene, const float normal[3], const float point[3], uint32_t mat_index);
/* a stand-alone triangle object, Primitive(const Triangle&) (ref: Include/Primitives.h:84-89); returns object index.  It has no BVH
 * (bvh_info / bvh_export / rebuild_bvh refuse it) and cannot be a light (the reference EXCEPTs, Main.cpp:383) */
int cgpth_scene_add_triangle(cgpth_scene* scene, const cgpt_triangle* triangle, uint32_t mat_index);
int cgpth_scene_add_light(cgpth_scene* scene, uint32_t obj_index);                            /* ref: Main.cpp:817; refuses an object with smooth normals or a transform */
/* smooth shading of object `obj_index` (cgpt_scene_update_smooth_normals holds the meaning): flag 0 or 1, a new object has 0.  Refused
 * with CGPT_ERR_INVALID and nothing changed: a bad index, a flag that is neither 0 nor 1, a 1 on a light.  Spheres and planes keep the
 * flag and ignore it.  Not part of cgpt_scene_desc: a host uploads the scene, then hands get_smooth_normals's values to the device */
int cgpth_scene_set_smooth_normals(cgpth_scene* scene, uint32_t obj_index, uint32_t flag);
/* out: n values, n == the scene's object count */
int cgpth_scene_get_smooth_normals(const cgpth_scene* scene, uint32_t* out, uint32_t n);
/* the object-to-world matrix of object `obj_index` (cgpt_scene_update_transforms holds the meaning): 12 floats, the rows of [A | b]; a new
 * object has the identity.  Refused with CGPT_ERR_INVALID and nothing changed, as the device call refuses: a bad index, an entry that is
 * not finite, an A that cannot be inverted, and anything but the bitwise identity on a sphere, a plane or a light.  Not part of
 * cgpt_scene_desc: a host uploads the scene, then hands get_transforms's values to the device */
int cgpth_scene_set_transform(cgpth_scene* scene, uint32_t obj_index, const float object_to_world[12]);
/* out: 12 n floats, n == the scene's object count */
int cgpth_scene_get_transforms(const cgpth_scene* scene, float* out, uint32_t n);
int cgpth_scene_set_camera(cgpth_scene* scene, const float pos[3], const float view_dir[3], float fov_deg, float aspect);
int cgpth_scene_set_settings(cgpth_scene* scene, const cgpt_settings* settings);
int cgpth_scene_rebuild_bvh(cgpth_scene* scene, uint32_t obj_index, int build_option);       /* ref: BVH.cpp:47-59 */
/* BVH::Rebuild with the re-split on the GPU: starts from the tree's current triangle order, as the reference does (ref: BVH.cpp:47-59);
 * on failure the BVH is left unchanged */
int cgpth_scene_rebuild_bvh_device(cgpth_scene* scene, uint32_t obj_index, int build_option, cgpt_ctx* ctx);
/* the host statement of cgpt_scene_refit_mesh (same contract, validation and errors): a mesh keeps its tree, its triangles, per-triangle
 * bounds and centroids (a later Rebuild re-splits on them), total_area and node bounds follow the new triangles; a triangle object
 * (n_tris = 1) is replaced.  On failure the scene is unchanged. */
int cgpth_scene_refit_mesh(cgpth_scene* scene, uint32_t obj_index, const cgpt_triangle* triangles, uint32_t n_tris);
/* Linear blend skinning, the host statement of cgpt_scene_skin_mesh's triangle pass (csrc/host/skinning.h states the operations and
 * their order; tests/skin_ref.py the same in numpy): out_triangles[t] is bind_triangles[t] with every corner moved by
 * the blend of its four joints -- joints[12 t + 4 c + k] and weights[12 t + 4 c + k] for corner c, influence k -- of joint_matrices
 * (n_joints x 12 floats, the rows of [A | b]).  No influence is skipped and weights are never renormalised; the blended A moves the
 * normal (renormalised; the bind normal where the result has no finite positive length).  Refused with CGPT_ERR_INVALID and nothing
 * written: a NULL array, n_joints 0 or above 1024, a joint index >= n_joints, a weight, bind float or matrix entry that is not finite. */
int cgpth_skin_triangles(const cgpt_triangle* bind_triangles, const uint16_t* joints, const float* weights, uint32_t n_tris,
                         const float* joint_matrices, uint32_t n_joints, cgpt_triangle* out_triangles);
/* cgpth_skin_triangles followed by cgpth_scene_refit_mesh of the result: the host statement of cgpt_scene_set_skin +
 * cgpt_scene_skin_mesh (the host scene keeps no skin; unlike the device call total_area follows the pose, as after any host refit).
 * Refused as the two device calls refuse, with the scene unchanged: a bad index, a sphere or a plane, a light, n_tris other than the
 * object's count, and what cgpth_skin_triangles refuses. */
int cgpth_scene_skin_mesh(cgpth_scene* scene, uint32_t obj_index, const cgpt_triangle* bind_triangles, const uint16_t* joints, const float* weights,
                          uint32_t n_tris, const float* joint_matrices, uint32_t n_joints);
/* Morph targets (blend shapes), the host statement of cgpt_scene_morph_mesh's triangle pass (csrc/host/morph.h states the operations
 * and their order; tests/morph_ref.py the same in numpy): every one of the 18 floats of out_triangles[t] is
 * base_triangles[t]'s plus weights[k] * target_deltas[k * n_tris + t]'s, k ascending, a target whose weight is +0 or -0 skipped; with
 * no active target the triangle is the base's bit for bit, otherwise the corners' normals are renormalised (the base normal where the
 * blend has no finite positive length).  Refused with CGPT_ERR_INVALID and nothing written: a NULL array, n_targets 0 or above 256, a
 * base float, delta float or weight that is not finite. */
int cgpth_morph_triangles(const cgpt_triangle* base_triangles, const cgpt_triangle* target_deltas, uint32_t n_tris, uint32_t n_targets,
                          const float* weights, cgpt_triangle* out_triangles);
/* cgpth_morph_triangles followed by cgpth_scene_refit_mesh of the result: the host statement of cgpt_scene_set_morph_targets +
 * cgpt_scene_morph_mesh (the host scene keeps no targets; unlike the device call total_area follows the pose).  Refused as the two
 * device calls refuse, with the scene unchanged: a bad index, a sphere or a plane, a light, n_tris other than the object's count, and
 * what cgpth_morph_triangles refuses.  A morphed and skinned object is cgpth_scene_skin_mesh with the morphed triangles as its bind pose. */
int cgpth_scene_morph_mesh(cgpth_scene* scene, uint32_t obj_index, const cgpt_triangle* base_triangles, const cgpt_triangle* target_deltas,
                           uint32_t n_tris, uint32_t n_targets, const float* weights);
/* Joint matrices from an animation clip, the host statement of cgpt_scene_animate_objects' kernel (csrc/host/animation.h states the
 * operations and their order; tests/anim_ref.py the same in numpy): out gets the skeleton's n_joints x 12 floats, the
 * rows of [A | b] of every joint's skinning matrix under `clip` at time t -- what cgpt_scene_pose_objects takes.  Refused with nothing
 * written: whatever cgpt_scene_set_skeleton refuses of a skeleton and cgpt_clip_create of a clip (CGPT_ERR_UNSUPPORTED for
 * CUBICSPLINE, else CGPT_ERR_INVALID), a clip whose n_joints differs from the skeleton's, n_joints other than the skeleton's, a time
 * that is not finite, out NULL. */
int cgpth_animate_joints(const cgpt_skeleton_desc* skeleton, const cgpt_clip_desc* clip, float time, float* out, uint32_t n_joints);
/* The host statement of cgpt_scene_animate_layers' kernel: the joint matrices of the skeleton under the blend of
 * n_layers layers, layer l playing clips[l] (layers[l].clip is not read) at layers[l].time wrapped over that clip's range by
 * layers[l].wrap, with weight layers[l].weight.  Refused with nothing written: what cgpth_animate_joints refuses of the skeleton, of
 * each clip (inactive layers' included: "layer l: ...") and of out / n_joints, clips or layers NULL, and every refusal of a layer that
 * cgpt_scene_animate_layers lists. */
int cgpth_animate_layers(const cgpt_skeleton_desc* skeleton, const cgpt_clip_desc* clips, const cgpt_clip_layer* layers, uint32_t n_layers,
                         float* out, uint32_t n_joints);
/* a clip's range as cgpt_clip_get_range reports it: the smallest first-key and the largest last-key time of its channels (none: 0, 0) */
int cgpth_clip_range(const cgpt_clip_desc* clip, float* begin, float* end);
/* animation.h's AnimWrapTime: t over [begin, end] by a CGPT_ANIM_WRAP_* mode.  Refused: out NULL, an unknown mode, a float that is not finite */
int cgpth_wrap_time(float t, float begin, float end, uint32_t mode, float* out);
/* the host statement of cgpt_scene_update_primitive: a sphere's centre and radius, or a plane's normal and point */
int cgpth_scene_update_primitive(cgpth_scene* scene, uint32_t obj_index, const cgpt_object* obj);
/* reorders the objects: the new object k is the old object order[k] (a permutation of 0 .. n_objects - 1, else refused and nothing
 * changed); smooth flags and transforms move with their objects, the light indices are renamed.  The object order is IntersectScene's
 * tie order: two surfaces at exactly the same t are won by the lower index. */
int cgpth_scene_permute_objects(cgpth_scene* scene, const uint32_t* order, uint32_t n_objects);
int cgpth_scene_bvh_info(const cgpth_scene* scene, uint32_t obj_index, cgpth_bvh_info* out);
/* nodes: nodes_used x cgpt_bvh_node; tri_indices: num_triangles */
int cgpth_scene_bvh_export(const cgpth_scene* scene, uint32_t obj_index, cgpt_bvh_node* nodes, uint32_t* tri_indices);
/* the host statement of cgpt_scene_tree_costs (csrc/host/tree_cost.h states the metric; tests/tree_cost_ref.py the same in numpy;
 * DESIGN.md 5.36): the cost of the tree in `nodes`, n_nodes records in the layout and numbering cgpth_scene_bvh_export and
 * cgpt_scene_export_bvh return (node 0 the root; prim_count 0: the children are left_first and left_first + 1).  The nodes are walked
 * from the root; the device sums in another order, so the two agree to rounding, not in every bit.  Refused with CGPT_ERR_INVALID and
 * nothing written: nodes or out NULL, n_nodes 0, a constant that is not finite and > 0, a child index outside the array, nodes that
 * form no tree.  A cost that is not finite is returned as it is. */
int cgpth_tree_cost(const cgpt_bvh_node* nodes, uint32_t n_nodes, double c_inner, double c_tri, cgpt_tree_cost* out);
/* the host statement of cgpt_tonemap (csrc/host/tonemap.h states the arithmetic; tests/tonemap_ref.py the same in numpy)
 * over a host image: params->source must be CGPT_TONEMAP_HOST.  `state` is what a context keeps between calls -- the adapted histogram
 * index and whether it holds a reading (zero-initialise it; clearing `valid` is cgpt_exposure_reset) -- read and written with
 * CGPT_TONEMAP_AUTO_EXPOSURE only and may be NULL otherwise; info_out (may be NULL) receives what cgpt_read_exposure would return after
 * the same call.  Bit for bit the device's results except behind CGPT_TRANSFER_SRGB, where the two powf differ by a few ulp.  Refused
 * with CGPT_ERR_INVALID and nothing written, the state included: what cgpt_tonemap refuses of its parameters and outputs, NULL params,
 * another source, auto exposure without a state. */
/* the histogram bin (0..255) of a luminance, or -1 for one that is not counted (<= 0, NaN, +inf) */
int cgpth_luminance_bin(float luminance);
typedef struct cgpth_exposure_state { double adapted_index; uint32_t valid, reserved; } cgpth_exposure_state;
int cgpth_tonemap(const cgpt_tonemap_params* params, cgpth_exposure_state* state, float* dst_rgba, size_t n_floats, uint32_t* dst_pixels,
                  size_t n_pixels, cgpt_exposure_info* info_out);
/* flatten for cgpt_scene_upload; pointers stay valid until the scene is changed or freed */
int cgpth_scene_flatten(cgpth_scene* scene, cgpt_scene_desc* out);
int cgpth_scene_get_camera(const cgpth_scene* scene, cgpt_camera* out);
int cgpth_scene_get_settings(const cgpth_scene* scene, cgpt_settings* out);

/* ---- framebuffer dump (replaces DX12 present, ref: Source/DX12.cpp:277-322) ---- */
int cgpth_write_ppm(const char* path, const uint32_t* pixels, uint32_t width, uint32_t height);
int cgpth_write_pfm(const char* path, const float* accumulator_rgba, uint32_t num_accumulated, uint32_t width, uint32_t height);
int cgpth_write_accumulator(const char* path, const float* accumulator_rgba, uint32_t num_accumulated, uint32_t width, uint32_t height);
int cgpth_read_accumulator(const char* path, float* accumulator_rgba, uint32_t* num_accumulated, uint32_t width, uint32_t height);

/* ---- self-check hook ---- */
/* the exact division-by-a-launch-constant the kernels use to map a path id to its pixel (csrc/device/fast_div.h), evaluated on
 * the host: equals n / d for every 32-bit n and every d >= 1 (tests/test_host.py checks it against integer division) */
uint32_t cgpth_fast_div(uint32_t n, uint32_t d);

/* the work-item rule of the wavefront pipeline's shade kernel (csrc/device/shade_items.h), evaluated on the host.  cgpth_shade_item_blocks:
 * the consecutive 64-path blocks a shade wave takes at a time from a list of n_blocks blocks walked by n_waves waves, at most `chunk`.
 * cgpth_shade_segment_blocks: the blocks the launcher sizes a wave's output segment for, from the pool's capacity in blocks, the
 * smallest shade grid in waves and the configured chunk.  tests/test_host_shade_items.py checks that no wave is ever dealt more.
 * 0 for n_waves, min_waves or chunk == 0. */
uint32_t cgpth_shade_item_blocks(uint32_t n_blocks, uint32_t n_waves, uint32_t chunk);
uint32_t cgpth_shade_segment_blocks(uint32_t cap_blocks, uint32_t min_waves, uint32_t chunk);

/* the per-object motion records of CGPT_TEMPORAL_FOLLOW_TRANSFORMS (csrc/device/transform_math.h), evaluated on the host: for
 * n_objects matrices of 12 floats each as they were when the history was stored (`prev`, n_prev objects) and as they are now (`cur`),
 * 24 words per object -- the rows {D row, translation} of D = M_prev M_cur^-1, then the rows {N row, 0} of N = A_prev^-T A_cur^T,
 * with the state word (0 unmoved, 1 moved, 2 drop) in place of the fourth row's last float.  Returns the number of objects that are
 * not unmoved.  tests/test_host_motion.py checks it word for word against tests/motion_ref.py. */
uint32_t cgpth_motion_records(const float* prev, uint32_t n_prev, const float* cur, uint32_t n_objects, float* records_out);

/* the device layout a cgpt_scene_upload of `scene` would install (csrc/device/device_scene.h), computed on the host with the same
 * validation, status and message (from cgpth_last_error()) as the upload; no GPU is touched.  tests/test_host_scene_layout.py checks
 * it against the layout's documentation.  The arrays live in thread-local storage of the library and stay valid until the next
 * call on the same thread.  Counts are elements: float4s (4 floats) for the float arrays, object_size bytes for `objects`. */
typedef struct cgpth_scene_layout_view {
    const float* node_pairs; size_t n_node_pairs;
    const float* tri_leaf; size_t n_tri_leaf;
    const float* tri_orig; size_t n_tri_orig;
    const float* tri_normal; size_t n_tri_normal;
    const float* materials; size_t n_materials;
    const float* obj_trace; size_t n_obj_trace;
    const void* objects; size_t n_objects; size_t object_size;     /* DevObject records */
    const uint32_t* lights; size_t n_lights;
    const uint32_t* refit_levels; size_t n_refit_levels;
    const uint32_t* record_perm; size_t n_record_perm;             /* child-pair record in the input's node order -> index in node_pairs */
    uint32_t stack_depth, n_top_records, n_pair_records, n_small_tris;
    /* per object (n_objects each): first tri_leaf record, first child-pair record before the renumbering (index into record_perm),
     * first entry in refit_levels; object i's records of depth d are refit_levels[level_begin[i] + o[d] .. level_begin[i] + o[d + 1])
     * with o = level_offsets + level_offsets_start[i], which has level_offsets_start[i + 1] - level_offsets_start[i] entries */
    const uint32_t* leaf_base; const uint32_t* pair_base; const uint32_t* level_begin;
    const uint32_t* level_offsets; const uint32_t* level_offsets_start;
    /* the other two vertex normals, {n1.xyz, -}, {n2.xyz, -} per triangle in tri_orig's order (2 float4s a triangle): the device keeps them
     * behind tri_normal's n0 records, in the same allocation */
    const float* tri_normal12; size_t n_tri_normal12;
    /* the transform records, {Ainv row r, binv_r}, 3 float4s an object: the device keeps them behind obj_trace's 2 n records, in the same
     * allocation.  The identity after cgpth_scene_layout, as after an upload */
    const float* obj_xform; size_t n_obj_xform;
} cgpth_scene_layout_view;
int cgpth_scene_layout(const cgpt_scene_desc* scene, cgpth_scene_layout_view* out);
/* the layout a cgpt_scene_upload_instanced would install: the same view; the objects of a mesh group show equal root_code, tri_base,
 * leaf_base, pair_base and levels */
int cgpth_scene_layout_instanced(const cgpt_scene_desc* scene, cgpth_scene_layout_view* out);
/* the same after a cgpt_scene_update_transforms(object_to_world, n_objects) on that upload, with that call's validation, status and
 * message: obj_xform holds the inverses, `objects` the xform words and obj_trace the flags the call would install */
int cgpth_scene_layout_transformed(const cgpt_scene_desc* scene, const float* object_to_world, uint32_t n_objects, cgpth_scene_layout_view* out);

/* ---- the plan of cgpt_scene_pose_objects (csrc/device/pose_plan.h), computed on the host; no GPU is touched ----
 * The batch is n_entries rows of five words {obj_index, n_joints of the skin that takes part (0: none), 1 if the object has morph
 * targets, 1 if they are stored in leaf-slot order, active targets} over the layout a cgpt_scene_upload of `scene` installs
 * (cgpt_scene_upload_instanced with instanced != 0), under the knobs skin_joints_lds and morph_max_blocks.  The view shows the tables
 * the launcher walks, as rows of 32-bit words:
 *   entries   16 words {source row, obj_index, kernel, leaf_base, tri_base, n_tris, n_joints, matrix_base, active_base, n_active,
 *             first_block, blocks, root_code, leaf_root, n_levels, 0}, grouped by kernel, the batch's order kept within one --
 *             0 skin_triangles<LDS = 0>, 1 <1>; morph_triangles<SKIN, LDS, LEAF>: 2 <0,0,0>, 3 <0,0,1>, 4 <1,0,0>, 5 <1,0,1>, 6 <1,1,0>, 7 <1,1,1>;
 *   launches  5 words {kernel, first_entry, n_entries, n_blocks, max_joints}: block b of a launch belongs to the last of its entries
 *             with first_block <= b, is block b - first_block of it, and its lanes take leaf slots (b - first_block) 256 + lane,
 *             + 256 blocks, ... below n_tris;
 *   segments  4 words {records_begin, count, tri_base, first_block}: refit_levels[records_begin .. records_begin + count);
 *   levels    4 words {depth, first_segment, n_segments, n_blocks}, one launch of the bound pass each, in launch order.
 * The refusals are the planner's (two entries naming one object or one instanced mesh group among them), with the message in
 * cgpth_last_error().  The arrays live in thread-local storage and stay valid until the next call on the same thread. */
typedef struct cgpth_pose_plan_view {
    const uint32_t* entries; size_t n_entries;
    const uint32_t* launches; size_t n_launches;
    const uint32_t* segments; size_t n_segments;
    const uint32_t* levels; size_t n_levels;
    uint32_t n_matrix_joints, n_active;
} cgpth_pose_plan_view;
int cgpth_pose_batch_plan(const cgpt_scene_desc* scene, int instanced, const uint32_t* batch, uint32_t n_entries, uint32_t skin_joints_lds,
                          uint32_t morph_max_blocks, cgpth_pose_plan_view* out);

/* ---- the bookkeeping of cgpt_scene_rebuild_mesh (csrc/device/rebuild_layout.h: PlanRebuild, RebuildNames, ApplyRebuild; tests/rebuild_ref.py
 * restates it) ----
 * Rebuilds of mesh obj_index, one after the other, over the layout a cgpt_scene_upload of `scene` installs (cgpt_scene_upload_instanced
 * with instanced != 0); no GPU is involved.  `trees` is n_trees runs of words {n, level_first[n], m, top_ranks[m]}: the builder's level
 * ranges of a new tree (level L = nodes [level_first[L], level_first[L + 1]), closed by the node count) and the preorder ranks of the
 * first m = min(K, pairs) splitting nodes of its level-ordered array, K = the top slots the mesh owns at that point.  assume_pair_records,
 * when not 0, stands for the current number of child-pair records (the tests of the 2^26 limit).  The view shows the last rebuild's plan --
 * members of the mesh group, top_slots, the new level_offsets, names[k] = record of the splitting node of rank k -- and the bookkeeping
 * after all of them: record_perm, and per object root_codes, span_bases (0xFFFFFFFF: never rebuilt) and node_counts.  The refusals are
 * the planner's (CGPT_ERR_UNSUPPORTED: deeper than the traversal stack; CGPT_ERR_INVALID: the span would pass 2^26 records), with the
 * message in cgpth_last_error().  The arrays live in thread-local storage and stay valid until the next call on the same thread. */
typedef struct cgpth_rebuild_plan_view {
    const uint32_t* members; size_t n_members;
    const uint32_t* top_slots; size_t n_top_slots;
    const uint32_t* level_offsets; size_t n_level_offsets;
    const uint32_t* names; size_t n_names;
    const uint32_t* record_perm; size_t n_record_perm;
    const uint32_t* root_codes; const uint32_t* span_bases; const uint32_t* node_counts; size_t n_objects;
    uint32_t span_base, level_begin, pair_base, leaf_base;
    uint32_t n_nodes, n_pairs, max_depth, grow;
    uint32_t n_pair_records, n_refit_levels, stack_depth, n_top_records;
} cgpth_rebuild_plan_view;
int cgpth_rebuild_plan(const cgpt_scene_desc* scene, int instanced, uint32_t obj_index, const uint32_t* trees, uint32_t n_trees,
                       uint32_t assume_pair_records, cgpth_rebuild_plan_view* out);

/* ---- the top-level tree of cgpt_set_top_level (csrc/device/scene_layout.h: LayoutTopLevel; tests/tlas_ref.py is its specification) ----
 * cgpth_top_level: the tree a cgpt_scene_upload of `scene` would build (cgpt_scene_upload_instanced builds the same: the boxes are per
 * object; the record limit that is checked is the instanced upload's), computed on the host with the upload's validation; no GPU is
 * touched.  nodes: n_nodes = 2 n_objects - 1 records of 8 floats in preorder, {lo.xyz, bits(skip) | hi.xyz, bits(object or 0xFFFFFFFF)};
 * entry: n_objects + 1 node indices.  The three calls behind it apply, to the state of this thread's last cgpth_top_level, what
 * cgpt_scene_update_transforms, cgpt_scene_refit_mesh and cgpt_scene_update_primitive apply to a context's (the same functions), and
 * show the tree again.  The arrays live in thread-local storage and stay valid until the next of these calls on the same thread. */
typedef struct cgpth_top_level_view {
    const float* nodes; size_t n_nodes;
    const uint32_t* entry; size_t n_entry;
} cgpth_top_level_view;
int cgpth_top_level(const cgpt_scene_desc* scene, cgpth_top_level_view* out);
int cgpth_top_level_transforms(const float* object_to_world, uint32_t n_objects, cgpth_top_level_view* out);
int cgpth_top_level_refit(uint32_t obj_index, const cgpt_triangle* triangles, uint32_t n_tris, cgpth_top_level_view* out);
int cgpth_top_level_primitive(uint32_t obj_index, const cgpt_object* obj, cgpth_top_level_view* out);

#ifdef __cplusplus
}
#endif
#endif
