// ctx_internal.h -- the context object behind the C ABI (shared by cgpt_abi.hip and multi_gpu.hip; not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "cpugpupt_abi.h"
#include "device_memory.h"
#include "device_scene.h"
#include "launch_common.h"
#include "scene_layout.h"
#include "transform_math.h"

namespace cgpt {
struct DeviceGroup;
}  // namespace cgpt

namespace cgpt {
// The device memory of a one-device context, by subsystem.  The kernel-argument structs (DevScene, DevRenderArgs) are filled from these.
struct SceneBuffers {                             // cgpt_scene_upload installs them (SceneInstall); refit.hip edits them in place
    DevBuf<float4> node_pairs, tri_leaf, tri_orig, tri_normal, materials;
    DevBuf<DevObject> objects;
    DevBuf<float4> obj_trace;
    DevBuf<uint32_t> lights;
    DevBuf<uint32_t> refit_levels;
    DevBuf<cgpt_triangle> refit_staging;          // host triangles of the last refit, grown on demand
    DevBuf<uint32_t> skin_scratch;                // cgpt_scene_skin_mesh: 8 words a pose reads back (refit.hip: kSkinScratchWords), allocated with the first skin
    DevBuf<uint32_t> pose_batch;                  // cgpt_scene_pose_objects: the tables and scratch of the last batch (refit.hip: PoseObjects), grown on demand
    DevBuf<uint32_t> anim_batch;                  // cgpt_scene_animate_objects / _layers: per entry a flag word, then the entry records the kernel reads, grown on demand
    DevBuf<uint32_t> tree_cost;                   // cgpt_scene_tree_costs: the results, entries and block partials of the last call (tree_cost.hip), grown on demand
};
// The skin of one object (cgpt_scene_set_skin): the bind pose, 12 joint indices and 12 weights a triangle, and the room of a pose's
// joint matrices.  Not part of the scene's footprint; an upload drops every skin.
struct SkinBuffers {
    DevBuf<cgpt_triangle> bind;
    DevBuf<uint16_t> joints;
    DevBuf<float> weights;
    DevBuf<float> matrices;                       // 12 n_joints floats, written by every cgpt_scene_skin_mesh
    uint32_t n_joints = 0;                        // 0: no skin
    // CGPT_TEMPORAL_FOLLOW_POSES (denoise.hip): the joint matrices of the last successful cgpt_scene_skin_mesh through this skin, or
    // pose_known = false ("no pose known": before the first pose, after a cgpt_scene_refit_mesh of the object or of a placement that shares
    // its copy, and after a pose through another skin of the same copy); serial names this installation among all of the context's
    std::vector<float> pose;
    bool pose_known = false;
    uint64_t serial = 0;
    // the skin's skeleton (cgpt_scene_set_skeleton), n_joints joints as the skin: parents, 12 floats of inverse bind and 10
    // of rest {T.xyz, R.xyzw, S.xyz} a joint, 12 floats of root matrix when has_root.  Lives and dies with the skin
    DevBuf<int32_t> parents;
    DevBuf<float> inverse_bind, rest, root;
    bool has_skeleton = false, has_root = false;
};
// An animation clip (cgpt_clip_create): what animation.h's sampler reads -- the (joint, path) -> channel table, the channels
// (animation.h: AnimChannel, four words each), the key times and values.  Belongs to the context, not to a scene
struct ClipBuffers {
    DevBuf<uint32_t> map, channels;
    DevBuf<float> times, values;
    uint32_t n_joints = 0;                        // 0: a destroyed clip's slot
    float begin = 0.0f, end = 0.0f;               // the clip's range (animation.h: ClipTable), what a layer's wrap mode wraps over
};
// The morph targets of one object (cgpt_scene_set_morph_targets): the base triangle and the n_targets displacement
// records of every triangle in one buffer of float2 -- set 0 is the base, set 1 + k is target k.  leaf_order: set s, plane p (0..8, two of
// a record's 18 floats), leaf slot i at data[(9 s + p) n_tris + i]; otherwise as given, triangle t's record at data[9 (s n_tris + t)].
// `active` is the table a pose compacts its nonzero weights into, {target index, bits(weight)} each.  Not part of the scene's footprint;
// an upload drops every object's targets.
struct MorphBuffers {
    DevBuf<float2> data;
    DevBuf<uint2> active;                         // n_targets entries of room, written by every pose of the object (from `weights` by a skin's)
    uint32_t n_targets = 0;                       // 0: no targets
    uint32_t leaf_order = 1;                      // the knob "morph_leaf_order" as cgpt_scene_set_morph_targets read it
    std::vector<float> weights;                   // the last weights given: all zero after the set
    // CGPT_TEMPORAL_FOLLOW_MORPHS (denoise.hip).  slot_of_tri: with leaf_order, the leaf slot of every triangle (the inverse
    // of the map the planes were permuted by; 4 B a triangle, empty otherwise).  The pose the copy shows, when it was made through these
    // targets: `weights` above and, if a skin took part, that skin's serial and matrices -- or pose_known = false ("no pose known": from
    // the set until the first accepted pose, after a cgpt_scene_refit_mesh of the object or of a placement that shares its copy, after a
    // pose of the copy through another placement's targets or skin).  serial names this installation among all of the context's
    DevBuf<uint32_t> slot_of_tri;
    bool pose_known = false;
    uint64_t serial = 0;
    uint64_t pose_skin_serial = 0;                // 0: the pose is the morph alone
    std::vector<float> pose_matrices;             // 12 floats a joint of that skin's pose
};
// What the temporal history keeps of the poses it was stored under (StoreTemporalKey): per object the index of the object whose skin
// posed its copy (-1: no pose known) and, at that index, the skin's serial and matrices.
struct PoseSnapshot {
    std::vector<int32_t> owner;
    std::vector<uint64_t> serial;
    std::vector<std::vector<float>> matrices;
};
// ... and of the morphed poses (CGPT_TEMPORAL_FOLLOW_MORPHS): per object the index of the object whose targets posed its copy (-1: none
// known) and, at that index, the key of the pose: the installation, the weights, and the skin part (serial 0: none)
struct MorphSnapshot {
    struct Key {
        uint64_t serial = 0, skin_serial = 0;
        std::vector<float> weights, matrices;
    };
    std::vector<int32_t> owner;
    std::vector<Key> key;
};
// One object's entry of the table the carry-back kernel reads (denoise.hip: pose_carry_back): 96 bytes, six float4
struct PoseRecord {
    uint32_t state;                               // transform_math.h: MotionState -- 0 unposed since the history, 1 re-posed, 2 drop
    uint32_t matrix_base;                         // state 1: the history's joint matrices start at float4 3 * matrix_base of dn.pose_matrices
    uint32_t tri_base, smooth;                    // DevObject::tri_base and ::smooth of the object
    const float2* bind;                           // state 1: the skin's arrays, as skin_triangles reads them
    const uint2* joints;
    const float4* weights;
    uint32_t n_tris, pad;                         // the object's triangle count
    float xform[12];                              // the object's current object-to-world matrix (top_state.xform)
};
static_assert(sizeof(PoseRecord) == 96, "six float4 per object");
// ... and of the second table morph_carry_back reads beside it (PoseRecord keeps its layout): 32 bytes, two float4.  A state-1 object
// with kMorphRecordMorph takes its bind corner from `data` and the history's active table; with kMorphRecordSkin that corner goes
// through PoseRecord's joints and weights, without it PoseRecord's skin pointers are null.
enum : uint32_t { kMorphRecordMorph = 1u, kMorphRecordLeaf = 2u, kMorphRecordSkin = 4u };
struct MorphRecord {
    const float2* data;                           // MorphBuffers::data of the copy's owner
    const uint32_t* slot_of_tri;                  // kMorphRecordLeaf: MorphBuffers::slot_of_tri
    uint32_t active_base, n_active;               // the history's active table: entries active_base .. of dn.morph_active
    uint32_t flags, pad;
};
static_assert(sizeof(MorphRecord) == 32, "two float4 per object");
struct FrameBuffers {                             // the framebuffer band (EnsureFramebuffer)
    DevBuf<float4> accumulator;
    DevBuf<uint32_t> pixels;
};
struct DenoiseBuffers {                           // denoise.hip; each group is reallocated when its pixel count changes
    DevBuf<float4> guides;                        // 3 float4 per pixel, the cgpt_read_guides layout
    DevBuf<float4> guide_demod;                   // per pixel: the albedo the filter divides by ({1,1,1} where it does not)
    DevBuf<float4> filter[2];                     // the filter's ping-pong buffers
    DevBuf<uint32_t> filter_pixels;
    DevBuf<float4> history[2];                    // cgpt_denoise_temporal: per pixel {merged colour, history length H}, ping-pong
    DevBuf<float4> history_guides[2];             // 2 float4 per pixel {x.xyz, t | n.xyz, bits(obj)} of the frame each history belongs to
    DevBuf<float> variance;                       // cgpt_denoise_variance_guided: per pixel, the variance pass 0 read (cgpt_read_variance)
    DevBuf<float4> moments[2];                    // ... per pixel {mu, v, K, 0} of the luminance, beside history[] (the same slot)
    DevBuf<float4> motion;                        // CGPT_TEMPORAL_FOLLOW_TRANSFORMS: 6 float4 per object (transform_math.h: MotionRecord), grown on
                                                  // demand and written only by a call in which an object moved
    // CGPT_TEMPORAL_FOLLOW_POSES
    DevBuf<uint32_t> guide_tri;                   // per pixel, beside guides: the first hit's triangle in the object's original order (0: a miss, a
                                                  // sphere, a plane, a triangle object); written by guides_tri_kernel, which runs while a skin or morph targets exist
    DevBuf<float4> pose_table;                    // 6 float4 per object (PoseRecord), grown on demand, written by a call in which a pose changed
    DevBuf<float4> pose_matrices;                 // ... the history's joint matrices of every re-posed skin, 3 float4 per joint
    DevBuf<float4> previous_hits;                 // 2 float4 per pixel {x_p.xyz, bits(state) | n_p.xyz, 0}: pose_carry_back's output (cgpt_read_previous_hits)
    // CGPT_TEMPORAL_FOLLOW_MORPHS: written by a call in which an object with targets is in state 1 (it runs morph_carry_back)
    DevBuf<float4> morph_table;                   // 2 float4 per object (MorphRecord), beside pose_table
    DevBuf<uint2> morph_active;                   // the history's active tables {target, bits(weight)} of every re-posed owner, one after the other
};
// The display stage (tonemap.hip): buffers of its own, each grown on demand.  table: the 256 bin counts and, behind them,
// the ignored pixels' tally -- zero between calls (exposure_resolve clears what it read); record: what exposure_resolve wrote
struct TonemapBuffers {
    DevBuf<float4> src, out;                      // a CGPT_TONEMAP_HOST image as uploaded; {r, g, b, 1}
    DevBuf<uint32_t> pixels;
    DevBuf<uint32_t> table;
    DevBuf<cgpt_exposure_info> record;
};
template <class... B> void ResetAll(B&... b) { (b.Reset(), ...); }
// What the uploaded scene has that a kernel variant must carry: a roughness > 0, a transmission roughness > 0, a smooth-normal flag (they live in
// h_objects[i].smooth), a transform that is no identity (the flags live in obj_trace).  All false after an upload, each kept by the edit that owns it.
struct SceneFeatures { bool rough_specular = false, rough_dielectric = false, smooth_normals = false, transforms = false; };
}  // namespace cgpt

struct cgpt_ctx {
    int device = 0;
    cgpt::DevStream own_stream;
    hipStream_t stream = nullptr;
    cgpt::DevEvent ev_start, ev_stop;
    std::string error;

    // device scene
    cgpt::SceneBuffers sb;
    cgpt::DevScene scene{};
    uint32_t n_materials = 0;
    bool has_scene = false;
    // the specular lobe's roughness and the dielectric lobe's transmission roughness per material (cgpt_scene_update_roughness,
    // cgpt_scene_update_transmission_roughness; 0 after every upload) and the packed material records as they are on the device (a roughness
    // or material update re-packs them); h_lights is the uploaded light_indices (a light can be neither smooth nor transformed)
    std::vector<float> h_roughness, h_transmission_roughness;
    std::vector<float4> h_materials;
    std::vector<uint32_t> h_lights;
    cgpt::SceneFeatures features;
    // cgpt_set_nee_candidates: context state like the stream (an upload keeps it).  A render with more than one candidate, NEE on and
    // TracePathAdvanced paths runs the RIS instantiations of the render kernels
    uint32_t nee_candidates = 1;
    // cgpt_set_top_level: context state too.  1: the renders, the guides and cgpt_intersect_rays reach the objects through the top-level tree
    // behind obj_trace's 5 n records (device_scene.h).  top_state is what its boxes are computed from; every edit that moves a box keeps
    // it current in either mode and rewrites the device tree in mode 1 (WriteTopLevel); turning the mode on writes it
    uint32_t top_level = 0;
    cgpt::TopLevelState top_state;

    // in-place edits of the uploaded scene (refit.hip): host copies of the objects, each mesh's child-pair records grouped by
    // depth, and where the renumbering put every record
    std::vector<cgpt::DevObject> h_objects;
    std::vector<cgpt::RefitObject> refit_objects;
    std::vector<uint32_t> record_perm;            // record index in the reference's depth-first order -> index in node_pairs
    // mesh instancing (cgpt_scene_upload_instanced): SceneLayout::mesh_group of the installed layout -- the objects that share object i's
    // one device copy are those with mesh_group[j] == mesh_group[i]; the identity after cgpt_scene_upload -- and what
    // cgpt_get_scene_footprint reports, filled by SceneInstall (of the edits only a mesh's first cgpt_scene_rebuild_mesh changes it);
    // n_refit_levels: the entries of sb.refit_levels in use (an empty table still has one element of room)
    std::vector<uint32_t> mesh_group;
    cgpt_scene_footprint footprint{};
    uint32_t n_refit_levels = 0;
    // skinning (cgpt_scene_set_skin): per object, empty or as long as h_objects; cleared with the scene.  skin_joints_lds is the
    // cgpt_set_tuning knob "skin_joints_lds": 1 (default) the skin kernel stages the joint matrices in LDS, 0 it reads them through the
    // vector cache (same results; DESIGN.md 5.26 has both timings)
    std::vector<cgpt::SkinBuffers> skins;
    uint32_t skin_joints_lds = 1;
    // morph targets (cgpt_scene_set_morph_targets): per object, empty or as long as h_objects; cleared with the scene.  The knobs
    // "morph_leaf_order" (what the next set stores: 1 leaf-slot order in component planes, 0 as given) and "morph_max_blocks" (the cap of
    // the morph kernel's grid, 1..1024: a small mesh can be made to stride)
    std::vector<cgpt::MorphBuffers> morphs;
    uint32_t morph_leaf_order = 1;
    uint32_t morph_max_blocks = 1024;
    // CGPT_TEMPORAL_FOLLOW_POSES: pose_generation counts the cgpt_scene_skin_mesh calls (they bump the other two generations as well);
    // pose_stamp[i] is its value at the last pose that wrote object i's copy (empty or as long as h_objects; cleared with the scene);
    // skin_serial numbers the cgpt_scene_set_skin installations
    uint64_t pose_generation = 0;
    std::vector<uint64_t> pose_stamp;
    uint64_t skin_serial = 0;
    // CGPT_TEMPORAL_FOLLOW_MORPHS: morph_generation counts the accepted cgpt_scene_morph_mesh calls (they bump scene_generation and
    // shape_generation as well, not pose_generation); morph_stamp[i] is its value at the last of them that wrote object i's copy (as
    // pose_stamp); morph_serial numbers the cgpt_scene_set_morph_targets installations
    uint64_t morph_generation = 0;
    std::vector<uint64_t> morph_stamp;
    uint64_t morph_serial = 0;
    // animation clips (cgpt_clip_create): handle k is clips[k - 1]; an upload keeps them
    std::vector<cgpt::ClipBuffers> clips;

    // framebuffer band
    cgpt::FrameBuffers fb;
    uint32_t width = 0, height = 0, n_rows = 0;
    uint32_t band_key[5] = { 0, 0, 0, 0, 0 };     // row_begin, row_end, interleave rows/count/index of the allocated band
    uint32_t num_accumulated = 0;

    cgpt::DevBuf<cgpt::DevCounters> counters;
    uint32_t kernel_launches = 0;
    double kernel_ms = 0.0;
    uint32_t dominant_launches = 0;
    double dominant_ms = 0.0;
    uint32_t dominant_waves_per_simd = 0;
    uint32_t dominant_round0_launches = 0;
    double dominant_round0_ms = 0.0;

    // wavefront workspace (owned by wavefront_kernels.hip) and the persistent kernel's (persistent_kernel.hip)
    void* wavefront_state = nullptr;
    void* persistent_state = nullptr;

    // a render that has been enqueued and not yet finished (RenderEnqueue / RenderFinish)
    uint32_t pending_kernel = 0;
    uint32_t pending_num_accumulated = 0;
    cgpt::ShadeVariant pending_variant{};
    cgpt::DevRenderArgs pending_args{};
    uint32_t last_debug_mode = 0;
    uint32_t last_kernel = 0;                     // cgpt_kernel the last render ran (AUTO resolved)

    // n_devices > 1 (or CGPT_CTX_FORCE_COLLECTIVE): this context is a group; the members are ordinary one-device contexts
    cgpt::DeviceGroup* group = nullptr;

    // the denoiser (denoise.hip): first-hit guides cached per camera, band and scene, and the filter's ping-pong buffers
    uint64_t scene_generation = 0;                // bumped by every scene upload and in-place edit
    uint64_t shape_generation = 0;                // ... by each of them but cgpt_scene_update_transforms: what a history that follows the transforms is kept across
                                                  // (pose_generation, with the skins above: ... by cgpt_scene_skin_mesh alone;
                                                  // morph_generation: ... by an accepted cgpt_scene_morph_mesh alone)
    cgpt::DenoiseBuffers dn;
    bool guides_valid = false;
    uint64_t guide_generation = 0;                // what the guides were computed for
    cgpt_camera guide_camera{};
    uint32_t guide_frame[4] = { 0, 0, 0, 0 };     // width, height, first global row, rows
    bool guide_tri_valid = false;                 // dn.guide_tri belongs to the cached guides (guides_tri_kernel computed them)
    // the temporal history (cgpt_denoise_temporal): dn.history[temporal_slot] and what it was stored for
    bool temporal_valid = false;
    uint32_t temporal_slot = 0;
    uint32_t temporal_demodulate = 0;
    uint64_t temporal_generation = 0;
    cgpt_camera temporal_camera{};
    uint32_t temporal_frame[4] = { 0, 0, 0, 0 };  // as guide_frame
    // CGPT_TEMPORAL_FOLLOW_TRANSFORMS: the shape generation and top_state.xform (12 floats per object) the history was stored for, and
    // the host copy of dn.motion of the last call in which an object moved (it outlives the asynchronous copy)
    uint64_t temporal_shape_generation = 0;
    std::vector<float> temporal_xform;
    std::vector<cgpt::MotionRecord> motion_records;
    // CGPT_TEMPORAL_FOLLOW_POSES: the pose generation and the poses the history was stored for; the host copies of dn.pose_table and
    // dn.pose_matrices of the last call in which a pose changed (they outlive the asynchronous copies); previous_hits_valid:
    // dn.previous_hits holds the records of the last successful flagged call that launched pose_carry_back, for previous_hits_frame
    uint64_t temporal_pose_generation = 0;
    cgpt::PoseSnapshot temporal_poses;
    std::vector<cgpt::PoseRecord> pose_records;
    std::vector<float> pose_matrices;
    bool previous_hits_valid = false;
    uint32_t previous_hits_frame[4] = { 0, 0, 0, 0 };
    // CGPT_TEMPORAL_FOLLOW_MORPHS: the morph generation and the morphed poses the history was stored for; the host copies of
    // dn.morph_table and dn.morph_active, as pose_records
    uint64_t temporal_morph_generation = 0;
    cgpt::MorphSnapshot temporal_morphs;
    std::vector<cgpt::MorphRecord> morph_records;
    std::vector<uint2> morph_active;
    // the variance-guided filter (cgpt_denoise_variance_guided): dn.moments[temporal_slot] belongs to the temporal history when
    // moments_valid (a cgpt_denoise_temporal call updates the colour without them); dn.variance is the last successful call's map
    bool moments_valid = false;
    bool variance_valid = false;
    uint32_t variance_frame[4] = { 0, 0, 0, 0 };  // as guide_frame
    // CGPT_TONEMAP_DENOISED: the float4 result of the last successful filter call, one of dn.filter[] (n pixels).  Dropped when a filter
    // call starts, by a render, cgpt_reset_accumulator, cgpt_write_accumulator, a framebuffer reallocation and DenoiseFree
    const float4* denoised = nullptr;
    size_t denoised_n = 0;

    // the display stage (tonemap.hip).  A multi-device context keeps all of it on its first member.  m_adapted: the adapted histogram
    // index (tonemap.h), context state that uploads and edits keep; exposure_info: the last successful auto-exposure call's reading
    cgpt::TonemapBuffers tm;
    uint32_t tonemap_cus = 0;                     // QueryCuCount
    double m_adapted = 0.0;
    bool m_adapted_valid = false;
    cgpt_exposure_info exposure_info{};
    bool exposure_info_valid = false;
};


namespace cgpt {
// The choice of kernel variant (kernel_variant.h states the ladder): these three functions are the only readers of ctx->features.
// ChooseVariant: for a render, or a cgpt_shade_samples call, with the translated settings st and the flags of cgpt_render_params.  The RIS
// instantiations run only where a candidate loop can: TracePath (BRUTE_FORCE) has no NEE, and NEE may be off.  The one place where DevSettings.nee
// becomes more than a flag: they read M from it, every other reader tests it for zero (device_scene.h); with one candidate it stays the caller's flag.
inline ShadeVariant ChooseVariant(const cgpt_ctx* ctx, DevSettings& st, uint32_t render_flags)
{
    const SceneFeatures& f = ctx->features;
    const bool ris = ctx->nee_candidates > 1u && st.nee != 0u && st.render_mode != CGPT_MODE_BRUTE_FORCE;
    if (ris) st.nee = ctx->nee_candidates;
    return { (render_flags & CGPT_RENDER_COUNTERS) != 0, (uint32_t)LobeLevel(f.rough_specular, f.rough_dielectric, f.smooth_normals, f.transforms), ris, ctx->top_level != 0u };
}
// guides_kernel<SMOOTH, XFORM, TREE> (denoise.hip) has a ladder of its own: 0 none, 1 SMOOTH, 2 + XFORM, 3 + TREE.  The tree has the one
// instantiation with everything on, a transform the one with smooth normals on.
constexpr int kGuideLevels = 4;
inline int ChooseGuideLevel(const cgpt_ctx* ctx) { return ctx->top_level ? 3 : ctx->features.transforms ? 2 : ctx->features.smooth_normals ? 1 : 0; }
// intersect_rays_kernel<XFORM, TREE> (path_kernels.hip): 0 none, 1 XFORM, 2 + TREE (one instantiation, transforms honoured)
inline int ChooseIntersectLevel(const cgpt_ctx* ctx) { return ctx->top_level ? 2 : ctx->features.transforms ? 1 : 0; }
// cgpt_settings as the kernels take them, for cgpt_render and cgpt_shade_samples: CGPT_OK, or the refusal with the context's error set
int TranslateSettings(cgpt_ctx* ctx, const cgpt_settings& settings, DevSettings& st);

// the device half of a scene upload (cgpt_abi.hip): frees the context's scene and installs the arrays and bookkeeping of a layout that
// LayoutScene (scene_layout.h) accepted; the caller has selected the device and drained the stream
int SceneInstall(cgpt_ctx* ctx, const SceneLayout& layout);
// the top-level tree of ctx->h_objects with the boxes' source `st`, copied behind obj_trace's 5 n records (a synchronous copy: the caller
// has selected the device and drained the stream); hipSuccess without a copy while the mode is 0
hipError_t WriteTopLevel(cgpt_ctx* ctx, const std::vector<DevObject>& objects, const TopLevelState& st);
// the two halves of cgpt_render: enqueue the kernels of one context without waiting, then wait and book the timings
int RenderEnqueue(cgpt_ctx* ctx, const cgpt_camera* camera, const cgpt_settings* settings, const cgpt_render_params* p);
int RenderFinish(cgpt_ctx* ctx);
hipError_t LaunchPackPixels(const float4* accumulator, uint32_t* pixels, size_t n_pixels, uint32_t num_accumulated, hipStream_t stream);   // path_kernels.hip

// multi_gpu.hip: the group behind a multi-device context
int GroupCreate(const int* device_ids, int n_devices, uint32_t flags, cgpt_ctx** out);
void GroupDestroy(cgpt_ctx* ctx);
int GroupSceneUpload(cgpt_ctx* ctx, const cgpt_scene_desc* scene, bool instanced);
int GroupUpdateMaterials(cgpt_ctx* ctx, const cgpt_material* materials, uint32_t n);
int GroupUpdateRoughness(cgpt_ctx* ctx, const float* roughness, uint32_t n);
int GroupUpdateTransmissionRoughness(cgpt_ctx* ctx, const float* roughness, uint32_t n);
int GroupUpdateSmoothNormals(cgpt_ctx* ctx, const uint32_t* smooth, uint32_t n);
int GroupUpdateTransforms(cgpt_ctx* ctx, const float* object_to_world, uint32_t n);
int GroupSetNeeCandidates(cgpt_ctx* ctx, uint32_t candidates);
int GroupSetTopLevel(cgpt_ctx* ctx, uint32_t mode);
int GroupRefitMesh(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_triangle* triangles, uint32_t n_tris, float* total_area_out);
int GroupUpdatePrimitive(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_object* obj);
int GroupSetSkin(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_triangle* bind_triangles, const uint16_t* joints, const float* weights, uint32_t n_tris, uint32_t n_joints);
int GroupSkinMesh(cgpt_ctx* ctx, uint32_t obj_index, const float* joint_matrices, uint32_t n_joints);
int GroupClearSkin(cgpt_ctx* ctx, uint32_t obj_index);
int GroupSetMorphTargets(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_triangle* base_triangles, const cgpt_triangle* target_deltas, uint32_t n_tris, uint32_t n_targets);
int GroupMorphMesh(cgpt_ctx* ctx, uint32_t obj_index, const float* weights, uint32_t n_targets);
int GroupClearMorphTargets(cgpt_ctx* ctx, uint32_t obj_index);
int GroupPoseObjects(cgpt_ctx* ctx, const cgpt_pose* poses, uint32_t n_poses);
int GroupSetSkeleton(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_skeleton_desc* skeleton);
int GroupClipCreate(cgpt_ctx* ctx, const cgpt_clip_desc* clip, uint32_t* clip_out);
int GroupClipDestroy(cgpt_ctx* ctx, uint32_t clip);
int GroupAnimateObjects(cgpt_ctx* ctx, const cgpt_animation* entries, uint32_t n_entries);
int GroupAnimateLayers(cgpt_ctx* ctx, const cgpt_layered_animation* entries, uint32_t n_entries);
int GroupRebuildMesh(cgpt_ctx* ctx, uint32_t obj_index, uint32_t build_option, uint32_t* n_nodes_out, uint32_t* max_depth_out);
int GroupTreeCosts(cgpt_ctx* ctx, const uint32_t* obj_indices, uint32_t n, double c_inner, double c_tri, cgpt_tree_cost* out);
int GroupRender(cgpt_ctx* ctx, const cgpt_camera* camera, const cgpt_settings* settings, const cgpt_render_params* p);
int GroupResetAccumulator(cgpt_ctx* ctx);
int GroupReadAccumulator(cgpt_ctx* ctx, float* dst, size_t n_floats);
int GroupReadPixels(cgpt_ctx* ctx, uint32_t* dst, size_t n_pixels);
int GroupWriteAccumulator(cgpt_ctx* ctx, const cgpt_render_params* p, const float* src, size_t n_floats, uint32_t num_accumulated);
int GroupDevicePtr(cgpt_ctx* ctx, bool pixels, void** ptr, size_t* n_bytes);
int GroupGetStats(cgpt_ctx* ctx, cgpt_stats* out);
int GroupGetRetraceUnwalked(cgpt_ctx* ctx, uint64_t* out);
int GroupResetStats(cgpt_ctx* ctx);
int GroupSetTuning(cgpt_ctx* ctx, const char* name, uint32_t value);
int GroupSynchronize(cgpt_ctx* ctx);
cgpt_ctx* GroupFirstMember(cgpt_ctx* ctx);
cgpt_ctx* GroupFirstMemberOrNull(cgpt_ctx* ctx);
int GroupForwarded(cgpt_ctx* ctx, int rc);     // a call forwarded to the first member returned rc: its message becomes the group's
// the denoiser's view of a group's frame: its size, samples and the debug mode of the last render; and the gathered full frame on
// device_ids[0] (the gather cgpt_read_accumulator does), with the group's gather state and statistics left as they were
void GroupFrameInfo(cgpt_ctx* ctx, uint32_t* width, uint32_t* height, uint32_t* num_accumulated, uint32_t* last_debug_mode);
int GroupGatherUncounted(cgpt_ctx* ctx, const float4** frame);

std::vector<uint2> ActiveTable(const float* weights, uint32_t n_targets);   // refit.hip: a pose's nonzero weights {target, bits(weight)}, ascending
// refit.hip: TriangleBounds of an object's n triangles as tri_orig holds them, folded on the device: out = {-, lo.xyz, hi.xyz, 1 where a position is
// not finite} (fold_object_box); the caller has selected the device
hipError_t FoldObjectBoxToHost(cgpt_ctx* ctx, uint32_t tri_base, uint32_t n_tris, uint32_t out[8]);
void DenoiseFree(cgpt_ctx* ctx);               // denoise.hip: the guide cache and filter buffers of a one-device context
}  // namespace cgpt

// Not part of the ABI (include/cpugpupt_abi.h): the bytes this library holds on all devices, for the tests of device_memory.h
extern "C" uint64_t cgpt_debug_live_device_bytes(void);
