/*
 * cpugpupt_abi.h -- the drop-in boundary: a C ABI around the reference's Render() (MI355X / gfx950).
 *
 * The reference (Contingencyy/CPUGPUPathtracing) has no plugin or FFI interface; the path sits behind
 * the implicit boundary around `void Render()` (ref: Source/Main.cpp:691-755), which reads the
 * file-static `data` (ref: Main.cpp:200-236) and writes `data.accumulator` / `data.pixels`.  Each
 * entry point below cites the reference interface it replaces.  "ref:" = file:line under the
 * reference checkout.  Plain pointers and sizes only; no C++ or torch types cross this boundary.
 *
 * Conventions: every function returns an int status (0 = CGPT_OK) and never throws; the message for
 * the last failure is available from cgpt_last_error().  One context is used from one host thread at
 * a time (Render() is not re-entrant in the reference either).  Every call blocks until its device work
 * is done -- cgpt_render returns with the accumulator updated, as Render() does; there are no
 * asynchronous variants.  The library copies everything it is handed; the caller keeps ownership of its
 * buffers.
 */
#ifndef CPUGPUPT_ABI_H
#define CPUGPUPT_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGPT_ABI_VERSION 2u   /* 2: cgpt_stats grew (gather_ms .. last_kernel), CGPT_KERNEL_* / CGPT_CTX_* values added since 1;
                                 CGPT_OBJECT_TRIANGLE is a new enum value only, no layout changed; the denoiser added new symbols
                                 (cgpt_read_guides, cgpt_denoise) and a new struct (cgpt_denoise_params) only; the microfacet specular
                                 lobe added one new symbol (cgpt_scene_update_roughness) only; CGPT_BUILD_SAH_BINNED is a new enum
                                 value only; the rough dielectric lobe added one new symbol
                                 (cgpt_scene_update_transmission_roughness) only; resampled light sampling added one new symbol
                                 only (cgpt_set_nee_candidates); smooth shading added one new symbol only
                                 (cgpt_scene_update_smooth_normals); per-object transforms added one new symbol only
                                 (cgpt_scene_update_transforms); the top-level tree added one new symbol only
                                 (cgpt_set_top_level); temporal reprojection added new symbols (cgpt_denoise_temporal,
                                 cgpt_temporal_reset, cgpt_read_temporal_history) and a new struct (cgpt_temporal_params) only;
                                 variance-guided edge stopping added new symbols (cgpt_denoise_variance_guided,
                                 cgpt_read_variance) and a new struct (cgpt_variance_params) only; following object transforms in
                                 the temporal stage is a new enum value only (CGPT_TEMPORAL_FOLLOW_TRANSFORMS); skinning added new
                                 symbols only (cgpt_scene_set_skin, cgpt_scene_skin_mesh, cgpt_scene_clear_skin); following poses in the
                                 temporal stage is a new enum value (CGPT_TEMPORAL_FOLLOW_POSES) and one new symbol
                                 (cgpt_read_previous_hits) only; morph targets added new symbols only
                                 (cgpt_scene_set_morph_targets, cgpt_scene_morph_mesh, cgpt_scene_clear_morph_targets); following
                                 morphs in the temporal stage is a new enum value only (CGPT_TEMPORAL_FOLLOW_MORPHS); posing many
                                 objects in one call added one new symbol (cgpt_scene_pose_objects) and a new struct (cgpt_pose) only */

enum cgpt_status {
    CGPT_OK = 0,
    CGPT_ERR_INVALID = 1,      /* bad argument / inconsistent scene description */
    CGPT_ERR_HIP = 2,          /* a HIP runtime call failed (message has hipGetErrorString) */
    CGPT_ERR_NO_SCENE = 3,     /* render before cgpt_scene_upload */
    CGPT_ERR_UNSUPPORTED = 4,  /* valid in the reference's type system but EXCEPTs there too (AABB objects, ref
                                  Primitives.cpp:302-305; lights that are neither a mesh nor a sphere, ref Main.cpp:383) */
    CGPT_ERR_NO_DEVICE = 5     /* no usable gfx950 device: the product never falls back to a CPU path */
};

/* ---- scene description: the reference's own layouts -------------------------------------------- */

/* ref: Include/Primitives.h:9-13 */
typedef struct cgpt_vertex { float pos[3]; float normal[3]; } cgpt_vertex;
/* ref: Include/Primitives.h:46-51 (72 bytes) */
typedef struct cgpt_triangle { cgpt_vertex v0, v1, v2; } cgpt_triangle;
/* ref: Include/BVH.h:29-34 (32 bytes; right child is always left_first + 1) */
typedef struct cgpt_bvh_node {
    float aabb_min[3]; uint32_t left_first;
    float aabb_max[3]; uint32_t prim_count;
} cgpt_bvh_node;
/* ref: Source/Main.cpp:51-69 (56 bytes; is_light is the reference's bool widened to 4 bytes = its padding) */
typedef struct cgpt_material {
    float albedo[3]; float specular;
    float refractivity; float absorption[3]; float ior;
    float emissive[3]; float intensity;
    uint32_t is_light;
} cgpt_material;

enum cgpt_object_kind {        /* ref: Main.cpp:245-275 (Object = mesh-with-BVH | Primitive); the one other Primitive kind, AABB,
                                  EXCEPTs in the reference (Primitives.cpp:302-305) and is CGPT_ERR_UNSUPPORTED here */
    CGPT_OBJECT_MESH = 0,
    CGPT_OBJECT_SPHERE = 1,    /* ref: Primitives.h:36-44 */
    CGPT_OBJECT_PLANE = 2,     /* ref: Primitives.h:30-34 */
    CGPT_OBJECT_TRIANGLE = 3   /* a stand-alone triangle, no BVH: Primitive(const Triangle&), ref: Primitives.h:84-89 */
};

typedef struct cgpt_object {
    uint32_t kind;             /* cgpt_object_kind */
    uint32_t mat_index;        /* ref: Main.cpp:268 */
    /* mesh: slices of the scene-wide arrays below (BVH internals, ref: BVH.h:46-52)
     * triangle: tri_offset names its entry of `triangles`, tri_count = 1, node_count = 0; its tri_indices entry is ignored */
    uint32_t node_offset, node_count;   /* m_nodes[0 .. m_current_node) ; node 0 is the root */
    uint32_t tri_offset, tri_count;     /* m_triangles and m_tri_indices (indices are object-local) */
    uint32_t max_depth;                 /* BVH::GetMaxDepth, ref: BVH.cpp:139-142 */
    float total_area;                   /* BVH::GetTotalArea, ref: BVH.cpp:144-147 */
    /* sphere */
    float sphere_center[3]; float sphere_radius;
    /* plane */
    float plane_normal[3]; float plane_point[3];
} cgpt_object;

/* what Render() reads from `data`: objects, materials, light_source_indices (ref: Main.cpp:209-212) */
typedef struct cgpt_scene_desc {
    const cgpt_object* objects; uint32_t n_objects;
    const cgpt_bvh_node* nodes; uint32_t n_nodes;
    const cgpt_triangle* triangles; uint32_t n_triangles;
    const uint32_t* tri_indices;               /* n_triangles entries */
    const cgpt_material* materials; uint32_t n_materials;
    const uint32_t* light_indices; uint32_t n_lights;
} cgpt_scene_desc;

/* Camera screen plane (ref: Main.cpp:162-168); cgpt_camera_from_view fills it like UpdateScreenPlane (:143-149) */
typedef struct cgpt_camera {
    float pos[3]; float top_left[3]; float top_right[3]; float bottom_left[3];
} cgpt_camera;

enum cgpt_render_mode { CGPT_MODE_COMPARISON = 0, CGPT_MODE_BRUTE_FORCE = 1, CGPT_MODE_ADVANCED = 2 };      /* ref: Main.cpp:172-178 */
enum cgpt_debug_mode { CGPT_DEBUG_NONE = 0, CGPT_DEBUG_RAY_DEPTH = 1, CGPT_DEBUG_BVH_DEPTH = 2 };           /* ref: Main.cpp:185-191 */

/* ref: Main.cpp:228-235 (Settings) + :215-216 (render_mode, debug_render_mode) */
typedef struct cgpt_settings {
    int32_t max_ray_depth;
    uint32_t next_event_estimation_enabled;
    uint32_t cosine_weighted_diffuse_reflection_enabled;
    uint32_t russian_roulette_enabled;
    uint32_t render_mode;
    uint32_t debug_render_mode;
} cgpt_settings;

/* three render paths with bit-identical results: the one-lane-per-pixel megakernel, the wavefront pipeline (trace / shade /
 * compact kernels per bounce round), and the persistent path kernel (one launch: lanes own paths, voted traversal + shade steps).
 * AUTO picks by speed alone (measured on MI355X): a one-sample call under 3 M paths -> megakernel; under 16 M
 * paths -> persistent; else the wavefront pipeline (which sizes its pools against the
 * free HBM: see cgpt_set_tuning).  All three run every render_mode (TracePathAdvanced, TracePath, COMPARISON) and debug view. */
enum cgpt_kernel { CGPT_KERNEL_AUTO = 0, CGPT_KERNEL_MEGAKERNEL = 1, CGPT_KERNEL_WAVEFRONT = 2, CGPT_KERNEL_PERSISTENT = 3 };
enum cgpt_render_flags { CGPT_RENDER_COUNTERS = 1u };   /* collect inner_steps / tri_tests / bvh_depth_sum / closest_hits */

typedef struct cgpt_render_params {
    uint32_t width, height;        /* framebuffer size (ref: Window::GetFramebufferSize, Main.cpp:698); any size, every
                                      pixel is rendered (the reference needs W%16==0 && H%16==0: SURVEY A-1) */
    uint32_t row_begin, row_end;   /* rows this context renders; [0,height) for the whole image (multi-GPU row tiling) */
    uint32_t first_sample;         /* = data.num_accumulated before the call (ref: Main.cpp:205,702) */
    uint32_t n_samples;            /* Render() calls folded into this one */
    uint32_t seed;                 /* RNG stream key; the reference's s_seed is 0x12345678 (ref: Random.h:4) */
    uint32_t kernel;               /* cgpt_kernel */
    uint32_t flags;                /* cgpt_render_flags */
    /* Interleaved row bands for load-balanced multi-GPU tiling (all zero = the contiguous rows [row_begin,row_end)):
     * with interleave_rows = h, interleave_count = R, interleave_index = r this context renders the global rows
     * (k*R + r)*h + j, k = 0,1,..., 0 <= j < h, that are < height; its band is stored compactly in that order.
     * row_begin/row_end must then be 0/height. */
    uint32_t interleave_rows, interleave_count, interleave_index;
} cgpt_render_params;

/* ref: Main.cpp:218-226 (Statistics), :207 (total_energy_received) + traversal counters for the roofline */
typedef struct cgpt_stats {
    uint64_t traced_rays;          /* IntersectScene calls, ref: Main.cpp:301 */
    uint64_t inner_steps;          /* executions of BVH.cpp:93-98 (valid with CGPT_RENDER_COUNTERS) */
    uint64_t tri_tests;            /* executions of BVH.cpp:76-77 (valid with CGPT_RENDER_COUNTERS) */
    uint64_t bvh_depth_sum;        /* sum of payload.bvh_depth, ref: BVH.cpp:118 (valid with CGPT_RENDER_COUNTERS) */
    uint64_t closest_hits;         /* mesh hits shaded, ref: Main.cpp:332 (valid with CGPT_RENDER_COUNTERS) */
    double total_energy_received;  /* ref: Main.cpp:735 */
    uint32_t num_accumulated;      /* ref: Main.cpp:205 */
    uint32_t kernel_launches;      /* render kernels launched since the last reset */
    double kernel_ms;              /* wall time of the render calls' device work, from hipEvents on the context's stream */
    uint32_t dominant_launches;    /* launches of the dominant kernel (megakernel, or the wavefront trace kernel) ... */
    uint32_t dominant_waves_per_simd; /* resident waves per SIMD of the dominant kernel (occupancy query): the setting the issue roof is measured at */
    double dominant_ms;            /* ... and their summed duration, from hipEvents on the streams they were launched on */
    /* multi-device context (one-device context: n_devices = 1, device_ms[0] = kernel_ms, the rest 0) */
    double gather_ms;              /* summed duration of the framebuffer exchanges since the last reset: grouped RCCL send/recv (or peer
                                      copies) + row reorder, hipEvents on device_ids[0]'s stream (the presenter's side of Main.cpp:935) */
    uint32_t gathers;              /* exchanges since the last reset */
    uint32_t n_devices;            /* devices (ranks) of the context */
    uint32_t rccl_ranks;           /* ranks of the RCCL communicator the exchange runs on (0: one-device context or peer-copy gather) */
    uint32_t last_kernel;          /* cgpt_kernel the last cgpt_render ran (AUTO resolved) */
    double device_ms[8];           /* kernel_ms of every device, rank order (kernel_ms above is their maximum: they run side by side) */
    /* the wavefront pipeline's round-0 trace launches (primary rays: the reference does not jitter, so the 64 rays of a wave are
       identical, SURVEY A-14) are a different population from the later rounds': their share of dominant_ms / dominant_launches */
    double dominant_round0_ms;
    uint32_t dominant_round0_launches;
    uint32_t chain_followers;      /* wavefront later-round extend rays not traced because the leader of their pixel's specular chain
                                      traced the same ray (the election of wavefront_kernels.hip); saturates at 2^32 - 1 */
    uint64_t probe_resolved;       /* wavefront rays that the shade kernel decided itself from the top of IntersectScene (object list, mesh
                                      roots, analytic primitives) and never queued for the trace kernel; each is counted in traced_rays too.
                                      0 with CGPT_RENDER_COUNTERS, in the debug views and with the tuning knob probe = 0 */
} cgpt_stats;

typedef struct cgpt_ctx cgpt_ctx;

uint32_t cgpt_abi_version(void);

/* replaces ThreadPool::Init / Exit (ref: Main.cpp:773,944; ThreadPool.cpp:81-121): binds 1..8 HIP devices of one node.
 * n_devices == 1: one GPU, one stream.  n_devices > 1: ONE context for the whole frame, as the reference has one Render() --
 * every call below takes the full image; the library cuts it into bands of rows dealt round-robin over the devices, renders
 * them side by side (scene replicated, no exchange while tracing), and cgpt_read_accumulator / cgpt_read_pixels run one grouped
 * RCCL exchange of the float4 bands to device_ids[0] over xGMI (csrc/device/multi_gpu.hip).  The image is bit-identical for
 * any device count.  Such a context takes row_begin = 0, row_end = height and no interleave in cgpt_render_params. */
enum cgpt_ctx_flags {
    CGPT_CTX_FORCE_COLLECTIVE = 1u,  /* n_devices == 1 too goes through the multi-device code: tiling, RCCL exchange (with itself), reorder */
    CGPT_CTX_GATHER_PEER_COPY = 2u   /* gather with hipMemcpyPeerAsync instead of RCCL; device ids may then repeat (several ranks on
                                        one GPU: how the tiling is tested on a one-GPU box) */
};
int cgpt_ctx_create(const int* device_ids, int n_devices, uint32_t flags, cgpt_ctx** out);
int cgpt_ctx_destroy(cgpt_ctx* ctx);
/* replaces EXCEPT/LOG_ERR (ref: Common.h:9): message of the last failing call on ctx (or of the last failing
 * cgpt_ctx_create when ctx is NULL). Never NULL. */
const char* cgpt_last_error(const cgpt_ctx* ctx);
/* run on a caller-provided hipStream_t (e.g. torch's current stream): the calls that follow are ordered behind what the caller queued
 * on it, and each still returns with its own work done.  NULL restores the context's own stream (non-blocking: it waits for nobody's
 * queued work).  NULL therefore never names the device's default stream -- which is what torch's current stream is on ROCm unless the
 * caller made another one current -- and the default stream cannot be named at all: hipStreamLegacy and hipStreamPerThread are refused
 * with CGPT_ERR_UNSUPPORTED and nothing changed (the renders join their pool streams back through event waits on this stream, which
 * the HIP runtime does not take on hipStreamLegacy: DESIGN.md 5.31).  Use a non-default stream (hipStreamCreate, torch.cuda.Stream);
 * Renderer.set_stream raises ValueError for a handle of 0 so that torch's default stream is never silently read as "own stream".
 * The previous stream is drained first; the stream stays the caller's (cgpt_ctx_destroy drains it and leaves it alone); a
 * multi-device context owns its streams and refuses with CGPT_ERR_UNSUPPORTED. */
int cgpt_set_stream(cgpt_ctx* ctx, void* hip_stream);
/* Resampled importance sampling of the NEE light sample (Talbot et al. 2005): at every bounce that samples a light,
 * `candidates` light samples are drawn as the reference draws its one, each is weighed by its unshadowed contribution, and one survivor
 * gets the shadow ray -- one shadow ray and the same expectation as before, at close to the variance of `candidates` NEE samples.
 * Context state like the stream, not scene state: the default is 1 (the reference's estimator, bit for bit), cgpt_scene_upload keeps the
 * value, and it may be set before a scene exists.  Range 1..32; 0 or more than 32 is refused with CGPT_ERR_INVALID and nothing changed.
 * Read by the renders that follow; ignored where there is no NEE (next_event_estimation_enabled == 0, CGPT_MODE_BRUTE_FORCE and the
 * TracePath half of CGPT_MODE_COMPARISON).  The caller resets the accumulator; the denoiser's cached guides stay valid (first hits do
 * not depend on it); a multi-device context sets every device. */
int cgpt_set_nee_candidates(cgpt_ctx* ctx, uint32_t candidates);
/* How IntersectScene reaches the objects.  0 (the default): the object list is walked in order, every object tested for
 * every ray -- every kernel is then the one it was before this call existed.  1: a balanced tree over the object index ranges with a
 * world-space box per node is walked in preorder; objects are still visited in index order (the strict t <, the object order on ties,
 * the BVH-depth view and the counters tri_tests, bvh_depth_sum, closest_hits are the list walk's), the tree only skips runs of objects
 * whose union box the ray misses, which pays from some tens of objects on when neighbouring indices are neighbours in space
 * (Scene.sort_objects_spatially in the Python package orders them).  inner_steps no longer counts the root step of a skipped mesh.
 * Context state like cgpt_set_nee_candidates: may be set before a scene exists, cgpt_scene_upload keeps it, any other value is refused
 * with CGPT_ERR_INVALID and nothing changed, a multi-device context sets every device.  The boxes follow cgpt_scene_upload,
 * cgpt_scene_update_transforms, cgpt_scene_refit_mesh and cgpt_scene_update_primitive.  The image does not depend on the mode: the
 * accumulator may be kept, and the denoiser's cached guides stay valid. */
int cgpt_set_top_level(cgpt_ctx* ctx, uint32_t mode);

/* replaces the implicit use of data.objects / materials / light_source_indices (ref: Main.cpp:209-212, 303-315) */
int cgpt_scene_upload(cgpt_ctx* ctx, const cgpt_scene_desc* scene);
/* Mesh instancing: cgpt_scene_upload with one device copy for the mesh objects that name the same geometry.  Mesh objects
 * whose node_offset, node_count, tri_offset and tri_count are all equal form a mesh group; the group's triangles and tree are laid out
 * once, from its first member, and every member reaches that copy.  Each member keeps its own material, total_area (as given), smooth
 * flag, transform and top-level box, so n placements of a mesh cost n object records and one mesh.  Slices that overlap only in part are
 * separate meshes; triangle objects, spheres and planes are laid out per object.  Validation, refusals, messages, what is reset
 * (roughnesses, smooth flags and transforms to 0 and the identity, the denoiser's guides and history) and what is kept
 * (cgpt_set_nee_candidates, cgpt_set_top_level) are cgpt_scene_upload's, on every device of a multi-device context; the 2^26 limit applies
 * to the records laid out, not to the sum over the objects.  No kernel differs: every render, probe and guide of an instanced upload
 * equals that of cgpt_scene_upload of the same scene bit for bit, counters included.
 * THE ONE DIFFERENCE: cgpt_scene_refit_mesh through any member moves EVERY instance of the group -- the one copy is refitted, and each
 * member's total_area and top-level box follow.  After cgpt_scene_upload a refit moves the named object alone, as it always has.
 * cgpt_scene_export_bvh through any member returns the group's tree.  The other edits (transforms, smooth normals, materials, roughness,
 * primitives) stay per object with their refusals: a light may share a group with objects that are no lights, and only the light itself
 * is held to the identity and to flat normals.  A later cgpt_scene_upload of the same scene returns to per-object copies.
 * An added export: CGPT_ABI_VERSION stays 2. */
int cgpt_scene_upload_instanced(cgpt_ctx* ctx, const cgpt_scene_desc* scene);
/* What the uploaded scene occupies, after either upload (CGPT_ERR_NO_SCENE without one; a multi-device context reports one device, and
 * every device holds the same).  Of the edits only cgpt_scene_rebuild_mesh changes it, at a mesh's first rebuild; the skin buffers of cgpt_scene_set_skin and the target buffers of
 * cgpt_scene_set_morph_targets are not counted.  An added export:
 * CGPT_ABI_VERSION stays 2. */
typedef struct cgpt_scene_footprint {
    uint64_t device_bytes;       /* bytes of the scene's allocations on one device: the triangle, node, normal, material, object and light
                                  * arrays, the refit levels and the room of the top-level tree (not the framebuffer, not a refit's staging) */
    uint32_t n_objects, n_mesh_objects, n_mesh_copies;   /* copies: the meshes actually laid out (== n_mesh_objects after cgpt_scene_upload) */
    uint32_t n_leaf_records, n_pair_records, n_orig_triangles;
} cgpt_scene_footprint;
int cgpt_get_scene_footprint(cgpt_ctx* ctx, cgpt_scene_footprint* out);
/* replaces Material::RenderImGui edits (ref: Main.cpp:71-91,263-265); the caller resets the accumulator as the reference does */
int cgpt_scene_update_materials(cgpt_ctx* ctx, const cgpt_material* materials, uint32_t n_materials);
/* Microfacet BRDF (reference README, "Planned"): the roughness in [0, 1] of every material's specular lobe (the `r < specular` branch),
 * one value per uploaded material.  0 is the reference's perfect mirror, bit for bit; r > 0 is isotropic GGX reflection with
 * alpha = r^2, visible-normal sampling, height-correlated Smith masking and the constant Fresnel `albedo`.  Light
 * materials and the dielectric lobe ignore it.  cgpt_scene_upload resets every roughness to 0; cgpt_scene_update_materials keeps it.
 * Refused, with nothing changed: no scene (CGPT_ERR_NO_SCENE); roughness NULL, n_materials other than the uploaded count, or a value
 * that is not finite or lies outside [0, 1] (CGPT_ERR_INVALID).  The caller resets the accumulator, as with the materials.  The
 * denoiser's cached guides stay valid: first hits and albedo do not depend on roughness.  A HIP failure during the write drops the
 * scene, as the geometry edits below do; a multi-device context updates every device. */
int cgpt_scene_update_roughness(cgpt_ctx* ctx, const float* roughness, uint32_t n_materials);
/* Rough dielectrics (frosted glass, Walter et al. 2007): the transmission roughness in [0, 1] of every material's dielectric lobe (the
 * `specular <= r < specular + refractivity` branch), one value per uploaded material.  0 is the reference's polished interface, bit for
 * bit; t > 0 refracts and reflects about a GGX microfacet normal with alpha_t = t^2, visible-normal sampling, the reference's Fresnel
 * term at the facet, height-correlated Smith masking and physical total internal reflection at the facet.  It is
 * separate from the roughness above: the specular lobe, the diffuse lobe and light materials ignore it, and the dielectric lobe ignores
 * `roughness`.  cgpt_scene_upload resets every value to 0; cgpt_scene_update_materials and cgpt_scene_update_roughness keep it, and it
 * keeps theirs.  Refused, with nothing changed: no scene (CGPT_ERR_NO_SCENE); the array NULL, n_materials other than the uploaded count,
 * or a value that is not finite or lies outside [0, 1] (CGPT_ERR_INVALID).  The caller resets the accumulator, as with the materials.
 * The denoiser's cached guides stay valid.  A HIP failure during the write drops the scene; a multi-device context updates every
 * device. */
int cgpt_scene_update_transmission_roughness(cgpt_ctx* ctx, const float* transmission_roughness, uint32_t n_materials);
/* Smooth shading: one word per uploaded object.  0 is the reference's flat shading normal, v0.normal of the hit triangle (ref:
 * Primitives.cpp:148-151), bit for bit; 1 shades a mesh or a stand-alone triangle object with the three vertex normals of the hit
 * triangle interpolated at the hit point and normalised, kept on the geometric side the ray sees (tests/smooth_ref.py
 * states the operations).  A triangle whose three normals are bitwise equal shades as with 0.  Spheres and planes ignore their entry.
 * cgpt_scene_upload resets every flag to 0; the material, roughness, refit and primitive edits keep the flags.  Refused, with nothing
 * changed: no scene (CGPT_ERR_NO_SCENE); smooth NULL, n_objects other than the uploaded count, or a value that is neither 0 nor 1
 * (CGPT_ERR_INVALID); a 1 on an object listed in light_indices (CGPT_ERR_INVALID: light sampling uses v0.normal, and the two must not
 * disagree).  The caller resets the accumulator.  The denoiser's cached guides are recomputed: they hold the normal.  A HIP failure
 * during the write drops the scene; a multi-device context updates every device. */
int cgpt_scene_update_smooth_normals(cgpt_ctx* ctx, const uint32_t* smooth, uint32_t n_objects);
/* Per-object transforms: 12 floats per uploaded object, the rows of [A | b], row-major, so that world = A p + b for a point p of the
 * object's uploaded (object-space) geometry.  Every trace and shade path honours it: a ray (o, d, t) enters a transformed mesh or
 * stand-alone triangle object as o' = A^-1 o - A^-1 b, d' = A^-1 d (d' is not renormalised, so t is the same number in both spaces),
 * the hit position stays o + d t of the world ray and the shading normal is normalize(A^-T n) (tests/transform_ref.py
 * states the operations).  An object whose 12 floats are bitwise the identity (1,0,0,0, 0,1,0,0, 0,0,1,0) is untransformed and is walked
 * exactly as without this call; with every object untransformed the renders run the kernels they ran before, bit for bit.  Mirrors
 * (det < 0) and non-uniform scale are allowed.  The reference's absolute determinant epsilon of the triangle test applies to the
 * object-space numbers, so scaling an object by its transform moves it.
 * cgpt_scene_upload resets every object to the identity; the material, roughness, transmission-roughness, smooth-normal, refit and
 * primitive edits keep the transforms.  cgpt_scene_refit_mesh takes object-space triangles (the result sits at A (new triangles) + b),
 * cgpt_scene_export_bvh returns object-space bounds, cgpt_intersect_rays takes world rays and returns world t.
 * Refused before any device write, with nothing changed: no scene (CGPT_ERR_NO_SCENE); object_to_world NULL or n_objects other than the
 * uploaded count; an entry that is not finite; an A that cannot be inverted -- the inverse is computed in double from the float entries,
 * and det == 0, a det that is not finite, or an entry of A^-1 or of -A^-1 b that is not finite once rounded to float refuses; anything
 * but the identity on a sphere or a plane (cgpt_scene_update_primitive moves those) or on an object listed in light_indices (mesh-light
 * sampling reads the object-space triangles and area) -- all CGPT_ERR_INVALID.  The caller resets the accumulator.  The denoiser's cached
 * guides are recomputed: they hold position and normal.  The temporal history (cgpt_denoise_temporal) is dropped, unless the next
 * temporal call sets CGPT_TEMPORAL_FOLLOW_TRANSFORMS: that call carries the hits on the moved objects back through M_prev M_cur^-1 and
 * keeps the history; until it has succeeded cgpt_read_temporal_history refuses.  A HIP failure during the write drops the scene; a
 * multi-device context updates every device. */
int cgpt_scene_update_transforms(cgpt_ctx* ctx, const float* object_to_world, uint32_t n_objects);

/* ---- in-place geometry edits of the uploaded scene (no re-upload; the caller resets the accumulator, as with the materials) ----
 * Every call validates before its first device write: a refused call leaves the device scene as it was.  If a HIP call fails after
 * the writes began, the scene is dropped (the next render returns CGPT_ERR_NO_SCENE) instead of a half-edited one being rendered.
 * A multi-device context edits every device's copy (and drops every copy on such a failure); the export reads the first device's. */
/* BVH refitting (reference README, "Planned"): new positions and normals for mesh `obj_index` with its tree kept -- node numbering,
 * left_first / prim_count and tri_indices stay; each node's bounds become BVH::CalculateNodeBounds (ref: BVH.cpp:188-202) over its
 * current leaf range of the new triangles, and total_area the sum of GetTriangleArea in original order (ref: BVH.cpp:22).
 * triangles: n_tris == the uploaded tri_count, in the object's original order.  A triangle object takes n_tris = 1 (it has no bounds
 * and no total_area: 0 is reported).  Spheres and planes: CGPT_ERR_INVALID.  total_area_out may be NULL.
 * The tree was built for the old positions: after a large deformation cgpt_scene_rebuild_mesh splits it again, in place.
 * After cgpt_scene_upload_instanced the refit moves every object that shares `obj_index`'s copy (see there). */
int cgpt_scene_refit_mesh(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_triangle* triangles, uint32_t n_tris, float* total_area_out);
/* BVH::Rebuild (ref: BVH.cpp:47-59) of uploaded mesh `obj_index`, in place on the device: the tree is split again over
 * the triangles the device copy holds now -- whatever last wrote them: an upload, a refit, a skin, a morph or a batch pose -- starting
 * from the mesh's current leaf order, as cgpth_scene_rebuild_bvh does on the host.  The triangles do not leave the device and the host
 * does no per-triangle work; of the nodes it keeps one word of bookkeeping each, for this mesh only.  Afterwards the device scene is what an upload of the host mirror after the same edits and
 * cgpth_scene_rebuild_bvh(scene, obj_index, build_option) would hold: cgpt_scene_export_bvh returns that tree word for word (its node
 * count in *n_nodes_out, its depth in *max_depth_out; either may be NULL), and renders, probes and guides are bit-identical to that
 * upload's, before and after any later edit applied to both.  total_area, materials, smooth flags, transforms, skins and morph targets
 * are kept.  The image may differ from the one before the call only where two triangles of the mesh tie in t (the visiting order
 * changes); the caller resets the accumulator.  The denoiser's guides are recomputed and the temporal history is dropped, with every
 * CGPT_TEMPORAL_FOLLOW_* flag, as after a refit -- but the triangles did not change, so a skin's or the targets' known pose stays known.
 * build_option: CGPT_BUILD_NAIVE_SPLIT, CGPT_BUILD_SAH_SPLIT_INTERVALS or CGPT_BUILD_SAH_BINNED; CGPT_BUILD_SAH_SPLIT_PRIMITIVES never
 * splits (SURVEY A-5): CGPT_ERR_UNSUPPORTED.  Refused before the first write to the scene, with nothing changed: no scene
 * (CGPT_ERR_NO_SCENE); an object out of range, a sphere, a plane or a triangle object, an unknown option (CGPT_ERR_INVALID); with
 * CGPT_BUILD_SAH_BINNED a position that is not finite or exceeds 1e30 in magnitude (CGPT_ERR_INVALID; checked on the device); a new
 * tree deeper than the 64-entry traversal stack (CGPT_ERR_UNSUPPORTED); a record span that would pass 2^26 records (CGPT_ERR_INVALID).
 * A mesh's first rebuild moves its records to a span of tri_count - 1 records at the end of the record array, which grows
 * (cgpt_get_scene_footprint); later rebuilds reuse the span.  After cgpt_scene_upload_instanced a rebuild through any placement
 * rebuilds the group's one copy.  An added export: CGPT_ABI_VERSION stays 2. */
int cgpt_scene_rebuild_mesh(cgpt_ctx* ctx, uint32_t obj_index, uint32_t build_option, uint32_t* n_nodes_out, uint32_t* max_depth_out);
/* the mesh's tree as it is now on the device, in the reference's 32-byte layout and node numbering (n_nodes == the uploaded node_count,
 * or what the last cgpt_scene_rebuild_mesh reported):
 * what a host that keeps its own BVH (the BVH panel, a later Rebuild) copies back after a refit */
int cgpt_scene_export_bvh(cgpt_ctx* ctx, uint32_t obj_index, cgpt_bvh_node* nodes_out, uint32_t n_nodes);
/* The surface-area cost of uploaded meshes' trees as they are now, summed on the device (csrc/host/tree_cost.h states the
 * metric, tests/tree_cost_ref.py the same in numpy): what tells a refitted tree that has gone bad from one that has not, without the
 * readback of cgpt_scene_export_bvh.  For a mesh whose root split, in double from the float bounds: H(box) = dx dy + dy dz + dz dx, the
 * root box = the union of the root's two child boxes, and
 *   cost = (c_inner (H(root) + sum of H over inner children) + c_tri sum of H n_tris over leaf children) / H(root)
 * over the child boxes of every splitting node -- the expected work of a ray that hits the root box, c_inner a node and c_tri a
 * triangle; it does not change with the mesh's scale.  A mesh whose root is a leaf reports c_tri n_tris, root_half_area 0, n_inner 0 and
 * n_leaves 1, with no device work.  n_inner counts the splitting nodes (the root among them), n_leaves the leaves.
 * One call serves n entries with two launches and one readback on the context's stream; the same object may be named twice.  The sums
 * have a fixed order: the same call returns the same bits, an entry returns the same bits alone or in any batch at any position, objects
 * that share a copy (cgpt_scene_upload_instanced) report equal bits, and so does every device of a multi-device context -- each sums its
 * own copy, the first device's numbers are returned, and a device that disagrees fails the call (CGPT_ERR_HIP; the scene is kept).
 * The call only reads: no generation moves, the denoiser's guides and temporal history stay, renders and exports are bit-identical
 * before and after.  Refused before any launch, with `out` unwritten and the entry named: no scene (CGPT_ERR_NO_SCENE); obj_indices or
 * out NULL with n > 0, an object out of range, a sphere, a plane or a triangle object, a constant that is not finite and > 0
 * (CGPT_ERR_INVALID).  n == 0 is CGPT_OK without a launch.  A cost that is not finite -- a bound that is not, or a root box without
 * area -- is CGPT_ERR_INVALID naming the first such entry, with `out` unwritten.  An added export: CGPT_ABI_VERSION stays 2. */
typedef struct cgpt_tree_cost {
    double cost, root_half_area;
    uint32_t n_inner, n_leaves, max_leaf_tris, reserved;   /* reserved: 0 */
} cgpt_tree_cost;
int cgpt_scene_tree_costs(cgpt_ctx* ctx, const uint32_t* obj_indices, uint32_t n, double c_inner, double c_tri, cgpt_tree_cost* out);
/* Rebuild the meshes whose trees have degraded: one cgpt_scene_tree_costs over all entries gives cost_before; cgpt_scene_rebuild_mesh
 * (build_option as there) then runs for every entry with cost_before > ratio * reference_cost, once per copy where several entries reach
 * one (cgpt_scene_upload_instanced; every entry that reaches a rebuilt copy reports rebuilt = 1); one more cost call over those entries
 * gives cost_after.  An entry whose copy was not rebuilt reports cost_after = cost_before and rebuilt = 0.  The call holds no baseline:
 * the caller keeps cost_after as the next reference_cost.  When nothing is rebuilt nothing of the scene changes and the temporal history
 * is kept; otherwise each rebuild acts as cgpt_scene_rebuild_mesh does.  A multi-device context decides once, from its first device's
 * costs, and rebuilds on every device, so the copies stay equal.
 * Refused up front, for every entry, before anything is rebuilt and with `results` unwritten: what cgpt_scene_tree_costs refuses; a
 * ratio or a reference_cost that is not finite and > 0; and what cgpt_scene_rebuild_mesh can refuse without a launch -- an unknown
 * build option, CGPT_BUILD_SAH_SPLIT_PRIMITIVES (CGPT_ERR_UNSUPPORTED), a first rebuild whose record span would pass 2^26 records.
 * Its other refusals need the device and may come mid-call: the binned build's domain check, a new tree deeper than the traversal
 * stack, and the 2^26 limit reached by the spans of several first rebuilds together.  The error then names the entry, `results` is
 * unwritten, and the meshes already rebuilt stay rebuilt and valid.  An added export: CGPT_ABI_VERSION stays 2. */
typedef struct cgpt_rebuild_candidate { uint32_t obj_index, reserved; double reference_cost; } cgpt_rebuild_candidate;
typedef struct cgpt_rebuild_result { double cost_before, cost_after; uint32_t rebuilt, reserved; } cgpt_rebuild_result;
int cgpt_scene_rebuild_degraded(cgpt_ctx* ctx, const cgpt_rebuild_candidate* entries, uint32_t n, double ratio, uint32_t build_option,
                                double c_inner, double c_tri, cgpt_rebuild_result* results);
/* Primitive::RenderImGui's sliders (ref: Primitives.cpp:385-410): a sphere's centre and radius (radius^2 = r*r, as at upload) or a
 * plane's normal and point.  obj->kind and obj->mat_index must equal the uploaded ones; the other fields of *obj are ignored. */
int cgpt_scene_update_primitive(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_object* obj);

/* ---- skinning: pose a mesh on the device from joint matrices (linear blend skinning, four influences per triangle corner) ----
 * The bind pose, the joint indices and the weights stay on the device; a pose is a write of n_joints x 48 bytes and one kernel in
 * front of the refit's bound pass, with no per-triangle work on the host (csrc/host/skinning.h states the arithmetic
 * and cgpth_skin_triangles evaluates it on the host, tests/skin_ref.py in numpy).  Added exports: CGPT_ABI_VERSION stays 2.
 *
 * cgpt_scene_set_skin: copies bind_triangles (n_tris triangles in the object's original order, as cgpt_scene_refit_mesh takes them),
 * joints and weights (12 n_tris entries each: corner c of triangle t has joints[12 t + 4 c + k] and weights[12 t + 4 c + k], k < 4) to
 * device buffers the context owns (72 + 24 + 48 bytes a triangle, on every device of a multi-device context).  THE SCENE DOES NOT
 * CHANGE: the geometry moves at the first cgpt_scene_skin_mesh.  A second call on the same object replaces its skin.  Meshes and
 * stand-alone triangle objects (n_tris = 1).  Refused before any device write, with nothing changed: no scene (CGPT_ERR_NO_SCENE); a
 * NULL array, an object out of range, a sphere or a plane, an object listed in light_indices (mesh-light sampling reads total_area,
 * which a pose does not recompute), n_tris other than the uploaded count, n_joints 0 or above 1024, a joint index >= n_joints, a weight
 * or a bind float that is not finite (CGPT_ERR_INVALID).
 *
 * cgpt_scene_skin_mesh: poses the object from joint_matrices -- n_joints (the skin's) x 12 floats, the rows of [A | b], row-major, the
 * layout of cgpt_scene_update_transforms: object-space skinning matrices (for glTF, jointGlobal * inverseBind).  A pose is always
 * computed from the bind pose, never from the previous pose.  Afterwards the device scene is what
 * cgpt_scene_refit_mesh(obj_index, <cgpth_skin_triangles of the skin and the matrices>) would have left, bit for bit -- the triangle
 * records, both normal records, every node's bounds, the top-level box -- WITH ONE EXCEPTION: the object's total_area keeps its
 * uploaded value.  Only mesh-light sampling reads it, and a skinned object cannot be a light.  Weights are used as given (never
 * renormalised, a zero weight's joint is still read); the blended A moves the normal, not its inverse transpose (exact for rigid
 * joints and uniform scale).  Everything else follows the refit: the caller resets the accumulator; the denoiser's guides are
 * recomputed and the temporal history is dropped, CGPT_TEMPORAL_FOLLOW_TRANSFORMS included, unless the next temporal call sets
 * CGPT_TEMPORAL_FOLLOW_POSES (below: it carries the hits on the re-posed objects back and keeps the history); transforms (the pose is in object space:
 * it appears at A pose + b), smooth flags, materials and roughnesses are kept; after cgpt_scene_upload_instanced every placement of
 * the object's group moves; a multi-device context poses every device's copy from that device's skin buffers; a HIP failure after the
 * first write drops the scene.  Refused, with nothing changed: no scene (CGPT_ERR_NO_SCENE); an object out of range or without a
 * skin, n_joints other than the skin's, joint_matrices NULL or an entry that is not finite (CGPT_ERR_INVALID).
 *
 * cgpt_scene_clear_skin: frees the object's skin buffers; the geometry stays at the last pose.  CGPT_OK without a skin on the object.
 * cgpt_scene_upload and cgpt_scene_upload_instanced drop every skin.  cgpt_scene_refit_mesh on a skinned object works as before and
 * keeps the skin; the next pose overwrites what it wrote. */
int cgpt_scene_set_skin(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_triangle* bind_triangles, const uint16_t* joints, const float* weights,
                        uint32_t n_tris, uint32_t n_joints);
int cgpt_scene_skin_mesh(cgpt_ctx* ctx, uint32_t obj_index, const float* joint_matrices, uint32_t n_joints);
int cgpt_scene_clear_skin(cgpt_ctx* ctx, uint32_t obj_index);

/* ---- morph targets (blend shapes): pose a mesh on the device from a few weights, fused with its skin ----
 * The base triangles and the targets' displacements stay on the device; a pose is a write of the active (index, weight) pairs and one
 * kernel in front of the refit's bound pass (csrc/host/morph.h states the arithmetic and cgpth_morph_triangles
 * evaluates it on the host, tests/morph_ref.py in numpy).  Added exports: CGPT_ABI_VERSION stays 2.
 *
 * cgpt_scene_set_morph_targets: copies base_triangles (n_tris triangles in the object's original order, as cgpt_scene_refit_mesh takes
 * them) and target_deltas (n_targets x n_tris records, target-major: target_deltas[k * n_tris + t]; a record has the cgpt_triangle
 * layout but holds displacements, per corner a position delta and a normal delta -- glTF's POSITION / NORMAL target accessors expanded
 * to unindexed corners) to device buffers the context owns (72 (n_targets + 1) bytes a triangle, on every device of a multi-device
 * context; stored in the order of the object's leaf slots, or in the given order with the cgpt_set_tuning knob "morph_leaf_order" 0).
 * THE SCENE DOES NOT CHANGE: the geometry moves at the first pose; the weights start at all zero.  A second call on the same object
 * replaces its targets.  Meshes and stand-alone triangle objects (n_tris = 1).  Refused before any device write, with nothing changed:
 * no scene (CGPT_ERR_NO_SCENE); a NULL array, an object out of range, a sphere or a plane, an object listed in light_indices (mesh-light
 * sampling reads total_area, which a pose does not recompute), n_tris other than the uploaded count, n_targets 0 or above 256, any
 * float that is not finite (CGPT_ERR_INVALID).
 *
 * cgpt_scene_morph_mesh: stores weights (n_targets, the installed count) and poses the object: each of a triangle's 18 floats is
 * x = base; x = x + weights[k] * delta_k for k ascending, a target whose weight is +0 or -0 skipped; with no active target the triangle
 * is the base triangle bit for bit, otherwise every corner's normal is renormalised (the base normal where the blend has no finite
 * positive length).  Weights are used as given: negative and above 1 are allowed.  A pose is always computed from the base, never from
 * the previous pose.  Afterwards the device scene is what cgpt_scene_refit_mesh(obj_index, <cgpth_morph_triangles of the targets and
 * the weights>) would have left, bit for bit, except that total_area keeps its uploaded value.  Everything else follows
 * cgpt_scene_skin_mesh: the caller resets the accumulator; guides are recomputed; transforms, smooth flags and materials are kept; every
 * placement of an instanced group moves; every device of a multi-device context is posed; a HIP failure after the first write drops the
 * scene.  The temporal history is dropped, CGPT_TEMPORAL_FOLLOW_POSES included, unless the next temporal call sets
 * CGPT_TEMPORAL_FOLLOW_MORPHS (below: it carries the hits on the morphed objects back and keeps the history).  Refused, with nothing
 * changed: no scene (CGPT_ERR_NO_SCENE); an object out of range or without targets, n_targets other than the installed count, weights
 * NULL or a weight that is not finite (CGPT_ERR_INVALID).
 *
 * WITH A SKIN (glTF order: morph, then skin): while an object has morph targets installed, the morphed base takes the place of the
 * skin's bind pose (the skin's own bind array is not read).  After either cgpt_scene_morph_mesh or cgpt_scene_skin_mesh on such an
 * object the scene is skin_triangles(morph_triangles(base, deltas, w_last), joints, skin_weights, M_last) of the two host mirrors --
 * w_last the last weights given (zeros if none), M_last the matrices of the skin's last cgpt_scene_skin_mesh since it was installed;
 * while the skin has not been posed the morph alone applies.  The order of the two calls does not matter; one kernel does both.  For
 * such an object a temporal call with CGPT_TEMPORAL_FOLLOW_POSES alone knows no pose: its history is dropped; with
 * CGPT_TEMPORAL_FOLLOW_MORPHS as well its pose is known by the weights and the matrices together.
 *
 * cgpt_scene_clear_morph_targets: frees the object's target buffers; the geometry stays where it is, and a skin goes back to its own
 * bind pose at its next cgpt_scene_skin_mesh.  CGPT_OK without targets on the object.  cgpt_scene_upload and
 * cgpt_scene_upload_instanced drop every object's targets.  cgpt_scene_refit_mesh on a morphed object works as before and keeps the
 * targets; the next pose overwrites what it wrote. */
int cgpt_scene_set_morph_targets(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_triangle* base_triangles, const cgpt_triangle* target_deltas,
                                 uint32_t n_tris, uint32_t n_targets);
int cgpt_scene_morph_mesh(cgpt_ctx* ctx, uint32_t obj_index, const float* weights, uint32_t n_targets);
int cgpt_scene_clear_morph_targets(cgpt_ctx* ctx, uint32_t obj_index);

/* ---- posing many objects in one call ----
 * cgpt_scene_pose_objects: what cgpt_scene_morph_mesh (an entry with weights) and then cgpt_scene_skin_mesh (an entry with matrices)
 * would do for each of n_poses entries in array order, with a number of kernel launches that does not grow with n_poses: one launch per
 * kernel instantiation in use, one per depth of the deepest tree among the entries, one for the boxes -- and one synchronise, one
 * readback and one rebuild of the top-level tree for the whole batch.  Afterwards the device scene is what those single calls leave, bit
 * for bit: triangle records, both normal records, every node's bounds, the top-level boxes, every placement of an instanced group, on
 * every device of a multi-device context; total_area stays untouched.  What a later cgpt_denoise_temporal call with
 * CGPT_TEMPORAL_FOLLOW_POSES / _MORPHS makes of its history is what it makes of it after the single calls.  An entry with both arrays is
 * posed once (the fused kernel); an entry with weights alone on an object whose skin has been posed takes that skin's last matrices, an
 * entry with matrices alone on an object with targets its last weights.
 * Everything is validated before the first device write: a refused call changes nothing, the denoiser's guides and temporal history
 * included.  CGPT_ERR_INVALID, with the entry's index in the message, for whatever the single call refuses of an entry, and for: poses
 * NULL; an entry with n_joints == 0 and n_targets == 0; a count with a NULL array; two entries that name one object; two entries that
 * name objects of one instanced mesh group (they share the copy: sequentially the last would win).  n_poses == 0: CGPT_OK, nothing
 * happens.  A HIP failure after the first write drops the scene, as in the single calls. */
typedef struct cgpt_pose {
    uint32_t obj_index;
    uint32_t n_joints;            /* 0: this entry gives no joint matrices */
    const float* joint_matrices;  /* n_joints x 12, as cgpt_scene_skin_mesh takes them */
    uint32_t n_targets;           /* 0: this entry gives no morph weights */
    const float* weights;         /* n_targets, as cgpt_scene_morph_mesh takes them */
} cgpt_pose;
int cgpt_scene_pose_objects(cgpt_ctx* ctx, const cgpt_pose* poses, uint32_t n_poses);

/* ---- animation clips: joint matrices computed on the device from keyframes ----
 * cgpt_scene_animate_objects is cgpt_scene_pose_objects with each entry's joint matrices computed on the device: the clip, the skeleton
 * and the skin are resident, a frame of an animated scene is one call with a clip and a time per object.  csrc/host/animation.h states
 * the arithmetic -- sampling (STEP, LINEAR; rotations by normalised lerp, not slerp), the local matrices, the bottom-up walk, the
 * inverse bind matrix, the root -- cgpth_animate_joints evaluates it on the host, tests/anim_ref.py in numpy, and the device agrees
 * with both bit for bit.  The data layout is glTF's.  Added exports: CGPT_ABI_VERSION stays 2.
 *
 * cgpt_scene_set_skeleton: copies a skeleton for the skin of object obj_index: parents (one per joint, -1 a root, any order),
 * inverse_bind (12 floats a joint, the rows of [A | b]), rest (10 floats a joint: T.xyz, R.xyzw, S.xyz) and an optional root matrix
 * (NULL: no multiply).  The object needs a skin with the same n_joints; the skeleton is replaced, cleared and dropped with that skin.
 * Refused (CGPT_ERR_INVALID): no skin, another joint count, a NULL array, a parent out of range, a cycle, a float that is not finite.
 *
 * cgpt_clip_create: copies a clip to every device of the context and returns its handle.  A clip belongs to the context, is shared by
 * any number of objects and survives uploads.  A channel animates one path of one joint: key i is times[first_time + i] with the 3
 * floats (translation, scale) or 4 floats (rotation xyzw) at values[first_value + width i].  At most one channel per (joint, path);
 * n_keys >= 1; times finite and strictly increasing; values finite; counts within times / values: otherwise CGPT_ERR_INVALID.
 * CGPT_ANIM_CUBICSPLINE: CGPT_ERR_UNSUPPORTED.  glTF `weights` channels are not built: morph weights come from the caller.
 * cgpt_clip_destroy: frees it; an unknown handle is CGPT_ERR_INVALID.
 *
 * cgpt_scene_animate_objects: phase 1 refuses whatever cgpt_scene_pose_objects refuses, and: an object without a skeleton, an unknown
 * or destroyed clip, a clip whose n_joints differs from the skeleton's, a time that is not finite; then one kernel evaluates every
 * entry's matrices and, after one synchronise, the host reads them back.  An entry with a matrix entry that is not finite refuses the
 * whole call (CGPT_ERR_INVALID with the entry's index): scene, guides, history and generations stay untouched.  Phase 2 is
 * cgpt_scene_pose_objects' own, reading the matrices where the kernel wrote them; they become the skin's last pose exactly as if the
 * caller had passed them, so the single calls, CGPT_TEMPORAL_FOLLOW_POSES / _MORPHS, cgpt_read_previous_hits, instanced groups and
 * cgpt_scene_rebuild_mesh follow without further work.  weights / n_targets are cgpt_pose's.
 *
 * cgpt_scene_get_joint_matrices: the n_joints x 12 matrices of the skin's last pose, however given.  CGPT_ERR_INVALID before one. */
enum { CGPT_ANIM_PATH_TRANSLATION = 0, CGPT_ANIM_PATH_ROTATION = 1, CGPT_ANIM_PATH_SCALE = 2 };
enum { CGPT_ANIM_STEP = 0, CGPT_ANIM_LINEAR = 1, CGPT_ANIM_CUBICSPLINE = 2 };
typedef struct cgpt_skeleton_desc {
    const int32_t* parents;
    const float* inverse_bind;
    const float* rest;
    const float* root;
    uint32_t n_joints;
} cgpt_skeleton_desc;
typedef struct cgpt_clip_channel {
    uint32_t joint, path, interpolation, n_keys, first_time, first_value;
} cgpt_clip_channel;
typedef struct cgpt_clip_desc {
    uint32_t n_joints, n_channels;
    const cgpt_clip_channel* channels;
    const float* times;
    uint32_t n_times;
    const float* values;
    uint32_t n_values;
} cgpt_clip_desc;
typedef struct cgpt_animation {
    uint32_t obj_index, clip;
    float time;
    uint32_t n_targets;           /* 0: this entry gives no morph weights */
    const float* weights;         /* n_targets, as cgpt_scene_morph_mesh takes them */
} cgpt_animation;
int cgpt_scene_set_skeleton(cgpt_ctx* ctx, uint32_t obj_index, const cgpt_skeleton_desc* skeleton);
int cgpt_clip_create(cgpt_ctx* ctx, const cgpt_clip_desc* clip, uint32_t* clip_out);
int cgpt_clip_destroy(cgpt_ctx* ctx, uint32_t clip);
int cgpt_scene_animate_objects(cgpt_ctx* ctx, const cgpt_animation* entries, uint32_t n_entries);
int cgpt_scene_get_joint_matrices(cgpt_ctx* ctx, uint32_t obj_index, float* out, uint32_t n_joints);

/* ---- layers: up to four clips blended per object, each at a wrapped time ----
 * cgpt_scene_animate_layers is cgpt_scene_animate_objects with every entry's joints blended from 1 .. CGPT_ANIM_MAX_LAYERS clips before
 * the hierarchy walk: a cross-fade of a walk into a run is one entry with two layers.  csrc/host/animation.h states the arithmetic:
 * every layer's time is wrapped over its clip's range [begin, end] (the smallest first-key and the largest last-key time of its
 * channels) by its wrap mode -- CLAMP leaves the time as given, LOOP repeats the range, PINGPONG plays it forth and back -- on the
 * host, once per layer; layers of weight 0 are never sampled; the others' weights are divided by their sum; T and S are the weighted
 * sums of the layers' sampled values, R the weighted sum of the rotations aligned to the first active layer's, normalised once.  An
 * entry with one active layer runs no blend arithmetic: with CLAMP it is cgpt_scene_animate_objects to the bit.  cgpth_animate_layers
 * evaluates the statement on the host, tests/anim_layer_ref.py in numpy, and the device agrees with both bit for bit.
 * The contract is cgpt_scene_animate_objects': the two phases, an entry whose matrices are not finite refusing the whole call with its
 * index, the matrices kept as the skin's last pose, n_entries 0 is CGPT_OK.  Refused further, before any device work, naming the entry
 * and the layer: layers NULL, n_layers 0 or above CGPT_ANIM_MAX_LAYERS, an unknown or destroyed clip or one with another joint count
 * in any layer (inactive ones included), a time that is not finite, a weight that is not finite or negative, no weight above zero, a
 * sum of weights that is not finite, an unknown wrap mode.
 * cgpt_clip_get_range: a clip's begin and end (a clip without channels: 0, 0); either pointer may be NULL. */
enum { CGPT_ANIM_WRAP_CLAMP = 0, CGPT_ANIM_WRAP_LOOP = 1, CGPT_ANIM_WRAP_PINGPONG = 2 };
#define CGPT_ANIM_MAX_LAYERS 4u
typedef struct cgpt_clip_layer {
    uint32_t clip;
    float time, weight;
    uint32_t wrap;                /* CGPT_ANIM_WRAP_* */
} cgpt_clip_layer;
typedef struct cgpt_layered_animation {
    uint32_t obj_index, n_layers;
    const cgpt_clip_layer* layers;
    uint32_t n_targets;           /* 0: this entry gives no morph weights */
    const float* weights;         /* n_targets, as cgpt_scene_morph_mesh takes them */
} cgpt_layered_animation;
int cgpt_scene_animate_layers(cgpt_ctx* ctx, const cgpt_layered_animation* entries, uint32_t n_entries);
int cgpt_clip_get_range(cgpt_ctx* ctx, uint32_t clip, float* begin, float* end);

/* UpdateScreenPlane (ref: Main.cpp:98-102,143-149): fov in degrees, plane at distance fov-in-radians (SURVEY A-13) */
int cgpt_camera_from_view(const float pos[3], const float view_dir[3], float fov_deg, float aspect, cgpt_camera* out);

/* replaces Render() x n_samples (ref: Main.cpp:691-755): accumulates into the context's float4 accumulator */
int cgpt_render(cgpt_ctx* ctx, const cgpt_camera* camera, const cgpt_settings* settings, const cgpt_render_params* params);
/* replaces ResetAccumulator (ref: Main.cpp:238-243) */
int cgpt_reset_accumulator(cgpt_ctx* ctx);
/* replaces reads of data.accumulator (ref: Main.cpp:204,740): (row_end-row_begin)*width*4 floats of the last render's band */
int cgpt_read_accumulator(cgpt_ctx* ctx, float* dst, size_t n_floats);
/* replaces data.pixels -> DX12::CopyToBackBuffer (ref: Main.cpp:203,741,935; packing MathLib.h:144-152) */
int cgpt_read_pixels(cgpt_ctx* ctx, uint32_t* dst, size_t n_pixels);
/* restores what cgpt_read_accumulator saved (checkpoint / resume of a long render): data.accumulator + data.num_accumulated
 * (ref: Main.cpp:204-205, the state ResetAccumulator :238-243 clears).  `band` names the framebuffer the floats belong to
 * (width, height, row_begin/row_end, interleave_*; its sample / seed / kernel fields are ignored), so it works on a fresh
 * context; src holds rows*width*4 floats in the band's own row order.  data.pixels is re-packed from the loaded sums.
 * Continue with cgpt_render(first_sample = num_accumulated): the result is bit-identical to an uninterrupted render. */
int cgpt_write_accumulator(cgpt_ctx* ctx, const cgpt_render_params* band, const float* src, size_t n_floats, uint32_t num_accumulated);
/* device pointers of the band just rendered (one-device context: for a gather by the host, e.g. torch.distributed in bench.py) or
 * of the gathered full frame on device_ids[0] (multi-device context) */
int cgpt_accumulator_device_ptr(cgpt_ctx* ctx, void** ptr, size_t* n_bytes);
int cgpt_pixels_device_ptr(cgpt_ctx* ctx, void** ptr, size_t* n_bytes);

/* replaces data.stats / total_energy_received (ref: Main.cpp:207,218-226,847-848) */
int cgpt_get_stats(cgpt_ctx* ctx, cgpt_stats* out);
int cgpt_reset_stats(cgpt_ctx* ctx);
/* One more counter of the same kind, with an accessor of its own because cgpt_stats keeps the size it has at ABI version 2: the
 * IntersectScene calls on a ray traced again after total internal reflection (SURVEY A-3) that the render kernels answered with the
 * ray's known hit instead of a walk.  Each is counted in traced_rays too; 0 with CGPT_RENDER_COUNTERS.  Since the last
 * cgpt_reset_stats; a multi-device context returns the sum over its devices.  An added export changes no existing symbol or layout, so
 * CGPT_ABI_VERSION stays 2, as it did for cgpt_set_nee_candidates; the Python binding resolves every declared symbol when it loads the
 * library, so an older library is refused there. */
int cgpt_get_retrace_unwalked(cgpt_ctx* ctx, uint64_t* out);

/* IntersectScene for a batch of host rays (ref: Main.cpp:299-316): the extend kernel on its own.
 * origins/dirs: n*3 floats; tmax: n floats or NULL (1e34f, ref: Primitives.h:75); outputs n entries each:
 * t, obj_idx (~0u on miss), tri_idx, bvh_depth (ref: Primitives.h:77-82) */
int cgpt_intersect_rays(cgpt_ctx* ctx, const float* origins, const float* dirs, const float* tmax, uint32_t n,
                        float* out_t, uint32_t* out_obj, uint32_t* out_tri, uint32_t* out_depth);

/* One bounce of TracePathAdvanced (ref: Main.cpp:404-573) for a batch of host samples: the shade step on its own, the counterpart of
 * cgpt_intersect_rays.  Sample i is a traced ray -- world o, d and its hit record t, obj (~0u: a miss), tri, bvh_depth -- and the
 * path's state before the bounce.  The kernel runs the render kernels' own bounce function once per sample, in the instantiation a
 * render of this context would run: the context's lobe level (roughness, transmission roughness, smooth normals, transforms) and the
 * resampled NEE when cgpt_set_nee_candidates is above 1 and settings enables NEE.  settings->render_mode selects nothing -- the bounce is
 * TracePathAdvanced's -- but a value cgpt_render refuses is refused here too.  Out: the bounce's return word (bit 0 the path ends, bit 1 a shadow ray is pending, bit 2 energy was added,
 * bits 4-5 the specular-chain choice), the next ray, the state after the bounce, the bounce's own energy (from 0), the shadow ray
 * and its pending contribution (zeros while bit 1 is clear) and the number of re-traces after total internal reflection that ran in
 * place.  No ray is traced and no random number is drawn on the host.
 * Refusals, all before any device work (a refused call changes nothing): no scene CGPT_ERR_NO_SCENE; a NULL argument, n == 0 or
 * n > 65536, obj neither ~0u nor an object index, a mesh hit whose tri is not below the mesh's triangle count (a triangle object
 * ignores tri), a hit whose t, o, d or throughput is not finite, depth > 255, or settings cgpt_render refuses: CGPT_ERR_INVALID.
 * A multi-device context runs it on its first device.  Reads the scene; the accumulator, cgpt_stats and the guides stay as they are.
 * An added export: CGPT_ABI_VERSION stays 2. */
typedef struct cgpt_shade_sample {
    float o[3], d[3], t;
    uint32_t obj, tri, bvh_depth;
    float throughput[3];
    uint32_t rng, depth, is_specular;   /* rng: the raw PCG state */
} cgpt_shade_sample;
typedef struct cgpt_shade_result {
    uint32_t flags;
    float o[3], d[3], throughput[3], energy[3];
    uint32_t rng, depth, is_specular;
    float shadow_o[3], shadow_d[3], shadow_tmax, pending[3];
    uint32_t unwalked, reserved;        /* reserved: 0 */
} cgpt_shade_result;
int cgpt_shade_samples(cgpt_ctx* ctx, const cgpt_settings* settings, const cgpt_shade_sample* samples, uint32_t n, cgpt_shade_result* results);

/* The trace step of the wavefront pipeline (CGPT_KERNEL_WAVEFRONT) on rays the host supplies: the production traversal on its own, as
 * cgpt_intersect_rays is the megakernel's.  No kernel of its own runs: each call makes the trace launch a render of this context makes --
 * the same instantiation (transforms, cgpt_set_top_level, counters), the same persistent grid, LDS layout and cgpt_set_tuning knobs
 * (refill, inner_repeat, leaf_repeat, obj_repeat, obj_shift, top_records, trace_blocks, shadow_any_hit, lds_tris, retire_misses,
 * first_lean) -- on ray slots and lists of its own, filled as the pipeline's other kernels leave them.
 * cgpt_trace_rays is the launch of a later bounce round: n_extend extend rays (closest hit) and n_shadow shadow rays (occlusion) in one
 * launch.  origins / dirs: 3 floats per ray; tmax: one float per ray or NULL (1e34f).  Per extend ray t, obj (~0u on a miss), tri and
 * bvh_depth as cgpt_intersect_rays returns them, with two differences.  While the retire_misses knob is 1 (the default; the probe takes the
 * knob alone, a render also turns it off for the debug views) the kernel stores no record for a ray that misses, and such a ray's
 * bvh_depth is returned as 0.  And tri means something for a hit on a mesh only: on a ray that met a stand-alone triangle object on its
 * way, a final hit on anything but a mesh may carry another stale tri than cgpt_intersect_rays's.
 * Per shadow ray one byte: 1 occluded (something was hit below tmax), 0 not.  flags: CGPT_TRACE_COUNTERS runs the counting instantiation,
 * as CGPT_RENDER_COUNTERS does for a render (shadow rays then walk to the end); CGPT_TRACE_REVERSED lays the rays out in their slots and
 * lists back to front (entry i of a list names slot n - 1 - i); the results come back in the caller's order either way.
 * cgpt_trace_first_hits is the launch of round 0: the primary ray of every pixel of rows [row_begin, row_end) of a width x height frame
 * seen from `camera`, in the lean per-lane walk or the voted one as the first_lean knob says.  Out, per pixel of the band in row-major
 * order: obj (~0u on a miss), tri, bvh_depth and t (1e34f on a miss).  flags: CGPT_TRACE_COUNTERS only.
 * Both add the rays they trace to traced_rays (one per ray and per pixel) and, with CGPT_TRACE_COUNTERS, their steps to inner_steps,
 * tri_tests and bvh_depth_sum; nothing else changes: the accumulator, data.pixels, num_accumulated, the guides, the temporal history,
 * the other fields of cgpt_stats and the memory a render holds stay as they are.
 * Refusals, all before any device work (a refused call changes nothing): no scene CGPT_ERR_NO_SCENE; a NULL argument that a count above 0
 * needs, unknown flag bits, more than 4194304 rays of a kind or padded pixels (the band in whole 8 x 8 tiles), width or height 0 or rows
 * outside the frame: CGPT_ERR_INVALID; a multi-device context: CGPT_ERR_UNSUPPORTED.  No ray at all is CGPT_OK and launches nothing.
 * Every direction must be finite and not zero.  Added exports: CGPT_ABI_VERSION stays 2. */
enum cgpt_trace_flags { CGPT_TRACE_COUNTERS = 1u, CGPT_TRACE_REVERSED = 2u };
int cgpt_trace_rays(cgpt_ctx* ctx, const float* ext_origins, const float* ext_dirs, const float* ext_tmax, uint32_t n_extend,
                    const float* sh_origins, const float* sh_dirs, const float* sh_tmax, uint32_t n_shadow, uint32_t flags,
                    float* out_t, uint32_t* out_obj, uint32_t* out_tri, uint32_t* out_depth, uint8_t* out_occluded);
int cgpt_trace_first_hits(cgpt_ctx* ctx, const cgpt_camera* camera, uint32_t width, uint32_t height, uint32_t row_begin, uint32_t row_end,
                          uint32_t flags, uint32_t* out_obj, uint32_t* out_tri, uint32_t* out_depth, float* out_t);

/* BVH::Build with BVHBuildOption_SAHSplitIntervals on the GPU (ref: Source/BVH.cpp:11-45,204-259,299-366; Main.cpp:789,802 use
 * this option for every mesh).  The result is the reference's tree bit for bit: same 32-byte nodes in the same allocation order,
 * same m_tri_indices permutation, same m_max_depth / m_total_area -- so it can be passed to cgpt_scene_upload (cgpt_object
 * node_offset/node_count/max_depth/total_area + cgpt_scene_desc tri_indices) in place of the host build.
 * triangles: n_tris host triangles; nodes_out: room for 2*n_tris-1 nodes; tri_indices_out: n_tris entries. */
int cgpt_bvh_build(cgpt_ctx* ctx, const cgpt_triangle* triangles, uint32_t n_tris, cgpt_bvh_node* nodes_out, uint32_t* n_nodes_out,
                   uint32_t* tri_indices_out, uint32_t* max_depth_out, float* total_area_out);
/* The same for any BuildOption (ref: Include/BVH.h:7-13; Source/BVH.cpp:208-224 naive split, :225-259 SAH split intervals, :260-297
 * SAH split primitives, which never splits: SURVEY A-5) and for BVH::Rebuild (ref: BVH.cpp:47-59, the "Rebuild BVH" button :182-185):
 * initial_tri_indices = NULL starts from the identity order as Build does (:25-29); otherwise it is the tree's CURRENT m_tri_indices
 * (a permutation of 0..n_tris-1), which Rebuild does not reset -- the swap partition is order-sensitive, so the result differs from a
 * fresh Build and equals the reference's Rebuild. */
/* CGPT_BUILD_SAH_BINNED is not one of the reference's options (its README, "Planned: Binned BVH build"); the host mirror
 * (csrc/host/mesh_bvh.cpp, BuildTreeBinned) is its specification and the device build equals it word for word.  Per node of n triangles,
 * with each triangle's box and centroid ((p0 + p1 + p2) * 0.3333f) as in the other options:
 *   - cmin, cmax: the bounds of the node's centroids.  Per axis a with cmax[a] > cmin[a]: scale = 16.0f / (cmax[a] - cmin[a]) and a
 *     triangle's bin is min(15, (uint32_t)((c[a] - cmin[a]) * scale)) (a product that is not below 16, an overflowed scale included, is
 *     bin 15).  Each of the 16 bins keeps a count, the union of its triangles' boxes and the bounds of their centroids;
 *   - every min / max is taken under the total order on floats in which -0 < +0, so no bound depends on the order of the fold;
 *   - candidates: axis outer, split s = 1..15 inner; left = bins [0, s), right = bins [s, 16); a candidate with an empty side is skipped;
 *     cost = (float)lc * half_area(left) + (float)rc * half_area(right); the first strictly cheaper candidate wins;
 *   - the node is a leaf if there is no candidate or !(best < half_area(node) * (float)n) (the reference's criterion, BVH.cpp:253);
 *   - the partition is stable (left iff the bin on the chosen axis is < s); the children's bounds are the unions of the bins of each side;
 *   - node numbering, left_first / prim_count, max_depth and total_area as for the other options; initial_tri_indices as for Rebuild.
 * Input domain of this option only: every position finite with |x| <= 1e30, otherwise CGPT_ERR_INVALID and nothing is built (the bin
 * index must stay defined).  The three reference options keep their behaviour on such inputs. */
enum cgpt_bvh_build_option { CGPT_BUILD_NAIVE_SPLIT = 0, CGPT_BUILD_SAH_SPLIT_INTERVALS = 1, CGPT_BUILD_SAH_SPLIT_PRIMITIVES = 2, CGPT_BUILD_SAH_BINNED = 3 };
int cgpt_bvh_build_ex(cgpt_ctx* ctx, const cgpt_triangle* triangles, uint32_t n_tris, uint32_t build_option, const uint32_t* initial_tri_indices,
                      cgpt_bvh_node* nodes_out, uint32_t* n_nodes_out, uint32_t* tri_indices_out, uint32_t* max_depth_out, float* total_area_out);

int cgpt_synchronize(cgpt_ctx* ctx);

/* ---- denoising (reference README, "Planned"): an edge-avoiding a-trous filter guided by first-hit buffers ----
 * The reference does not jitter primary rays (every sample of a pixel has the same first hit), so the guides -- position, normal and
 * albedo of each pixel's primary hit, computed by the render paths' own device functions -- take one primary trace per camera; the
 * context keeps them until the camera, the band or the scene (upload, material update, refit, primitive update) changes.
 * `camera` is the one the accumulator was rendered with (so the calls also work after cgpt_write_accumulator on a fresh context).
 * Both calls run on the context's stream and block; they leave the accumulator, data.pixels, num_accumulated and cgpt_stats alone.
 * Bands: a one-device context works on its contiguous band (the filter sees only its rows; an interleaved band is CGPT_ERR_INVALID);
 * a multi-device context works on the full frame on device_ids[0], after the gather cgpt_read_accumulator does.
 * Refusals (checked before any device work; a refused call changes nothing): no scene CGPT_ERR_NO_SCENE; no band yet, the last render
 * a debug view, num_accumulated == 0 (denoise only), iterations > 10, a sigma not finite and > 0, unknown flag bits, wrong sizes or
 * both outputs NULL: CGPT_ERR_INVALID. */
enum cgpt_denoise_flags { CGPT_DENOISE_DEMODULATE_ALBEDO = 1u };   /* filter radiance / albedo, multiply the albedo back afterwards */
typedef struct cgpt_denoise_params {
    uint32_t iterations;   /* 0..10 passes of step 1, 2, 4, ...; 0 returns accumulator / num_accumulated unchanged */
    uint32_t flags;        /* cgpt_denoise_flags */
    float sigma_color, sigma_normal, sigma_position;
} cgpt_denoise_params;
/* NULL params = the defaults: iterations 5, CGPT_DENOISE_DEMODULATE_ALBEDO, sigma_color 4.0, sigma_normal 0.2, sigma_position 0.3
 * (tuned on the reference layout at 4 spp) */
/* 12 floats per pixel of the band, row-major: {x.xyz, t | n.xyz, bits(obj) | albedo.xyz, bits(mat_index)} of the primary hit;
 * a miss is x = n = albedo = 0, t = 1e34, obj = mat_index = 0xFFFFFFFF */
int cgpt_read_guides(cgpt_ctx* ctx, const cgpt_camera* camera, float* dst, size_t n_floats);
/* the filtered radiance of the band as float4 {rgb, 1} (dst_rgba, 4 floats per pixel) and/or packed as data.pixels is (dst_pixels);
 * either output may be NULL, not both */
int cgpt_denoise(cgpt_ctx* ctx, const cgpt_camera* camera, const cgpt_denoise_params* params, float* dst_rgba, size_t n_floats,
                 uint32_t* dst_pixels, size_t n_pixels);

/* ---- temporal reprojection for a moving camera (the temporal stage of SVGF, Schied et al. 2017) ----
 * cgpt_denoise_temporal is cgpt_denoise with a temporal stage in front of the passes: the history of the earlier calls -- a merged
 * colour and a history length H (in samples) per pixel, with the guides and the camera of the frame it was stored for -- is reprojected
 * onto `camera` through the current first hits, validated, and merged with the current frame weighted by sample counts,
 *   c = (He c_h + N c_0) / (He + N),  He = min(H, max_history),  H' = min(He + N, max_history),  N = num_accumulated,
 * where c_0 is the accumulator / N (divided by the albedo with CGPT_DENOISE_DEMODULATE_ALBEDO).  The passes then filter c;
 * iterations = 0 returns c (times the albedo) packed as data.pixels is.  (c, H') becomes the new history.
 * Intended use per frame: cgpt_reset_accumulator, cgpt_render(n samples), cgpt_denoise_temporal(the camera of that render).  Each
 * call consumes the accumulator's N samples once: a second call without a new render counts the same samples twice.
 * Reprojection: a hit at x maps to (a, b, c) = Minv (x - pos_prev), Minv the inverse of [top_left - pos | top_right - top_left |
 * bottom_left - top_left] of the history's camera; a <= 0 (behind it) or a singular camera: no history; the history is sampled
 * bilinearly at (b / a width, c / a height - first_row); a tap counts when it lies in the band, hit the same object,
 * n_prev . n >= normal_cos_min and |n . (x_prev - x)| <= plane_tolerance t; valid weights summing to <= 0.01: no history.  A camera
 * whose bytes equal the history's maps every pixel to itself without validation.  A first hit on a material with specular > 0 or
 * refractivity > 0 shows a reflection or refraction that does not move with the surface: after a camera change it takes no history
 * unless CGPT_TEMPORAL_KEEP_VIEW_DEPENDENT is set.  A pixel without history: c = c_0, H' = min(N, max_history).
 * The history is absent after cgpt_ctx_create, cgpt_temporal_reset and a call that failed, and when the band (width, height, rows), the
 * scene (every upload and in-place edit that recomputes the guides) or the demodulate flag differ from the call's.
 * Moving objects (CGPT_TEMPORAL_FOLLOW_TRANSFORMS): without the flag every scene edit drops the history.  With it a
 * history stored before one or more cgpt_scene_update_transforms calls stays usable as long as nothing else changed the scene (an
 * upload, a material, smooth-normal, refit or primitive edit still drops it; the roughness setters keep it, as they do without the
 * flag).  A pixel whose first hit lies on an object whose 12 matrix floats differ bytewise from those in force when the history was
 * stored is carried back before the map above is applied: x' = D x with D = M_prev M_cur^-1 (a 3x4 affine) and n' = normalize(N n) with
 * N = A_prev^-T A_cur^T, both matrices formed in double from the float entries and rounded to float once per entry, x' and n' evaluated
 * in double and rounded to float once; the map, the four taps, the validity tests, the 0.01 floor and the merge then run on x', n', the
 * unchanged t and object index.  A pixel on an unmoved object takes x and n untouched.  A call in which no object moved is the call
 * without the flag bit for bit; one in which an object moved reprojects (and applies the view-dependent rule) even when the camera
 * bytes equal the history's.  An object whose D or N has an entry that is not finite takes no history.  The stored history holds the
 * current frame's own guides.  Limits: only mesh and stand-alone triangle objects can move (spheres, planes and lights take the
 * identity only, and a sphere moved by cgpt_scene_update_primitive drops the history); a refit, also through an instanced placement,
 * drops it; the light carried by the history is the old frames', so a moving object's shadow and the shading of a turning surface lag
 * by up to max_history samples.
 * Skinned poses (CGPT_TEMPORAL_FOLLOW_POSES): with this flag a history stored before one or more cgpt_scene_skin_mesh calls
 * stays usable as long as nothing but poses changed the scene (and transforms, when CGPT_TEMPORAL_FOLLOW_TRANSFORMS is set as well; each
 * flag alone keeps the history across its own kind of edit only).  Per skinned object the context remembers the joint matrices of the last
 * pose, or that no pose is known (before the first pose of a skin, after a cgpt_scene_refit_mesh of the object or of a placement sharing
 * its copy); the history remembers the same.  An object whose copy no pose has written since the history was stored, or whose matrices
 * equal the history's bytewise (A -> B -> A), is unposed; one whose matrices differ is re-posed; one where either side knows no pose, or
 * the skin was installed anew, takes no history.  After cgpt_scene_upload_instanced every placement of the posed copy follows.  A pixel
 * whose first hit lies on triangle tri of a re-posed object is carried back before anything else, in double on the float inputs:
 *   P = x, or Ainv x + binv with the float inverse the scene holds for an object with a transform;
 *   e1 = p1 - p0, e2 = p2 - p0, w = P - p0, g = e1 x e2, u = ((w x e2) . g) / (g . g), v = ((e1 x w) . g) / (g . g), with p0, p1, p2 the
 *   current pose's corners; not clamped; g . g zero or not finite: no history;
 *   q_c, m_c = the corners and normals cgpt_scene_skin_mesh's float arithmetic gives bind[tri], joints[tri], weights[tri] under the
 *   history's matrices: bit for bit the triangle the history's pose wrote;
 *   x' = (q0 + u (q1 - q0)) + v (q2 - q0);  n' = m0, or for an object with the smooth flag ((1 - u - v) m0 + u m1) + v m2 over its
 *   length (m0 where the squared length is not > 1e-12);
 *   x_p = A x' + b and n_p = normalize(Ainv^T n') through the object's current transform (x', n' themselves for an object without one),
 *   each rounded to float once; anything not finite: no history.
 * The reprojection then runs on x_p, n_p, the unchanged t and object index; with both flags an object that was re-posed and moved goes
 * through its pose and then through D, two roundings to float.  A call in which no object was re-posed is the call without the flag bit for
 * bit; one in which an object was reprojects (and applies the view-dependent rule) even when the camera bytes equal the history's.
 * Morph targets (CGPT_TEMPORAL_FOLLOW_MORPHS): with this flag a history stored before one or more accepted
 * cgpt_scene_morph_mesh calls stays usable as long as nothing but morphs changed the scene (and poses or transforms, when their flags are
 * set as well: each flag keeps the history across its own kind of edit only, so a character with a skeleton and blend shapes needs
 * CGPT_TEMPORAL_FOLLOW_POSES | CGPT_TEMPORAL_FOLLOW_MORPHS).  For an object with morph targets the context remembers the pose its copy
 * shows as the targets' installation, the weights of the last accepted pose and -- if a skin took part in it -- that skin's installation
 * and matrices; or that no pose is known (from cgpt_scene_set_morph_targets until the first accepted pose through either call, after a
 * cgpt_scene_refit_mesh of the object or of a placement sharing its copy, after a pose of the copy through another placement).  The
 * history remembers the same.  An object whose copy was not posed since the history, or whose key is bytewise equal (A -> B -> A), is
 * treated as without the flag; the same installations and counts with other weights or matrices: the hit is carried back as above,
 * with step 3 = the base triangle morphed by the history's weights (morph.h's float arithmetic: MorphAccumulate over its nonzero
 * weights in ascending order, then MorphNormalise) and then, if the history's pose had a skin part, skinned by the history's matrices
 * -- the bits that pose wrote; anything else (no pose known on either side, targets or skin installed anew, a skin part that came or
 * went, targets cleared): no history on that object's pixels.  Such an object reaches the first two states only in a call with this
 * flag; objects without targets follow the rules above.  Every placement of an instanced copy takes the state of the copy.  Both
 * layouts of the knob "morph_leaf_order" are followed.  Limits, beyond those below: recomputing the history's pose costs 72 bytes of
 * gathers per history-active target and re-posed pixel; a cgpt_scene_refit_mesh is not followed; morphed lights do not exist.
 * cgpt_read_previous_hits returns the records of the last successful call that carried a pose back, 8 floats per pixel of its band:
 * {x_p.xyz, bits(state), n_p.xyz, 0}, state 0 (a miss, an object that was not re-posed: the pixel's own x, n), 1 (re-posed) or 2 (no
 * history: its own x, n) -- with the guides, what a caller needs for motion vectors.  Limits: the light carried by the history lags, as
 * for a moved object; the tree a posed mesh is traced through is the bind pose's, refitted; the side fallback of smooth normals (the
 * geometric normal where the ray sees the interpolated one from behind) is not replayed for n', which only feeds the two validity tests;
 * the pixels a pose uncovers start again; skinned lights do not exist.
 * Limits: without the flag camera motion only (an edit drops the history); first-hit reprojection only (what is seen
 * in a mirror or through glass is not followed); a multi-device context keeps the history on device_ids[0].
 * Like cgpt_denoise it leaves the accumulator, data.pixels, num_accumulated, cgpt_stats and the guides alone, and cgpt_denoise's output
 * does not depend on temporal calls.  Refusals (before any device work; nothing changes, the history included): every refusal of
 * cgpt_denoise; max_history not finite or < 1; normal_cos_min outside [-1, 1] or NaN; plane_tolerance not finite or <= 0; unknown
 * flag bits; cgpt_read_temporal_history without a history or with a wrong size -- all CGPT_ERR_INVALID. */
enum cgpt_temporal_flags { CGPT_TEMPORAL_KEEP_VIEW_DEPENDENT = 1u, CGPT_TEMPORAL_FOLLOW_TRANSFORMS = 4u, CGPT_TEMPORAL_FOLLOW_POSES = 16u, CGPT_TEMPORAL_FOLLOW_MORPHS = 32u };   /* 2u, 8u and everything above 32u are no flags: they stay refused as unknown bits, as before */
typedef struct cgpt_temporal_params {
    float    max_history;      /* cap on a pixel's history length, in samples; finite, >= 1 */
    float    normal_cos_min;   /* a tap is valid only if n_prev . n_cur >= this; in [-1, 1] */
    float    plane_tolerance;  /* ... and |n_cur . (x_prev - x_cur)| <= this * t_cur; finite, > 0 */
    uint32_t flags;            /* cgpt_temporal_flags */
} cgpt_temporal_params;        /* NULL = the defaults: 64, 0.9, 0.01, 0 */
int cgpt_denoise_temporal(cgpt_ctx* ctx, const cgpt_camera* camera, const cgpt_denoise_params* params, const cgpt_temporal_params* temporal,
                          float* dst_rgba, size_t n_floats, uint32_t* dst_pixels, size_t n_pixels);
/* drops the history; CGPT_OK when there is none */
int cgpt_temporal_reset(cgpt_ctx* ctx);
/* 4 floats per pixel of the band the history was stored for: the merged colour c (the filter's input domain: demodulated when the call
 * was) and the history length H' */
int cgpt_read_temporal_history(cgpt_ctx* ctx, float* dst, size_t n_floats);
/* 8 floats per pixel of the band of the last successful temporal call with CGPT_TEMPORAL_FOLLOW_POSES or CGPT_TEMPORAL_FOLLOW_MORPHS in
 * which an object was re-posed:
 * {x_p.xyz, bits(state), n_p.xyz, 0} (above).  CGPT_ERR_INVALID when no such call has happened, or for a wrong size. */
int cgpt_read_previous_hits(cgpt_ctx* ctx, float* dst, size_t n_floats);

/* ---- variance-guided edge stopping (the third part of SVGF, Schied et al. 2017) ----
 * cgpt_denoise_variance_guided is cgpt_denoise with the colour edge-stop measured in standard deviations of each pixel instead of
 * by the constant sigma_color: pass i weighs a tap by
 *   h(dx) h(dy) exp(-|l(c_q) - l(c_p)| / (sigma_luminance sqrt(gbar(p)) + 1e-6)) times cgpt_denoise's geometry term,
 * l(c) = 0.2126 r + 0.7152 g + 0.0722 b in the filter's input domain, gbar(p) the 3x3 Gaussian (1 2 1; 2 4 2; 1 2 1) / 16 of the
 * variance over p's immediate neighbours.  The variance travels with the colour, var' = sum w^2 var_q / (sum w)^2, so later passes
 * tighten by themselves: sigma_luminance is the same in every pass.  `params` means what it means for cgpt_denoise: iterations, the
 * demodulate flag, sigma_normal and sigma_position apply; sigma_color is validated and not used.
 * The variance pass 0 reads is estimated per pixel.  Spatially: the variance of l over a 7x7 window of the image the passes read, each
 * tap weighted by the geometry term (two misses: 1; a hit and a miss never mix), var_s = max(0, sum w d^2 / sum w - (sum w d / sum w)^2)
 * with d = l(c_q) - l(c_p).  With CGPT_VARIANCE_TEMPORAL the call runs cgpt_denoise_temporal's stage in front -- the colour merge and
 * the stored history are that call's bit for bit, either call may continue the other's colour history, `temporal` NULL means its
 * defaults -- and keeps luminance moments {mu, v, K} (mean, population variance, samples covered) beside the colour history,
 * reprojected with the colour's taps, validity tests and weights and merged by the pooled-variance update
 *   mu' = (Ke mu_h + N l0) / (Ke + N),  v' = (Ke (v_h + (mu_h - mu')^2) + N (l0 - mu')^2) / (Ke + N),  K' = min(Ke + N, max_history),
 * Ke = min(K_h, max_history), l0 = l(c_0); without moments mu' = l0, v' = 0, K' = N.  A pixel with Ke + N >= min_history_frames N
 * takes var_t = v' N / (Ke + N), every other pixel var_s.  The moments are absent wherever and whenever the colour history is, and
 * after a cgpt_denoise_temporal call (which updates the colour without them).  Without the flag no history is read or written.
 * CGPT_TEMPORAL_FOLLOW_TRANSFORMS in `temporal` means what it means for cgpt_denoise_temporal: the moments ride on the taps and weights
 * of the carried-back hits.
 * iterations = 0 returns the unfiltered image (cgpt_denoise's, or with the flag cgpt_denoise_temporal's) and still estimates the variance.
 * Bands, multi-device contexts, stream and blocking are cgpt_denoise's.  The call leaves the accumulator, data.pixels, num_accumulated,
 * cgpt_stats and the guides alone, and the outputs of cgpt_denoise and cgpt_denoise_temporal do not depend on it.
 * Refusals (before any device work; nothing changes, the histories and the variance map included): every refusal of cgpt_denoise;
 * with the flag every refusal of cgpt_denoise_temporal's parameters; sigma_luminance not finite or <= 0, min_history_frames == 0,
 * unknown flag bits; cgpt_read_variance without an earlier successful call for the current band or with a wrong size -- all
 * CGPT_ERR_INVALID.  Added exports: CGPT_ABI_VERSION stays 2. */
enum cgpt_variance_flags { CGPT_VARIANCE_TEMPORAL = 1u };   /* run cgpt_denoise_temporal's stage in front, and keep luminance moments with its history */
typedef struct cgpt_variance_params {
    float    sigma_luminance;      /* the luminance edge-stop, in standard deviations; finite, > 0 */
    uint32_t min_history_frames;   /* temporal variance is used from this many frames' worth of samples on; >= 1 */
    uint32_t flags;                /* cgpt_variance_flags */
} cgpt_variance_params;            /* NULL = the defaults: 4.0, 4, 0 */
int cgpt_denoise_variance_guided(cgpt_ctx* ctx, const cgpt_camera* camera, const cgpt_denoise_params* params,
                                 const cgpt_temporal_params* temporal, const cgpt_variance_params* variance,
                                 float* dst_rgba, size_t n_floats, uint32_t* dst_pixels, size_t n_pixels);
/* one float per pixel of the band: the variance pass 0 of the last successful cgpt_denoise_variance_guided read (its input, before any
 * pass) */
int cgpt_read_variance(cgpt_ctx* ctx, float* dst, size_t n_floats);

/* ---- the display stage (no reference counterpart) ---------------------------------------------------- */
/* Linear radiance to a displayable image on the device: auto exposure from a luminance histogram, a tone curve, the sRGB transfer
 * function, and the pixel packed as data.pixels is.  csrc/host/tonemap.h states the arithmetic once for the kernels and the host mirror
 * (cgpth_tonemap), tests/tonemap_ref.py the same in numpy; all of it but the sRGB curve's powf is bit-identical across the three.
 *   source   ACCUMULATOR: the band of the last render divided by num_accumulated as cgpt_read_pixels divides it (any band, an interleaved
 *            one included; a multi-device context's gathered frame, on device_ids[0]).  DENOISED: the float4 result of the context's last
 *            successful cgpt_denoise / cgpt_denoise_temporal / cgpt_denoise_variance_guided call, still on the device; every such call drops
 *            it when it starts and sets it when it succeeds; cgpt_render, cgpt_reset_accumulator, cgpt_write_accumulator and a framebuffer
 *            reallocation drop it.  HOST: src_rgba, src_width x src_height float4 pixels, uploaded; needs no scene.
 *   exposure manual: exposure_scale 2^ev_bias.  CGPT_TONEMAP_AUTO_EXPOSURE: the luminance Y = (0.2126 r + 0.7152 g) + 0.0722 b of every
 *            source pixel is counted in 256 bins over [2^-16, 2^16), eight an octave (a Y that is <= 0, NaN or +inf is not counted but
 *            tallied in n_ignored); the lowest low_fraction and the highest high_fraction of the counted pixels are dropped; the mean bin
 *            index m of the rest (in eighths of an octave) is the frame's reading; the context's adapted index moves towards it,
 *            m_adapted += (m - m_adapted) alpha (the first reading sets it; a frame without a reading keeps it); the luminance L at
 *            m_adapted is brought to `key`: exposure = key / L  exposure_scale 2^ev_bias.  With no reading ever the metered factor is 1.
 *            m_adapted is context state like cgpt_set_nee_candidates: uploads and edits keep it, cgpt_exposure_reset forgets it.
 *   curve    per channel on x = max(c exposure, 0), a NaN as 0.  CLAMP: x (the reference's Vec4ToUint clamps when it packs).  REINHARD:
 *            x (1 + x / white^2) / (1 + x).  ACES: Narkowicz's fit.  HABLE: Hable's filmic curve over its value at `white`.
 *   transfer LINEAR: nothing.  SRGB: the sRGB encoding of min(y, 1).
 * dst_rgba receives {r, g, b, 1} per pixel, dst_pixels Vec4ToUint of the same; either may be NULL, not both; n_floats = 4 n and
 * n_pixels = n for the source's n pixels.  NULL params: the accumulator, ACES, SRGB, auto exposure, key 0.18, fractions 0.5 / 0.02,
 * alpha 1, white 4, exposure_scale 1, ev_bias 0.
 * The call blocks, runs on the context's stream (cgpt_set_stream), writes buffers of its own and leaves the accumulator, data.pixels,
 * num_accumulated, the denoiser's outputs, guides and history and cgpt_stats as they are.
 * Refused with nothing changed, m_adapted and the last reading included (CGPT_ERR_INVALID unless noted): an unknown enum value or flag
 * bit; exposure_scale or white not finite and > 0; |ev_bias| > 64; with AUTO_EXPOSURE a key not finite and > 0, a fraction outside
 * [0, 1), low + high >= 1, alpha outside [0, 1] or NaN; HOST without an image or with a zero size; both outputs NULL or a wrong size;
 * ACCUMULATOR / DENOISED without a scene (CGPT_ERR_NO_SCENE), before a render, with num_accumulated == 0 or after a debug view; DENOISED
 * without a valid result.  Added exports: CGPT_ABI_VERSION stays 2. */
enum cgpt_tonemap_source   { CGPT_TONEMAP_ACCUMULATOR = 0, CGPT_TONEMAP_DENOISED = 1, CGPT_TONEMAP_HOST = 2 };
enum cgpt_tonemap_curve    { CGPT_CURVE_CLAMP = 0, CGPT_CURVE_REINHARD = 1, CGPT_CURVE_ACES = 2, CGPT_CURVE_HABLE = 3 };
enum cgpt_tonemap_transfer { CGPT_TRANSFER_LINEAR = 0, CGPT_TRANSFER_SRGB = 1 };
enum cgpt_tonemap_flags    { CGPT_TONEMAP_AUTO_EXPOSURE = 1u };
typedef struct cgpt_tonemap_params {
    uint32_t source, curve, transfer, flags;
    float exposure_scale; int32_t ev_bias; float white;
    float key, low_fraction, high_fraction, alpha;           /* read with AUTO_EXPOSURE only */
    const float* src_rgba; uint32_t src_width, src_height;   /* CGPT_TONEMAP_HOST only */
} cgpt_tonemap_params;
int cgpt_tonemap(cgpt_ctx* ctx, const cgpt_tonemap_params* params, float* dst_rgba, size_t n_floats, uint32_t* dst_pixels, size_t n_pixels);
/* The reading of the last successful auto-exposure call.  valid: bit 0 (CGPT_EXPOSURE_ADAPTED) adapted_index holds a reading, this
 * frame's or an earlier one's; bit 1 (CGPT_EXPOSURE_METERED) this frame gave one (mean_index; 0 otherwise).  n_counted is N before the
 * trimming; histogram the 256 counts.  CGPT_ERR_INVALID before any auto-exposure call of the context. */
enum cgpt_exposure_valid { CGPT_EXPOSURE_ADAPTED = 1u, CGPT_EXPOSURE_METERED = 2u };
typedef struct cgpt_exposure_info { double mean_index, adapted_index; float exposure; uint32_t valid;
                                    uint64_t n_counted, n_ignored; uint32_t histogram[256]; } cgpt_exposure_info;
int cgpt_read_exposure(cgpt_ctx* ctx, cgpt_exposure_info* out);
/* forgets m_adapted: the next reading sets it.  The last reading (cgpt_read_exposure) stays */
int cgpt_exposure_reset(cgpt_ctx* ctx);

/* ---- tuning and measurement aids (no reference counterpart) ------------------------------------------------------- */
/* Overrides one tuning knob of the wavefront pipeline for this context (the CGPT_WF_* environment variables set the same
 * knobs process-wide; names are the variable names without the prefix, lower case: "pools", "batch", "max_batch",
 * "refill", "inner_repeat", ...; DESIGN.md 5.1 lists them).  Results never depend on a knob, only speed does.
 * "skin_joints_lds" (0 | 1, default 1) is cgpt_scene_skin_mesh's: whether its kernel stages the joint matrices in LDS or reads them
 * through the vector cache.  "morph_leaf_order" (0 | 1, default 1), read by cgpt_scene_set_morph_targets: whether
 * the targets are stored in the order of the object's leaf slots as component planes, or as given; "morph_max_blocks" (1..1024,
 * default 1024): the cap of the morph kernel's grid.  cgpt_scene_pose_objects reads "skin_joints_lds" the same way
 * and applies "morph_max_blocks" to every entry's share of a launch. */
int cgpt_set_tuning(cgpt_ctx* ctx, const char* name, uint32_t value);
/* Measures the vector-instruction issue rate of the device -- the roof bench.py prices the trace kernel against: every
 * SIMD of every CU runs `iters` x 64 independent instructions of one kind per wave at `waves_per_simd` resident waves.
 * kind: 0 v_mul_f32, 1 v_pk_mul_f32, 2 v_pk_add_f32, 3 v_rcp_f32, 4/5/6 scalar : packed mixes (3:1 interleaved, 3:1 grouped,
 * 1:1 alternating), 7 v_cndmask_b32 (VCC), 8 v_mul_lo_u32, 9 v_cndmask_b32_e64 (SGPR pair), 10 v_cmp + v_cndmask pairs,
 * 11 v_add_u32, 12 v_min3_f32.
 * Returns wave64 instructions per second over the whole chip (and the launch duration in ms_out, may be NULL). */
int cgpt_measure_issue_rate(cgpt_ctx* ctx, uint32_t kind, uint32_t waves_per_simd, uint32_t iters, double* wave_insts_per_sec, double* ms_out);

#ifdef __cplusplus
}
#endif
#endif
