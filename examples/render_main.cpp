// render_main.cpp -- headless analogue of the reference's main loop (ref: Source/Main.cpp:757-949) on the C ABI:
// scene set-up as Main.cpp:775-819 (with the synthetic dragon stand-in, or a glTF given on the command line),
// N x Render(), then a host framebuffer dump instead of the DX12 present (ref: Main.cpp:935-936).
//
//   g++ -std=c++17 -Iinclude -Icpugpupathtracing_amd/csrc/host examples/render_main.cpp
//       -Lcpugpupathtracing_amd/lib -lcpugpupt -Wl,-rpath,$PWD/cpugpupathtracing_amd/lib -o render_main   (one command line)
//   ./render_main [--gpus N [--collective]] [--denoise] [--temporal] [--spin DEG] [--variance-guided] [--ground-roughness R] [--glass-roughness R] [--bvh intervals|binned] [--nee-candidates M] [--top-level] [--instances N] [--smooth] [--mesh-transform m00 .. m23] [--bend DEG] [--animate T [--loop] [--crossfade W]] [--bulge W] [--crowd N] [--rebuild [naive|intervals|binned]] [--rebuild-ratio R] [--tonemap clamp|reinhard|aces|hable] [--srgb] [--exposure auto|EV] [--adapt ALPHA] [model.gltf] [width height spp [preview_every [move_at right up forward]]]
// --gpus N: ONE context over the first N GPUs of the node (cgpt_ctx_create with n_devices = N): every frame is spread over them in
// interleaved row bands and the read-back gathers the float4 bands with one RCCL exchange over xGMI; the loop below does not
// change.  --collective: take that code path with N = 1 too (what a one-GPU box can test).
// preview_every > 0 writes preview_NNNN.ppm every that many samples: the progressive display the reference gets from
// presenting data.pixels after every Render() (ref: Main.cpp:935-936, Source/DX12.cpp:277-322).
// --denoise: also write the image through cgpt_denoise (default parameters) next to each preview (preview_NNNN_denoised.ppm) and at the
// end (render_denoised.ppm) -- what a viewer with a "Denoise" toggle presents; the accumulator and the raw dumps are not affected.
// --temporal: a moving camera instead of the accumulating loop -- 8 frames of an orbit around the scene (2 degrees a frame), each `spp` samples
// from a reset accumulator, as a viewer renders while the camera moves; every frame is written raw (temporal_NN_raw.ppm), through
// cgpt_denoise (temporal_NN_denoised.ppm) and through cgpt_denoise_temporal, which reprojects the frames before it (temporal_NN_temporal.ppm;
// DESIGN.md 5.19).  Takes [width height spp] only.
// --spin DEG: a moving object instead -- 8 frames under the scene's camera in which the mesh (object 0) turns by DEG degrees a frame about the
// vertical axis through its centre (cgpt_scene_update_transforms, on top of --mesh-transform), each `spp` samples from a reset accumulator;
// every frame is written raw (spin_NN_raw.ppm), through cgpt_denoise (spin_NN_denoised.ppm) and through cgpt_denoise_temporal with
// CGPT_TEMPORAL_FOLLOW_TRANSFORMS, which carries the mesh's pixels back through the turn and keeps everyone's history (spin_NN_temporal.ppm;
// DESIGN.md 5.25).  Takes [width height spp] only.
// --variance-guided: the filter with the colour edge-stop in standard deviations of each pixel (cgpt_denoise_variance_guided).
// With --denoise it is written next to every denoised image (preview_NNNN_variance_guided.ppm, render_variance_guided.ppm); with --temporal
// it takes cgpt_denoise_temporal's place with CGPT_VARIANCE_TEMPORAL set (temporal_NN_variance_guided.ppm instead of temporal_NN_temporal.ppm:
// one call per rendered frame may consume its samples).
// --ground-roughness R: a glossy ground -- its material (1) gets specular 0.5 and roughness R in [0, 1] (cgpt_scene_update_roughness after
// the upload; 0 keeps the mirror half of the lobe perfect).
// --glass-roughness R: a frosted mesh -- its material (3, the glass) gets the transmission roughness R in [0, 1]
// (cgpt_scene_update_transmission_roughness after the upload; 0 is the reference's polished glass).
// --bvh binned: build the mesh's tree with BuildOption_SAHBinned (16 bins per axis) on the host instead of the reference's
// SAH split intervals (the default; image parity with the reference is defined on that tree).
// --top-level: IntersectScene reaches the objects through the top-level tree (cgpt_set_top_level(1)): the same image, bit for bit.
// --instances N: mesh instancing -- N more placements of the mesh (object 0) stand behind it on a jittered grid over the ground, each a third
// of its size under a rotation and shift of its own; they share the mesh's triangles and tree on the host, and the scene is uploaded with
// cgpt_scene_upload_instanced, so the device holds the mesh once however large N is.  The footprint is printed.
// --nee-candidates M: resampled light sampling -- every NEE light sample is the survivor of M candidates in 1..32 (cgpt_set_nee_candidates,
// set before the upload: it is context state; 1, the default, is the reference's single sample).
// --smooth: smooth shading -- every mesh object that is not a light shades with its interpolated vertex normals
// (cgpt_scene_update_smooth_normals after the upload; without it the reference's flat v0.normal).
// --mesh-transform m00 m01 m02 m03 m10 .. m23: the mesh (object 0, the dragon or its stand-in) is placed by this object-to-world matrix, the
// rows of [A | b] with world = A p + b (cgpt_scene_update_transforms after the upload); the other objects keep the identity.
// --bend DEG: a deforming mesh -- the mesh (object 0) gets a procedural two-joint skin on the device (cgpt_scene_set_skin: the weights come from a
// vertex's height between the mesh's lowest and highest point) and is posed once per frame (cgpt_scene_skin_mesh; joint 1 turns about the x axis
// through the middle of the mesh, DEG degrees further every frame): 8 frames under the scene's camera, each `spp` samples from a
// reset accumulator; every frame is written raw (bend_NN_raw.ppm), through cgpt_denoise (bend_NN_denoised.ppm) and through cgpt_denoise_temporal
// with CGPT_TEMPORAL_FOLLOW_POSES, which carries the mesh's pixels back to where the same surface points were under the frame before and keeps
// everyone's history (bend_NN_temporal.ppm).  Takes [width height spp] only.  A demonstration of the device calls, not a loader
// feature: glTF skins are not imported.
// --bulge W: a morphing mesh -- the mesh (object 0) gets one procedural morph target on the device (cgpt_scene_set_morph_targets: every corner
// pushed out along its normal by its height between the mesh's lowest and highest point) and is posed once per frame with weight W * frame / 7
// (cgpt_scene_morph_mesh); frames as for --bend, named bulge_NN_*.ppm.  With --bend DEG as well the mesh has both and one
// kernel morphs and skins it (the frames keep the bend_ names).  With --bulge the temporal call sets CGPT_TEMPORAL_FOLLOW_POSES |
// CGPT_TEMPORAL_FOLLOW_MORPHS: the mesh's pixels are carried back to where the same surface points were under the weight (and the bend) of the
// frame before, and everyone keeps their history.
// --crowd N: many deforming meshes -- N separate copies of the mesh stand in a row (each its own triangles and tree on the device, unlike
// --instances; without a model the stand-in is built at level 4, 5120 triangles a copy), every one with the skin of --bend (and, with
// --bulge W, its morph target), bent by an angle of its own: copy k by DEG (k + 1) / N degrees a frame (DEG from --bend, 10 without it).  All of
// them are posed by ONE call a frame (cgpt_scene_pose_objects): the launches do not grow with N.  Frames and the temporal
// call as for --bend (crowd_NN_*.ppm).
// --animate T: with --bend DEG (and --crowd N), the bend is played from an animation clip on the device instead of from matrices the host
// computes: every posed mesh gets a two-joint skeleton under its skin (cgpt_scene_set_skeleton) and they all share one generated clip
// (cgpt_clip_create) whose rotation channel takes joint 1 from 0 to DEG over one second; ONE frame is rendered, at clip time T, posed by
// cgpt_scene_animate_objects -- with --crowd N character k plays at its own phase, T (k + 1) / N.  The joint matrices
// never exist on the host.  Frames are named animate_00_*.ppm.
// --loop: with --animate T, the clip repeats: T is wrapped over the clip's range (cgpt_clip_get_range) by CGPT_ANIM_WRAP_LOOP on the way to
// the device, so --animate 2.25 --loop shows what --animate 0.25 shows.  The frame is posed by cgpt_scene_animate_layers.
// --crossfade W: with --animate T, the bend clip is blended with a second clip, the opposite bend (0 to -DEG), at weight W in [0, 1] against
// 1 - W: one cgpt_scene_animate_layers entry of two layers per mesh -- with --crowd N character k fades at its own weight, W (k + 1) / N.
// --rebuild [OPTION]: with --bend / --bulge / --crowd, every posed mesh's tree is split again in place on the device after each frame's pose
// (cgpt_scene_rebuild_mesh), with the binned builder unless OPTION says otherwise: the refit keeps a tree that was split
// for the bind pose, and after a large bend its boxes overlap.  The triangles never leave the device.  A rebuild drops the temporal
// history, as a refit does.
// --rebuild-ratio R: rebuild only where it pays -- the cost of every posed mesh's tree (cgpt_scene_tree_costs) is measured once
// at the bind pose, and after each frame's pose one cgpt_scene_rebuild_degraded call rebuilds the meshes whose cost has grown past R times
// their reference (with --rebuild's builder; the reference of a rebuilt mesh becomes its new cost).  A line a frame and mesh gives the cost
// before and after, and says where a mesh was rebuilt.  A frame in which nothing is rebuilt keeps the temporal history.
// --tonemap CURVE, --srgb, --exposure auto|EV, --adapt ALPHA: the display stage (cgpt_tonemap).  Any of them sends every PPM
// the run writes -- raw, --denoise, --temporal, --variance-guided, the frames of a sequence -- through an exposure, the tone curve (clamp
// without --tonemap), and with --srgb the sRGB transfer function, on the device from the image's own source (the accumulator, or the filter's
// result where it lies).  --exposure auto (the default) meters each frame's luminance histogram and, in a --temporal / --spin / --bend /
// --animate sequence, moves the exposure towards it by ALPHA a frame (1, the default: every frame its own); --exposure EV is 2^EV, fixed.
// render.pfm and render.acc stay linear.
// move_at > 0 scripts the input half of Update(dt) (ref: Main.cpp:277-297, Camera::Update :104-131): after that many samples the
// camera is translated by (right, up, forward) as the A/D, Space/Shift, W/S keys would, the view changes, and the accumulator
// is reset (ref: ResetAccumulator, Main.cpp:238-243) before the remaining samples are rendered from the new position.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "cpugpupt_abi.h"
#include "gltf_loader.h"
#include "image_io.h"
#include "mesh_gen.h"
#include "scene.h"

using namespace cgpt;

#define CHECK(call)                                                                   \
    do {                                                                              \
        int rc_ = (call);                                                             \
        if (rc_ != CGPT_OK) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, cgpt_last_error(ctx)); return 1; } \
    } while (0)

int main(int argc, char** argv)
{
    int n_gpus = 1; uint32_t ctx_flags = 0; bool denoise = false; bool temporal = false; bool spin = false; float spin_deg = 0.0f; bool variance_guided = false; float ground_roughness = -1.0f, glass_roughness = -1.0f; uint32_t nee_candidates = 1; bool smooth = false; bool top_level = false; uint32_t n_instances = 0; bool bend = false; float bend_deg = 0.0f; bool bulge = false; float bulge_w = 0.0f; uint32_t crowd = 0; bool animate = false; float animate_t = 0.0f; bool loop = false; bool crossfade = false; float crossfade_w = 0.0f;
    bool rebuild = false; uint32_t rebuild_option = CGPT_BUILD_SAH_BINNED;
    bool rebuild_degraded = false; double rebuild_ratio = 0.0;
    bool tonemap = false;                                                // --tonemap / --srgb / --exposure / --adapt: the display stage in front of every PPM
    cgpt_tonemap_params tm = { CGPT_TONEMAP_ACCUMULATOR, CGPT_CURVE_CLAMP, CGPT_TRANSFER_LINEAR, CGPT_TONEMAP_AUTO_EXPOSURE, 1.0f, 0, 4.0f, 0.18f, 0.5f, 0.02f, 1.0f, nullptr, 0u, 0u };
    bool has_transform = false; float mesh_transform[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    MeshBVH::BuildOption bvh_option = MeshBVH::BuildOption_SAHSplitIntervals;
    while (argc > 1 && std::string(argv[1]).rfind("--", 0) == 0) {
        if (std::string(argv[1]) == "--gpus" && argc > 2) { n_gpus = atoi(argv[2]); argv += 2; argc -= 2; }
        else if (std::string(argv[1]) == "--collective") { ctx_flags |= CGPT_CTX_FORCE_COLLECTIVE; argv += 1; argc -= 1; }
        else if (std::string(argv[1]) == "--denoise") { denoise = true; argv += 1; argc -= 1; }
        else if (std::string(argv[1]) == "--temporal") { temporal = true; argv += 1; argc -= 1; }
        else if (std::string(argv[1]) == "--spin" && argc > 2) { spin = true; spin_deg = (float)atof(argv[2]); argv += 2; argc -= 2; }
        else if (std::string(argv[1]) == "--bend" && argc > 2) { bend = true; bend_deg = (float)atof(argv[2]); argv += 2; argc -= 2; }
        else if (std::string(argv[1]) == "--bulge" && argc > 2) { bulge = true; bulge_w = (float)atof(argv[2]); argv += 2; argc -= 2; }
        else if (std::string(argv[1]) == "--animate" && argc > 2) { animate = true; animate_t = (float)atof(argv[2]); argv += 2; argc -= 2; }
        else if (std::string(argv[1]) == "--loop") { loop = true; argv += 1; argc -= 1; }
        else if (std::string(argv[1]) == "--crossfade" && argc > 2) { crossfade = true; crossfade_w = (float)atof(argv[2]); argv += 2; argc -= 2; }
        else if (std::string(argv[1]) == "--crowd" && argc > 2) { crowd = (uint32_t)atoi(argv[2]); argv += 2; argc -= 2; }
        else if (std::string(argv[1]) == "--rebuild") {
            rebuild = true; argv += 1; argc -= 1;
            const std::string opt = argc > 1 ? argv[1] : "";
            if (opt == "naive" || opt == "intervals" || opt == "binned") {
                rebuild_option = opt == "naive" ? CGPT_BUILD_NAIVE_SPLIT : opt == "intervals" ? CGPT_BUILD_SAH_SPLIT_INTERVALS : CGPT_BUILD_SAH_BINNED;
                argv += 1; argc -= 1;
            }
        }
        else if (std::string(argv[1]) == "--rebuild-ratio" && argc > 2) {
            rebuild_degraded = true; rebuild_ratio = atof(argv[2]); argv += 2; argc -= 2;
            if (!(rebuild_ratio > 0.0) || !std::isfinite(rebuild_ratio)) { fprintf(stderr, "--rebuild-ratio needs a finite ratio > 0\n"); return 2; }
        }
        else if (std::string(argv[1]) == "--tonemap" && argc > 2) {
            const std::string c = argv[2];
            if (c != "clamp" && c != "reinhard" && c != "aces" && c != "hable") { fprintf(stderr, "--tonemap needs clamp, reinhard, aces or hable\n"); return 2; }
            tonemap = true; tm.curve = c == "clamp" ? CGPT_CURVE_CLAMP : c == "reinhard" ? CGPT_CURVE_REINHARD : c == "aces" ? CGPT_CURVE_ACES : CGPT_CURVE_HABLE;
            argv += 2; argc -= 2;
        }
        else if (std::string(argv[1]) == "--srgb") { tonemap = true; tm.transfer = CGPT_TRANSFER_SRGB; argv += 1; argc -= 1; }
        else if (std::string(argv[1]) == "--exposure" && argc > 2) {
            tonemap = true;
            if (std::string(argv[2]) == "auto") tm.flags = CGPT_TONEMAP_AUTO_EXPOSURE;
            else {
                char* end = nullptr;
                const double ev = strtod(argv[2], &end);
                if (end == argv[2] || *end || !(std::fabs(ev) <= 64.0)) { fprintf(stderr, "--exposure needs auto or an EV in [-64, 64]\n"); return 2; }
                tm.flags = 0u; tm.exposure_scale = (float)std::exp2(ev);
            }
            argv += 2; argc -= 2;
        }
        else if (std::string(argv[1]) == "--adapt" && argc > 2) {
            tonemap = true; tm.alpha = (float)atof(argv[2]); argv += 2; argc -= 2;
            if (!(tm.alpha >= 0.0f && tm.alpha <= 1.0f)) { fprintf(stderr, "--adapt needs an alpha in [0, 1]\n"); return 2; }
        }
        else if (std::string(argv[1]) == "--variance-guided") { variance_guided = true; argv += 1; argc -= 1; }
        else if (std::string(argv[1]) == "--smooth") { smooth = true; argv += 1; argc -= 1; }
        else if (std::string(argv[1]) == "--mesh-transform" && argc > 13) {
            for (int k = 0; k < 12; ++k) mesh_transform[k] = (float)atof(argv[2 + k]);
            has_transform = true; argv += 13; argc -= 13;
        }
        else if (std::string(argv[1]) == "--ground-roughness" && argc > 2) { ground_roughness = (float)atof(argv[2]); argv += 2; argc -= 2; }
        else if (std::string(argv[1]) == "--glass-roughness" && argc > 2) { glass_roughness = (float)atof(argv[2]); argv += 2; argc -= 2; }
        else if (std::string(argv[1]) == "--top-level") { top_level = true; argv += 1; argc -= 1; }
        else if (std::string(argv[1]) == "--instances" && argc > 2) { n_instances = (uint32_t)atoi(argv[2]); argv += 2; argc -= 2; }
        else if (std::string(argv[1]) == "--nee-candidates" && argc > 2) { nee_candidates = (uint32_t)atoi(argv[2]); argv += 2; argc -= 2; }
        else if (std::string(argv[1]) == "--bvh" && argc > 2 && (std::string(argv[2]) == "binned" || std::string(argv[2]) == "intervals")) {
            bvh_option = std::string(argv[2]) == "binned" ? MeshBVH::BuildOption_SAHBinned : MeshBVH::BuildOption_SAHSplitIntervals; argv += 2; argc -= 2;
        }
        else { fprintf(stderr, "unknown option %s\n", argv[1]); return 2; }
    }
    std::string model = argc > 1 && std::string(argv[1]).find(".gltf") != std::string::npos ? argv[1] : "";
    const int base = model.empty() ? 1 : 2;
    const uint32_t W = argc > base ? (uint32_t)atoi(argv[base]) : 1280, H = argc > base + 1 ? (uint32_t)atoi(argv[base + 1]) : 720;
    const uint32_t spp = argc > base + 2 ? (uint32_t)atoi(argv[base + 2]) : 64;
    const uint32_t preview_every = argc > base + 3 ? (uint32_t)atoi(argv[base + 3]) : 0;
    const uint32_t move_at = argc > base + 7 ? (uint32_t)atoi(argv[base + 4]) : 0;
    const float move_right = move_at ? (float)atof(argv[base + 5]) : 0.0f, move_up = move_at ? (float)atof(argv[base + 6]) : 0.0f;
    const float move_forward = move_at ? (float)atof(argv[base + 7]) : 0.0f;

    Mesh mesh;
    if ((crowd || animate) && !bend) { bend = true; bend_deg = 10.0f; }
    if (model.empty()) mesh = MakeDragonStandIn(crowd ? 4 : 6);
    else { std::string err; if (!GLTFLoader::Load(model, mesh, err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; } }   // ref: Main.cpp:785
    std::vector<Mesh> crowd_meshes;                                      // --crowd: copy k of the mesh, shrunk about its centre and shifted along x
    if (crowd) {
        float lo[3] = { 1e30f, 1e30f, 1e30f }, hi[3] = { -1e30f, -1e30f, -1e30f };
        for (const cgpt_vertex& v : mesh.vertices)
            for (int a = 0; a < 3; ++a) { lo[a] = std::fmin(lo[a], v.pos[a]); hi[a] = std::fmax(hi[a], v.pos[a]); }
        const float scale = std::fmin(1.0f, 3.0f / (float)crowd), step = 1.1f * scale * (hi[0] - lo[0]);
        for (uint32_t k = 0; k < crowd; ++k) {
            Mesh copy = mesh;
            for (cgpt_vertex& v : copy.vertices)
                for (int a = 0; a < 3; ++a) v.pos[a] = 0.5f * (lo[a] + hi[a]) + scale * (v.pos[a] - 0.5f * (lo[a] + hi[a])) + (a == 0 ? step * ((float)k - 0.5f * (float)(crowd - 1)) : 0.0f);
            crowd_meshes.push_back(std::move(copy));
        }
        mesh = crowd_meshes[0];
    }
    Scene scene = MakeReferenceScene(mesh, 3, (float)W / (float)H, bvh_option);            // ref: Main.cpp:777-819
    std::vector<uint32_t> posed(1, 0u);                                  // the objects --bend / --bulge pose: the mesh, and with --crowd its copies
    for (uint32_t k = 1; k < crowd; ++k) {
        posed.push_back((uint32_t)scene.objects.size());
        scene.objects.push_back(Object("Crowd", crowd_meshes[k], k % 2 ? 0u : 3u, bvh_option));
        if (!scene.objects.back().valid) { fprintf(stderr, "copy %u of the mesh could not be built\n", k); return 1; }
    }
    if (!scene.objects[0].valid) { fprintf(stderr, "the mesh is empty, or (--bvh binned) has a position that is not finite or beyond 1e30\n"); return 1; }
    if (ground_roughness >= 0.0f) { scene.materials[1].specular = 0.5f; scene.materials[1].roughness = ground_roughness; }
    if (glass_roughness >= 0.0f) scene.materials[3].transmission_roughness = glass_roughness;
    if (has_transform) for (int k = 0; k < 12; ++k) scene.objects[0].transform[k] = mesh_transform[k];
    if (n_instances) {                                                   // a jittered grid behind the mesh, rows of `side`
        const uint32_t side = (uint32_t)std::ceil(std::sqrt((double)n_instances));
        uint32_t rng = 0x2545F491u;
        auto jitter = [&rng]() { rng = rng * 1664525u + 1013904223u; return (float)(rng >> 8) / 16777216.0f - 0.5f; };   // [-0.5, 0.5)
        for (uint32_t k = 0; k < n_instances; ++k) {
            Object instance("Instance", scene.objects[0], k % 2 ? 0u : 3u);  // shares the mesh; built before the vector may move object 0
            const float angle = 6.2831853f * jitter(), scale = 0.33f, c = scale * std::cos(angle), sn = scale * std::sin(angle);
            const float x = 2.5f * ((float)(k % side) - 0.5f * (float)(side - 1)) + 0.8f * jitter(), z = -6.0f - 2.5f * (float)(k / side) + 0.8f * jitter();
            const float m[12] = { c, 0.0f, sn, x, 0.0f, scale, 0.0f, -2.0f, -sn, 0.0f, c, z };
            for (int i = 0; i < 12; ++i) instance.transform[i] = m[i];
            scene.objects.push_back(std::move(instance));
        }
    }

    cgpt_ctx* ctx = nullptr;
    // ThreadPool::Init: device_ids = NULL means devices 0 .. n_gpus-1
    if (cgpt_ctx_create(nullptr, n_gpus, ctx_flags, &ctx) != CGPT_OK) { fprintf(stderr, "%s\n", cgpt_last_error(nullptr)); return 1; }
    // The display stage: with one of its options every image below goes through cgpt_tonemap on its way to a PPM -- `px`
    // holds what the run would have written and receives the mapped pixels of the same source, still on the device.  The first image of
    // a frame adapts the exposure by --adapt; the others of that frame keep it (alpha 0), so a frame adapts once
    const float adapt_alpha = tm.alpha;
    auto present = [&](uint32_t source, std::vector<uint32_t>& px, bool first_of_frame) -> int {
        if (!tonemap) return CGPT_OK;
        tm.source = source; tm.alpha = first_of_frame ? adapt_alpha : 0.0f;
        return cgpt_tonemap(ctx, &tm, nullptr, 0, px.data(), px.size());
    };
    CHECK(cgpt_set_top_level(ctx, top_level ? 1u : 0u));                  // context state too
    CHECK(cgpt_set_nee_candidates(ctx, nee_candidates));                 // context state: allowed before a scene exists, kept by every upload
    Scene::FlatStorage flat;
    cgpt_scene_desc desc = scene.Flatten(flat);
    CHECK(n_instances ? cgpt_scene_upload_instanced(ctx, &desc) : cgpt_scene_upload(ctx, &desc));
    if (n_instances) {
        cgpt_scene_footprint fp{};
        CHECK(cgpt_get_scene_footprint(ctx, &fp));
        printf("%u objects, %u mesh objects in %u device copies: %u triangles, %.1f MB on the device\n", fp.n_objects, fp.n_mesh_objects, fp.n_mesh_copies,
               fp.n_orig_triangles, (double)fp.device_bytes / 1e6);
    }
    if (ground_roughness >= 0.0f) {                                      // roughness is not part of the scene description: set after the upload
        std::vector<float> roughness;
        for (const Material& m : scene.materials) roughness.push_back(m.roughness);
        CHECK(cgpt_scene_update_roughness(ctx, roughness.data(), (uint32_t)roughness.size()));
    }
    if (glass_roughness >= 0.0f) {                                       // nor is the transmission roughness
        std::vector<float> roughness;
        for (const Material& m : scene.materials) roughness.push_back(m.transmission_roughness);
        CHECK(cgpt_scene_update_transmission_roughness(ctx, roughness.data(), (uint32_t)roughness.size()));
    }
    if (smooth) {                                                        // nor are the smooth-normal flags
        std::vector<uint32_t> flags;
        for (const Object& o : scene.objects) flags.push_back(o.has_bvh ? 1u : 0u);
        for (const uint32_t li : scene.light_source_indices) flags[li] = 0u;
        CHECK(cgpt_scene_update_smooth_normals(ctx, flags.data(), (uint32_t)flags.size()));
    }
    if (has_transform || n_instances) {                                  // nor are the transforms: object 0 (the mesh) and the instances
        std::vector<float> matrices;
        for (const Object& o : scene.objects) matrices.insert(matrices.end(), o.transform, o.transform + 12);
        CHECK(cgpt_scene_update_transforms(ctx, matrices.data(), (uint32_t)scene.objects.size()));
    }

    const cgpt_settings settings = scene.AbiSettings();
    if (temporal) {                                                      // the camera moves every frame: ResetAccumulator, Render, present
        std::vector<uint32_t> px((size_t)W * H);
        for (uint32_t frame = 0; frame < 8; ++frame) {
            const float angle = 2.0f * (float)frame * 3.14159265f / 180.0f;
            const float pos[3] = { 8.0f * std::sin(angle), 0.0f, 8.0f * std::cos(angle) }, dir[3] = { -std::sin(angle), 0.0f, -std::cos(angle) };   // towards the origin
            cgpt_camera cam;
            CHECK(cgpt_camera_from_view(pos, dir, 60.0f, (float)W / (float)H, &cam));
            CHECK(cgpt_reset_accumulator(ctx));
            cgpt_render_params p{};
            p.width = W; p.height = H; p.row_begin = 0; p.row_end = H;
            p.first_sample = 0; p.n_samples = spp; p.seed = 0x12345678u + frame; p.kernel = CGPT_KERNEL_AUTO;
            CHECK(cgpt_render(ctx, &cam, &settings, &p));
            char name[64]; std::string err;
            CHECK(cgpt_read_pixels(ctx, px.data(), px.size())); CHECK(present(CGPT_TONEMAP_ACCUMULATOR, px, true));
            snprintf(name, sizeof(name), "temporal_%02u_raw.ppm", frame); WritePPM(name, px.data(), W, H, err);
            CHECK(cgpt_denoise(ctx, &cam, nullptr, nullptr, 0, px.data(), px.size())); CHECK(present(CGPT_TONEMAP_DENOISED, px, false));
            snprintf(name, sizeof(name), "temporal_%02u_denoised.ppm", frame); WritePPM(name, px.data(), W, H, err);
            if (variance_guided) {                                       // the temporal stage with the luminance moments, once per rendered frame
                const cgpt_variance_params vp = { 4.0f, 4u, CGPT_VARIANCE_TEMPORAL };
                CHECK(cgpt_denoise_variance_guided(ctx, &cam, nullptr, nullptr, &vp, nullptr, 0, px.data(), px.size())); CHECK(present(CGPT_TONEMAP_DENOISED, px, false));
                snprintf(name, sizeof(name), "temporal_%02u_variance_guided.ppm", frame); WritePPM(name, px.data(), W, H, err);
                continue;
            }
            CHECK(cgpt_denoise_temporal(ctx, &cam, nullptr, nullptr, nullptr, 0, px.data(), px.size()));   // once per rendered frame
            CHECK(present(CGPT_TONEMAP_DENOISED, px, false));
            snprintf(name, sizeof(name), "temporal_%02u_temporal.ppm", frame); WritePPM(name, px.data(), W, H, err);
        }
        cgpt_ctx_destroy(ctx);
        return 0;
    }
    if (spin) {                                                          // the mesh moves every frame: UpdateTransforms, ResetAccumulator, Render, present
        std::vector<uint32_t> px((size_t)W * H);
        std::vector<float> matrices;
        for (const Object& o : scene.objects) matrices.insert(matrices.end(), o.transform, o.transform + 12);
        float lo[3] = { 1e30f, 1e30f, 1e30f }, hi[3] = { -1e30f, -1e30f, -1e30f };
        for (const cgpt_vertex& v : mesh.vertices)
            for (int a = 0; a < 3; ++a) { lo[a] = std::fmin(lo[a], v.pos[a]); hi[a] = std::fmax(hi[a], v.pos[a]); }
        const float* const m0 = scene.objects[0].transform;               // the mesh's placement; the turn is about its centre in the world
        double centre[3];
        for (int r = 0; r < 3; ++r) centre[r] = m0[4 * r] * 0.5 * (lo[0] + hi[0]) + m0[4 * r + 1] * 0.5 * (lo[1] + hi[1]) + m0[4 * r + 2] * 0.5 * (lo[2] + hi[2]) + m0[4 * r + 3];
        const cgpt_camera cam = scene.camera.Abi();
        const cgpt_temporal_params tp = { 64.0f, 0.9f, 0.01f, CGPT_TEMPORAL_FOLLOW_TRANSFORMS };
        for (uint32_t frame = 0; frame < 8; ++frame) {
            const double angle = (double)spin_deg * (double)frame * 3.14159265358979 / 180.0, c = std::cos(angle), sn = std::sin(angle);
            const double rot[3][3] = { { c, 0.0, sn }, { 0.0, 1.0, 0.0 }, { -sn, 0.0, c } };
            for (int r = 0; r < 3; ++r) {                                // R (M0 p - centre) + centre
                for (int k = 0; k < 3; ++k) matrices[4 * r + k] = (float)(rot[r][0] * m0[k] + rot[r][1] * m0[4 + k] + rot[r][2] * m0[8 + k]);
                matrices[4 * r + 3] = (float)(rot[r][0] * (m0[3] - centre[0]) + rot[r][1] * (m0[7] - centre[1]) + rot[r][2] * (m0[11] - centre[2]) + centre[r]);
            }
            CHECK(cgpt_scene_update_transforms(ctx, matrices.data(), (uint32_t)scene.objects.size()));
            CHECK(cgpt_reset_accumulator(ctx));
            cgpt_render_params p{};
            p.width = W; p.height = H; p.row_begin = 0; p.row_end = H;
            p.first_sample = 0; p.n_samples = spp; p.seed = 0x12345678u + frame; p.kernel = CGPT_KERNEL_AUTO;
            CHECK(cgpt_render(ctx, &cam, &settings, &p));
            char name[64]; std::string err;
            CHECK(cgpt_read_pixels(ctx, px.data(), px.size())); CHECK(present(CGPT_TONEMAP_ACCUMULATOR, px, true));
            snprintf(name, sizeof(name), "spin_%02u_raw.ppm", frame); WritePPM(name, px.data(), W, H, err);
            CHECK(cgpt_denoise(ctx, &cam, nullptr, nullptr, 0, px.data(), px.size())); CHECK(present(CGPT_TONEMAP_DENOISED, px, false));
            snprintf(name, sizeof(name), "spin_%02u_denoised.ppm", frame); WritePPM(name, px.data(), W, H, err);
            CHECK(cgpt_denoise_temporal(ctx, &cam, nullptr, &tp, nullptr, 0, px.data(), px.size()));   // once per rendered frame
            CHECK(present(CGPT_TONEMAP_DENOISED, px, false));
            snprintf(name, sizeof(name), "spin_%02u_temporal.ppm", frame); WritePPM(name, px.data(), W, H, err);
        }
        cgpt_ctx_destroy(ctx);
        return 0;
    }
    // --bend: a procedural two-joint skin of the mesh (object 0).  A corner's weight on joint 1 is its height between the mesh's lowest and
    // highest point; joint 0 stays, joint 1 turns about the x axis through the middle of the mesh.  The skin goes to the device once.
    // --bulge: one procedural morph target of the same mesh, a push along the normal by the same height; it goes to the device once too.
    if (bend || bulge) {
        std::vector<float> pivots;                                       // y and z of every posed object's middle
        for (const uint32_t obj : posed) {
            const cgpt_object& o = desc.objects[obj];
            const cgpt_triangle* bind = desc.triangles + o.tri_offset;  // original order, as cgpt_scene_refit_mesh takes them
            float lo[3] = { 1e30f, 1e30f, 1e30f }, hi[3] = { -1e30f, -1e30f, -1e30f };
            for (uint32_t t = 0; t < o.tri_count; ++t)
                for (const cgpt_vertex* v : { &bind[t].v0, &bind[t].v1, &bind[t].v2 })
                    for (int a = 0; a < 3; ++a) { lo[a] = std::fmin(lo[a], v->pos[a]); hi[a] = std::fmax(hi[a], v->pos[a]); }
            pivots.push_back(0.5f * (lo[1] + hi[1])); pivots.push_back(0.5f * (lo[2] + hi[2]));
            std::vector<uint16_t> joints(12 * (size_t)o.tri_count, 0);
            std::vector<float> weights(12 * (size_t)o.tri_count, 0.0f);
            for (uint32_t t = 0; t < o.tri_count; ++t) {
                const cgpt_vertex* const corner[3] = { &bind[t].v0, &bind[t].v1, &bind[t].v2 };
                for (int c = 0; c < 3; ++c) {
                    const float h = hi[1] > lo[1] ? (corner[c]->pos[1] - lo[1]) / (hi[1] - lo[1]) : 0.0f;
                    joints[12 * (size_t)t + 4 * c + 1] = 1;
                    weights[12 * (size_t)t + 4 * c] = 1.0f - h; weights[12 * (size_t)t + 4 * c + 1] = h;
                }
            }
            if (bend) CHECK(cgpt_scene_set_skin(ctx, obj, bind, joints.data(), weights.data(), o.tri_count, 2));
            if (bulge) {
                std::vector<cgpt_triangle> target(o.tri_count);          // displacements in the cgpt_triangle layout: position delta = height * normal, no normal delta
                for (uint32_t t = 0; t < o.tri_count; ++t) {
                    const cgpt_vertex* const corner[3] = { &bind[t].v0, &bind[t].v1, &bind[t].v2 };
                    cgpt_vertex* const d[3] = { &target[t].v0, &target[t].v1, &target[t].v2 };
                    for (int c = 0; c < 3; ++c)
                        for (int a = 0; a < 3; ++a) { d[c]->pos[a] = weights[12 * (size_t)t + 4 * c + 1] * corner[c]->normal[a]; d[c]->normal[a] = 0.0f; }
                }
                CHECK(cgpt_scene_set_morph_targets(ctx, obj, bind, target.data(), o.tri_count, 1));
            }
        }

        // --animate: the same bend as a clip.  Joint 0 is the root at the origin, joint 1 its child at the pivot; the inverse bind matrices
        // undo the rest pose, so M_1 = T(pivot) R_x T(-pivot) as below.  One clip for everyone: joint 1's rotation, 0 -> DEG over a second.
        uint32_t clip = 0, clip_back = 0;
        if (animate) {
            const double half = 0.5 * (double)bend_deg * 3.14159265358979 / 180.0;
            const cgpt_clip_channel channel = { 1u, CGPT_ANIM_PATH_ROTATION, CGPT_ANIM_LINEAR, 2u, 0u, 0u };
            const float key_times[2] = { 0.0f, 1.0f };
            const float key_values[8] = { 0.0f, 0.0f, 0.0f, 1.0f, (float)std::sin(half), 0.0f, 0.0f, (float)std::cos(half) };
            const cgpt_clip_desc cd = { 2u, 1u, &channel, key_times, 2u, key_values, 8u };
            CHECK(cgpt_clip_create(ctx, &cd, &clip));
            if (crossfade) {                                             // --crossfade: the opposite bend, 0 -> -DEG over the same second
                const float back_values[8] = { 0.0f, 0.0f, 0.0f, 1.0f, (float)-std::sin(half), 0.0f, 0.0f, (float)std::cos(half) };
                const cgpt_clip_desc back = { 2u, 1u, &channel, key_times, 2u, back_values, 8u };
                CHECK(cgpt_clip_create(ctx, &back, &clip_back));
            }
            for (size_t k = 0; k < posed.size(); ++k) {
                const float py = pivots[2 * k], pz = pivots[2 * k + 1];
                const int32_t parents[2] = { -1, 0 };
                const float inverse_bind[24] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, -py, 0, 0, 1, -pz };
                const float rest[20] = { 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, py, pz, 0, 0, 0, 1, 1, 1, 1 };
                const cgpt_skeleton_desc sd = { parents, inverse_bind, rest, nullptr, 2u };
                CHECK(cgpt_scene_set_skeleton(ctx, posed[k], &sd));
            }
        }
        std::vector<cgpt_rebuild_candidate> candidates;                  // --rebuild-ratio: every posed mesh with its tree's cost at the bind pose
        if (rebuild_degraded) {
            std::vector<cgpt_tree_cost> costs(posed.size());
            CHECK(cgpt_scene_tree_costs(ctx, posed.data(), (uint32_t)posed.size(), 1.0, 1.0, costs.data()));
            for (size_t k = 0; k < posed.size(); ++k) candidates.push_back({ posed[k], 0u, costs[k].cost });
        }
        std::vector<uint32_t> px((size_t)W * H);                         // the mesh bends every frame: SkinMesh, ResetAccumulator, Render, present
        const cgpt_camera cam = scene.camera.Abi();
        const cgpt_temporal_params tp = { 64.0f, 0.9f, 0.01f, CGPT_TEMPORAL_FOLLOW_POSES | (bulge ? (uint32_t)CGPT_TEMPORAL_FOLLOW_MORPHS : 0u) };   // each flag keeps its own kind of edit
        for (uint32_t frame = 0; frame < (animate ? 1u : 8u); ++frame) {  // the pose of this frame: 48 bytes a joint go to the device
            std::vector<float> joint_matrices(24 * posed.size());
            for (size_t k = 0; k < posed.size(); ++k) {                  // copy k of a crowd bends by its own share of the angle
                const double share = crowd ? (double)(k + 1) / (double)crowd : 1.0;
                const double angle = share * (double)bend_deg * (double)frame * 3.14159265358979 / 180.0, c = std::cos(angle), sn = std::sin(angle);
                const float py = pivots[2 * k], pz = pivots[2 * k + 1];
                const float m[24] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0,                                    // joint 0 stays
                                      1, 0, 0, 0, 0, (float)c, (float)-sn, (float)(py - c * py + sn * pz),    // joint 1: R_x (p - pivot) + pivot
                                      0, (float)sn, (float)c, (float)(pz - sn * py - c * pz) };
                for (int i = 0; i < 24; ++i) joint_matrices[24 * k + i] = m[i];
            }
            const float morph_weight = bulge_w * (float)frame / 7.0f;
            if (animate && (loop || crossfade)) {                        // --loop / --crossfade: up to two layers per object, wrapped and blended on the device's side
                float begin = 0.0f, end = 0.0f;
                CHECK(cgpt_clip_get_range(ctx, clip, &begin, &end));
                const uint32_t wrap = loop ? (uint32_t)CGPT_ANIM_WRAP_LOOP : (uint32_t)CGPT_ANIM_WRAP_CLAMP;
                std::vector<cgpt_clip_layer> layers(2 * posed.size());
                std::vector<cgpt_layered_animation> entries(posed.size());
                for (size_t k = 0; k < posed.size(); ++k) {
                    const float share = crowd ? (float)(k + 1) / (float)crowd : 1.0f;
                    const float w = crossfade ? std::fmin(std::fmax(crossfade_w * share, 0.0f), 1.0f) : 0.0f;
                    layers[2 * k] = { clip, animate_t * share, 1.0f - w, wrap };
                    layers[2 * k + 1] = { crossfade ? clip_back : clip, animate_t * share, w, wrap };   // weight 0 without --crossfade: never sampled
                    entries[k] = { posed[k], 2u, layers.data() + 2 * k, bulge ? 1u : 0u, bulge ? &morph_weight : nullptr };
                }
                CHECK(cgpt_scene_animate_layers(ctx, entries.data(), (uint32_t)entries.size()));
                if (frame == 0) printf("clip range [%g, %g]%s%s\n", (double)begin, (double)end, loop ? ", looped" : "", crossfade ? ", cross-faded with the opposite bend" : "");
            } else if (animate) {                                        // a clip and a time per object: nothing else goes to the device
                std::vector<cgpt_animation> entries(posed.size());
                for (size_t k = 0; k < posed.size(); ++k)
                    entries[k] = { posed[k], clip, crowd ? animate_t * (float)(k + 1) / (float)crowd : animate_t, bulge ? 1u : 0u, bulge ? &morph_weight : nullptr };
                CHECK(cgpt_scene_animate_objects(ctx, entries.data(), (uint32_t)entries.size()));
            } else if (crowd) {                                          // every copy in one call: an entry with both arrays is posed once, by the fused kernel
                std::vector<cgpt_pose> poses(posed.size());
                for (size_t k = 0; k < posed.size(); ++k) poses[k] = { posed[k], 2u, joint_matrices.data() + 24 * k, bulge ? 1u : 0u, bulge ? &morph_weight : nullptr };
                CHECK(cgpt_scene_pose_objects(ctx, poses.data(), (uint32_t)poses.size()));
            } else {
                if (bulge) CHECK(cgpt_scene_morph_mesh(ctx, 0, &morph_weight, 1));       // 4 bytes a target go to the device
                if (bend) CHECK(cgpt_scene_skin_mesh(ctx, 0, joint_matrices.data(), 2)); // on a mesh with targets: the morphed base through the joints, one kernel
            }
            if (rebuild) {                                               // the trees follow the pose: split again on the device, from the current leaf order
                for (const uint32_t obj : posed) {
                    uint32_t n_nodes = 0, depth = 0;
                    CHECK(cgpt_scene_rebuild_mesh(ctx, obj, rebuild_option, &n_nodes, &depth));
                    printf("frame %u: object %u rebuilt, %u nodes, depth %u\n", frame, obj, n_nodes, depth);
                }
            }
            if (rebuild_degraded) {                                      // ... or only the trees the pose has degraded: one call for all of them
                std::vector<cgpt_rebuild_result> results(candidates.size());
                CHECK(cgpt_scene_rebuild_degraded(ctx, candidates.data(), (uint32_t)candidates.size(), rebuild_ratio, rebuild_option, 1.0, 1.0, results.data()));
                for (size_t k = 0; k < candidates.size(); ++k) {
                    printf("frame %u: object %u tree cost %.4f -> %.4f (reference %.4f)%s\n", frame, candidates[k].obj_index, results[k].cost_before, results[k].cost_after,
                           candidates[k].reference_cost, results[k].rebuilt ? ", rebuilt" : "");
                    if (results[k].rebuilt) candidates[k].reference_cost = results[k].cost_after;
                }
            }
            CHECK(cgpt_reset_accumulator(ctx));
            cgpt_render_params p{};
            p.width = W; p.height = H; p.row_begin = 0; p.row_end = H;
            p.first_sample = 0; p.n_samples = spp; p.seed = 0x12345678u + frame; p.kernel = CGPT_KERNEL_AUTO;
            CHECK(cgpt_render(ctx, &cam, &settings, &p));
            char name[64]; std::string err;
            CHECK(cgpt_read_pixels(ctx, px.data(), px.size())); CHECK(present(CGPT_TONEMAP_ACCUMULATOR, px, true));
            const char* tag = animate ? "animate" : crowd ? "crowd" : bend ? "bend" : "bulge";
            snprintf(name, sizeof(name), "%s_%02u_raw.ppm", tag, frame); WritePPM(name, px.data(), W, H, err);
            CHECK(cgpt_denoise(ctx, &cam, nullptr, nullptr, 0, px.data(), px.size())); CHECK(present(CGPT_TONEMAP_DENOISED, px, false));
            snprintf(name, sizeof(name), "%s_%02u_denoised.ppm", tag, frame); WritePPM(name, px.data(), W, H, err);
            CHECK(cgpt_denoise_temporal(ctx, &cam, nullptr, &tp, nullptr, 0, px.data(), px.size()));   // once per rendered frame
            CHECK(present(CGPT_TONEMAP_DENOISED, px, false));
            snprintf(name, sizeof(name), "%s_%02u_temporal.ppm", tag, frame); WritePPM(name, px.data(), W, H, err);
        }
        cgpt_ctx_destroy(ctx);
        return 0;
    }
    uint32_t num_accumulated = 0;                                        // data.num_accumulated
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> pixels((size_t)W * H), denoised(denoise ? (size_t)W * H : 0);
    const uint32_t chunk = preview_every ? preview_every : 16;           // Render() calls folded into one launch
    bool moved = false;
    for (uint32_t frame = 0; frame < spp; frame += chunk) {              // the frame loop
        if (move_at && !moved && frame >= move_at) {                     // Update(dt): camera input, then ResetAccumulator() if the view changed
            moved = true;
            if (scene.camera.Move(move_right, move_up, move_forward)) {
                CHECK(cgpt_reset_accumulator(ctx));
                num_accumulated = 0;
            }
        }
        cgpt_render_params p{};
        p.width = W; p.height = H; p.row_begin = 0; p.row_end = H;
        p.first_sample = num_accumulated; p.n_samples = spp - frame < chunk ? spp - frame : chunk;
        p.seed = 0x12345678u; p.kernel = CGPT_KERNEL_AUTO;
        CHECK(cgpt_render(ctx, &scene.camera.Abi(), &settings, &p));
        num_accumulated += p.n_samples;
        if (preview_every) {                                             // DX12::CopyToBackBuffer + Present
            CHECK(cgpt_read_pixels(ctx, pixels.data(), pixels.size())); CHECK(present(CGPT_TONEMAP_ACCUMULATOR, pixels, true));
            char name[64]; snprintf(name, sizeof(name), "preview_%04u.ppm", num_accumulated);
            std::string err; WritePPM(name, pixels.data(), W, H, err);
            if (denoise) {                                               // the "Denoise" toggle: the filtered image instead of data.pixels
                CHECK(cgpt_denoise(ctx, &scene.camera.Abi(), nullptr, nullptr, 0, denoised.data(), denoised.size())); CHECK(present(CGPT_TONEMAP_DENOISED, denoised, false));
                snprintf(name, sizeof(name), "preview_%04u_denoised.ppm", num_accumulated);
                WritePPM(name, denoised.data(), W, H, err);
                if (variance_guided) {
                    CHECK(cgpt_denoise_variance_guided(ctx, &scene.camera.Abi(), nullptr, nullptr, nullptr, nullptr, 0, denoised.data(), denoised.size())); CHECK(present(CGPT_TONEMAP_DENOISED, denoised, false));
                    snprintf(name, sizeof(name), "preview_%04u_variance_guided.ppm", num_accumulated);
                    WritePPM(name, denoised.data(), W, H, err);
                }
            }
        }
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    cgpt_stats st{};
    CHECK(cgpt_get_stats(ctx, &st));
    printf("%d GPU(s), %ux%u, %u spp (%u accumulated): %.1f ms/frame, %.1f Mrays/s, total energy %.3f\n", n_gpus, W, H, spp, num_accumulated, 1e3 * sec / spp,
           st.traced_rays / sec / 1e6, st.total_energy_received);

    std::vector<float> acc((size_t)W * H * 4);
    CHECK(cgpt_read_pixels(ctx, pixels.data(), pixels.size()));          // DX12::CopyToBackBuffer(data.pixels)
    CHECK(present(CGPT_TONEMAP_ACCUMULATOR, pixels, true));
    CHECK(cgpt_read_accumulator(ctx, acc.data(), acc.size()));
    std::string err;
    WritePPM("render.ppm", pixels.data(), W, H, err);
    WritePFM("render.pfm", acc.data(), num_accumulated, W, H, err);
    WriteAccumulator("render.acc", acc.data(), num_accumulated, W, H, err);
    if (denoise) {
        CHECK(cgpt_denoise(ctx, &scene.camera.Abi(), nullptr, nullptr, 0, denoised.data(), denoised.size())); CHECK(present(CGPT_TONEMAP_DENOISED, denoised, false));
        WritePPM("render_denoised.ppm", denoised.data(), W, H, err);
        if (variance_guided) {
            CHECK(cgpt_denoise_variance_guided(ctx, &scene.camera.Abi(), nullptr, nullptr, nullptr, nullptr, 0, denoised.data(), denoised.size())); CHECK(present(CGPT_TONEMAP_DENOISED, denoised, false));
            WritePPM("render_variance_guided.ppm", denoised.data(), W, H, err);
        }
    }
    cgpt_ctx_destroy(ctx);                                               // ThreadPool::Exit
    return 0;
}
