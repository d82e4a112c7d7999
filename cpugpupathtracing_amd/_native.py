"""ctypes view of libcpugpupt.so: the structs and prototypes of include/cpugpupt_abi.h and include/cpugpupt_host.h.

The library is the product; if it is missing or a symbol is absent this module raises -- there is no Python or CPU
fallback for the render path.
"""
from __future__ import annotations

import ctypes as C
import os

from ._paths import LIB_PATH

ABI_VERSION = 2
CGPT_OK, CGPT_ERR_INVALID, CGPT_ERR_HIP, CGPT_ERR_NO_SCENE, CGPT_ERR_UNSUPPORTED, CGPT_ERR_NO_DEVICE = range(6)
OBJECT_MESH, OBJECT_SPHERE, OBJECT_PLANE, OBJECT_TRIANGLE = 0, 1, 2, 3
MODE_COMPARISON, MODE_BRUTE_FORCE, MODE_ADVANCED = 0, 1, 2
DEBUG_NONE, DEBUG_RAY_DEPTH, DEBUG_BVH_DEPTH = 0, 1, 2
KERNEL_AUTO, KERNEL_MEGAKERNEL, KERNEL_WAVEFRONT, KERNEL_PERSISTENT = 0, 1, 2, 3
RENDER_COUNTERS = 1
CTX_FORCE_COLLECTIVE, CTX_GATHER_PEER_COPY = 1, 2
BUILD_NAIVE, BUILD_SAH_INTERVALS, BUILD_SAH_PRIMITIVES = 0, 1, 2
BUILD_SAH_BINNED = 3        # not in the reference: 16 bins per axis, stable partition (include/cpugpupt_abi.h)
DENOISE_DEMODULATE_ALBEDO = 1
TRACE_COUNTERS, TRACE_REVERSED = 1, 2
TEMPORAL_KEEP_VIEW_DEPENDENT = 1
TEMPORAL_FOLLOW_TRANSFORMS = 4
TEMPORAL_FOLLOW_POSES = 16
TEMPORAL_FOLLOW_MORPHS = 32
VARIANCE_TEMPORAL = 1
SKIN_MAX_JOINTS = 1024      # cgpt_scene_set_skin
MORPH_MAX_TARGETS = 256     # cgpt_scene_set_morph_targets
ANIM_PATH_TRANSLATION, ANIM_PATH_ROTATION, ANIM_PATH_SCALE = 0, 1, 2   # cgpt_clip_channel.path
ANIM_STEP, ANIM_LINEAR, ANIM_CUBICSPLINE = 0, 1, 2                     # cgpt_clip_channel.interpolation
ANIM_WRAP_CLAMP, ANIM_WRAP_LOOP, ANIM_WRAP_PINGPONG = 0, 1, 2          # cgpt_clip_layer.wrap
ANIM_MAX_LAYERS = 4
HIP_STREAM_LEGACY, HIP_STREAM_PER_THREAD = 1, 2   # hipStreamLegacy, hipStreamPerThread (hip_runtime_api.h): refused by cgpt_set_stream

f3 = C.c_float * 3


class Vertex(C.Structure):
    _fields_ = [("pos", f3), ("normal", f3)]


class Triangle(C.Structure):
    _fields_ = [("v0", Vertex), ("v1", Vertex), ("v2", Vertex)]


class BvhNode(C.Structure):
    _fields_ = [("aabb_min", f3), ("left_first", C.c_uint32), ("aabb_max", f3), ("prim_count", C.c_uint32)]


class Material(C.Structure):
    _fields_ = [("albedo", f3), ("specular", C.c_float), ("refractivity", C.c_float), ("absorption", f3),
                ("ior", C.c_float), ("emissive", f3), ("intensity", C.c_float), ("is_light", C.c_uint32)]


class Object(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("mat_index", C.c_uint32), ("node_offset", C.c_uint32), ("node_count", C.c_uint32),
                ("tri_offset", C.c_uint32), ("tri_count", C.c_uint32), ("max_depth", C.c_uint32), ("total_area", C.c_float),
                ("sphere_center", f3), ("sphere_radius", C.c_float), ("plane_normal", f3), ("plane_point", f3)]


class SceneDesc(C.Structure):
    _fields_ = [("objects", C.POINTER(Object)), ("n_objects", C.c_uint32),
                ("nodes", C.POINTER(BvhNode)), ("n_nodes", C.c_uint32),
                ("triangles", C.POINTER(Triangle)), ("n_triangles", C.c_uint32),
                ("tri_indices", C.POINTER(C.c_uint32)),
                ("materials", C.POINTER(Material)), ("n_materials", C.c_uint32),
                ("light_indices", C.POINTER(C.c_uint32)), ("n_lights", C.c_uint32)]


class Camera(C.Structure):
    _fields_ = [("pos", f3), ("top_left", f3), ("top_right", f3), ("bottom_left", f3)]


class Settings(C.Structure):
    _fields_ = [("max_ray_depth", C.c_int32), ("next_event_estimation_enabled", C.c_uint32),
                ("cosine_weighted_diffuse_reflection_enabled", C.c_uint32), ("russian_roulette_enabled", C.c_uint32),
                ("render_mode", C.c_uint32), ("debug_render_mode", C.c_uint32)]


class RenderParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("row_begin", C.c_uint32), ("row_end", C.c_uint32),
                ("first_sample", C.c_uint32), ("n_samples", C.c_uint32), ("seed", C.c_uint32), ("kernel", C.c_uint32),
                ("flags", C.c_uint32), ("interleave_rows", C.c_uint32), ("interleave_count", C.c_uint32),
                ("interleave_index", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("traced_rays", C.c_uint64), ("inner_steps", C.c_uint64), ("tri_tests", C.c_uint64),
                ("bvh_depth_sum", C.c_uint64), ("closest_hits", C.c_uint64), ("total_energy_received", C.c_double),
                ("num_accumulated", C.c_uint32), ("kernel_launches", C.c_uint32), ("kernel_ms", C.c_double),
                ("dominant_launches", C.c_uint32), ("dominant_waves_per_simd", C.c_uint32), ("dominant_ms", C.c_double),
                ("gather_ms", C.c_double), ("gathers", C.c_uint32), ("n_devices", C.c_uint32), ("rccl_ranks", C.c_uint32),
                ("last_kernel", C.c_uint32), ("device_ms", C.c_double * 8),
                ("dominant_round0_ms", C.c_double), ("dominant_round0_launches", C.c_uint32), ("chain_followers", C.c_uint32),
                ("probe_resolved", C.c_uint64)]
    retrace_unwalked = 0    # not a field of cgpt_stats (the struct keeps its size): Renderer.stats() fills it from cgpt_get_retrace_unwalked


class DenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("flags", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_position", C.c_float)]


class TemporalParams(C.Structure):
    _fields_ = [("max_history", C.c_float), ("normal_cos_min", C.c_float), ("plane_tolerance", C.c_float), ("flags", C.c_uint32)]


class VarianceParams(C.Structure):
    _fields_ = [("sigma_luminance", C.c_float), ("min_history_frames", C.c_uint32), ("flags", C.c_uint32)]


class ShadeSample(C.Structure):
    """cgpt_shade_sample: a traced ray with its hit record and the path state before the bounce (16 words)."""
    _fields_ = [("o", f3), ("d", f3), ("t", C.c_float), ("obj", C.c_uint32), ("tri", C.c_uint32), ("bvh_depth", C.c_uint32),
                ("throughput", f3), ("rng", C.c_uint32), ("depth", C.c_uint32), ("is_specular", C.c_uint32)]


class ShadeResult(C.Structure):
    """cgpt_shade_result: what one bounce left (28 words)."""
    _fields_ = [("flags", C.c_uint32), ("o", f3), ("d", f3), ("throughput", f3), ("energy", f3),
                ("rng", C.c_uint32), ("depth", C.c_uint32), ("is_specular", C.c_uint32),
                ("shadow_o", f3), ("shadow_d", f3), ("shadow_tmax", C.c_float), ("pending", f3),
                ("unwalked", C.c_uint32), ("reserved", C.c_uint32)]


class BvhInfo(C.Structure):
    _fields_ = [("num_triangles", C.c_uint32), ("nodes_used", C.c_uint32), ("num_leaves", C.c_uint32),
                ("max_leaf_size", C.c_uint32), ("max_depth", C.c_uint32), ("total_area", C.c_float)]


_vp = C.c_void_p
_fp = C.POINTER(C.c_float)
_up = C.POINTER(C.c_uint32)
_u16p = C.POINTER(C.c_uint16)


class SceneLayoutView(C.Structure):
    """cgpth_scene_layout_view: counts are elements (float4s for the float arrays, object_size bytes for objects)."""
    _fields_ = [("node_pairs", _fp), ("n_node_pairs", C.c_size_t), ("tri_leaf", _fp), ("n_tri_leaf", C.c_size_t),
                ("tri_orig", _fp), ("n_tri_orig", C.c_size_t), ("tri_normal", _fp), ("n_tri_normal", C.c_size_t),
                ("materials", _fp), ("n_materials", C.c_size_t), ("obj_trace", _fp), ("n_obj_trace", C.c_size_t),
                ("objects", _vp), ("n_objects", C.c_size_t), ("object_size", C.c_size_t),
                ("lights", _up), ("n_lights", C.c_size_t), ("refit_levels", _up), ("n_refit_levels", C.c_size_t),
                ("record_perm", _up), ("n_record_perm", C.c_size_t),
                ("stack_depth", C.c_uint32), ("n_top_records", C.c_uint32), ("n_pair_records", C.c_uint32), ("n_small_tris", C.c_uint32),
                ("leaf_base", _up), ("pair_base", _up), ("level_begin", _up), ("level_offsets", _up), ("level_offsets_start", _up),
                ("tri_normal12", _fp), ("n_tri_normal12", C.c_size_t),
                ("obj_xform", _fp), ("n_obj_xform", C.c_size_t)]


class PosePlanView(C.Structure):
    """cgpth_pose_plan_view: rows of 32-bit words -- entries 16, launches 5, segments 4, levels 4 a row"""
    _fields_ = [("entries", _up), ("n_entries", C.c_size_t), ("launches", _up), ("n_launches", C.c_size_t),
                ("segments", _up), ("n_segments", C.c_size_t), ("levels", _up), ("n_levels", C.c_size_t),
                ("n_matrix_joints", C.c_uint32), ("n_active", C.c_uint32)]


class RebuildPlanView(C.Structure):
    """cgpth_rebuild_plan_view"""
    _fields_ = [("members", _up), ("n_members", C.c_size_t), ("top_slots", _up), ("n_top_slots", C.c_size_t),
                ("level_offsets", _up), ("n_level_offsets", C.c_size_t), ("names", _up), ("n_names", C.c_size_t),
                ("record_perm", _up), ("n_record_perm", C.c_size_t),
                ("root_codes", _up), ("span_bases", _up), ("node_counts", _up), ("n_objects", C.c_size_t),
                ("span_base", C.c_uint32), ("level_begin", C.c_uint32), ("pair_base", C.c_uint32), ("leaf_base", C.c_uint32),
                ("n_nodes", C.c_uint32), ("n_pairs", C.c_uint32), ("max_depth", C.c_uint32), ("grow", C.c_uint32),
                ("n_pair_records", C.c_uint32), ("n_refit_levels", C.c_uint32), ("stack_depth", C.c_uint32), ("n_top_records", C.c_uint32)]


class Pose(C.Structure):
    """cgpt_pose: one entry of cgpt_scene_pose_objects"""
    _fields_ = [("obj_index", C.c_uint32), ("n_joints", C.c_uint32), ("joint_matrices", _fp), ("n_targets", C.c_uint32), ("weights", _fp)]


class SkeletonDesc(C.Structure):
    """cgpt_skeleton_desc"""
    _fields_ = [("parents", C.POINTER(C.c_int32)), ("inverse_bind", _fp), ("rest", _fp), ("root", _fp), ("n_joints", C.c_uint32)]


class ClipChannel(C.Structure):
    """cgpt_clip_channel"""
    _fields_ = [("joint", C.c_uint32), ("path", C.c_uint32), ("interpolation", C.c_uint32), ("n_keys", C.c_uint32),
                ("first_time", C.c_uint32), ("first_value", C.c_uint32)]


class ClipDesc(C.Structure):
    """cgpt_clip_desc"""
    _fields_ = [("n_joints", C.c_uint32), ("n_channels", C.c_uint32), ("channels", C.POINTER(ClipChannel)), ("times", _fp),
                ("n_times", C.c_uint32), ("values", _fp), ("n_values", C.c_uint32)]


class Animation(C.Structure):
    """cgpt_animation: one entry of cgpt_scene_animate_objects"""
    _fields_ = [("obj_index", C.c_uint32), ("clip", C.c_uint32), ("time", C.c_float), ("n_targets", C.c_uint32), ("weights", _fp)]


class ClipLayer(C.Structure):
    """cgpt_clip_layer: one clip of a blend, its time, weight and wrap mode"""
    _fields_ = [("clip", C.c_uint32), ("time", C.c_float), ("weight", C.c_float), ("wrap", C.c_uint32)]


class LayeredAnimation(C.Structure):
    """cgpt_layered_animation: one entry of cgpt_scene_animate_layers"""
    _fields_ = [("obj_index", C.c_uint32), ("n_layers", C.c_uint32), ("layers", C.POINTER(ClipLayer)), ("n_targets", C.c_uint32), ("weights", _fp)]


class SceneFootprint(C.Structure):
    """cgpt_scene_footprint"""
    _fields_ = [("device_bytes", C.c_uint64), ("n_objects", C.c_uint32), ("n_mesh_objects", C.c_uint32), ("n_mesh_copies", C.c_uint32),
                ("n_leaf_records", C.c_uint32), ("n_pair_records", C.c_uint32), ("n_orig_triangles", C.c_uint32)]


class TreeCost(C.Structure):
    """cgpt_tree_cost"""
    _fields_ = [("cost", C.c_double), ("root_half_area", C.c_double), ("n_inner", C.c_uint32), ("n_leaves", C.c_uint32),
                ("max_leaf_tris", C.c_uint32), ("reserved", C.c_uint32)]


class RebuildCandidate(C.Structure):
    """cgpt_rebuild_candidate: one entry of cgpt_scene_rebuild_degraded"""
    _fields_ = [("obj_index", C.c_uint32), ("reserved", C.c_uint32), ("reference_cost", C.c_double)]


class RebuildResult(C.Structure):
    """cgpt_rebuild_result"""
    _fields_ = [("cost_before", C.c_double), ("cost_after", C.c_double), ("rebuilt", C.c_uint32), ("reserved", C.c_uint32)]


TONEMAP_ACCUMULATOR, TONEMAP_DENOISED, TONEMAP_HOST = 0, 1, 2               # cgpt_tonemap_source
CURVE_CLAMP, CURVE_REINHARD, CURVE_ACES, CURVE_HABLE = 0, 1, 2, 3           # cgpt_tonemap_curve
TRANSFER_LINEAR, TRANSFER_SRGB = 0, 1                                       # cgpt_tonemap_transfer
TONEMAP_AUTO_EXPOSURE = 1                                                   # cgpt_tonemap_flags
EXPOSURE_ADAPTED, EXPOSURE_METERED = 1, 2                                   # cgpt_exposure_info.valid


class TonemapParams(C.Structure):
    """cgpt_tonemap_params"""
    _fields_ = [("source", C.c_uint32), ("curve", C.c_uint32), ("transfer", C.c_uint32), ("flags", C.c_uint32),
                ("exposure_scale", C.c_float), ("ev_bias", C.c_int32), ("white", C.c_float),
                ("key", C.c_float), ("low_fraction", C.c_float), ("high_fraction", C.c_float), ("alpha", C.c_float),
                ("src_rgba", C.POINTER(C.c_float)), ("src_width", C.c_uint32), ("src_height", C.c_uint32)]


class ExposureInfo(C.Structure):
    """cgpt_exposure_info"""
    _fields_ = [("mean_index", C.c_double), ("adapted_index", C.c_double), ("exposure", C.c_float), ("valid", C.c_uint32),
                ("n_counted", C.c_uint64), ("n_ignored", C.c_uint64), ("histogram", C.c_uint32 * 256)]


class ExposureState(C.Structure):
    """cgpth_exposure_state: what a context keeps between auto-exposure calls"""
    _fields_ = [("adapted_index", C.c_double), ("valid", C.c_uint32), ("reserved", C.c_uint32)]


class TopLevelView(C.Structure):
    """cgpth_top_level_view: n_nodes records of 8 floats {lo.xyz, bits(skip) | hi.xyz, bits(object)}, n_entry node indices."""
    _fields_ = [("nodes", _fp), ("n_nodes", C.c_size_t), ("entry", _up), ("n_entry", C.c_size_t)]


# name -> (restype, argtypes).  Every symbol declared in include/*.h is listed; tests check the list against the headers.
PROTOTYPES = {
    # cpugpupt_abi.h
    "cgpt_abi_version": (C.c_uint32, []),
    "cgpt_ctx_create": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_uint32, C.POINTER(_vp)]),
    "cgpt_ctx_destroy": (C.c_int, [_vp]),
    "cgpt_last_error": (C.c_char_p, [_vp]),
    "cgpt_set_stream": (C.c_int, [_vp, _vp]),
    "cgpt_set_nee_candidates": (C.c_int, [_vp, C.c_uint32]),
    "cgpt_set_top_level": (C.c_int, [_vp, C.c_uint32]),
    "cgpt_scene_upload": (C.c_int, [_vp, C.POINTER(SceneDesc)]),
    "cgpt_scene_upload_instanced": (C.c_int, [_vp, C.POINTER(SceneDesc)]),
    "cgpt_get_scene_footprint": (C.c_int, [_vp, C.POINTER(SceneFootprint)]),
    "cgpt_scene_update_materials": (C.c_int, [_vp, C.POINTER(Material), C.c_uint32]),
    "cgpt_scene_update_roughness": (C.c_int, [_vp, _fp, C.c_uint32]),
    "cgpt_scene_update_transmission_roughness": (C.c_int, [_vp, _fp, C.c_uint32]),
    "cgpt_scene_update_smooth_normals": (C.c_int, [_vp, _up, C.c_uint32]),
    "cgpt_scene_update_transforms": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_uint32]),
    "cgpt_scene_refit_mesh": (C.c_int, [_vp, C.c_uint32, C.POINTER(Triangle), C.c_uint32, _fp]),
    "cgpt_scene_rebuild_mesh": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _up, _up]),
    "cgpt_scene_export_bvh": (C.c_int, [_vp, C.c_uint32, C.POINTER(BvhNode), C.c_uint32]),
    "cgpt_scene_tree_costs": (C.c_int, [_vp, _up, C.c_uint32, C.c_double, C.c_double, C.POINTER(TreeCost)]),
    "cgpt_scene_rebuild_degraded": (C.c_int, [_vp, C.POINTER(RebuildCandidate), C.c_uint32, C.c_double, C.c_uint32, C.c_double, C.c_double,
                                              C.POINTER(RebuildResult)]),
    "cgpt_scene_update_primitive": (C.c_int, [_vp, C.c_uint32, C.POINTER(Object)]),
    "cgpt_scene_set_skin": (C.c_int, [_vp, C.c_uint32, C.POINTER(Triangle), _u16p, _fp, C.c_uint32, C.c_uint32]),
    "cgpt_scene_skin_mesh": (C.c_int, [_vp, C.c_uint32, _fp, C.c_uint32]),
    "cgpt_scene_clear_skin": (C.c_int, [_vp, C.c_uint32]),
    "cgpt_scene_set_morph_targets": (C.c_int, [_vp, C.c_uint32, C.POINTER(Triangle), C.POINTER(Triangle), C.c_uint32, C.c_uint32]),
    "cgpt_scene_morph_mesh": (C.c_int, [_vp, C.c_uint32, _fp, C.c_uint32]),
    "cgpt_scene_clear_morph_targets": (C.c_int, [_vp, C.c_uint32]),
    "cgpt_scene_pose_objects": (C.c_int, [_vp, C.POINTER(Pose), C.c_uint32]),
    "cgpt_scene_set_skeleton": (C.c_int, [_vp, C.c_uint32, C.POINTER(SkeletonDesc)]),
    "cgpt_clip_create": (C.c_int, [_vp, C.POINTER(ClipDesc), _up]),
    "cgpt_clip_destroy": (C.c_int, [_vp, C.c_uint32]),
    "cgpt_scene_animate_objects": (C.c_int, [_vp, C.POINTER(Animation), C.c_uint32]),
    "cgpt_scene_animate_layers": (C.c_int, [_vp, C.POINTER(LayeredAnimation), C.c_uint32]),
    "cgpt_clip_get_range": (C.c_int, [_vp, C.c_uint32, _fp, _fp]),
    "cgpt_scene_get_joint_matrices": (C.c_int, [_vp, C.c_uint32, _fp, C.c_uint32]),
    "cgpt_camera_from_view": (C.c_int, [_fp, _fp, C.c_float, C.c_float, C.POINTER(Camera)]),
    "cgpt_render": (C.c_int, [_vp, C.POINTER(Camera), C.POINTER(Settings), C.POINTER(RenderParams)]),
    "cgpt_reset_accumulator": (C.c_int, [_vp]),
    "cgpt_read_accumulator": (C.c_int, [_vp, _fp, C.c_size_t]),
    "cgpt_read_pixels": (C.c_int, [_vp, _up, C.c_size_t]),
    "cgpt_accumulator_device_ptr": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "cgpt_pixels_device_ptr": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "cgpt_get_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "cgpt_reset_stats": (C.c_int, [_vp]),
    "cgpt_get_retrace_unwalked": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "cgpt_intersect_rays": (C.c_int, [_vp, _fp, _fp, _fp, C.c_uint32, _fp, _up, _up, _up]),
    "cgpt_shade_samples": (C.c_int, [_vp, C.POINTER(Settings), C.POINTER(ShadeSample), C.c_uint32, C.POINTER(ShadeResult)]),
    "cgpt_trace_rays": (C.c_int, [_vp, _fp, _fp, _fp, C.c_uint32, _fp, _fp, _fp, C.c_uint32, C.c_uint32, _fp, _up, _up, _up, C.POINTER(C.c_uint8)]),
    "cgpt_trace_first_hits": (C.c_int, [_vp, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _up, _up, _up, _fp]),
    "cgpt_bvh_build": (C.c_int, [_vp, C.POINTER(Triangle), C.c_uint32, C.POINTER(BvhNode), _up, _up, _up, _fp]),
    "cgpt_bvh_build_ex": (C.c_int, [_vp, C.POINTER(Triangle), C.c_uint32, C.c_uint32, _up, C.POINTER(BvhNode), _up, _up, _up, _fp]),
    "cgpt_synchronize": (C.c_int, [_vp]),
    "cgpt_write_accumulator": (C.c_int, [_vp, C.POINTER(RenderParams), _fp, C.c_size_t, C.c_uint32]),
    "cgpt_set_tuning": (C.c_int, [_vp, C.c_char_p, C.c_uint32]),
    "cgpt_read_guides": (C.c_int, [_vp, C.POINTER(Camera), _fp, C.c_size_t]),
    "cgpt_denoise": (C.c_int, [_vp, C.POINTER(Camera), C.POINTER(DenoiseParams), _fp, C.c_size_t, _up, C.c_size_t]),
    "cgpt_denoise_temporal": (C.c_int, [_vp, C.POINTER(Camera), C.POINTER(DenoiseParams), C.POINTER(TemporalParams), _fp, C.c_size_t, _up,
                                        C.c_size_t]),
    "cgpt_temporal_reset": (C.c_int, [_vp]),
    "cgpt_read_temporal_history": (C.c_int, [_vp, _fp, C.c_size_t]),
    "cgpt_read_previous_hits": (C.c_int, [_vp, _fp, C.c_size_t]),
    "cgpt_denoise_variance_guided": (C.c_int, [_vp, C.POINTER(Camera), C.POINTER(DenoiseParams), C.POINTER(TemporalParams),
                                               C.POINTER(VarianceParams), _fp, C.c_size_t, _up, C.c_size_t]),
    "cgpt_read_variance": (C.c_int, [_vp, _fp, C.c_size_t]),
    "cgpt_tonemap": (C.c_int, [_vp, C.POINTER(TonemapParams), _fp, C.c_size_t, _up, C.c_size_t]),
    "cgpt_read_exposure": (C.c_int, [_vp, C.POINTER(ExposureInfo)]),
    "cgpt_exposure_reset": (C.c_int, [_vp]),
    "cgpt_measure_issue_rate": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    # cpugpupt_host.h
    "cgpth_last_error": (C.c_char_p, []),
    "cgpth_mesh_load_gltf": (_vp, [C.c_char_p]),
    "cgpth_mesh_from_arrays": (_vp, [C.POINTER(Vertex), C.c_uint32, _up, C.c_uint32]),
    "cgpth_mesh_dragon_standin": (_vp, [C.c_uint32]),
    "cgpth_mesh_bumpy_icosphere": (_vp, [C.c_uint32, _fp, _fp, C.c_float]),
    "cgpth_mesh_save_gltf": (C.c_int, [_vp, C.c_char_p]),
    "cgpth_mesh_num_vertices": (C.c_uint32, [_vp]),
    "cgpth_mesh_num_indices": (C.c_uint32, [_vp]),
    "cgpth_mesh_vertices": (C.POINTER(Vertex), [_vp]),
    "cgpth_mesh_indices": (_up, [_vp]),
    "cgpth_mesh_free": (None, [_vp]),
    "cgpth_scene_new": (_vp, []),
    "cgpth_scene_free": (None, [_vp]),
    "cgpth_scene_reference_layout": (_vp, [_vp, C.c_uint32, C.c_float, C.c_int]),
    "cgpth_scene_add_material": (C.c_int, [_vp, C.POINTER(Material)]),
    "cgpth_scene_set_material": (C.c_int, [_vp, C.c_uint32, C.POINTER(Material)]),
    "cgpth_scene_set_roughness": (C.c_int, [_vp, C.c_uint32, C.c_float]),
    "cgpth_scene_get_roughness": (C.c_int, [_vp, _fp, C.c_uint32]),
    "cgpth_scene_set_transmission_roughness": (C.c_int, [_vp, C.c_uint32, C.c_float]),
    "cgpth_scene_get_transmission_roughness": (C.c_int, [_vp, _fp, C.c_uint32]),
    "cgpth_scene_add_mesh": (C.c_int, [_vp, _vp, C.c_uint32, C.c_int]),
    "cgpth_scene_add_instance": (C.c_int, [_vp, C.c_uint32, C.c_uint32]),
    "cgpth_scene_add_mesh_device_built": (C.c_int, [_vp, _vp, C.c_uint32, _vp]),
    "cgpth_scene_add_mesh_device_built_ex": (C.c_int, [_vp, _vp, C.c_uint32, _vp, C.c_int]),
    "cgpth_scene_rebuild_bvh_device": (C.c_int, [_vp, C.c_uint32, C.c_int, _vp]),
    "cgpth_scene_add_sphere": (C.c_int, [_vp, _fp, C.c_float, C.c_uint32]),
    "cgpth_scene_add_plane": (C.c_int, [_vp, _fp, _fp, C.c_uint32]),
    "cgpth_scene_add_triangle": (C.c_int, [_vp, C.POINTER(Triangle), C.c_uint32]),
    "cgpth_scene_add_light": (C.c_int, [_vp, C.c_uint32]),
    "cgpth_scene_set_smooth_normals": (C.c_int, [_vp, C.c_uint32, C.c_uint32]),
    "cgpth_scene_get_smooth_normals": (C.c_int, [_vp, _up, C.c_uint32]),
    "cgpth_scene_set_transform": (C.c_int, [_vp, C.c_uint32, C.POINTER(C.c_float)]),
    "cgpth_scene_get_transforms": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_uint32]),
    "cgpth_scene_set_camera": (C.c_int, [_vp, _fp, _fp, C.c_float, C.c_float]),
    "cgpth_scene_set_settings": (C.c_int, [_vp, C.POINTER(Settings)]),
    "cgpth_scene_rebuild_bvh": (C.c_int, [_vp, C.c_uint32, C.c_int]),
    "cgpth_scene_refit_mesh": (C.c_int, [_vp, C.c_uint32, C.POINTER(Triangle), C.c_uint32]),
    "cgpth_skin_triangles": (C.c_int, [C.POINTER(Triangle), _u16p, _fp, C.c_uint32, _fp, C.c_uint32, C.POINTER(Triangle)]),
    "cgpth_scene_skin_mesh": (C.c_int, [_vp, C.c_uint32, C.POINTER(Triangle), _u16p, _fp, C.c_uint32, _fp, C.c_uint32]),
    "cgpth_morph_triangles": (C.c_int, [C.POINTER(Triangle), C.POINTER(Triangle), C.c_uint32, C.c_uint32, _fp, C.POINTER(Triangle)]),
    "cgpth_scene_morph_mesh": (C.c_int, [_vp, C.c_uint32, C.POINTER(Triangle), C.POINTER(Triangle), C.c_uint32, C.c_uint32, _fp]),
    "cgpth_animate_joints": (C.c_int, [C.POINTER(SkeletonDesc), C.POINTER(ClipDesc), C.c_float, _fp, C.c_uint32]),
    "cgpth_animate_layers": (C.c_int, [C.POINTER(SkeletonDesc), C.POINTER(ClipDesc), C.POINTER(ClipLayer), C.c_uint32, _fp, C.c_uint32]),
    "cgpth_clip_range": (C.c_int, [C.POINTER(ClipDesc), _fp, _fp]),
    "cgpth_wrap_time": (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_uint32, _fp]),
    "cgpth_scene_update_primitive": (C.c_int, [_vp, C.c_uint32, C.POINTER(Object)]),
    "cgpth_scene_bvh_info": (C.c_int, [_vp, C.c_uint32, C.POINTER(BvhInfo)]),
    "cgpth_scene_bvh_export": (C.c_int, [_vp, C.c_uint32, C.POINTER(BvhNode), _up]),
    "cgpth_tree_cost": (C.c_int, [C.POINTER(BvhNode), C.c_uint32, C.c_double, C.c_double, C.POINTER(TreeCost)]),
    "cgpth_luminance_bin": (C.c_int, [C.c_float]),
    "cgpth_tonemap": (C.c_int, [C.POINTER(TonemapParams), C.POINTER(ExposureState), _fp, C.c_size_t, _up, C.c_size_t, C.POINTER(ExposureInfo)]),
    "cgpth_scene_flatten": (C.c_int, [_vp, C.POINTER(SceneDesc)]),
    "cgpth_scene_get_camera": (C.c_int, [_vp, C.POINTER(Camera)]),
    "cgpth_scene_get_settings": (C.c_int, [_vp, C.POINTER(Settings)]),
    "cgpth_write_ppm": (C.c_int, [C.c_char_p, _up, C.c_uint32, C.c_uint32]),
    "cgpth_write_pfm": (C.c_int, [C.c_char_p, _fp, C.c_uint32, C.c_uint32, C.c_uint32]),
    "cgpth_write_accumulator": (C.c_int, [C.c_char_p, _fp, C.c_uint32, C.c_uint32, C.c_uint32]),
    "cgpth_read_accumulator": (C.c_int, [C.c_char_p, _fp, _up, C.c_uint32, C.c_uint32]),
    "cgpth_fast_div": (C.c_uint32, [C.c_uint32, C.c_uint32]),
    "cgpth_motion_records": (C.c_uint32, [_fp, C.c_uint32, _fp, C.c_uint32, _fp]),
    "cgpth_shade_item_blocks": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "cgpth_shade_segment_blocks": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "cgpth_scene_layout": (C.c_int, [C.POINTER(SceneDesc), C.POINTER(SceneLayoutView)]),
    "cgpth_scene_layout_instanced": (C.c_int, [C.POINTER(SceneDesc), C.POINTER(SceneLayoutView)]),
    "cgpth_scene_layout_transformed": (C.c_int, [C.POINTER(SceneDesc), C.POINTER(C.c_float), C.c_uint32, C.POINTER(SceneLayoutView)]),
    "cgpth_pose_batch_plan": (C.c_int, [C.POINTER(SceneDesc), C.c_int, _up, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(PosePlanView)]),
    "cgpth_rebuild_plan": (C.c_int, [C.POINTER(SceneDesc), C.c_int, C.c_uint32, _up, C.c_uint32, C.c_uint32, C.POINTER(RebuildPlanView)]),
    "cgpth_scene_permute_objects":(C.c_int, [_vp, _up, C.c_uint32]),
    "cgpth_top_level": (C.c_int, [C.POINTER(SceneDesc), C.POINTER(TopLevelView)]),
    "cgpth_top_level_transforms": (C.c_int, [C.POINTER(C.c_float), C.c_uint32, C.POINTER(TopLevelView)]),
    "cgpth_top_level_refit": (C.c_int, [C.c_uint32, C.POINTER(Triangle), C.c_uint32, C.POINTER(TopLevelView)]),
    "cgpth_top_level_primitive": (C.c_int, [C.c_uint32, C.POINTER(Object), C.POINTER(TopLevelView)]),
}

# exported for the tests, declared in csrc/device/ctx_internal.h: not part of the ABI that include/*.h declares
DEBUG_PROTOTYPES = {
    "cgpt_debug_live_device_bytes": (C.c_uint64, []),
}

_lib = None


class NativeLibraryError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Loads libcpugpupt.so (built in-tree by cpugpupathtracing_amd.build).  Fails loudly when absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} is missing: run `python -m cpugpupathtracing_amd.build` (hipcc, gfx950). "
            "There is no CPU or Python fallback for the render path.")
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in {**PROTOTYPES, **DEBUG_PROTOTYPES}.items():
        try:
            fn = getattr(L, name)
        except AttributeError as e:
            raise NativeLibraryError(f"{LIB_PATH} does not export {name}; rebuild it") from e
        fn.restype = restype
        fn.argtypes = argtypes
    if L.cgpt_abi_version() != ABI_VERSION:
        raise NativeLibraryError(f"ABI version mismatch: library reports {L.cgpt_abi_version()}, binding expects {ABI_VERSION}")
    _lib = L
    return L
