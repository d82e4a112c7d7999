// pose_plan.h -- the host half of cgpt_scene_pose_objects (refit.hip): which kernel instantiation poses each entry of a
// batch, which blocks of which launch belong to it, and which records of which entry every launch of the bound pass refits.  No HIP
// runtime call and no context, in the manner of scene_layout.h: refit.hip fills the device tables from the result, cgpth_pose_batch_plan
// (cpugpupt_host.h) shows it to the CPU tests.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "device_scene.h"
#include "scene_layout.h"

namespace cgpt {

constexpr uint32_t kPoseThreads = 256;          // a block of every pose kernel (refit.hip: kRefitThreads)
constexpr uint32_t kSkinMaxBlocks = 1024;       // the cap of skin_triangles' grid, 4 blocks a CU: per entry in a batch

// The instantiation that poses an entry: what the single call would launch for it.  kPoseSkin*: skin_triangles<LDS> (an object without
// morph targets); kPoseMorph*: morph_triangles<SKIN, LDS, LEAF>.
enum PoseKernel : uint32_t {
    kPoseSkin = 0, kPoseSkinLds, kPoseMorph, kPoseMorphLeaf, kPoseMorphSkin, kPoseMorphSkinLeaf, kPoseMorphSkinLds, kPoseMorphSkinLdsLeaf, kPoseKernels
};

// One entry of a batch as the planner takes it: the caller has resolved what the single calls would pose with
struct PosePlanInput {
    uint32_t obj_index;
    uint32_t n_joints;                          // the joints of the skin that takes part; 0: none does
    uint32_t morphed;                           // the object has morph targets ...
    uint32_t leaf_order;                        // ... stored in leaf-slot order (MorphBuffers::leaf_order)
    uint32_t n_active;                          // ... of which the pose's weights leave this many active
};

// An entry as the kernels see it, in launch order: grouped by instantiation, the caller's order kept within one (16 words)
struct PosePlanEntry {
    uint32_t source;                            // its index in the caller's array
    uint32_t obj_index, kernel;
    uint32_t leaf_base, tri_base, n_tris;       // RefitObject::leaf_base, DevObject::tri_base, RefitObject::tri_count
    uint32_t n_joints, matrix_base;             // its matrices start at joint matrix_base of the batch's packed matrix array
    uint32_t active_base, n_active;             // its slice of the batch's packed active table
    uint32_t first_block, blocks;               // blocks first_block .. first_block + blocks of its launch; they stride by `blocks`
    uint32_t root_code, leaf_root;              // DevObject::root_code; 1: no root record (a leaf-rooted mesh, a triangle object)
    uint32_t n_levels, pad;                     // the depth of its tree in child-pair records
};
struct PosePlanLaunch { uint32_t kernel, first_entry, n_entries, n_blocks, max_joints; };   // one launch of the triangle pass
struct PosePlanSegment { uint32_t records_begin, count, tri_base, first_block; };          // an entry's records of one depth: refit_levels[records_begin ..]
struct PosePlanLevel { uint32_t depth, first_segment, n_segments, n_blocks; };              // one launch of the bound pass

struct PosePlan {
    std::vector<PosePlanEntry> entries;
    std::vector<PosePlanLaunch> launches;       // ascending kernel; at most kPoseKernels
    std::vector<PosePlanSegment> segments;      // level by level
    std::vector<PosePlanLevel> levels;          // deepest first
    uint32_t n_matrix_joints = 0, n_active = 0; // the sizes of the two packed arrays
};

inline uint32_t ChoosePoseKernel(const PosePlanInput& in, uint32_t skin_joints_lds)
{
    const bool skinned = in.n_joints != 0u, lds = skin_joints_lds != 0u, leaf = in.leaf_order != 0u;
    if (!in.morphed) return lds ? kPoseSkinLds : kPoseSkin;
    if (!skinned) return leaf ? kPoseMorphLeaf : kPoseMorph;
    if (!lds) return leaf ? kPoseMorphSkinLeaf : kPoseMorphSkin;
    return leaf ? kPoseMorphSkinLdsLeaf : kPoseMorphSkinLds;
}

// The plan of a batch over an installed layout.  Refuses (CGPT_ERR_INVALID, the reason in `error`, naming the entries) an object out of
// range or without triangles, an entry that is neither skinned nor morphed, two entries that name one object, and two that name objects
// of one instanced mesh group (in one launch their writes would race).  skin_joints_lds and morph_max_blocks are the context's knobs.
int PlanPoseBatch(const std::vector<DevObject>& objects, const std::vector<RefitObject>& refit_objects, const std::vector<uint32_t>& mesh_group,
                  const PosePlanInput* in, uint32_t n, uint32_t skin_joints_lds, uint32_t morph_max_blocks, PosePlan& out, std::string& error);

}  // namespace cgpt
