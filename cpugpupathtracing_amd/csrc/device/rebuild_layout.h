// rebuild_layout.h -- the host half of cgpt_scene_rebuild_mesh (bvh_build.hip): where the records of a tree that the
// builder has just made go in the installed layout, and what the layout's bookkeeping becomes.  No HIP runtime call and no context, in
// the manner of pose_plan.h: bvh_build.hip writes the device records from the plan, cgpth_rebuild_plan (cpugpupt_host.h) shows it to the
// CPU tests, tests/rebuild_ref.py restates it in numpy.
//
// Record names (device_scene.h: "a record's index is only a name").  The builder's node array is level-ordered and every splitting node
// carries `rank`, its preorder rank among the splitting nodes -- the reference pair index (left_first - 1) / 2.
//   * span: at its first rebuild a mesh gets room for tri_count - 1 records at the end of node_pairs (a binary tree over n leaves of
//     at least one triangle has no more), and slices of the same length at the end of refit_levels and of record_perm.  Its old records
//     below n_top_records stay its own; the others are never read again (64 B each, once).  Later rebuilds reuse the three slices.
//   * the splitting node of rank k is named span_base + k, except for the first K splitting nodes of the level-ordered array, which
//     take the K top slots the mesh owns -- its names below n_top_records (the trace kernels mirror those records in LDS), in
//     ascending order.  A tree with fewer than K splitting nodes leaves the other slots as they are and the mesh gives them up.
//   * refit_levels: the records of depth d are the splitting nodes of the builder's level d; the children of level L are exactly
//     level L + 1, so level_offsets[d] = (level_first[d + 1] - 1) / 2.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "device_scene.h"
#include "scene_layout.h"

namespace cgpt {

struct RebuildPlan {
    std::vector<uint32_t> members;              // the objects of obj_index's mesh group, ascending: each takes `refit` and the root code
    std::vector<uint32_t> top_slots;            // the K names below n_top_records the mesh owns, ascending
    RefitObject refit;                          // the group's new RefitObject
    uint32_t n_nodes = 0, n_pairs = 0, max_depth = 0;
    uint32_t grow = 0;                          // 1: the first rebuild -- node_pairs, refit_levels and record_perm grow by tri_count - 1
    uint32_t n_pair_records = 0, n_refit_levels = 0, n_record_perm = 0;   // the sizes of the three afterwards
    uint32_t stack_depth = 0;                   // DevScene::stack_depth afterwards, as the upload computes it
};

// The plan of a rebuild of mesh obj_index whose new tree has the builder's level ranges level_first (level L = nodes
// [level_first[L], level_first[L + 1]), closed by the node count).  The caller has checked that obj_index is a mesh.
// n_pair_records / n_refit_levels: the current record counts of node_pairs and refit_levels.
// CGPT_ERR_UNSUPPORTED: the tree is deeper than the traversal stack; CGPT_ERR_INVALID: the span would pass 2^26 records.
int PlanRebuild(const std::vector<DevObject>& objects, const std::vector<RefitObject>& refit_objects, const std::vector<uint32_t>& record_perm,
                const std::vector<uint32_t>& mesh_group, uint32_t n_top_records, uint32_t n_pair_records, uint32_t n_refit_levels,
                uint32_t obj_index, const std::vector<uint32_t>& level_first, RebuildPlan& out, std::string& error);

// The names of the new tree's records, given the ranks of the first min(K, n_pairs) splitting nodes of the level-ordered array in slot
// order (what the device reads back): the splitting node of rank k is named RebuildName(plan, ranks, n, k).  CheckTopRanks: false for a
// count that does not fit the plan, a rank out of range or one given twice (work in K <= kTopRecords, not in the node count).
bool CheckTopRanks(const RebuildPlan& plan, const uint32_t* top_ranks, uint32_t n_top_ranks);
inline uint32_t RebuildName(const RebuildPlan& plan, const uint32_t* top_ranks, uint32_t n_top_ranks, uint32_t rank)
{
    for (uint32_t j = 0; j < n_top_ranks; ++j)
        if (top_ranks[j] == rank) return plan.top_slots[j];
    return plan.refit.span_base + rank;
}

// The traversal code of the new root: the name of rank 0, or the mesh's first leaf slot for a tree of one node
inline uint32_t RebuildRootCode(const RebuildPlan& plan, const uint32_t* top_ranks, uint32_t n_top_ranks)
{
    return plan.n_pairs == 0u ? (kLeafBit | plan.refit.leaf_base) : RebuildName(plan, top_ranks, n_top_ranks, 0u);
}

// The bookkeeping after the rebuild, in two parts so that a caller can keep what may throw in front of its first device write.
// ApplyRebuildObjects: every member's RefitObject and root code.  ApplyRebuildPerm: the mesh's record_perm slice in place, grown first if
// the plan says so (reserve plan.n_record_perm beforehand and it cannot throw) -- one pass over the mesh's own n_pairs entries.  With
// PlanRebuild's look through the old slice for the top slots it is all the host work of a rebuild that grows with a node count, and
// it grows with this mesh's, not with the scene's.
void ApplyRebuildObjects(const RebuildPlan& plan, uint32_t root_code, std::vector<DevObject>& objects, std::vector<RefitObject>& refit_objects);
void ApplyRebuildPerm(const RebuildPlan& plan, const uint32_t* top_ranks, uint32_t n_top_ranks, std::vector<uint32_t>& record_perm);

}  // namespace cgpt
