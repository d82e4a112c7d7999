// rebuild_layout.hip -- PlanRebuild and its companions (rebuild_layout.h), and cgpth_rebuild_plan, which shows them to the CPU tests.
// Host code only (no kernel, no HIP runtime call, no context); a .hip file because device_scene.h needs the HIP headers for float4.
#include "rebuild_layout.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <exception>

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

uint32_t RecordLevels(const RefitObject& ro) { return ro.level_offsets.empty() ? 0u : (uint32_t)ro.level_offsets.size() - 1u; }

}  // namespace

int PlanRebuild(const std::vector<DevObject>& objects, const std::vector<RefitObject>& refit_objects, const std::vector<uint32_t>& record_perm,
                const std::vector<uint32_t>& mesh_group, uint32_t n_top_records, uint32_t n_pair_records, uint32_t n_refit_levels,
                uint32_t obj_index, const std::vector<uint32_t>& level_first, RebuildPlan& out, std::string& error)
{
    out = RebuildPlan();
    if (refit_objects.size() != objects.size() || mesh_group.size() != objects.size()) return Refuse(error, CGPT_ERR_INVALID, "the layout's per-object tables disagree");
    if (obj_index >= objects.size() || objects[obj_index].kind != CGPT_OBJECT_MESH) return Refuse(error, CGPT_ERR_INVALID, "object %u is no mesh", obj_index);
    const RefitObject& old = refit_objects[obj_index];
    const uint32_t n_tris = old.tri_count;

    // the builder's levels: 0 = the root alone, every later level the children of the one before (an even count), closed by the node count
    if (level_first.size() < 2 || level_first[0] != 0u || level_first[1] != 1u) return Refuse(error, CGPT_ERR_INVALID, "level_first does not start with the root");
    for (size_t l = 1; l + 1 < level_first.size(); ++l)
        if (level_first[l + 1] <= level_first[l] || ((level_first[l + 1] - level_first[l]) & 1u) != 0u)
            return Refuse(error, CGPT_ERR_INVALID, "level %zu of the new tree holds %u nodes: not a positive even count", l, level_first[l + 1] - level_first[l]);
    const uint32_t n_nodes = level_first.back(), n_levels = (uint32_t)level_first.size() - 1u;   // node levels; the deepest node has depth n_levels - 1
    if (n_tris == 0u || n_nodes > 2u * n_tris - 1u) return Refuse(error, CGPT_ERR_INVALID, "%u nodes over %u triangles", n_nodes, n_tris);
    out.n_nodes = n_nodes; out.n_pairs = n_nodes / 2u; out.max_depth = n_levels - 1u;
    if (out.max_depth + 1u > 64u) return Refuse(error, CGPT_ERR_UNSUPPORTED, "BVH depth %u exceeds the traversal stack of 64 (ref: BVH.cpp:66)", out.max_depth);

    for (uint32_t j = 0; j < objects.size(); ++j)
        if (mesh_group[j] == mesh_group[obj_index]) out.members.push_back(j);

    // the top slots the mesh owns: its names below n_top_records
    const uint32_t old_pairs = old.node_count / 2u;
    if ((uint64_t)old.pair_base + old_pairs > record_perm.size()) return Refuse(error, CGPT_ERR_INVALID, "object %u: record_perm slice out of range", obj_index);
    for (uint32_t k = 0; k < old_pairs; ++k)
        if (record_perm[old.pair_base + k] < n_top_records) out.top_slots.push_back(record_perm[old.pair_base + k]);
    std::sort(out.top_slots.begin(), out.top_slots.end());

    RefitObject& ro = out.refit;
    ro = old;
    ro.node_count = n_nodes;
    const uint32_t room = n_tris - 1u;
    out.n_pair_records = n_pair_records; out.n_refit_levels = n_refit_levels; out.n_record_perm = (uint32_t)record_perm.size();
    if (old.span_base == kNoSpan) {
        // record byte offsets are computed in 32 bits on the device (LayoutMesh's limit)
        if ((uint64_t)n_pair_records + room >= (1u << 26)) return Refuse(error, CGPT_ERR_INVALID, "scene too large: more than 2^26 triangles or inner nodes");
        if ((uint64_t)n_refit_levels + room > 0xFFFFFFFFull || (uint64_t)record_perm.size() + room > 0xFFFFFFFFull) return Refuse(error, CGPT_ERR_INVALID, "scene too large: the record tables pass 2^32 entries");
        out.grow = 1u;
        ro.span_base = n_pair_records; ro.level_begin = n_refit_levels; ro.pair_base = (uint32_t)record_perm.size();
        out.n_pair_records += room; out.n_refit_levels += room; out.n_record_perm += room;
    }
    ro.level_offsets.clear();
    if (out.n_pairs != 0u)
        for (uint32_t d = 0; d < n_levels; ++d) ro.level_offsets.push_back((level_first[d + 1] - 1u) / 2u);   // d = n_levels - 1 closes it with n_pairs

    // stack_depth as the upload computes it: the deepest node of any mesh, plus one
    uint32_t deepest = RecordLevels(ro);
    for (uint32_t j = 0; j < objects.size(); ++j)
        if (mesh_group[j] != mesh_group[obj_index]) deepest = std::max(deepest, RecordLevels(refit_objects[j]));
    out.stack_depth = deepest + 1u;
    return CGPT_OK;
}

bool CheckTopRanks(const RebuildPlan& plan, const uint32_t* top_ranks, uint32_t n_top_ranks)
{
    if (n_top_ranks != std::min<size_t>(plan.top_slots.size(), plan.n_pairs) || (n_top_ranks && !top_ranks)) return false;
    std::vector<uint32_t> sorted(top_ranks, top_ranks + n_top_ranks);
    std::sort(sorted.begin(), sorted.end());
    for (uint32_t j = 0; j < n_top_ranks; ++j)
        if (sorted[j] >= plan.n_pairs || (j && sorted[j] == sorted[j - 1])) return false;
    return true;
}

void ApplyRebuildObjects(const RebuildPlan& plan, uint32_t root_code, std::vector<DevObject>& objects, std::vector<RefitObject>& refit_objects)
{
    for (const uint32_t j : plan.members) { refit_objects[j] = plan.refit; objects[j].root_code = root_code; }
}

void ApplyRebuildPerm(const RebuildPlan& plan, const uint32_t* top_ranks, uint32_t n_top_ranks, std::vector<uint32_t>& record_perm)
{
    if (plan.grow) record_perm.resize(plan.n_record_perm, 0xFFFFFFFFu);
    uint32_t* slice = record_perm.data() + plan.refit.pair_base;
    for (uint32_t k = 0; k < plan.n_pairs; ++k) slice[k] = plan.refit.span_base + k;
    for (uint32_t j = 0; j < n_top_ranks; ++j) slice[top_ranks[j]] = plan.top_slots[j];
}

}  // namespace cgpt

using namespace cgpt;

extern "C" int cgpth_rebuild_plan(const cgpt_scene_desc* scene, int instanced, uint32_t obj_index, const uint32_t* trees, uint32_t n_trees,
                                  uint32_t assume_pair_records, cgpth_rebuild_plan_view* view)
{
    struct Storage { SceneLayout layout; RebuildPlan plan; std::vector<uint32_t> slice, root_codes, span_bases, node_counts; };
    thread_local Storage st;
    try {
        if (!scene || !view || !trees || n_trees == 0u) { HostSetError("null argument or no tree"); return CGPT_ERR_INVALID; }
        std::string error;
        int rc = LayoutScene(*scene, st.layout, error, instanced != 0);
        if (rc != CGPT_OK) { HostSetError(error.c_str()); return rc; }
        SceneLayout& l = st.layout;
        uint32_t n_pair_records = assume_pair_records ? assume_pair_records : l.n_pair_records, n_refit_levels = (uint32_t)l.refit_levels.size();
        const uint32_t* w = trees;
        for (uint32_t t = 0; t < n_trees; ++t) {
            const uint32_t n_lf = *w++;
            const std::vector<uint32_t> level_first(w, w + n_lf); w += n_lf;
            const uint32_t n_ranks = *w++;
            const uint32_t* ranks = w; w += n_ranks;
            rc = PlanRebuild(l.objects, l.refit_objects, l.record_perm, l.mesh_group, l.n_top_records, n_pair_records, n_refit_levels, obj_index, level_first, st.plan, error);
            if (rc != CGPT_OK) { HostSetError(error.c_str()); return rc; }
            if (!CheckTopRanks(st.plan, ranks, n_ranks)) { HostSetError("the top ranks do not fit the plan"); return CGPT_ERR_INVALID; }
            ApplyRebuildObjects(st.plan, RebuildRootCode(st.plan, ranks, n_ranks), l.objects, l.refit_objects);
            ApplyRebuildPerm(st.plan, ranks, n_ranks, l.record_perm);
            st.slice.assign(l.record_perm.begin() + st.plan.refit.pair_base, l.record_perm.begin() + st.plan.refit.pair_base + st.plan.n_pairs);
            n_pair_records = st.plan.n_pair_records; n_refit_levels = st.plan.n_refit_levels; l.stack_depth = st.plan.stack_depth;
        }
        const RebuildPlan& p = st.plan;
        st.root_codes.clear(); st.span_bases.clear(); st.node_counts.clear();
        for (size_t j = 0; j < l.objects.size(); ++j) {
            st.root_codes.push_back(l.objects[j].root_code); st.span_bases.push_back(l.refit_objects[j].span_base); st.node_counts.push_back(l.refit_objects[j].node_count);
        }
        view->members = p.members.data(); view->n_members = p.members.size();
        view->top_slots = p.top_slots.data(); view->n_top_slots = p.top_slots.size();
        view->level_offsets = p.refit.level_offsets.data(); view->n_level_offsets = p.refit.level_offsets.size();
        view->names = st.slice.data(); view->n_names = st.slice.size();
        view->record_perm = l.record_perm.data(); view->n_record_perm = l.record_perm.size();
        view->root_codes = st.root_codes.data(); view->span_bases = st.span_bases.data(); view->node_counts = st.node_counts.data(); view->n_objects = l.objects.size();
        view->span_base = p.refit.span_base; view->level_begin = p.refit.level_begin; view->pair_base = p.refit.pair_base; view->leaf_base = p.refit.leaf_base;
        view->n_nodes = p.n_nodes; view->n_pairs = p.n_pairs; view->max_depth = p.max_depth; view->grow = p.grow;
        view->n_pair_records = p.n_pair_records; view->n_refit_levels = p.n_refit_levels; view->stack_depth = p.stack_depth; view->n_top_records = l.n_top_records;
        return CGPT_OK;
    } catch (const std::exception& e) {
        HostSetError(e.what());
        return CGPT_ERR_INVALID;
    }
}
