// pose_plan.hip -- PlanPoseBatch: the tables cgpt_scene_pose_objects walks (pose_plan.h), and cgpth_pose_batch_plan, which shows them
// to the CPU tests.  Host code only (no kernel, no HIP runtime call, no context); a .hip file because device_scene.h needs the HIP
// headers for float4.
#include "pose_plan.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <exception>

#include "cpugpupt_host.h"

namespace cgpt {
void HostSetError(const char* msg);                                           // host_capi.cpp: the text behind cgpth_last_error()

namespace {

int Refuse(std::string& error, const char* fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    error = buf;
    return CGPT_ERR_INVALID;
}

}  // namespace

int PlanPoseBatch(const std::vector<DevObject>& objects, const std::vector<RefitObject>& refit_objects, const std::vector<uint32_t>& mesh_group,
                  const PosePlanInput* in, uint32_t n, uint32_t skin_joints_lds, uint32_t morph_max_blocks, PosePlan& out, std::string& error)
{
    out = PosePlan();
    if (n == 0) return CGPT_OK;
    if (!in) return Refuse(error, "poses is null");
    if (morph_max_blocks == 0u) return Refuse(error, "morph_max_blocks 0");
    if (refit_objects.size() != objects.size() || mesh_group.size() != objects.size()) return Refuse(error, "the layout's per-object tables disagree");

    // one entry a copy: an object twice, or two placements of one instanced group (sequentially the last would win; in one launch they race)
    std::vector<int64_t> entry_of_group(objects.size(), -1);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t o = in[i].obj_index;
        if (o >= objects.size()) return Refuse(error, "entry %u: object %u out of range (%zu objects)", i, o, objects.size());
        if (objects[o].kind != CGPT_OBJECT_MESH && objects[o].kind != CGPT_OBJECT_TRIANGLE) return Refuse(error, "entry %u: object %u has no triangles to pose", i, o);
        if (in[i].n_joints == 0u && in[i].morphed == 0u) return Refuse(error, "entry %u: object %u is posed by neither a skin nor morph targets", i, o);
        int64_t& seen = entry_of_group[mesh_group[o]];
        if (seen >= 0) {
            const uint32_t first = in[seen].obj_index;
            if (first == o) return Refuse(error, "entries %u and %u both name object %u", (uint32_t)seen, i, o);
            return Refuse(error, "entries %u and %u name objects %u and %u of one instanced mesh group: they share one copy, which one pose writes", (uint32_t)seen, i, first, o);
        }
        seen = i;
    }

    // grouped by the instantiation the single call would launch, the caller's order kept within one
    std::vector<uint32_t> kernel(n), order(n);
    for (uint32_t i = 0; i < n; ++i) { kernel[i] = ChoosePoseKernel(in[i], skin_joints_lds); order[i] = i; }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return kernel[a] < kernel[b]; });

    out.entries.resize(n);
    uint64_t joints = 0, active = 0;
    uint32_t deepest = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const PosePlanInput& src = in[order[k]];
        const DevObject& d = objects[src.obj_index];
        const RefitObject& ro = refit_objects[src.obj_index];
        PosePlanEntry& e = out.entries[k];
        e = PosePlanEntry{};
        e.source = order[k]; e.obj_index = src.obj_index; e.kernel = kernel[order[k]];
        e.leaf_base = ro.leaf_base; e.tri_base = d.tri_base; e.n_tris = ro.tri_count;
        e.n_joints = src.n_joints; e.matrix_base = (uint32_t)joints;
        e.active_base = (uint32_t)active; e.n_active = src.morphed ? src.n_active : 0u;
        joints += e.n_joints; active += e.n_active;
        const uint32_t cap = src.morphed ? morph_max_blocks : kSkinMaxBlocks;
        e.blocks = std::max(1u, std::min((e.n_tris + kPoseThreads - 1) / kPoseThreads, cap));
        e.root_code = d.root_code; e.leaf_root = (d.root_code & kLeafBit) != 0u ? 1u : 0u;
        e.n_levels = ro.level_offsets.empty() ? 0u : (uint32_t)ro.level_offsets.size() - 1u;
        deepest = std::max(deepest, e.n_levels);
        if (joints > 0xFFFFFFFFull / 3 || active > 0xFFFFFFFFull) return Refuse(error, "the batch's joint matrices or active targets pass the 32-bit index range");
    }
    out.n_matrix_joints = (uint32_t)joints; out.n_active = (uint32_t)active;

    // triangle pass: one launch an instantiation in use, an entry's blocks side by side
    for (uint32_t k = 0; k < n;) {
        PosePlanLaunch l = { out.entries[k].kernel, k, 0u, 0u, 0u };
        uint64_t blocks = 0;
        for (; k < n && out.entries[k].kernel == l.kernel; ++k) {
            out.entries[k].first_block = (uint32_t)blocks;
            blocks += out.entries[k].blocks;
            l.max_joints = std::max(l.max_joints, out.entries[k].n_joints);
            ++l.n_entries;
        }
        if (blocks > 0x7FFFFFFFull) return Refuse(error, "the batch needs more than 2^31 blocks in one launch");
        l.n_blocks = (uint32_t)blocks;
        out.launches.push_back(l);
    }

    // bound pass: one launch a depth over every entry whose tree reaches it, deepest first; a thread a record, so a segment takes whole blocks
    for (uint32_t depth = deepest; depth-- > 0;) {
        PosePlanLevel lv = { depth, (uint32_t)out.segments.size(), 0u, 0u };
        uint64_t blocks = 0;
        for (const PosePlanEntry& e : out.entries) {
            if (e.n_levels <= depth) continue;
            const RefitObject& ro = refit_objects[e.obj_index];
            const uint32_t first = ro.level_offsets[depth], count = ro.level_offsets[depth + 1] - first;
            if (count == 0) continue;
            out.segments.push_back({ ro.level_begin + first, count, e.tri_base, (uint32_t)blocks });
            blocks += (count + kPoseThreads - 1) / kPoseThreads;
            ++lv.n_segments;
        }
        if (blocks > 0x7FFFFFFFull) return Refuse(error, "the batch needs more than 2^31 blocks in one launch");
        lv.n_blocks = (uint32_t)blocks;
        if (lv.n_segments != 0u) out.levels.push_back(lv);
    }
    return CGPT_OK;
}

}  // namespace cgpt

using namespace cgpt;

extern "C" int cgpth_pose_batch_plan(const cgpt_scene_desc* scene, int instanced, const uint32_t* batch, uint32_t n_entries, uint32_t skin_joints_lds,
                                     uint32_t morph_max_blocks, cgpth_pose_plan_view* view)
{
    static_assert(sizeof(PosePlanEntry) == 64 && sizeof(PosePlanLaunch) == 20 && sizeof(PosePlanSegment) == 16 && sizeof(PosePlanLevel) == 16, "rows of words, as cpugpupt_host.h documents them");
    struct Storage { SceneLayout layout; PosePlan plan; };
    thread_local Storage st;
    try {
        if (!scene || !view || (n_entries && !batch)) { HostSetError("null argument"); return CGPT_ERR_INVALID; }
        std::string error;
        int rc = LayoutScene(*scene, st.layout, error, instanced != 0);
        if (rc != CGPT_OK) { HostSetError(error.c_str()); return rc; }
        std::vector<PosePlanInput> in(n_entries);
        for (uint32_t i = 0; i < n_entries; ++i) in[i] = { batch[5 * i], batch[5 * i + 1], batch[5 * i + 2], batch[5 * i + 3], batch[5 * i + 4] };
        rc = PlanPoseBatch(st.layout.objects, st.layout.refit_objects, st.layout.mesh_group, in.data(), n_entries, skin_joints_lds, morph_max_blocks, st.plan, error);
        if (rc != CGPT_OK) { HostSetError(error.c_str()); return rc; }
        const PosePlan& p = st.plan;
        view->entries = reinterpret_cast<const uint32_t*>(p.entries.data()); view->n_entries = p.entries.size();
        view->launches = reinterpret_cast<const uint32_t*>(p.launches.data()); view->n_launches = p.launches.size();
        view->segments = reinterpret_cast<const uint32_t*>(p.segments.data()); view->n_segments = p.segments.size();
        view->levels = reinterpret_cast<const uint32_t*>(p.levels.data()); view->n_levels = p.levels.size();
        view->n_matrix_joints = p.n_matrix_joints; view->n_active = p.n_active;
        return CGPT_OK;
    } catch (const std::exception& e) {
        HostSetError(e.what());
        return CGPT_ERR_INVALID;
    }
}
