// host_capi.cpp -- C entry points of the host mirror (include/cpugpupt_host.h).
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "cpugpupt_host.h"
#include "fast_div.h"
#include "animation.h"
#include "gltf_loader.h"
#include "image_io.h"
#include "mesh_gen.h"
#include "morph.h"
#include "scene.h"
#include "shade_items.h"
#include "skinning.h"
#include "transform_math.h"
#include "tree_cost.h"

using namespace cgpt;

struct cgpth_mesh { Mesh mesh; };
struct cgpth_scene {
    Scene scene;
    Scene::FlatStorage flat;
};

namespace {
thread_local std::string g_error;
int Fail(const std::string& msg) { g_error = msg; return CGPT_ERR_INVALID; }
Vec3 V(const float p[3]) { return { p[0], p[1], p[2] }; }

Material FromAbi(const cgpt_material& m)
{
    Material out;
    out.albedo = V(m.albedo); out.specular = m.specular; out.refractivity = m.refractivity;
    out.absorption = V(m.absorption); out.ior = m.ior; out.emissive = V(m.emissive);
    out.intensity = m.intensity; out.is_light = m.is_light != 0;
    return out;
}
bool ValidOption(int o) { return o >= 0 && o < MeshBVH::BuildOption_NumOptions; }

// Nothing may unwind through the C ABI: a corrupt file or an allocation failure inside the C++ mirror (std::bad_alloc,
// std::length_error) becomes an error status and a message, never std::terminate in the host application.
template <class R, class F>
R Guarded(R on_error, F&& body) noexcept
{
    try {
        return body();
    } catch (const std::exception& e) {
        try { g_error = std::string("exception in the host mirror: ") + e.what(); } catch (...) {}
    } catch (...) {
        try { g_error = "unknown exception in the host mirror"; } catch (...) {}
    }
    return on_error;
}
}  // namespace

namespace cgpt {
// for cgpth_scene_layout, the one entry point of cpugpupt_host.h that lives beside the device code (csrc/device/scene_layout.hip)
void HostSetError(const char* msg) { try { g_error = msg; } catch (...) {} }
}  // namespace cgpt

extern "C" {

const char* cgpth_last_error(void) { return g_error.c_str(); }

cgpth_mesh* cgpth_mesh_load_gltf(const char* path)
{
    return Guarded<cgpth_mesh*>(nullptr, [&]() -> cgpth_mesh* {
        if (!path) { Fail("null path"); return nullptr; }
        cgpth_mesh* m = new (std::nothrow) cgpth_mesh;
        if (!m) { Fail("out of memory"); return nullptr; }
        std::string err;
        if (!GLTFLoader::Load(path, m->mesh, err)) { Fail(err); delete m; return nullptr; }
        return m;
    });
}

cgpth_mesh* cgpth_mesh_from_arrays(const cgpt_vertex* vertices, uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices)
{
    return Guarded<cgpth_mesh*>(nullptr, [&]() -> cgpth_mesh* {
        if ((!vertices && n_vertices) || (!indices && n_indices)) { Fail("null array"); return nullptr; }
        cgpth_mesh* m = new (std::nothrow) cgpth_mesh;
        if (!m) { Fail("out of memory"); return nullptr; }
        m->mesh.vertices.assign(vertices, vertices + n_vertices);
        m->mesh.indices.assign(indices, indices + n_indices);
        return m;
    });
}

cgpth_mesh* cgpth_mesh_dragon_standin(uint32_t level)
{
    return Guarded<cgpth_mesh*>(nullptr, [&]() -> cgpth_mesh* {
        if (level > 9) { Fail("icosphere level > 9 (5.2 M triangles) refused"); return nullptr; }
        cgpth_mesh* m = new (std::nothrow) cgpth_mesh;
        if (!m) { Fail("out of memory"); return nullptr; }
        m->mesh = MakeDragonStandIn(level);
        return m;
    });
}

cgpth_mesh* cgpth_mesh_bumpy_icosphere(uint32_t level, const float center[3], const float radii[3], float bump)
{
    return Guarded<cgpth_mesh*>(nullptr, [&]() -> cgpth_mesh* {
        if (level > 9 || !center || !radii) { Fail("bad icosphere arguments"); return nullptr; }
        cgpth_mesh* m = new (std::nothrow) cgpth_mesh;
        if (!m) { Fail("out of memory"); return nullptr; }
        m->mesh = MakeBumpyIcosphere(level, center, radii, bump);
        return m;
    });
}

int cgpth_mesh_save_gltf(const cgpth_mesh* mesh, const char* gltf_path)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!mesh || !gltf_path) return Fail("null argument");
        std::string err;
        if (!GLTFLoader::Save(gltf_path, mesh->mesh, err)) return Fail(err);
        return CGPT_OK;
    });
}

uint32_t cgpth_mesh_num_vertices(const cgpth_mesh* mesh) { return mesh ? (uint32_t)mesh->mesh.vertices.size() : 0; }
uint32_t cgpth_mesh_num_indices(const cgpth_mesh* mesh) { return mesh ? (uint32_t)mesh->mesh.indices.size() : 0; }
const cgpt_vertex* cgpth_mesh_vertices(const cgpth_mesh* mesh) { return mesh ? mesh->mesh.vertices.data() : nullptr; }
const uint32_t* cgpth_mesh_indices(const cgpth_mesh* mesh) { return mesh ? mesh->mesh.indices.data() : nullptr; }
void cgpth_mesh_free(cgpth_mesh* mesh) { delete mesh; }

cgpth_scene* cgpth_scene_new(void)
{
    return Guarded<cgpth_scene*>(nullptr, [&]() -> cgpth_scene* {
        cgpth_scene* s = new (std::nothrow) cgpth_scene;
        if (!s) Fail("out of memory");
        return s;
    });
}
void cgpth_scene_free(cgpth_scene* scene) { delete scene; }

cgpth_scene* cgpth_scene_reference_layout(const cgpth_mesh* mesh, uint32_t mesh_material, float aspect, int build_option)
{
    return Guarded<cgpth_scene*>(nullptr, [&]() -> cgpth_scene* {
        if (!mesh || !ValidOption(build_option) || mesh_material > 3) { Fail("bad argument to cgpth_scene_reference_layout"); return nullptr; }
        cgpth_scene* s = cgpth_scene_new();
        if (!s) return nullptr;
        s->scene = MakeReferenceScene(mesh->mesh, mesh_material, aspect, (MeshBVH::BuildOption)build_option);
        if (!s->scene.objects[0].valid) { Fail("mesh is empty or has out-of-range indices"); delete s; return nullptr; }
        return s;
    });
}

int cgpth_scene_add_material(cgpth_scene* scene, const cgpt_material* material)
{
    return Guarded<int>(-CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !material) return -Fail("null argument");
        scene->scene.materials.push_back(FromAbi(*material));
        return (int)scene->scene.materials.size() - 1;
    });
}

int cgpth_scene_set_material(cgpth_scene* scene, uint32_t index, const cgpt_material* material)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !material || index >= scene->scene.materials.size()) return Fail("bad material index");
        const float roughness = scene->scene.materials[index].roughness;
        const float transmission_roughness = scene->scene.materials[index].transmission_roughness;
        scene->scene.materials[index] = FromAbi(*material);
        scene->scene.materials[index].roughness = roughness;
        scene->scene.materials[index].transmission_roughness = transmission_roughness;
        return CGPT_OK;
    });
}

int cgpth_scene_set_roughness(cgpth_scene* scene, uint32_t index, float roughness)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || index >= scene->scene.materials.size()) return Fail("bad material index");
        if (!(roughness >= 0.0f && roughness <= 1.0f)) return Fail("roughness " + std::to_string(roughness) + " outside [0, 1]");
        scene->scene.materials[index].roughness = roughness;
        return CGPT_OK;
    });
}

int cgpth_scene_get_roughness(const cgpth_scene* scene, float* out, uint32_t n)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !out) return Fail("null argument");
        if (n != scene->scene.materials.size()) return Fail("expected " + std::to_string(scene->scene.materials.size()) + " values, got " + std::to_string(n));
        for (uint32_t i = 0; i < n; ++i) out[i] = scene->scene.materials[i].roughness;
        return CGPT_OK;
    });
}

int cgpth_scene_set_transmission_roughness(cgpth_scene* scene, uint32_t index, float roughness)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || index >= scene->scene.materials.size()) return Fail("bad material index");
        if (!(roughness >= 0.0f && roughness <= 1.0f)) return Fail("transmission roughness " + std::to_string(roughness) + " outside [0, 1]");
        scene->scene.materials[index].transmission_roughness = roughness;
        return CGPT_OK;
    });
}

int cgpth_scene_get_transmission_roughness(const cgpth_scene* scene, float* out, uint32_t n)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !out) return Fail("null argument");
        if (n != scene->scene.materials.size()) return Fail("expected " + std::to_string(scene->scene.materials.size()) + " values, got " + std::to_string(n));
        for (uint32_t i = 0; i < n; ++i) out[i] = scene->scene.materials[i].transmission_roughness;
        return CGPT_OK;
    });
}

int cgpth_scene_add_mesh(cgpth_scene* scene, const cgpth_mesh* mesh, uint32_t mat_index, int build_option)
{
    return Guarded<int>(-CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !mesh || !ValidOption(build_option)) return -Fail("bad argument to cgpth_scene_add_mesh");
        scene->scene.objects.emplace_back("mesh", mesh->mesh, mat_index, (MeshBVH::BuildOption)build_option);
        if (!scene->scene.objects.back().valid) {
            scene->scene.objects.pop_back();
            return -Fail(build_option == MeshBVH::BuildOption_SAHBinned ? "mesh is empty, has out-of-range indices, or a position is not finite or beyond 1e30"
                                                                         : "mesh is empty or has out-of-range indices");
        }
        return (int)scene->scene.objects.size() - 1;
    });
}

int cgpth_scene_add_instance(cgpth_scene* scene, uint32_t of_obj_index, uint32_t mat_index)
{
    return Guarded<int>(-CGPT_ERR_INVALID, [&]() -> int {
        if (!scene) return -Fail("scene is null");
        if (of_obj_index >= scene->scene.objects.size())
            return -Fail("object " + std::to_string(of_obj_index) + " out of range (" + std::to_string(scene->scene.objects.size()) + " objects)");
        if (!scene->scene.objects[of_obj_index].has_bvh) {
            const Object& of = scene->scene.objects[of_obj_index];
            const char* kind = of.kind == CGPT_OBJECT_SPHERE ? "sphere" : of.kind == CGPT_OBJECT_PLANE ? "plane" : "triangle object";
            return -Fail("object " + std::to_string(of_obj_index) + " is a " + kind + ": only a mesh has instances");
        }
        Object instance("mesh instance", scene->scene.objects[of_obj_index], mat_index);   // built first: emplace_back may move the original
        scene->scene.objects.push_back(std::move(instance));
        return (int)scene->scene.objects.size() - 1;
    });
}

// the device builder behind MeshBVH::BuildWith / RebuildWith: cgpt_bvh_build_ex on ctx; keeps the device's message
static MeshBVH::TreeBuilder DeviceBuilder(cgpt_ctx* ctx, std::string& device_error)
{
    return [ctx, &device_error](const cgpt_triangle* tris, uint32_t n, int option, const uint32_t* initial, cgpt_bvh_node* nodes, uint32_t* n_nodes,
                                uint32_t* tri_indices, uint32_t* depth) {
        float area = 0.0f;
        if (cgpt_bvh_build_ex(ctx, tris, n, (uint32_t)option, initial, nodes, n_nodes, tri_indices, depth, &area) == CGPT_OK) return true;
        device_error = cgpt_last_error(ctx);
        return false;
    };
}

int cgpth_scene_add_mesh_device_built_ex(cgpth_scene* scene, const cgpth_mesh* mesh, uint32_t mat_index, cgpt_ctx* ctx, int build_option)
{
    return Guarded<int>(-CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !mesh || !ctx || !ValidOption(build_option)) return -Fail("bad argument to cgpth_scene_add_mesh_device_built");
        std::string device_error;
        scene->scene.objects.emplace_back("mesh", mesh->mesh, mat_index, (MeshBVH::BuildOption)build_option, DeviceBuilder(ctx, device_error));
        if (!scene->scene.objects.back().valid) {
            scene->scene.objects.pop_back();
            return -Fail(device_error.empty() ? std::string("mesh is empty, has out-of-range indices, or the device returned a malformed tree")
                                              : "device BVH build failed: " + device_error);
        }
        return (int)scene->scene.objects.size() - 1;
    });
}

int cgpth_scene_add_mesh_device_built(cgpth_scene* scene, const cgpth_mesh* mesh, uint32_t mat_index, cgpt_ctx* ctx)
{
    return cgpth_scene_add_mesh_device_built_ex(scene, mesh, mat_index, ctx, (int)MeshBVH::BuildOption_SAHSplitIntervals);
}

int cgpth_scene_rebuild_bvh_device(cgpth_scene* scene, uint32_t obj_index, int build_option, cgpt_ctx* ctx)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !ctx || obj_index >= scene->scene.objects.size() || !scene->scene.objects[obj_index].has_bvh || !ValidOption(build_option))
            return Fail("bad argument to cgpth_scene_rebuild_bvh_device");
        std::string device_error;
        if (!scene->scene.objects[obj_index].bvh->RebuildWith((MeshBVH::BuildOption)build_option, DeviceBuilder(ctx, device_error)))
            return Fail(device_error.empty() ? std::string("the device returned a malformed tree (the BVH is unchanged)") : "device BVH rebuild failed: " + device_error);
        return CGPT_OK;
    });
}

int cgpth_scene_add_sphere(cgpth_scene* scene, const float center[3], float radius, uint32_t mat_index)
{
    return Guarded<int>(-CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !center) return -Fail("null argument");
        scene->scene.objects.emplace_back("sphere", Sphere{ V(center), radius }, mat_index);
        return (int)scene->scene.objects.size() - 1;
    });
}

int cgpth_scene_add_plane(cgpth_scene* scene, const float normal[3], const float point[3], uint32_t mat_index)
{
    return Guarded<int>(-CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !normal || !point) return -Fail("null argument");
        scene->scene.objects.emplace_back("plane", Plane{ V(normal), V(point) }, mat_index);
        return (int)scene->scene.objects.size() - 1;
    });
}

int cgpth_scene_add_triangle(cgpth_scene* scene, const cgpt_triangle* triangle, uint32_t mat_index)
{
    return Guarded<int>(-CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !triangle) return -Fail("null argument");
        scene->scene.objects.emplace_back("triangle", *triangle, mat_index);
        return (int)scene->scene.objects.size() - 1;
    });
}

static const char* KindName(const Object& o)
{
    return o.has_bvh ? "mesh" : o.kind == CGPT_OBJECT_SPHERE ? "sphere" : o.kind == CGPT_OBJECT_PLANE ? "plane" : "triangle object";
}

int cgpth_scene_add_light(cgpth_scene* scene, uint32_t obj_index)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || obj_index >= scene->scene.objects.size()) return Fail("bad object index");
        const Object& o = scene->scene.objects[obj_index];
        // ref: Main.cpp:371-384: only meshes and sphere primitives can be sampled, anything else EXCEPTs
        if (!o.has_bvh && o.kind != CGPT_OBJECT_SPHERE) { g_error = "only meshes and spheres can be light sources"; return CGPT_ERR_UNSUPPORTED; }
        if (o.smooth) return Fail("object " + std::to_string(obj_index) + " has smooth normals: a light's sampled normal is v0.normal");
        if (!IsIdentityTransform(o.transform)) return Fail("object " + std::to_string(obj_index) + " has a transform: a light is sampled in object space");
        scene->scene.light_source_indices.push_back(obj_index);
        return CGPT_OK;
    });
}

int cgpth_scene_permute_objects(cgpth_scene* scene, const uint32_t* order, uint32_t n_objects)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !order || n_objects != scene->scene.objects.size()) return Fail("expected one index per object");
        std::vector<uint32_t> new_index(n_objects, 0xFFFFFFFFu);
        for (uint32_t k = 0; k < n_objects; ++k) {
            if (order[k] >= n_objects || new_index[order[k]] != 0xFFFFFFFFu) return Fail("order is not a permutation of the object indices");
            new_index[order[k]] = k;
        }
        auto& objects = scene->scene.objects;
        std::remove_reference_t<decltype(objects)> moved;
        moved.reserve(n_objects);
        for (uint32_t k = 0; k < n_objects; ++k) moved.push_back(std::move(objects[order[k]]));   // smooth flag and transform travel inside the object
        objects.swap(moved);
        for (auto& li : scene->scene.light_source_indices) li = new_index[li];
        return CGPT_OK;
    });
}

int cgpth_scene_set_smooth_normals(cgpth_scene* scene, uint32_t obj_index, uint32_t flag)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene) return Fail("scene is null");
        if (obj_index >= scene->scene.objects.size())
            return Fail("object " + std::to_string(obj_index) + " out of range (" + std::to_string(scene->scene.objects.size()) + " objects)");
        if (flag > 1u) return Fail("smooth-normal flag " + std::to_string(flag) + " is neither 0 nor 1");
        if (flag)
            for (const uint32_t li : scene->scene.light_source_indices)
                if (li == obj_index) return Fail("object " + std::to_string(obj_index) + " is a light: its sampled normal is v0.normal, so it cannot shade with smooth normals");
        scene->scene.objects[obj_index].smooth = flag != 0u;
        return CGPT_OK;
    });
}

int cgpth_scene_get_smooth_normals(const cgpth_scene* scene, uint32_t* out, uint32_t n)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !out) return Fail("null argument");
        if (n != scene->scene.objects.size()) return Fail("expected " + std::to_string(scene->scene.objects.size()) + " values, got " + std::to_string(n));
        for (uint32_t i = 0; i < n; ++i) out[i] = scene->scene.objects[i].smooth ? 1u : 0u;
        return CGPT_OK;
    });
}

int cgpth_scene_set_transform(cgpth_scene* scene, uint32_t obj_index, const float object_to_world[12])
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !object_to_world) return Fail("null argument");
        if (obj_index >= scene->scene.objects.size())
            return Fail("object " + std::to_string(obj_index) + " out of range (" + std::to_string(scene->scene.objects.size()) + " objects)");
        Object& o = scene->scene.objects[obj_index];
        if (!IsIdentityTransform(object_to_world)) {
            float inverse[12];
            if (!InvertTransform(object_to_world, inverse)) return Fail("object " + std::to_string(obj_index) + ": the transform is not finite or cannot be inverted in float range");
            if (!o.has_bvh && o.kind != CGPT_OBJECT_TRIANGLE)
                return Fail("object " + std::to_string(obj_index) + " is a " + KindName(o) + ": it takes no transform (update_primitive moves it)");
            for (const uint32_t li : scene->scene.light_source_indices)
                if (li == obj_index) return Fail("object " + std::to_string(obj_index) + " is a light: it is sampled in object space, so it takes no transform");
        }
        memcpy(o.transform, object_to_world, sizeof(o.transform));
        return CGPT_OK;
    });
}

int cgpth_scene_get_transforms(const cgpth_scene* scene, float* out, uint32_t n)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !out) return Fail("null argument");
        if (n != scene->scene.objects.size()) return Fail("expected " + std::to_string(scene->scene.objects.size()) + " matrices, got " + std::to_string(n));
        for (uint32_t i = 0; i < n; ++i) memcpy(out + 12 * (size_t)i, scene->scene.objects[i].transform, sizeof(float) * 12);
        return CGPT_OK;
    });
}

int cgpth_scene_set_camera(cgpth_scene* scene, const float pos[3], const float view_dir[3], float fov_deg, float aspect)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !pos || !view_dir) return Fail("null argument");
        scene->scene.camera = Camera(V(pos), V(view_dir), fov_deg, aspect);
        return CGPT_OK;
    });
}

int cgpth_scene_set_settings(cgpth_scene* scene, const cgpt_settings* s)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !s) return Fail("null argument");
        scene->scene.settings.max_ray_depth = s->max_ray_depth;
        scene->scene.settings.next_event_estimation_enabled = s->next_event_estimation_enabled != 0;
        scene->scene.settings.cosine_weighted_diffuse_reflection_enabled = s->cosine_weighted_diffuse_reflection_enabled != 0;
        scene->scene.settings.russian_roulette_enabled = s->russian_roulette_enabled != 0;
        scene->scene.render_mode = s->render_mode;
        scene->scene.debug_render_mode = s->debug_render_mode;
        return CGPT_OK;
    });
}

int cgpth_scene_rebuild_bvh(cgpth_scene* scene, uint32_t obj_index, int build_option)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || obj_index >= scene->scene.objects.size() || !scene->scene.objects[obj_index].has_bvh || !ValidOption(build_option))
            return Fail("bad argument to cgpth_scene_rebuild_bvh");
        if (!scene->scene.objects[obj_index].bvh->Rebuild((MeshBVH::BuildOption)build_option))
            return Fail("the binned build needs finite positions of magnitude <= 1e30 (the BVH is unchanged)");
        return CGPT_OK;
    });
}

int cgpth_tree_cost(const cgpt_bvh_node* nodes, uint32_t n_nodes, double c_inner, double c_tri, cgpt_tree_cost* out)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!nodes || !out) return Fail("bad argument to cgpth_tree_cost: a null array");
        if (n_nodes == 0u) return Fail("cgpth_tree_cost: no nodes");
        if (!TreeCostConstantOk(c_inner) || !TreeCostConstantOk(c_tri)) return Fail("cgpth_tree_cost: c_inner and c_tri must be finite and > 0");
        const cgpt_bvh_node& root = nodes[0];
        if (root.prim_count != 0u) {                                          // a root that never split (tree_cost.h)
            *out = { c_tri * (double)root.prim_count, 0.0, 0u, 1u, root.prim_count, 0u };
            return CGPT_OK;
        }
        TreeCostSums s;
        std::vector<uint32_t> stack{ 0u };
        uint32_t n_inner = 0;
        while (!stack.empty()) {
            const uint32_t i = stack.back(); stack.pop_back();
            const uint32_t l = nodes[i].left_first;
            if (l == 0u || l >= n_nodes || l + 1u >= n_nodes) return Fail("cgpth_tree_cost: node " + std::to_string(i) + " names children outside the array");
            if (++n_inner > n_nodes / 2u) return Fail("cgpth_tree_cost: the nodes form no tree");
            for (uint32_t c = l + 1u; c + 1u > l; --c) {                      // right, then left: the left subtree is walked first
                const cgpt_bvh_node& n = nodes[c];
                TreeCostAddChild(s, TreeCostHalfArea(n.aabb_min[0], n.aabb_min[1], n.aabb_min[2], n.aabb_max[0], n.aabb_max[1], n.aabb_max[2]), n.prim_count);
                if (n.prim_count == 0u) stack.push_back(c);
            }
        }
        const cgpt_bvh_node& a = nodes[root.left_first];
        const cgpt_bvh_node& b = nodes[root.left_first + 1u];
        const double h_root = TreeCostRootHalfArea(a.aabb_min, a.aabb_max, b.aabb_min, b.aabb_max);
        *out = { TreeCostTotal(c_inner, c_tri, h_root, s.inner, s.leaf), h_root, n_inner, s.n_leaves, s.max_leaf_tris, 0u };
        return CGPT_OK;
    });
}

int cgpth_scene_refit_mesh(cgpth_scene* scene, uint32_t obj_index, const cgpt_triangle* triangles, uint32_t n_tris)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene) return Fail("scene is null");
        if (obj_index >= scene->scene.objects.size())
            return Fail("object " + std::to_string(obj_index) + " out of range (" + std::to_string(scene->scene.objects.size()) + " objects)");
        Object& o = scene->scene.objects[obj_index];
        if (!o.has_bvh && o.kind != CGPT_OBJECT_TRIANGLE)
            return Fail("object " + std::to_string(obj_index) + " is a " + KindName(o) + ": it has no triangles (update_primitive edits it)");
        if (!triangles) return Fail("triangles is null");
        const uint32_t n = o.has_bvh ? o.bvh->NumTriangles() : 1u;
        if (n_tris != n)
            return Fail("object " + std::to_string(obj_index) + " has " + std::to_string(n) + " triangles, got " + std::to_string(n_tris) + " (a refit keeps the topology)");
        if (o.has_bvh) { if (!o.bvh->Refit(triangles, n_tris)) return Fail("refit failed"); }
        else o.triangle = triangles[0];
        return CGPT_OK;
    });
}

int cgpth_skin_triangles(const cgpt_triangle* bind_triangles, const uint16_t* joints, const float* weights, uint32_t n_tris,
                         const float* joint_matrices, uint32_t n_joints, cgpt_triangle* out_triangles)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        std::string err;
        if (!CheckSkin(bind_triangles, joints, weights, n_tris, n_joints, err) || !CheckJointMatrices(joint_matrices, n_joints, err)) return Fail(err);
        if (!out_triangles) return Fail("out_triangles is null");
        SkinTriangles(bind_triangles, joints, weights, n_tris, joint_matrices, out_triangles);
        return CGPT_OK;
    });
}

int cgpth_scene_skin_mesh(cgpth_scene* scene, uint32_t obj_index, const cgpt_triangle* bind_triangles, const uint16_t* joints, const float* weights,
                          uint32_t n_tris, const float* joint_matrices, uint32_t n_joints)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene) return Fail("scene is null");
        if (obj_index >= scene->scene.objects.size())
            return Fail("object " + std::to_string(obj_index) + " out of range (" + std::to_string(scene->scene.objects.size()) + " objects)");
        const Object& o = scene->scene.objects[obj_index];
        if (!o.has_bvh && o.kind != CGPT_OBJECT_TRIANGLE)
            return Fail("object " + std::to_string(obj_index) + " is a " + KindName(o) + ": it has no triangles to skin");
        for (const uint32_t li : scene->scene.light_source_indices)
            if (li == obj_index) return Fail("object " + std::to_string(obj_index) + " is a light: a pose does not recompute the area its sampling reads, so it takes no skin");
        const uint32_t n = o.has_bvh ? o.bvh->NumTriangles() : 1u;
        if (n_tris != n)
            return Fail("object " + std::to_string(obj_index) + " has " + std::to_string(n) + " triangles, got " + std::to_string(n_tris) + " (a skin keeps the topology)");
        std::string err;
        if (!CheckSkin(bind_triangles, joints, weights, n_tris, n_joints, err) || !CheckJointMatrices(joint_matrices, n_joints, err)) return Fail(err);
        std::vector<cgpt_triangle> posed(n_tris);
        SkinTriangles(bind_triangles, joints, weights, n_tris, joint_matrices, posed.data());
        return cgpth_scene_refit_mesh(scene, obj_index, posed.data(), n_tris);
    });
}

int cgpth_morph_triangles(const cgpt_triangle* base_triangles, const cgpt_triangle* target_deltas, uint32_t n_tris, uint32_t n_targets,
                          const float* weights, cgpt_triangle* out_triangles)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        std::string err;
        if (!CheckMorphTargets(base_triangles, target_deltas, n_tris, n_targets, err) || !CheckMorphWeights(weights, n_targets, err)) return Fail(err);
        if (!out_triangles) return Fail("out_triangles is null");
        MorphTriangles(base_triangles, target_deltas, n_tris, n_targets, weights, out_triangles);
        return CGPT_OK;
    });
}

int cgpth_scene_morph_mesh(cgpth_scene* scene, uint32_t obj_index, const cgpt_triangle* base_triangles, const cgpt_triangle* target_deltas,
                           uint32_t n_tris, uint32_t n_targets, const float* weights)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene) return Fail("scene is null");
        if (obj_index >= scene->scene.objects.size())
            return Fail("object " + std::to_string(obj_index) + " out of range (" + std::to_string(scene->scene.objects.size()) + " objects)");
        const Object& o = scene->scene.objects[obj_index];
        if (!o.has_bvh && o.kind != CGPT_OBJECT_TRIANGLE)
            return Fail("object " + std::to_string(obj_index) + " is a " + KindName(o) + ": it has no triangles to morph");
        for (const uint32_t li : scene->scene.light_source_indices)
            if (li == obj_index) return Fail("object " + std::to_string(obj_index) + " is a light: a pose does not recompute the area its sampling reads, so it takes no morph targets");
        const uint32_t n = o.has_bvh ? o.bvh->NumTriangles() : 1u;
        if (n_tris != n)
            return Fail("object " + std::to_string(obj_index) + " has " + std::to_string(n) + " triangles, got " + std::to_string(n_tris) + " (a morph keeps the topology)");
        std::string err;
        if (!CheckMorphTargets(base_triangles, target_deltas, n_tris, n_targets, err) || !CheckMorphWeights(weights, n_targets, err)) return Fail(err);
        std::vector<cgpt_triangle> posed(n_tris);
        MorphTriangles(base_triangles, target_deltas, n_tris, n_targets, weights, posed.data());
        return cgpth_scene_refit_mesh(scene, obj_index, posed.data(), n_tris);
    });
}

int cgpth_animate_joints(const cgpt_skeleton_desc* skeleton, const cgpt_clip_desc* clip, float time, float* out, uint32_t n_joints)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        std::string err;
        ClipTable table;
        bool unsupported = false;
        if (!CheckSkeleton(skeleton, err)) return Fail(err);
        if (!CheckClip(clip, table, err, unsupported)) { Fail(err); return unsupported ? (int)CGPT_ERR_UNSUPPORTED : (int)CGPT_ERR_INVALID; }
        if (table.n_joints != skeleton->n_joints)
            return Fail("the clip animates " + std::to_string(table.n_joints) + " joints, the skeleton has " + std::to_string(skeleton->n_joints));
        if (n_joints != skeleton->n_joints) return Fail("the skeleton has " + std::to_string(skeleton->n_joints) + " joints, got room for " + std::to_string(n_joints));
        if (!std::isfinite(time)) return Fail("time is not finite");
        if (!out) return Fail("out is null");
        AnimateJoints(*skeleton, table, time, out);
        return CGPT_OK;
    });
}

int cgpth_animate_layers(const cgpt_skeleton_desc* skeleton, const cgpt_clip_desc* clips, const cgpt_clip_layer* layers, uint32_t n_layers,
                         float* out, uint32_t n_joints)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        std::string err;
        if (!CheckSkeleton(skeleton, err)) return Fail(err);
        if (!layers) return Fail("layers is null");
        if (n_layers == 0u || n_layers > CGPT_ANIM_MAX_LAYERS) return Fail("n_layers " + std::to_string(n_layers) + " outside [1, " + std::to_string(CGPT_ANIM_MAX_LAYERS) + "]");
        if (!clips) return Fail("clips is null");
        std::vector<ClipTable> tables(n_layers);
        const ClipTable* table_of[CGPT_ANIM_MAX_LAYERS];
        float ranges[CGPT_ANIM_MAX_LAYERS][2];
        for (uint32_t l = 0; l < n_layers; ++l) {
            const std::string where = "layer " + std::to_string(l) + ": ";
            bool unsupported = false;
            if (!CheckClip(clips + l, tables[l], err, unsupported)) { Fail(where + err); return unsupported ? (int)CGPT_ERR_UNSUPPORTED : (int)CGPT_ERR_INVALID; }
            if (tables[l].n_joints != skeleton->n_joints)
                return Fail(where + "the clip animates " + std::to_string(tables[l].n_joints) + " joints, the skeleton has " + std::to_string(skeleton->n_joints));
            table_of[l] = &tables[l];
            ranges[l][0] = tables[l].begin; ranges[l][1] = tables[l].end;
        }
        AnimActiveLayers active;
        if (!ResolveLayers(layers, n_layers, ranges, active, err)) return Fail(err);
        if (n_joints != skeleton->n_joints) return Fail("the skeleton has " + std::to_string(skeleton->n_joints) + " joints, got room for " + std::to_string(n_joints));
        if (!out) return Fail("out is null");
        AnimateLayers(*skeleton, table_of, active, out);
        return CGPT_OK;
    });
}

int cgpth_clip_range(const cgpt_clip_desc* clip, float* begin, float* end)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        std::string err;
        ClipTable table;
        bool unsupported = false;
        if (!CheckClip(clip, table, err, unsupported)) { Fail(err); return unsupported ? (int)CGPT_ERR_UNSUPPORTED : (int)CGPT_ERR_INVALID; }
        if (begin) *begin = table.begin;
        if (end) *end = table.end;
        return CGPT_OK;
    });
}

int cgpth_wrap_time(float t, float begin, float end, uint32_t mode, float* out)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!out) return Fail("out is null");
        if (mode > CGPT_ANIM_WRAP_PINGPONG) return Fail("wrap mode " + std::to_string(mode) + " is none of CLAMP, LOOP, PINGPONG");
        if (!std::isfinite(t) || !std::isfinite(begin) || !std::isfinite(end)) return Fail("time, begin or end is not finite");
        *out = AnimWrapTime(t, begin, end, mode);
        return CGPT_OK;
    });
}

int cgpth_scene_update_primitive(cgpth_scene* scene, uint32_t obj_index, const cgpt_object* obj)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene) return Fail("scene is null");
        if (obj_index >= scene->scene.objects.size())
            return Fail("object " + std::to_string(obj_index) + " out of range (" + std::to_string(scene->scene.objects.size()) + " objects)");
        Object& o = scene->scene.objects[obj_index];
        if (!obj) return Fail("obj is null");
        if (o.has_bvh || (o.kind != CGPT_OBJECT_SPHERE && o.kind != CGPT_OBJECT_PLANE))
            return Fail("object " + std::to_string(obj_index) + " is a " + KindName(o) + ": refit_mesh edits it");
        if (obj->kind != o.kind) return Fail("object " + std::to_string(obj_index) + " is a " + KindName(o) + ", got kind " + std::to_string(obj->kind));
        if (obj->mat_index != o.mat_index)
            return Fail("object " + std::to_string(obj_index) + " has material " + std::to_string(o.mat_index) + ", got " + std::to_string(obj->mat_index) + " (materials are not changed here)");
        if (o.kind == CGPT_OBJECT_SPHERE) o.sphere = Sphere{ V(obj->sphere_center), obj->sphere_radius };
        else o.plane = Plane{ V(obj->plane_normal), V(obj->plane_point) };
        return CGPT_OK;
    });
}

int cgpth_scene_bvh_info(const cgpth_scene* scene, uint32_t obj_index, cgpth_bvh_info* out)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !out || obj_index >= scene->scene.objects.size() || !scene->scene.objects[obj_index].has_bvh) return Fail("not a mesh object");
        const MeshBVH& b = *scene->scene.objects[obj_index].bvh;
        *out = cgpth_bvh_info{};
        out->num_triangles = b.NumTriangles(); out->nodes_used = b.NumNodes(); out->max_depth = b.GetMaxDepth(); out->total_area = b.GetTotalArea();
        for (uint32_t i = 0; i < b.NumNodes(); ++i) {
            const uint32_t c = b.Nodes()[i].prim_count;
            if (c > 0) { out->num_leaves++; if (c > out->max_leaf_size) out->max_leaf_size = c; }
        }
        return CGPT_OK;
    });
}

int cgpth_scene_bvh_export(const cgpth_scene* scene, uint32_t obj_index, cgpt_bvh_node* nodes, uint32_t* tri_indices)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !nodes || !tri_indices || obj_index >= scene->scene.objects.size() || !scene->scene.objects[obj_index].has_bvh) return Fail("not a mesh object");
        const MeshBVH& b = *scene->scene.objects[obj_index].bvh;
        memcpy(nodes, b.Nodes(), sizeof(cgpt_bvh_node) * b.NumNodes());
        memcpy(tri_indices, b.TriIndices(), sizeof(uint32_t) * b.NumTriangles());
        return CGPT_OK;
    });
}

int cgpth_scene_flatten(cgpth_scene* scene, cgpt_scene_desc* out)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !out) return Fail("null argument");
        *out = scene->scene.Flatten(scene->flat);
        return CGPT_OK;
    });
}

int cgpth_scene_get_camera(const cgpth_scene* scene, cgpt_camera* out)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !out) return Fail("null argument");
        *out = scene->scene.camera.Abi();
        return CGPT_OK;
    });
}

int cgpth_scene_get_settings(const cgpth_scene* scene, cgpt_settings* out)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        if (!scene || !out) return Fail("null argument");
        *out = scene->scene.AbiSettings();
        return CGPT_OK;
    });
}

int cgpth_write_ppm(const char* path, const uint32_t* pixels, uint32_t width, uint32_t height)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        std::string err;
        if (!path || !pixels) return Fail("null argument");
        return WritePPM(path, pixels, width, height, err) ? CGPT_OK : Fail(err);
    });
}
int cgpth_write_pfm(const char* path, const float* acc, uint32_t n, uint32_t width, uint32_t height)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        std::string err;
        if (!path || !acc) return Fail("null argument");
        return WritePFM(path, acc, n, width, height, err) ? CGPT_OK : Fail(err);
    });
}
int cgpth_write_accumulator(const char* path, const float* acc, uint32_t n, uint32_t width, uint32_t height)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        std::string err;
        if (!path || !acc) return Fail("null argument");
        return WriteAccumulator(path, acc, n, width, height, err) ? CGPT_OK : Fail(err);
    });
}
int cgpth_read_accumulator(const char* path, float* acc, uint32_t* n, uint32_t width, uint32_t height)
{
    return Guarded<int>((int)CGPT_ERR_INVALID, [&]() -> int {
        std::string err;
        if (!path || !acc || !n) return Fail("null argument");
        return ReadAccumulator(path, acc, n, width, height, err) ? CGPT_OK : Fail(err);
    });
}

uint32_t cgpth_fast_div(uint32_t n, uint32_t d) { return d == 0u ? 0u : fast_div(n, MakeFastDiv(d)); }

uint32_t cgpth_shade_item_blocks(uint32_t n_blocks, uint32_t n_waves, uint32_t chunk) { return n_waves == 0u || chunk == 0u ? 0u : shade_item_blocks(n_blocks, n_waves, chunk); }
uint32_t cgpth_shade_segment_blocks(uint32_t cap_blocks, uint32_t min_waves, uint32_t chunk) { return min_waves == 0u || chunk == 0u ? 0u : shade_segment_blocks(cap_blocks, min_waves, chunk); }

uint32_t cgpth_motion_records(const float* prev, uint32_t n_prev, const float* cur, uint32_t n_objects, float* records_out)
{
    if (!prev || !cur || !records_out) return 0u;
    static_assert(sizeof(MotionRecord) == 24 * sizeof(float), "24 words per object");
    return (uint32_t)CompareTransforms(prev, n_prev, cur, n_objects, reinterpret_cast<MotionRecord*>(records_out));
}

}  // extern "C"
