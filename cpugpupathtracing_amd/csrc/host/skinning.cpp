// skinning.cpp -- the host mirror of cgpt_scene_skin_mesh's triangle pass (skinning.h states the arithmetic) and the validation of a
// skin and of a pose.  Host only.
#include "skinning.h"

namespace cgpt {

void SkinTriangles(const cgpt_triangle* bind, const uint16_t* joints, const float* weights, uint32_t n_tris, const float* joint_matrices,
                   cgpt_triangle* out)
{
    for (uint32_t t = 0; t < n_tris; ++t) {
        const cgpt_vertex* const in[3] = { &bind[t].v0, &bind[t].v1, &bind[t].v2 };
        cgpt_vertex* const posed[3] = { &out[t].v0, &out[t].v1, &out[t].v2 };
        for (int c = 0; c < 3; ++c) {
            const uint16_t* j = joints + 12 * (size_t)t + 4 * c;
            const float* w = weights + 12 * (size_t)t + 4 * c;
            const float* a0 = joint_matrices + 12 * (size_t)j[0];
            const float* a1 = joint_matrices + 12 * (size_t)j[1];
            const float* a2 = joint_matrices + 12 * (size_t)j[2];
            const float* a3 = joint_matrices + 12 * (size_t)j[3];
            float m[12];
            for (int e = 0; e < 12; ++e) m[e] = SkinBlend(w[0], a0[e], w[1], a1[e], w[2], a2[e], w[3], a3[e]);
            const float pn[6] = { in[c]->pos[0], in[c]->pos[1], in[c]->pos[2], in[c]->normal[0], in[c]->normal[1], in[c]->normal[2] };
            float o[6];
            SkinCorner(m, pn, o);
            for (int k = 0; k < 3; ++k) { posed[c]->pos[k] = o[k]; posed[c]->normal[k] = o[3 + k]; }
        }
    }
}

bool CheckSkin(const cgpt_triangle* bind, const uint16_t* joints, const float* weights, uint32_t n_tris, uint32_t n_joints, std::string& error)
{
    if (!bind) { error = "bind_triangles is null"; return false; }
    if (!joints) { error = "joints is null"; return false; }
    if (!weights) { error = "weights is null"; return false; }
    if (n_joints == 0 || n_joints > kSkinMaxJoints) {
        error = "n_joints " + std::to_string(n_joints) + " outside [1, " + std::to_string(kSkinMaxJoints) + "]";
        return false;
    }
    static_assert(sizeof(cgpt_triangle) == 18 * sizeof(float), "a triangle is 18 floats");
    const float* b = reinterpret_cast<const float*>(bind);
    for (size_t k = 0; k < 18 * (size_t)n_tris; ++k)
        if (!std::isfinite(b[k])) { error = "bind triangle " + std::to_string(k / 18) + ": float " + std::to_string(k % 18) + " is not finite"; return false; }
    for (size_t k = 0; k < 12 * (size_t)n_tris; ++k) {
        if (joints[k] >= n_joints) {
            error = "triangle " + std::to_string(k / 12) + ": joint index " + std::to_string(joints[k]) + " >= n_joints " + std::to_string(n_joints);
            return false;
        }
        if (!std::isfinite(weights[k])) { error = "triangle " + std::to_string(k / 12) + ": weight " + std::to_string(k % 12) + " is not finite"; return false; }
    }
    return true;
}

bool CheckJointMatrices(const float* joint_matrices, uint32_t n_joints, std::string& error)
{
    if (!joint_matrices) { error = "joint_matrices is null"; return false; }
    for (size_t k = 0; k < 12 * (size_t)n_joints; ++k)
        if (!std::isfinite(joint_matrices[k])) { error = "joint " + std::to_string(k / 12) + ": entry " + std::to_string(k % 12) + " is not finite"; return false; }
    return true;
}

}  // namespace cgpt
