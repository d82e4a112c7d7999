// morph.cpp -- the host mirror of cgpt_scene_morph_mesh's triangle pass (morph.h states the arithmetic) and the validation of a set of
// targets and of a pose's weights.  Host only.
#include "morph.h"

#include <cstring>

namespace cgpt {

void MorphTriangles(const cgpt_triangle* base, const cgpt_triangle* deltas, uint32_t n_tris, uint32_t n_targets, const float* weights,
                    cgpt_triangle* out)
{
    static_assert(sizeof(cgpt_triangle) == 18 * sizeof(float), "a triangle is 18 floats");
    for (uint32_t t = 0; t < n_tris; ++t) {
        float b[18], x[18];
        memcpy(b, &base[t], sizeof(b));
        memcpy(x, b, sizeof(x));
        bool active = false;
        for (uint32_t k = 0; k < n_targets; ++k) {
            if (weights[k] == 0.0f) continue;                                  // +0 and -0
            float d[18];
            memcpy(d, &deltas[(size_t)k * n_tris + t], sizeof(d));
            MorphAccumulate(x, weights[k], d);
            active = true;
        }
        if (active) MorphNormalise(b, x);
        memcpy(&out[t], x, sizeof(x));
    }
}

bool CheckMorphTargets(const cgpt_triangle* base, const cgpt_triangle* deltas, uint32_t n_tris, uint32_t n_targets, std::string& error)
{
    if (!base) { error = "base_triangles is null"; return false; }
    if (!deltas) { error = "target_deltas is null"; return false; }
    if (n_targets == 0 || n_targets > kMorphMaxTargets) {
        error = "n_targets " + std::to_string(n_targets) + " outside [1, " + std::to_string(kMorphMaxTargets) + "]";
        return false;
    }
    const float* b = reinterpret_cast<const float*>(base);
    for (size_t k = 0; k < 18 * (size_t)n_tris; ++k)
        if (!std::isfinite(b[k])) { error = "base triangle " + std::to_string(k / 18) + ": float " + std::to_string(k % 18) + " is not finite"; return false; }
    const float* d = reinterpret_cast<const float*>(deltas);
    const size_t per_target = 18 * (size_t)n_tris;
    for (size_t k = 0; k < per_target * n_targets; ++k)
        if (!std::isfinite(d[k])) {
            error = "target " + std::to_string(k / per_target) + ", triangle " + std::to_string(k % per_target / 18) + ": float " + std::to_string(k % 18) + " is not finite";
            return false;
        }
    return true;
}

bool CheckMorphWeights(const float* weights, uint32_t n_targets, std::string& error)
{
    if (!weights) { error = "weights is null"; return false; }
    for (uint32_t k = 0; k < n_targets; ++k)
        if (!std::isfinite(weights[k])) { error = "morph weight " + std::to_string(k) + " is not finite"; return false; }
    return true;
}

}  // namespace cgpt
