// morph.h -- morph targets (blend shapes) of an unindexed triangle array: the arithmetic, stated once for the host mirror (morph.cpp)
// and the device kernel (csrc/device/refit.hip: morph_triangles), and the validation both sides share.  tests/morph_ref.py states the
// same operations in numpy; DESIGN.md 5.28.
//
// A target is n_tris records of the cgpt_triangle layout that hold displacements: per corner a position delta and a normal delta
// (glTF's POSITION / NORMAL target accessors expanded to unindexed corners).  All float, -ffp-contract=off, for each of the 18 floats
// of a triangle in exactly this order:
//   x = base
//   for k = 0 .. n_targets-1, ascending, only where weights[k] != 0.0f (+0 and -0 are both skipped):
//       x = x + weights[k] * delta_k                                    (product rounded, then sum rounded)
// With no active target the triangle is the base triangle bit for bit (-0 + 0*d would be +0: the skip is part of the statement).  With
// at least one, each corner's blended normal q is normalised by SkinCorner's rule (skinning.h): l2 = (qx*qx + qy*qy) + qz*qz; l2 finite
// and > 0: n = q * (1.0f / sqrtf(l2)); otherwise the base normal unchanged.  Positions are used as blended.  Weights are used as given
// (negative and above 1 are allowed).  glTF applies morphs before the skin: the morphed corner is the pn of SkinCorner.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "cpugpupt_abi.h"

#ifdef __HIP__
#define CGPT_MORPH_FN __host__ __device__ inline
#else
#define CGPT_MORPH_FN inline
#endif

namespace cgpt {

constexpr uint32_t kMorphMaxTargets = 256;

// one active target: x = x + w * d over the 18 floats of a triangle
CGPT_MORPH_FN void MorphAccumulate(float x[18], float w, const float d[18])
{
    for (int j = 0; j < 18; ++j) x[j] = x[j] + w * d[j];
}

// after at least one active target: the three corners' normals (floats 3..5 of each six), by SkinCorner's rule
CGPT_MORPH_FN void MorphNormalise(const float base[18], float x[18])
{
    for (int c = 0; c < 3; ++c) {
        float* q = x + 6 * c + 3;
        const float l2 = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
        if (l2 > 0.0f && l2 < INFINITY) {
            const float rcp = 1.0f / sqrtf(l2);
            q[0] = q[0] * rcp; q[1] = q[1] * rcp; q[2] = q[2] * rcp;
        } else {
            q[0] = base[6 * c + 3]; q[1] = base[6 * c + 4]; q[2] = base[6 * c + 5];
        }
    }
}

// The morph of n_tris base triangles: deltas is n_targets x n_tris records, target-major.  The inputs have passed CheckMorphTargets and
// CheckMorphWeights.  out may not alias the inputs.
void MorphTriangles(const cgpt_triangle* base, const cgpt_triangle* deltas, uint32_t n_tris, uint32_t n_targets, const float* weights,
                    cgpt_triangle* out);

// What cgpt_scene_set_morph_targets and cgpth_morph_triangles refuse of a set of targets: a NULL array, n_targets 0 or above
// kMorphMaxTargets, a base or delta float that is not finite.  true, or false with the reason in `error`.
bool CheckMorphTargets(const cgpt_triangle* base, const cgpt_triangle* deltas, uint32_t n_tris, uint32_t n_targets, std::string& error);
// ... and of a pose: NULL, or one of the n_targets weights not finite
bool CheckMorphWeights(const float* weights, uint32_t n_targets, std::string& error);

}  // namespace cgpt
