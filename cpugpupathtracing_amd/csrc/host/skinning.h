// skinning.h -- linear blend skinning of an unindexed triangle array: the arithmetic, stated once for the host mirror (skinning.cpp)
// and the device kernel (csrc/device/refit.hip: skin_triangles), and the validation both sides share.  tests/skin_ref.py states the same
// operations in numpy; DESIGN.md 5.26.
//
// A skin is per corner: corner c of triangle t has four joint indices joints[12 t + 4 c + k] and four weights weights[12 t + 4 c + k].
// A joint matrix is 12 floats, the rows of [A | b], row-major (the layout of cgpt_scene_update_transforms): object-space skinning
// matrices.  All float, -ffp-contract=off, in exactly this order:
//   blended entry    m = w0*a0; m = m + w1*a1; m = m + w2*a2; m = m + w3*a3      (no influence skipped, weights never renormalised)
//   position, row r  p'_r = ((m_r0*px + m_r1*py) + m_r2*pz) + m_r3
//   normal, row r    q_r = (m_r0*nx + m_r1*ny) + m_r2*nz;  l2 = (qx*qx + qy*qy) + qz*qz;
//                    l2 finite and > 0: n' = q * (1.0f / sqrtf(l2))  (normalize, ref: MathLib.h:93); otherwise the bind normal unchanged
// The blended A moves the normal, not its inverse transpose: exact for rigid joints and uniform scale.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "cpugpupt_abi.h"

#ifdef __HIP__
#define CGPT_SKIN_FN __host__ __device__ inline
#else
#define CGPT_SKIN_FN inline
#endif

namespace cgpt {

constexpr uint32_t kSkinMaxJoints = 1024;

CGPT_SKIN_FN float SkinBlend(float w0, float a0, float w1, float a1, float w2, float a2, float w3, float a3)
{
    float m = w0 * a0;
    m = m + w1 * a1;
    m = m + w2 * a2;
    m = m + w3 * a3;
    return m;
}

// one corner: m the 12 blended entries, pn = {pos.xyz, normal.xyz} of the bind pose, out the posed six
CGPT_SKIN_FN void SkinCorner(const float m[12], const float pn[6], float out[6])
{
    float q[3];
    for (int r = 0; r < 3; ++r) {
        out[r] = ((m[4 * r] * pn[0] + m[4 * r + 1] * pn[1]) + m[4 * r + 2] * pn[2]) + m[4 * r + 3];
        q[r] = (m[4 * r] * pn[3] + m[4 * r + 1] * pn[4]) + m[4 * r + 2] * pn[5];
    }
    const float l2 = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
    if (l2 > 0.0f && l2 < INFINITY) {
        const float rcp = 1.0f / sqrtf(l2);
        out[3] = q[0] * rcp; out[4] = q[1] * rcp; out[5] = q[2] * rcp;
    } else {
        out[3] = pn[3]; out[4] = pn[4]; out[5] = pn[5];
    }
}

// The pose of n_tris bind triangles.  The inputs have passed CheckSkin and CheckJointMatrices.
void SkinTriangles(const cgpt_triangle* bind, const uint16_t* joints, const float* weights, uint32_t n_tris, const float* joint_matrices,
                   cgpt_triangle* out);

// What cgpt_scene_set_skin and cgpth_skin_triangles refuse of a skin: a NULL array, n_joints 0 or above kSkinMaxJoints, a joint index
// >= n_joints, a weight or a bind float that is not finite.  true, or false with the reason in `error`.
bool CheckSkin(const cgpt_triangle* bind, const uint16_t* joints, const float* weights, uint32_t n_tris, uint32_t n_joints, std::string& error);
// ... and of a pose: NULL, or one of the n_joints x 12 floats not finite
bool CheckJointMatrices(const float* joint_matrices, uint32_t n_joints, std::string& error);

}  // namespace cgpt
