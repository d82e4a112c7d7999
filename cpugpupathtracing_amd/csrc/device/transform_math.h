// transform_math.h -- the host arithmetic of a per-object transform (cgpt_scene_update_transforms): the identity test and the inverse.
// Plain C++, no HIP: shared by the upload's layout unit (scene_layout.h) and the host mirror (host_capi.cpp).
// tests/transform_ref.py states the same operations in numpy.
#pragma once
#include <cmath>
#include <cstring>

namespace cgpt {

// An object-to-world matrix is 12 floats, the rows of [A | b]: world = A p + b.
inline bool IsIdentityTransform(const float m[12])                            // bitwise: -0 is not the identity's 0
{
    static const float kIdentity[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    return memcmp(m, kIdentity, sizeof(kIdentity)) == 0;
}

// out = the rows {Ainv row r, binv_r} with Ainv = A^-1 (adjugate / determinant) and binv = -A^-1 b, in double from the float entries, each
// rounded to float once; a zero result is stored as +0 (x + 0.0f: 0 / det and -(0) are -0 for half of the sign flips, and with +0 a
// sign flip maps an axis-aligned normal to itself bit for bit).  False (out untouched) when an entry is not finite, the determinant is 0 or not finite, or a result is not
// finite as a float.
inline bool InvertTransform(const float m[12], float out[12])
{
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(m[i])) return false;
    const double a00 = m[0], a01 = m[1], a02 = m[2], b0 = m[3], a10 = m[4], a11 = m[5], a12 = m[6], b1 = m[7], a20 = m[8], a21 = m[9], a22 = m[10], b2 = m[11];
    const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;   // cofactors of row 0
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    if (det == 0.0 || !std::isfinite(det)) return false;
    const double inv[3][3] = {
        { c00 / det, (a02 * a21 - a01 * a22) / det, (a01 * a12 - a02 * a11) / det },
        { c01 / det, (a00 * a22 - a02 * a20) / det, (a02 * a10 - a00 * a12) / det },
        { c02 / det, (a01 * a20 - a00 * a21) / det, (a00 * a11 - a01 * a10) / det },
    };
    float r[12];
    for (int i = 0; i < 3; ++i) {
        const double binv = -((inv[i][0] * b0 + inv[i][1] * b1) + inv[i][2] * b2);
        r[4 * i] = (float)inv[i][0]; r[4 * i + 1] = (float)inv[i][1]; r[4 * i + 2] = (float)inv[i][2]; r[4 * i + 3] = (float)binv;
    }
    for (int i = 0; i < 12; ++i) r[i] += 0.0f;                                 // -0 -> +0, nothing else changes
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(r[i])) return false;
    memcpy(out, r, sizeof(r));
    return true;
}

// ---- boxes of the top-level tree (cgpt_set_top_level; tests/tlas_ref.py states the same operations in numpy) ------------------------
// A box is 6 floats, {lo.xyz, hi.xyz}.  The unbounded box (a plane, geometry that is not finite) is (-inf, +inf) on every axis.
inline void UnboundedBox(float box[6])
{
    for (int a = 0; a < 3; ++a) { box[a] = -INFINITY; box[3 + a] = INFINITY; }
}
inline bool IsFiniteBox(const float box[6])
{
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(box[i])) return false;
    return true;
}
// the largest float <= v and the smallest float >= v
inline float FloatBelow(double v) { const float f = (float)v; return (double)f > v ? std::nextafter(f, -INFINITY) : f; }
inline float FloatAbove(double v) { const float f = (float)v; return (double)f < v ? std::nextafter(f, INFINITY) : f; }
// the box of the 8 corners of `local` under world = A p + b: ((a0 x + a1 y) + a2 z) + b per row in double, min / max over the corners,
// rounded outward to float
inline void TransformBox(const float m[12], const float local[6], float out[6])
{
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int c = 0; c < 8; ++c) {
        const double x = local[(c & 1) ? 3 : 0], y = local[(c & 2) ? 4 : 1], z = local[(c & 4) ? 5 : 2];
        for (int r = 0; r < 3; ++r) {
            const double w = (((double)m[4 * r] * x + (double)m[4 * r + 1] * y) + (double)m[4 * r + 2] * z) + (double)m[4 * r + 3];
            if (w < lo[r]) lo[r] = w;
            if (w > hi[r]) hi[r] = w;
        }
    }
    for (int r = 0; r < 3; ++r) { out[r] = FloatBelow(lo[r]); out[3 + r] = FloatAbove(hi[r]); }
}
// Every leaf box is padded outward: per axis pad = kBoxPad * max(|lo|, |hi|, hi - lo) in float, then one nextafter outward.  A box with a
// bound that is not finite (before or after) becomes the unbounded box.  tests/tlas_ref.py: PAD states the factor and why.
static constexpr float kBoxPad = 1e-4f;
inline void PadBox(float box[6])
{
    if (!IsFiniteBox(box)) { UnboundedBox(box); return; }
    for (int a = 0; a < 3; ++a) {
        const float lo = box[a], hi = box[3 + a];
        const float ext = hi - lo;
        float m = std::fabs(lo) > std::fabs(hi) ? std::fabs(lo) : std::fabs(hi);
        if (ext > m) m = ext;
        const float pad = kBoxPad * m;
        box[a] = std::nextafter(lo - pad, -INFINITY);
        box[3 + a] = std::nextafter(hi + pad, INFINITY);
    }
    if (!IsFiniteBox(box)) UnboundedBox(box);
}

}  // namespace cgpt
