// transform_math.h -- the host arithmetic of a per-object transform (cgpt_scene_update_transforms): the identity test, the inverse, and an
// object's motion between two frames for the temporal denoiser.
// Plain C++, no HIP: shared by the upload's layout unit (scene_layout.h) and the host mirror (host_capi.cpp).
// tests/transform_ref.py states the same operations in numpy.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
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

// ---- an object's motion between two frames (CGPT_TEMPORAL_FOLLOW_TRANSFORMS; tests/motion_ref.py states the same operations in numpy) ----
// What carries a first hit on an object back to where it was when the temporal history was stored: rows 0..2 are {D row r, its
// translation} of D = M_prev M_cur^-1 (x' = D x), rows 3..5 {N row r, 0} of N = A_prev^-T A_cur^T (n' = normalize(N n)); the state word
// is the bits of rows[3][3].  Both inverses are the adjugate / determinant in double from the float entries (InvertTransform's cofactors,
// not rounded in between), every product ((p0 q0 + p1 q1) + p2 q2) in double, and each entry is rounded to float once.
enum MotionState : uint32_t { kMotionUnmoved = 0, kMotionMoved = 1, kMotionDrop = 2 };
struct MotionRecord { float rows[6][4]; };
static_assert(sizeof(MotionRecord) == 96, "6 float4 per object");

inline uint32_t MotionRecordState(const MotionRecord& r) { uint32_t s; memcpy(&s, &r.rows[3][3], sizeof(s)); return s; }

// the double inverse of the linear part of m: false when the determinant is 0 or not finite
inline bool InvertLinearDouble(const float m[12], double inv[3][3])
{
    const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
    const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;   // cofactors of row 0
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    if (det == 0.0 || !std::isfinite(det)) return false;
    inv[0][0] = c00 / det; inv[0][1] = (a02 * a21 - a01 * a22) / det; inv[0][2] = (a01 * a12 - a02 * a11) / det;
    inv[1][0] = c01 / det; inv[1][1] = (a00 * a22 - a02 * a20) / det; inv[1][2] = (a02 * a10 - a00 * a12) / det;
    inv[2][0] = c02 / det; inv[2][1] = (a01 * a20 - a00 * a21) / det; inv[2][2] = (a00 * a11 - a01 * a10) / det;
    return true;
}

// The record of an object whose matrix was `prev` when the history was stored and is `cur` now.  Unmoved: the 12 floats are equal
// bytewise (the rows are zero: the kernel takes x and n untouched).  Drop: an inverse does not exist or an entry of D or N is not finite
// as a float (the rows are zero).  Moved: everything else.
inline MotionRecord MakeMotionRecord(const float prev[12], const float cur[12])
{
    MotionRecord rec;
    memset(&rec, 0, sizeof(rec));
    const auto with_state = [&rec](uint32_t s) { memcpy(&rec.rows[3][3], &s, sizeof(s)); return rec; };
    if (memcmp(prev, cur, 12 * sizeof(float)) == 0) return with_state(kMotionUnmoved);
    double ic[3][3], ip[3][3];
    if (!InvertLinearDouble(cur, ic) || !InvertLinearDouble(prev, ip)) return with_state(kMotionDrop);
    const double bc[3] = { cur[3], cur[7], cur[11] };
    double binv[3];                                                            // -A_cur^-1 b_cur
    for (int i = 0; i < 3; ++i) binv[i] = -((ic[i][0] * bc[0] + ic[i][1] * bc[1]) + ic[i][2] * bc[2]);
    float out[6][4] = {};
    for (int r = 0; r < 3; ++r) {
        const double p0 = prev[4 * r], p1 = prev[4 * r + 1], p2 = prev[4 * r + 2], pb = prev[4 * r + 3];
        for (int c = 0; c < 3; ++c) {
            out[r][c] = (float)((p0 * ic[0][c] + p1 * ic[1][c]) + p2 * ic[2][c]);
            out[3 + r][c] = (float)((ip[0][r] * (double)cur[4 * c] + ip[1][r] * (double)cur[4 * c + 1]) + ip[2][r] * (double)cur[4 * c + 2]);
        }
        out[r][3] = (float)(((p0 * binv[0] + p1 * binv[1]) + p2 * binv[2]) + pb);
    }
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 4; ++c)
            if (!std::isfinite(out[r][c])) return with_state(kMotionDrop);
    memcpy(rec.rows, out, sizeof(out));
    return with_state(kMotionMoved);
}

// The snapshot and compare helpers of the temporal history: the matrices (12 floats per object) in force when it was stored, and the
// records of every object against the current ones.  Returns the number of objects that are not unmoved; `records` gets n of them.
// A snapshot of another size than `cur` (n_prev != n) cannot be followed: every object is a drop.
inline void SnapshotTransforms(const float* xform, size_t n_objects, float* snapshot) { if (n_objects) memcpy(snapshot, xform, 12 * n_objects * sizeof(float)); }
inline size_t CompareTransforms(const float* prev, size_t n_prev, const float* cur, size_t n, MotionRecord* records)
{
    size_t changed = 0;
    for (size_t i = 0; i < n; ++i) {
        if (n_prev != n) { memset(&records[i], 0, sizeof(MotionRecord)); const uint32_t s = kMotionDrop; memcpy(&records[i].rows[3][3], &s, sizeof(s)); }
        else records[i] = MakeMotionRecord(prev + 12 * i, cur + 12 * i);
        if (MotionRecordState(records[i]) != kMotionUnmoved) ++changed;
    }
    return changed;
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
