// animation.h -- joint matrices from an animation clip: the arithmetic, stated once for the host mirror (animation.cpp: AnimateJoints)
// and the device kernel (csrc/device/refit.hip: animate_joints_batch), and the validation both sides share.  tests/anim_ref.py states
// the same operations in numpy; DESIGN.md 5.33.  The data layout is glTF's (skins / animations), so an importer is a copy loop.
// Further down: wrapped times and the blend of up to four clips per joint (AnimateLayers, animate_layers_batch; tests/anim_layer_ref.py;
// DESIGN.md 5.35), stated where they are defined.
//
// A skeleton has n_joints joints: parents[j] (-1: a root; any order, no cycle), inverse_bind[12 j ..] the rows of [A | b], rest[10 j ..]
// = T.xyz, R.xyzw, S.xyz, and an optional root matrix [A | b] applied last (absent: no multiply at all).  A clip has channels
// {joint, path T / R / S, STEP or LINEAR, n_keys, first_time, first_value}: key i of a channel is times[first_time + i] and the 3 (T, S)
// or 4 (R) floats at values[first_value + width i].  All float, -ffp-contract=off, only + - * / and sqrtf, in exactly this order:
//   key           k = the last key with times[k] <= t, the first key when there is none (a binary search over the channel's keys)
//   value         key k as stored when t lies before the first key, k is the last key, or the channel is STEP; otherwise LINEAR with
//                 a = key k, b = key k + 1:  u = (t - t_k) / (t_k1 - t_k);   v_c = a_c + u * (b_c - a_c)
//                 for R, b is negated first when ((a.x*b.x + a.y*b.y) + a.z*b.z) + a.w*b.w < 0
//   rotation      every rotation, sampled or rest:  l2 = ((x*x + y*y) + z*z) + w*w;  l2 finite and > 0: q * (1.0f / sqrtf(l2)), else (0, 0, 0, 1)
//   no channel    a (joint, path) without a channel takes rest
//   R(q)          r00 = 1 - 2*(yy + zz)   r01 = 2*(xy - wz)       r02 = 2*(xz + wy)           with xx = x*x, xy = x*y, ... wz = w*z
//                 r10 = 2*(xy + wz)       r11 = 1 - 2*(xx + zz)   r12 = 2*(yz - wx)
//                 r20 = 2*(xz - wy)       r21 = 2*(yz + wx)       r22 = 1 - 2*(xx + yy)
//   local         L_j = [R(q) diag(S) | T]:  row r = { r_r0*S.x, r_r1*S.y, r_r2*S.z, T_r }
//   product       C = A o B, 3x4 affine:  C_rc = (A_r0*B_0c + A_r1*B_1c) + A_r2*B_2c  (c < 3);   C_r3 = ((A_r0*B_03 + A_r1*B_13) + A_r2*B_23) + A_r3
//   global        G = L_j;  p = parents[j];  while (p >= 0) { G = L_p o G;  p = parents[p]; }      (bottom-up: a memoised top-down walk associates differently)
//   joint matrix  M_j = G o IB_j, then root o M_j if a root was given
// Rotations are therefore a normalised lerp, not a slerp: the price of bit equality with the mirror.  Between two keys that are theta
// apart the nlerp follows the slerp's arc at a slightly different speed; the largest angle between the two over a key interval
// (tests/anim_ref.py: nlerp_slerp_table, float64) is
//   theta   15 deg      30 deg      60 deg      90 deg
//   error   0.0041 deg  0.0331 deg  0.2675 deg  0.9188 deg
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "cpugpupt_abi.h"

#ifdef __HIP__
#define CGPT_ANIM_FN __host__ __device__ inline
#else
#define CGPT_ANIM_FN inline
#endif

namespace cgpt {

constexpr uint32_t kAnimNoChannel = 0xFFFFFFFFu;

// a channel as the sampler reads it: found through map[3 joint + path], so joint and path are not repeated
struct AnimChannel { uint32_t interpolation, n_keys, first_time, first_value; };

// the last key with times[k] <= t; 0 when there is none
CGPT_ANIM_FN uint32_t AnimFindKey(const float* times, uint32_t n_keys, float t)
{
    uint32_t lo = 0, hi = n_keys;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) / 2u;
        if (times[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

CGPT_ANIM_FN void AnimNormaliseRotation(float q[4])
{
    const float l2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
    if (l2 > 0.0f && l2 < INFINITY) {
        const float rcp = 1.0f / sqrtf(l2);
        q[0] = q[0] * rcp; q[1] = q[1] * rcp; q[2] = q[2] * rcp; q[3] = q[3] * rcp;
    } else {
        q[0] = 0.0f; q[1] = 0.0f; q[2] = 0.0f; q[3] = 1.0f;
    }
}

// `width` floats of channel c at time t (3, or 4 with `rotation`): not yet normalised
CGPT_ANIM_FN void AnimSampleChannel(const AnimChannel& c, const float* times, const float* values, float t, int width, bool rotation, float* out)
{
    const float* ct = times + c.first_time;
    const float* cv = values + c.first_value;
    const uint32_t k = AnimFindKey(ct, c.n_keys, t);
    const float* a = cv + (size_t)width * k;
    if (c.interpolation != CGPT_ANIM_LINEAR || k + 1u >= c.n_keys || !(ct[k] <= t)) {
        for (int i = 0; i < width; ++i) out[i] = a[i];
        return;
    }
    const float u = (t - ct[k]) / (ct[k + 1u] - ct[k]);
    float b[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    for (int i = 0; i < width; ++i) b[i] = a[width + i];
    if (rotation) {
        const float dot = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3];
        if (dot < 0.0f) { b[0] = -b[0]; b[1] = -b[1]; b[2] = -b[2]; b[3] = -b[3]; }
    }
    for (int i = 0; i < width; ++i) out[i] = a[i] + u * (b[i] - a[i]);
}

// T, q, S of joint j at time t: map holds 3 n_joints channel indices (kAnimNoChannel: take rest), rest 10 floats a joint; q is normalised
CGPT_ANIM_FN void AnimSampleJoint(const uint32_t* map, const AnimChannel* channels, const float* times, const float* values, const float* rest,
                                  uint32_t j, float t, float T[3], float q[4], float S[3])
{
    const float* r = rest + 10 * (size_t)j;
    T[0] = r[0]; T[1] = r[1]; T[2] = r[2]; q[0] = r[3]; q[1] = r[4]; q[2] = r[5]; q[3] = r[6]; S[0] = r[7]; S[1] = r[8]; S[2] = r[9];
    const uint32_t ct = map[3 * (size_t)j + CGPT_ANIM_PATH_TRANSLATION], cr = map[3 * (size_t)j + CGPT_ANIM_PATH_ROTATION], cs = map[3 * (size_t)j + CGPT_ANIM_PATH_SCALE];
    if (ct != kAnimNoChannel) AnimSampleChannel(channels[ct], times, values, t, 3, false, T);
    if (cr != kAnimNoChannel) AnimSampleChannel(channels[cr], times, values, t, 4, true, q);
    if (cs != kAnimNoChannel) AnimSampleChannel(channels[cs], times, values, t, 3, false, S);
    AnimNormaliseRotation(q);
}

// L_j = [R(q) diag(S) | T]
CGPT_ANIM_FN void AnimComposeLocal(const float T[3], const float q[4], const float S[3], float L[12])
{
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    const float rot[9] = { 1.0f - 2.0f * (yy + zz), 2.0f * (xy - wz), 2.0f * (xz + wy),
                           2.0f * (xy + wz), 1.0f - 2.0f * (xx + zz), 2.0f * (yz - wx),
                           2.0f * (xz - wy), 2.0f * (yz + wx), 1.0f - 2.0f * (xx + yy) };
    for (int row = 0; row < 3; ++row) {
        L[4 * row] = rot[3 * row] * S[0];
        L[4 * row + 1] = rot[3 * row + 1] * S[1];
        L[4 * row + 2] = rot[3 * row + 2] * S[2];
        L[4 * row + 3] = T[row];
    }
}

// L_j at time t
CGPT_ANIM_FN void AnimLocalMatrix(const uint32_t* map, const AnimChannel* channels, const float* times, const float* values, const float* rest,
                                  uint32_t j, float t, float L[12])
{
    float T[3], q[4], S[3];
    AnimSampleJoint(map, channels, times, values, rest, j, t, T, q, S);
    AnimComposeLocal(T, q, S, L);
}

// ---- layers: wrapped times and a weighted blend of up to CGPT_ANIM_MAX_LAYERS clips (cgpt_scene_animate_layers) --------
//   range         begin = the smallest first-key time of the clip's channels, end = the largest last-key time (selections: exact); no channel: 0, 0
//   wrap          d = end - begin;  CLAMP, or !(d > 0 and d finite): t as given (the sampler holds the end keys)
//                 s = t - begin;  p = d (LOOP) or d + d (PINGPONG);  p not finite: t
//                 n = floorf(s / p);  r = s - n * p;  r < 0: r = r + p;  !(r >= 0 and r < p): r = 0;  PINGPONG and r > d: r = p - r;  begin + r
//   weights       a layer of weight 0 is inactive and never sampled; over the active ones in ascending order W = ((w0 + w1) + w2) + w3, a_l = w_l / W
//   blend         one active layer: its T, q, S as sampled.  Otherwise, componentwise over the active layers l0 < l1 < ...:
//                 T = a_l0 * T_l0, then T = T + a_l * T_l; S likewise; q likewise with q_l (l > l0) negated first when
//                 ((q_l0.x*q_l.x + q_l0.y*q_l.y) + q_l0.z*q_l.z) + q_l0.w*q_l.w < 0, and normalised once at the end
// floorf is exact, so it joins + - * / sqrtf without breaking bit equality.
CGPT_ANIM_FN float AnimWrapTime(float t, float begin, float end, uint32_t mode)
{
    const float d = end - begin;
    if (mode == CGPT_ANIM_WRAP_CLAMP || !(d > 0.0f && d < INFINITY)) return t;
    const float s = t - begin;
    const float p = mode == CGPT_ANIM_WRAP_LOOP ? d : d + d;
    if (!(p < INFINITY)) return t;
    const float n = floorf(s / p);
    float r = s - n * p;
    if (r < 0.0f) r = r + p;
    if (!(r >= 0.0f && r < p)) r = 0.0f;
    if (mode == CGPT_ANIM_WRAP_PINGPONG && r > d) r = p - r;
    return begin + r;
}

// One clip of a blend as the sampler reads it, with its wrapped time and normalised weight: 40 bytes
struct AnimLayer {
    const uint32_t* map;
    const AnimChannel* channels;
    const float* times;
    const float* values;
    float time, weight;
};

// T, q, S of joint j under n >= 1 active layers
CGPT_ANIM_FN void AnimBlendJoint(const AnimLayer* layers, uint32_t n, const float* rest, uint32_t j, float T[3], float q[4], float S[3])
{
    AnimSampleJoint(layers[0].map, layers[0].channels, layers[0].times, layers[0].values, rest, j, layers[0].time, T, q, S);
    if (n == 1u) return;
    const float q0[4] = { q[0], q[1], q[2], q[3] };
    const float a0 = layers[0].weight;
    for (int i = 0; i < 3; ++i) { T[i] = a0 * T[i]; S[i] = a0 * S[i]; }
    for (int i = 0; i < 4; ++i) q[i] = a0 * q[i];
    for (uint32_t l = 1; l < n; ++l) {
        float Tl[3], ql[4], Sl[3];
        AnimSampleJoint(layers[l].map, layers[l].channels, layers[l].times, layers[l].values, rest, j, layers[l].time, Tl, ql, Sl);
        const float dot = ((q0[0] * ql[0] + q0[1] * ql[1]) + q0[2] * ql[2]) + q0[3] * ql[3];
        if (dot < 0.0f) { ql[0] = -ql[0]; ql[1] = -ql[1]; ql[2] = -ql[2]; ql[3] = -ql[3]; }
        const float a = layers[l].weight;
        for (int i = 0; i < 3; ++i) { T[i] = T[i] + a * Tl[i]; S[i] = S[i] + a * Sl[i]; }
        for (int i = 0; i < 4; ++i) q[i] = q[i] + a * ql[i];
    }
    AnimNormaliseRotation(q);
}

// C = A o B; C may be neither A nor B
CGPT_ANIM_FN void AnimCompose(const float A[12], const float B[12], float C[12])
{
    for (int r = 0; r < 3; ++r) {
        const float a0 = A[4 * r], a1 = A[4 * r + 1], a2 = A[4 * r + 2], a3 = A[4 * r + 3];
        C[4 * r] = (a0 * B[0] + a1 * B[4]) + a2 * B[8];
        C[4 * r + 1] = (a0 * B[1] + a1 * B[5]) + a2 * B[9];
        C[4 * r + 2] = (a0 * B[2] + a1 * B[6]) + a2 * B[10];
        C[4 * r + 3] = ((a0 * B[3] + a1 * B[7]) + a2 * B[11]) + a3;
    }
}

// M_j from every joint's local matrix (12 floats a joint at locals): the bottom-up walk, the inverse bind matrix, the root (null: none)
CGPT_ANIM_FN void AnimJointMatrix(const float* locals, const int32_t* parents, const float* inverse_bind, const float* root, uint32_t j, float M[12])
{
    float G[12], N[12];
    for (int i = 0; i < 12; ++i) G[i] = locals[12 * (size_t)j + i];
    for (int32_t p = parents[j]; p >= 0; p = parents[p]) {
        AnimCompose(locals + 12 * (size_t)p, G, N);
        for (int i = 0; i < 12; ++i) G[i] = N[i];
    }
    AnimCompose(G, inverse_bind + 12 * (size_t)j, N);
    if (root) AnimCompose(root, N, M);
    else for (int i = 0; i < 12; ++i) M[i] = N[i];
}

// A clip as the sampler reads it: what CheckClip accepted, with the (joint, path) -> channel table
struct ClipTable {
    uint32_t n_joints = 0;
    std::vector<uint32_t> map;                                                // 3 n_joints
    std::vector<AnimChannel> channels;
    std::vector<float> times, values;
    float begin = 0.0f, end = 0.0f;                                           // the smallest first-key and the largest last-key time; no channel: 0, 0
};

// What cgpt_scene_set_skeleton and cgpth_animate_joints refuse of a skeleton: NULL, n_joints 0 or above kSkinMaxJoints, a parent below -1
// or >= n_joints, a cycle (a self-parent is one), an inverse bind, rest or root float that is not finite.  true, or false with the reason
bool CheckSkeleton(const cgpt_skeleton_desc* s, std::string& error);
// ... and cgpt_clip_create of a clip: NULL arrays, a channel whose joint, path or interpolation is out of range (CUBICSPLINE:
// `unsupported` is set), n_keys 0, keys that overrun times or values, two channels of one (joint, path), times that are not finite or
// not strictly increasing, a value that is not finite.  On success `table` is filled
bool CheckClip(const cgpt_clip_desc* c, ClipTable& table, std::string& error, bool& unsupported);
// The n_joints x 12 joint matrices of the skeleton under the clip at time t (finite).  The inputs have passed the two checks.
void AnimateJoints(const cgpt_skeleton_desc& s, const ClipTable& clip, float t, float* out);

// What cgpt_scene_animate_layers and cgpth_animate_layers refuse of an entry's layers once its clips are known (ranges[l] = {begin, end}
// of layer l's clip): n_layers outside [1, CGPT_ANIM_MAX_LAYERS], a time that is not finite, a weight that is not finite or negative, an
// unknown wrap mode, no weight above zero, a sum of weights that is not finite.  On success the active layers (weight > 0) in ascending
// order: index[k] their position in `layers`, time[k] wrapped, weight[k] normalised.  false with the reason ("layer l: ...")
struct AnimActiveLayers { uint32_t n = 0, index[CGPT_ANIM_MAX_LAYERS]; float time[CGPT_ANIM_MAX_LAYERS], weight[CGPT_ANIM_MAX_LAYERS]; };
bool ResolveLayers(const cgpt_clip_layer* layers, uint32_t n_layers, const float (*ranges)[2], AnimActiveLayers& active, std::string& error);
// The joint matrices under the blend of `active`'s layers of clips[active.index[k]]
void AnimateLayers(const cgpt_skeleton_desc& s, const ClipTable* const* clips, const AnimActiveLayers& active, float* out);

}  // namespace cgpt
