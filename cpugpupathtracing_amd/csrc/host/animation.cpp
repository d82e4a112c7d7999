// animation.cpp -- the host mirror of cgpt_scene_animate_objects' joint matrices (animation.h states the arithmetic) and the validation
// of a skeleton and of a clip.  Host only.
#include "animation.h"

#include "skinning.h"

namespace cgpt {

void AnimateJoints(const cgpt_skeleton_desc& s, const ClipTable& clip, float t, float* out)
{
    std::vector<float> locals(12 * (size_t)s.n_joints);
    for (uint32_t j = 0; j < s.n_joints; ++j)
        AnimLocalMatrix(clip.map.data(), clip.channels.data(), clip.times.data(), clip.values.data(), s.rest, j, t, locals.data() + 12 * (size_t)j);
    for (uint32_t j = 0; j < s.n_joints; ++j)
        AnimJointMatrix(locals.data(), s.parents, s.inverse_bind, s.root, j, out + 12 * (size_t)j);
}

void AnimateLayers(const cgpt_skeleton_desc& s, const ClipTable* const* clips, const AnimActiveLayers& active, float* out)
{
    AnimLayer layers[CGPT_ANIM_MAX_LAYERS];
    for (uint32_t k = 0; k < active.n; ++k) {
        const ClipTable& c = *clips[active.index[k]];
        layers[k] = { c.map.data(), c.channels.data(), c.times.data(), c.values.data(), active.time[k], active.weight[k] };
    }
    std::vector<float> locals(12 * (size_t)s.n_joints);
    for (uint32_t j = 0; j < s.n_joints; ++j) {
        float T[3], q[4], S[3];
        AnimBlendJoint(layers, active.n, s.rest, j, T, q, S);
        AnimComposeLocal(T, q, S, locals.data() + 12 * (size_t)j);
    }
    for (uint32_t j = 0; j < s.n_joints; ++j)
        AnimJointMatrix(locals.data(), s.parents, s.inverse_bind, s.root, j, out + 12 * (size_t)j);
}

bool ResolveLayers(const cgpt_clip_layer* layers, uint32_t n_layers, const float (*ranges)[2], AnimActiveLayers& active, std::string& error)
{
    AnimActiveLayers out;
    for (uint32_t l = 0; l < n_layers; ++l) {
        const cgpt_clip_layer& y = layers[l];
        const std::string where = "layer " + std::to_string(l) + ": ";
        if (!std::isfinite(y.time)) { error = where + "time is not finite"; return false; }
        if (!std::isfinite(y.weight)) { error = where + "weight is not finite"; return false; }
        if (y.weight < 0.0f) { error = where + "weight " + std::to_string(y.weight) + " is negative"; return false; }
        if (y.wrap > CGPT_ANIM_WRAP_PINGPONG) { error = where + "wrap mode " + std::to_string(y.wrap) + " is none of CLAMP, LOOP, PINGPONG"; return false; }
        if (y.weight == 0.0f) continue;                                       // inactive: never sampled
        out.index[out.n] = l;
        out.time[out.n] = AnimWrapTime(y.time, ranges[l][0], ranges[l][1], y.wrap);
        out.weight[out.n] = y.weight;
        ++out.n;
    }
    if (out.n == 0u) { error = "no layer has a weight above zero"; return false; }
    float W = out.weight[0];
    for (uint32_t k = 1; k < out.n; ++k) W = W + out.weight[k];
    if (!std::isfinite(W)) { error = "the sum of the layers' weights is not finite"; return false; }
    for (uint32_t k = 0; k < out.n; ++k) out.weight[k] = out.weight[k] / W;
    active = out;
    return true;
}

bool CheckSkeleton(const cgpt_skeleton_desc* s, std::string& error)
{
    if (!s) { error = "skeleton is null"; return false; }
    if (!s->parents) { error = "parents is null"; return false; }
    if (!s->inverse_bind) { error = "inverse_bind is null"; return false; }
    if (!s->rest) { error = "rest is null"; return false; }
    const uint32_t n = s->n_joints;
    if (n == 0 || n > kSkinMaxJoints) {
        error = "n_joints " + std::to_string(n) + " outside [1, " + std::to_string(kSkinMaxJoints) + "]";
        return false;
    }
    for (uint32_t j = 0; j < n; ++j)
        if (s->parents[j] < -1 || s->parents[j] >= (int32_t)n) {
            error = "joint " + std::to_string(j) + ": parent " + std::to_string(s->parents[j]) + " outside [-1, " + std::to_string(n) + ")";
            return false;
        }
    for (uint32_t j = 0; j < n; ++j) {                                        // a walk that has not reached a root after n steps goes round
        int32_t p = s->parents[j];
        for (uint32_t steps = 0; p >= 0; p = s->parents[p])
            if (++steps >= n) { error = "joint " + std::to_string(j) + ": its parents form a cycle"; return false; }
    }
    for (size_t k = 0; k < 12 * (size_t)n; ++k)
        if (!std::isfinite(s->inverse_bind[k])) { error = "joint " + std::to_string(k / 12) + ": inverse bind entry " + std::to_string(k % 12) + " is not finite"; return false; }
    for (size_t k = 0; k < 10 * (size_t)n; ++k)
        if (!std::isfinite(s->rest[k])) { error = "joint " + std::to_string(k / 10) + ": rest float " + std::to_string(k % 10) + " is not finite"; return false; }
    if (s->root)
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(s->root[k])) { error = "root entry " + std::to_string(k) + " is not finite"; return false; }
    return true;
}

bool CheckClip(const cgpt_clip_desc* c, ClipTable& table, std::string& error, bool& unsupported)
{
    unsupported = false;
    if (!c) { error = "clip is null"; return false; }
    if (c->n_joints == 0 || c->n_joints > kSkinMaxJoints) {
        error = "n_joints " + std::to_string(c->n_joints) + " outside [1, " + std::to_string(kSkinMaxJoints) + "]";
        return false;
    }
    if (c->n_channels != 0 && !c->channels) { error = "channels is null"; return false; }
    if (c->n_times != 0 && !c->times) { error = "times is null"; return false; }
    if (c->n_values != 0 && !c->values) { error = "values is null"; return false; }
    if (c->n_channels > 3 * c->n_joints) { error = std::to_string(c->n_channels) + " channels for " + std::to_string(c->n_joints) + " joints: at most one per joint and path"; return false; }
    ClipTable out;
    out.n_joints = c->n_joints;
    out.map.assign(3 * (size_t)c->n_joints, kAnimNoChannel);
    out.channels.resize(c->n_channels);
    for (uint32_t i = 0; i < c->n_channels; ++i) {
        const cgpt_clip_channel& ch = c->channels[i];
        const std::string where = "channel " + std::to_string(i) + ": ";
        if (ch.joint >= c->n_joints) { error = where + "joint " + std::to_string(ch.joint) + " >= n_joints " + std::to_string(c->n_joints); return false; }
        if (ch.path > CGPT_ANIM_PATH_SCALE) { error = where + "path " + std::to_string(ch.path) + " is none of translation, rotation, scale"; return false; }
        if (ch.interpolation == CGPT_ANIM_CUBICSPLINE) { error = where + "CUBICSPLINE interpolation is not built"; unsupported = true; return false; }
        if (ch.interpolation > CGPT_ANIM_LINEAR) { error = where + "interpolation " + std::to_string(ch.interpolation) + " is neither STEP nor LINEAR"; return false; }
        if (ch.n_keys == 0) { error = where + "n_keys is 0"; return false; }
        const uint64_t width = ch.path == CGPT_ANIM_PATH_ROTATION ? 4u : 3u;
        if ((uint64_t)ch.first_time + ch.n_keys > c->n_times) { error = where + "keys " + std::to_string(ch.first_time) + " .. +" + std::to_string(ch.n_keys) + " overrun the " + std::to_string(c->n_times) + " times"; return false; }
        if ((uint64_t)ch.first_value + width * ch.n_keys > c->n_values) { error = where + "keys overrun the " + std::to_string(c->n_values) + " values"; return false; }
        uint32_t& slot = out.map[3 * (size_t)ch.joint + ch.path];
        if (slot != kAnimNoChannel) { error = where + "joint " + std::to_string(ch.joint) + " already has a channel of path " + std::to_string(ch.path) + " (channel " + std::to_string(slot) + ")"; return false; }
        slot = i;
        const float* t = c->times + ch.first_time;
        for (uint32_t k = 0; k < ch.n_keys; ++k) {
            if (!std::isfinite(t[k])) { error = where + "time " + std::to_string(k) + " is not finite"; return false; }
            if (k > 0 && !(t[k] > t[k - 1])) { error = where + "time " + std::to_string(k) + " does not lie after time " + std::to_string(k - 1); return false; }
        }
        const float* v = c->values + ch.first_value;
        for (uint64_t k = 0; k < width * ch.n_keys; ++k)
            if (!std::isfinite(v[k])) { error = where + "key " + std::to_string(k / width) + ": value " + std::to_string(k % width) + " is not finite"; return false; }
        out.channels[i] = { ch.interpolation, ch.n_keys, ch.first_time, ch.first_value };
        out.begin = i == 0 || t[0] < out.begin ? t[0] : out.begin;            // the range: selections, hence exact
        out.end = i == 0 || t[ch.n_keys - 1] > out.end ? t[ch.n_keys - 1] : out.end;
    }
    if (c->n_times) out.times.assign(c->times, c->times + c->n_times);
    if (c->n_values) out.values.assign(c->values, c->values + c->n_values);
    table = std::move(out);
    return true;
}

}  // namespace cgpt
