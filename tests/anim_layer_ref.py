"""Joint matrices from a blend of animation clips in numpy: the layer part of csrc/host/animation.h restated.

joint_matrices_layers(skeleton, layers, np.float32) performs the header's float operations in the header's order, one rounding each,
and equals the host mirror (cgpth_animate_layers) and the device kernel bit for bit; with np.float64 the same statement is the model
the float32 one is held to.  skeleton and clip are tests/anim_ref.py's; layers = [(clip, time, weight, wrap), ...].

The wrap is evaluated in float32 for either dtype: a wrapped time is an input of the blend as a key time is, and the float64 model
takes the same float32 inputs.  What the wrap itself guarantees is tested by its own properties (tests/test_anim_layer_reference.py).
"""
import numpy as np

from anim_ref import LINEAR, PATH_R, compose, normalise_rotations, sample_channel

WRAP_CLAMP, WRAP_LOOP, WRAP_PINGPONG = 0, 1, 2
MAX_LAYERS = 4


def clip_range(clip):
    """(begin, end) as float32: the smallest first-key and the largest last-key time of the clip's channels; (0, 0) without channels"""
    _, channels, times, _ = clip
    times = np.asarray(times, np.float32)
    channels = np.asarray(channels, np.int64).reshape(-1, 6)
    if channels.shape[0] == 0:
        return np.float32(0), np.float32(0)
    return times[channels[:, 4]].min(), times[channels[:, 4] + channels[:, 3] - 1].max()


def wrap_time(t, begin, end, mode):
    """AnimWrapTime in float32, one rounding an operation"""
    f = np.float32
    t, begin, end = f(t), f(begin), f(end)
    with np.errstate(all="ignore"):
        d = end - begin
        if mode == WRAP_CLAMP or not (d > 0 and np.isfinite(d)):
            return t
        s = t - begin
        p = d if mode == WRAP_LOOP else d + d
        if not np.isfinite(p):
            return t
        n = np.floor(s / p)
        r = s - n * p
        if r < 0:
            r = r + p
        if not (r >= 0 and r < p):
            r = f(0)
        if mode == WRAP_PINGPONG and r > d:
            r = p - r
        return begin + r


def sample_joints(clip, rest, t, dt):
    """T (n, 3), q (n, 4) normalised, S (n, 3) of every joint at time t: AnimSampleJoint"""
    _, channels, times, values = clip
    times, values = np.asarray(times, np.float32).astype(dt), np.asarray(values, np.float32).astype(dt)
    rest = np.asarray(rest, np.float32).reshape(-1, 10).astype(dt)
    t = dt(np.float32(t))
    T, q, S = rest[:, 0:3].copy(), rest[:, 3:7].copy(), rest[:, 7:10].copy()
    for joint, path, interpolation, n_keys, first_time, first_value in np.asarray(channels, np.int64).reshape(-1, 6):
        width = 4 if path == PATH_R else 3
        v = sample_channel(times[first_time:first_time + n_keys], values[first_value:first_value + width * n_keys].reshape(n_keys, width),
                           interpolation, t, path == PATH_R, dt)
        (T, q, S)[path][joint] = v
    return T, normalise_rotations(q, dt), S


def compose_local(T, q, S, dt):
    """L_j (n, 12) = [R(q) diag(S) | T]: AnimComposeLocal"""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    one, two = dt(1), dt(2)
    rot = [one - two * (yy + zz), two * (xy - wz), two * (xz + wy),
           two * (xy + wz), one - two * (xx + zz), two * (yz - wx),
           two * (xz - wy), two * (yz + wx), one - two * (xx + yy)]
    L = np.empty((T.shape[0], 12), dt)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                L[:, 4 * r + c] = rot[3 * r + c] * S[:, c]
            L[:, 4 * r + 3] = T[:, r]
    return L


def active_layers(layers, dt):
    """[(clip, wrapped time float32, normalised weight dt)] of the layers with a weight above zero, in order: ResolveLayers"""
    act = [(clip, wrap_time(t, *clip_range(clip), wrap), np.float32(w)) for clip, t, w, wrap in layers if np.float32(w) != 0]
    assert act, "no layer has a weight above zero"
    W = dt(act[0][2])
    for _, _, w in act[1:]:
        W = W + dt(w)
    return [(clip, t, dt(w) / W) for clip, t, w in act]


def blend_joints(layers, rest, dt):
    """T, q, S of every joint under the layers: AnimBlendJoint"""
    act = active_layers(layers, dt)
    T, q, S = sample_joints(act[0][0], rest, act[0][1], dt)
    if len(act) == 1:
        return T, q, S
    q0 = q
    a0 = act[0][2]
    with np.errstate(all="ignore"):
        T, q, S = a0 * T, a0 * q, a0 * S
        for clip, t, a in act[1:]:
            Tl, ql, Sl = sample_joints(clip, rest, t, dt)
            dot = ((q0[:, 0] * ql[:, 0] + q0[:, 1] * ql[:, 1]) + q0[:, 2] * ql[:, 2]) + q0[:, 3] * ql[:, 3]
            ql = np.where((dot < 0)[:, None], -ql, ql)
            T, q, S = T + a * Tl, q + a * ql, S + a * Sl
    return T, normalise_rotations(q, dt), S


def joint_matrices_layers(skeleton, layers, dt=np.float32):
    """M_j (n, 12) under the blend: the local matrices from the blended T, q, S, then anim_ref.joint_matrices' walk"""
    parents, inverse_bind, rest, root = skeleton
    parents = np.asarray(parents, np.int64)
    L = compose_local(*blend_joints(layers, rest, dt), dt)
    G = L.copy()
    p = parents.copy()
    while True:
        live = np.nonzero(p >= 0)[0]
        if live.size == 0:
            break
        G[live] = compose(L[p[live]], G[live])
        p[live] = parents[p[live]]
    M = compose(G, np.asarray(inverse_bind, np.float32).reshape(-1, 12).astype(dt))
    if root is not None:
        M = compose(np.broadcast_to(np.asarray(root, np.float32).reshape(1, 12).astype(dt), M.shape), M)
    return M
