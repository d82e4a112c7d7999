"""Joint matrices from an animation clip in numpy: csrc/host/animation.h restated.

joint_matrices(skeleton, clip, t, np.float32) performs the header's float operations in the header's order, one rounding each, and
equals the host mirror (cgpth_animate_joints) and the device kernel bit for bit; with np.float64 the same statement is the model the
float32 one is held to.  skeleton = (parents, inverse_bind (n, 12), rest (n, 10), root (12,) or None); clip = (n_joints, channels
(m, 6) {joint, path, interpolation, n_keys, first_time, first_value}, times, values).
"""
import numpy as np

PATH_T, PATH_R, PATH_S = 0, 1, 2
STEP, LINEAR, CUBICSPLINE = 0, 1, 2


def find_key(times, t):
    """the last key with times[k] <= t, 0 when there is none: the header's binary search"""
    lo, hi = 0, len(times)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if times[mid] <= t:
            lo = mid
        else:
            hi = mid
    return lo


def sample_channel(times, values, interpolation, t, rotation, dt):
    """one channel's value at t, not yet normalised: times (n_keys,), values (n_keys, width), all of dtype dt"""
    k = find_key(times, t)
    a = values[k]
    if interpolation != LINEAR or k + 1 >= len(times) or not (times[k] <= t):
        return a.copy()
    u = (t - times[k]) / (times[k + 1] - times[k])
    b = values[k + 1]
    if rotation:
        dot = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]
        if dot < 0:
            b = -b
    return a + u * (b - a)


def normalise_rotations(q, dt):
    l2 = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
    ok = (l2 > 0) & np.isfinite(l2)
    with np.errstate(all="ignore"):
        rcp = dt(1) / np.sqrt(l2)
        out = q * rcp[:, None]
    out[~ok] = np.array([0, 0, 0, 1], dt)
    return out


def local_matrices(clip, rest, t, dt):
    """L_j (n, 12) at time t"""
    n_joints, channels, times, values = clip
    times, values = np.asarray(times, np.float32).astype(dt), np.asarray(values, np.float32).astype(dt)
    rest = np.asarray(rest, np.float32).reshape(-1, 10).astype(dt)
    t = dt(np.float32(t))
    T, q, S = rest[:, 0:3].copy(), rest[:, 3:7].copy(), rest[:, 7:10].copy()
    for joint, path, interpolation, n_keys, first_time, first_value in np.asarray(channels, np.int64).reshape(-1, 6):
        width = 4 if path == PATH_R else 3
        v = sample_channel(times[first_time:first_time + n_keys], values[first_value:first_value + width * n_keys].reshape(n_keys, width),
                           interpolation, t, path == PATH_R, dt)
        (T, q, S)[path][joint] = v
    q = normalise_rotations(q, dt)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    one, two = dt(1), dt(2)
    rot = [one - two * (yy + zz), two * (xy - wz), two * (xz + wy),
           two * (xy + wz), one - two * (xx + zz), two * (yz - wx),
           two * (xz - wy), two * (yz + wx), one - two * (xx + yy)]
    L = np.empty((rest.shape[0], 12), dt)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                L[:, 4 * r + c] = rot[3 * r + c] * S[:, c]
            L[:, 4 * r + 3] = T[:, r]
    return L


def compose(A, B):
    """C = A o B row by row of (n, 12) arrays: the header's summation order"""
    C = np.empty_like(B)
    with np.errstate(all="ignore"):
        for r in range(3):
            a0, a1, a2, a3 = A[:, 4 * r], A[:, 4 * r + 1], A[:, 4 * r + 2], A[:, 4 * r + 3]
            for c in range(3):
                C[:, 4 * r + c] = (a0 * B[:, c] + a1 * B[:, 4 + c]) + a2 * B[:, 8 + c]
            C[:, 4 * r + 3] = ((a0 * B[:, 3] + a1 * B[:, 7]) + a2 * B[:, 11]) + a3
    return C


def joint_matrices(skeleton, clip, t, dt=np.float32):
    """M_j (n, 12): the bottom-up walk of every joint at once, the inverse bind matrix, the root"""
    parents, inverse_bind, rest, root = skeleton
    parents = np.asarray(parents, np.int64)
    L = local_matrices(clip, rest, t, dt)
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


def rest_globals(parents, rest):
    """float64: every joint's global matrix (n, 3, 4) of the rest pose -- what an inverse bind matrix inverts"""
    n = len(parents)
    empty = (n, np.zeros((0, 6), np.uint32), np.zeros(0, np.float32), np.zeros(0, np.float32))
    ident = np.tile(np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]), (n, 1))
    return joint_matrices((parents, ident, rest, None), empty, 0.0, np.float64).reshape(n, 3, 4)


def nlerp_slerp_table(angles=(15.0, 30.0, 60.0, 90.0), steps=4001):
    """float64: for two keys theta apart, the largest angle in degrees between the normalised lerp and the slerp over the interval"""
    out = {}
    for deg in angles:
        h = np.deg2rad(deg) / 2
        a, b = np.array([0.0, 0.0, 0.0, 1.0]), np.array([np.sin(h), 0.0, 0.0, np.cos(h)])
        u = np.linspace(0.0, 1.0, steps)[:, None]
        q = a + u * (b - a)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        s = np.concatenate([np.sin(u * h), 0 * u, 0 * u, np.cos(u * h)], axis=1)
        out[deg] = float(np.rad2deg(2 * np.arccos(np.clip(np.abs((q * s).sum(1)), 0, 1))).max())
    return out
