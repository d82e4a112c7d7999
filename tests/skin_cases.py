"""Skins and poses shared by the skinning tests (tests/test_skin_reference.py, test_host_skinning.py, test_gpu_skinning.py).

A case is (joints (n, 3, 4) uint16, weights (n, 3, 4) float32, n_joints, matrices (n_joints, 12) float32) for a given (n, 18) bind array.
"""
import numpy as np

POSES = ("rigid", "bend", "four", "half", "one_joint", "wide")


def rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * (k @ k)


def matrix(a=None, b=(0.0, 0.0, 0.0), about=(0.0, 0.0, 0.0)):
    """the 12 floats of [A | b'] with b' = b + about - A about: A applied about a pivot, then a translation"""
    a = np.eye(3) if a is None else np.asarray(a, np.float64)
    about = np.asarray(about, np.float64)
    t = np.asarray(b, np.float64) + about - a @ about
    return np.concatenate([a, t[:, None]], axis=1).astype(np.float32).reshape(12)


def strip_mesh(n_tris, origin=(0.0, 0.0, 0.0), step=0.05, height=0.6):
    """a zig-zag triangle strip of n_tris triangles in the plane z = origin.z, with vertex normals that lean along the strip"""
    k = np.arange(n_tris + 2)
    v = np.zeros((n_tris + 2, 6), np.float32)
    v[:, 0] = origin[0] + step * k
    v[:, 1] = origin[1] + height * (k % 2)
    v[:, 2] = origin[2] + 0.02 * np.sin(0.3 * k)
    nrm = np.stack([0.3 * np.sin(0.2 * k), 0.2 * np.cos(0.1 * k), np.ones(len(k))], axis=1)
    v[:, 3:] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    t = np.arange(n_tris)
    idx = np.stack([t, np.where(t % 2 == 0, t + 1, t + 2), np.where(t % 2 == 0, t + 2, t + 1)], axis=1)
    return v, idx.astype(np.uint32).ravel()


def _heights(tris):
    """every corner's height between the mesh's lowest and highest point, in [0, 1] (along x for a mesh that is flat in y)"""
    p = tris.reshape(-1, 3, 6)[:, :, :3].astype(np.float64)
    y = p[:, :, 1] if p[:, :, 1].max() > p[:, :, 1].min() else p[:, :, 0]
    lo, hi = y.min(), y.max()
    return (y - lo) / (hi - lo) if hi > lo else np.zeros_like(y)


def make_case(pose, tris, seed=0):
    """the skin and the joint matrices of one of POSES for the bind triangles `tris`"""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 18)
    n = tris.shape[0]
    rng = np.random.default_rng(seed + 97 * POSES.index(pose))
    centre = tris.reshape(-1, 6)[:, :3].astype(np.float64).mean(axis=0)
    j = np.zeros((n, 3, 4), np.uint16)
    w = np.zeros((n, 3, 4), np.float32)
    if pose == "rigid":                                                      # one rigid joint carries everything; the others are named with weight 0
        n_joints = 3
        j[..., 0] = 2; j[..., 1] = 1
        w[..., 0] = 1.0
        m = [matrix(rotation((1, 2, 0.5), 70.0)), matrix(b=(50.0, 0.0, 0.0)), matrix(rotation((0.2, 1, 0.3), 25.0), (0.3, 0.2, -0.4), centre)]
    elif pose == "bend":                                                     # two joints, blended by height
        n_joints = 2
        t = _heights(tris).astype(np.float32)
        j[..., 1] = 1
        w[..., 0] = np.float32(1.0) - t; w[..., 1] = t
        m = [matrix(), matrix(rotation((1, 0, 0), 35.0), about=centre)]
    elif pose == "four":                                                     # four nonzero influences; a mirrored and a non-uniformly scaled joint among them
        n_joints = 6
        j[:] = np.argsort(rng.random((n, 3, n_joints)), axis=-1)[..., :4].astype(np.uint16)
        j[..., 0] = 4; j[..., 1] = 5                                        # the mirror and the scale reach every corner
        x = rng.uniform(0.1, 1.0, (n, 3, 4))
        w[:] = (x / x.sum(-1, keepdims=True)).astype(np.float32)
        m = [matrix(rotation(rng.normal(size=3), rng.uniform(-20, 20)), rng.uniform(-0.2, 0.2, 3), centre) for _ in range(4)]
        m.append(matrix(np.diag([-1.0, 1.0, 1.0]), about=centre))
        m.append(matrix(np.diag([1.3, 0.6, 0.9]) @ rotation((0, 0, 1), 15.0), about=centre))
    elif pose == "half":                                                     # weights that sum to 0.5 are used as given: the mesh shrinks towards the origin
        n_joints = 2
        t = _heights(tris).astype(np.float32)
        j[..., 1] = 1
        w[..., 0] = np.float32(0.5) * (np.float32(1.0) - t); w[..., 1] = np.float32(0.5) * t
        m = [matrix(b=2.0 * centre * 0.5), matrix(rotation((0, 0, 1), 20.0), 2.0 * centre * 0.5)]
    elif pose == "one_joint":
        n_joints = 1
        x = rng.uniform(0.1, 1.0, (n, 3, 4))
        w[:] = (x / x.sum(-1, keepdims=True)).astype(np.float32)            # four influences, all of joint 0
        m = [matrix(rotation((0, 1, 0), -40.0), (0.1, 0.3, 0.0), centre)]
    elif pose == "wide":                                                     # the joint limit, with corners on the last joint
        n_joints = 1024
        j[:] = rng.integers(0, n_joints, (n, 3, 4)).astype(np.uint16)
        j[0, 0, 0] = 1023; j[-1, 2, 3] = 1023
        x = rng.uniform(0.0, 1.0, (n, 3, 4))
        w[:] = (x / x.sum(-1, keepdims=True)).astype(np.float32)
        m = [matrix(rotation(rng.normal(size=3), rng.uniform(-8, 8)), rng.uniform(-0.05, 0.05, 3), centre) for _ in range(n_joints)]
    else:
        raise ValueError(pose)
    return j, w, n_joints, np.stack(m).astype(np.float32)
