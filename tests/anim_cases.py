"""Skeletons and clips shared by the animation tests (tests/test_anim_reference.py, test_host_animation.py, test_gpu_animation.py).

A case is (skeleton, clip, times): skeleton = (parents int32 (n,), inverse_bind float32 (n, 12), rest float32 (n, 10), root float32
(12,) or None), clip = (n_joints, channels uint32 (m, 6), times float32, values float32), times the instants to evaluate it at.
"""
import numpy as np

from anim_ref import LINEAR, PATH_R, PATH_S, PATH_T, STEP, rest_globals

IDENTITY = np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])


def quat(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = np.deg2rad(deg) / 2
    return np.concatenate([np.sin(h) * a, [np.cos(h)]])


def inverse_bind_of(parents, rest):
    """the inverses of the rest pose's global matrices, float64 rounded once: the rest pose then skins to (nearly) the identity"""
    g = rest_globals(parents, rest)
    out = np.empty((len(parents), 12), np.float32)
    for j, m in enumerate(g):
        a = np.linalg.inv(m[:, :3])
        out[j] = np.concatenate([a, (-a @ m[:, 3])[:, None]], axis=1).reshape(12)
    return out


class ClipBuilder:
    def __init__(self, n_joints):
        self.n_joints, self.channels, self.times, self.values = n_joints, [], [], []

    def add(self, joint, path, interpolation, times, values):
        times = np.asarray(times, np.float32).ravel()
        values = np.asarray(values, np.float32).reshape(times.size, -1)
        assert values.shape[1] == (4 if path == PATH_R else 3)
        self.channels.append((joint, path, interpolation, times.size, len(self.times), len(self.values)))
        self.times += times.tolist()
        self.values += values.ravel().tolist()
        return self

    def clip(self):
        return (self.n_joints, np.asarray(self.channels, np.uint32).reshape(-1, 6), np.asarray(self.times, np.float32), np.asarray(self.values, np.float32))


def arm():
    """three joints in a chain, every edge of the sampler by hand: t before the first key, on a key, between keys, on and after the
    last; a one-key channel; STEP; a joint without a channel; consecutive rotation keys with a negative dot; a zero quaternion key;
    rest rotations that are not unit"""
    parents = np.int32([-1, 0, 1])
    rest = np.float32([[0.0, 0.0, 0.0, 0, 0, 0, 2.0, 1, 1, 1],                # a rest rotation of length 2
                       [0.0, 0.5, 0.0, *quat((0, 0, 1), 10.0), 1.0, 1.1, 0.9],
                       [0.0, 0.4, 0.1, *(1.5 * quat((1, 1, 0), -20.0)), 1, 1, 1]])
    b = ClipBuilder(3)
    q0, q1, q2 = quat((1, 0, 0), 0.0), quat((1, 0, 0), 80.0), quat((1, 0, 0), 200.0)
    b.add(1, PATH_R, LINEAR, [0.25, 0.5, 1.0, 1.5], [q0, -q1, q2, [0, 0, 0, 0]])   # dot(q0, -q1) < 0, dot(-q1, q2) < 0; the last key has no length
    b.add(1, PATH_T, LINEAR, [0.0, 1.0], [[0, 0.5, 0], [0.2, 0.7, -0.1]])
    b.add(2, PATH_S, STEP, [0.0, 0.5, 1.0], [[1, 1, 1], [1.2, 0.8, 1.0], [0.5, 0.5, 2.0]])
    b.add(0, PATH_T, LINEAR, [0.75], [[0.1, 0.0, -0.3]])                      # one key
    b.add(2, PATH_R, STEP, [0.1, 0.9], [quat((0, 1, 0), 30.0), 3.0 * quat((0, 1, 0), -45.0)])
    times = [-1.0, 0.0, 0.1, 0.25, 0.3, 0.5, 0.75, 0.8, 0.9, 1.0, 1.25, 1.4, 1.5, 3.0]
    return (parents, inverse_bind_of(parents, rest), rest, None), b.clip(), times


def rig(n, seed=0, shape="tree", root=False, swing=25.0):
    """n joints: a chain (as deep as n), a chain `reversed` in index order (children before parents), a random `tree` in shuffled
    index order, or `two_roots`; about two thirds of the (joint, path) pairs have a channel of 1 .. 5 keys, STEP or LINEAR"""
    rng = np.random.default_rng(1000 * n + seed)
    if shape == "chain":
        parents = np.arange(-1, n - 1)
    elif shape == "reversed":
        parents = np.concatenate([np.arange(1, n), [-1]])
    else:
        parents = np.array([-1] + [int(rng.integers(0, j)) for j in range(1, n)])
        if shape == "two_roots" and n > 1:
            parents[1] = -1
        order = rng.permutation(n)                                            # old index -> new index: parents land on either side of their children
        moved = np.empty(n, np.int64)
        moved[order] = np.where(parents >= 0, order[np.maximum(parents, 0)], -1)
        parents = moved
    parents = parents.astype(np.int32)
    k = 1.0 / np.sqrt(n)                                                      # a chain of n such joints stays within a few units
    rest = np.empty((n, 10), np.float32)
    rest[:, 0:3] = rng.uniform(-0.4, 0.4, (n, 3)) * k
    rest[:, 3:7] = [rng.uniform(0.5, 1.5) * quat(rng.normal(size=3), rng.uniform(-swing, swing) * k) for _ in range(n)]
    rest[:, 7:10] = 1.0 + rng.uniform(-0.2, 0.2, (n, 3)) * k
    b = ClipBuilder(n)
    for j in range(n):
        for path in (PATH_T, PATH_R, PATH_S):
            if rng.random() > 0.67:
                continue
            keys = int(rng.choice([1, 2, 3, 5]))
            t = np.cumsum(rng.uniform(0.05, 0.4, keys)) - 0.1
            if path == PATH_R:
                v = [rng.choice([-1.0, 1.0]) * quat(rng.normal(size=3), rng.uniform(-swing, swing) * k) for _ in range(keys)]
            elif path == PATH_T:
                v = rest[j, 0:3] + rng.uniform(-0.2, 0.2, (keys, 3)) * k
            else:
                v = rest[j, 7:10] + rng.uniform(-0.1, 0.1, (keys, 3)) * k
            b.add(j, path, int(rng.choice([STEP, LINEAR])), t, v)
    root_m = None
    if root:
        a = np.eye(3) * 0.9
        a[0, 1] = 0.1
        root_m = np.concatenate([a, [[0.05], [-0.1], [0.02]]], axis=1).astype(np.float32).reshape(12)
    times = [-0.5, 0.0, 0.37, 0.7, 1.0, 2.5]
    return (parents, inverse_bind_of(parents, rest), rest, root_m), b.clip(), times


def overflow(n=3):
    """three chained scales of 1e30: the composed matrix leaves float's range"""
    parents = np.arange(-1, n - 1).astype(np.int32)
    rest = np.tile(np.float32([0, 0, 0, 0, 0, 0, 1, 1e30, 1e30, 1e30]), (n, 1))
    return (parents, np.tile(IDENTITY, (n, 1)), rest, None), ClipBuilder(n).clip(), [0.0]


CASES = {
    "arm": arm,
    "one": lambda: rig(1, 1, "chain"),
    "reversed": lambda: rig(5, 2, "reversed", root=True),
    "two_roots": lambda: rig(6, 3, "two_roots", root=True),
    "deep": lambda: rig(64, 4, "chain"),
    "j255": lambda: rig(255, 5),
    "j256": lambda: rig(256, 6, root=True),
    "j257": lambda: rig(257, 7, "chain"),                                     # a chain as deep as the joint count, past one block's stride
    "j1024": lambda: rig(1024, 8),
}
