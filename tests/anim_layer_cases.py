"""Skeletons, clips and layer sets shared by the layer tests (tests/test_anim_layer_reference.py, test_host_animation_layers.py,
test_gpu_animation_layers.py).

A case is (skeleton, sets): skeleton as in tests/anim_cases.py, sets a list of layer lists [(clip, time, weight, wrap), ...] to
evaluate on it.  Every set keeps the first active layer's normalised weight at 0.05 or above (the smallest here is 0.25 / 3.75), so
the blended quaternion is well conditioned for the float64 comparison.
"""
import numpy as np

from anim_cases import ClipBuilder, arm, quat, rig
from anim_layer_ref import WRAP_CLAMP, WRAP_LOOP, WRAP_PINGPONG, clip_range
from anim_ref import LINEAR, PATH_R, PATH_S, PATH_T, STEP

C, L, P = WRAP_CLAMP, WRAP_LOOP, WRAP_PINGPONG
EMPTY = lambda n: ClipBuilder(n).clip()


def clip_for(rest, seed, cover=0.67, swing=25.0, start=-0.1):
    """a random clip on the skeleton with `rest`, as anim_cases.rig draws one: about `cover` of the (joint, path) pairs have a channel of
    1 .. 5 keys, STEP or LINEAR; rotation keys carry random signs, so layers meet with negative dots; the keys begin near `start`"""
    n = len(rest)
    rng = np.random.default_rng(77000 + 1000 * n + seed)
    k = 1.0 / np.sqrt(n)
    b = ClipBuilder(n)
    for j in range(n):
        for path in (PATH_T, PATH_R, PATH_S):
            if rng.random() > cover:
                continue
            keys = int(rng.choice([1, 2, 3, 5]))
            t = np.cumsum(rng.uniform(0.05, 0.4, keys)) + start
            if path == PATH_R:
                v = [rng.choice([-1.0, 1.0]) * quat(rng.normal(size=3), rng.uniform(-swing, swing) * k) for _ in range(keys)]
            elif path == PATH_T:
                v = rest[j, 0:3] + rng.uniform(-0.2, 0.2, (keys, 3)) * k
            else:
                v = rest[j, 7:10] + rng.uniform(-0.1, 0.1, (keys, 3)) * k
            b.add(j, path, int(rng.choice([STEP, LINEAR])), t, v)
    return b.clip()


def negated(clip):
    """the same motion with every rotation key negated: each sampled rotation has a negative dot with the original's"""
    n, ch, t, v = clip
    v = v.copy()
    for joint, path, _, n_keys, _, first_value in ch:
        if path == PATH_R:
            v[first_value:first_value + 4 * n_keys] *= np.float32(-1)
    return n, ch, t, v


def clips_of(n, seed, shape, root):
    """a skeleton of n joints and four clips on it that cover different (joint, path) sets: rig's own, a sparse one (most joints take
    rest), a dense one that begins later, and the first with its rotations negated"""
    skeleton, own, _ = rig(n, seed, shape, root)
    rest = skeleton[2]
    return skeleton, [own, clip_for(rest, seed + 1, cover=0.3), clip_for(rest, seed + 2, cover=0.9, start=0.2), negated(own)]


def blends(n, seed, shape="tree", root=False):
    """1 .. 4 layers, an inactive layer first, in the middle and last, wrap modes mixed, each layer at its own time"""
    skeleton, (a, b, c, d) = clips_of(n, seed, shape, root)
    sets = [[(a, 0.37, 1.0, C)],
            [(a, 0.37, 0.25, C), (b, 0.9, 0.75, L)],
            [(b, -0.2, 2.0, P), (d, 0.5, 0.5, C), (c, 1.7, 1.0, L)],
            [(a, 0.1, 1.0, L), (b, 0.6, 0.5, P), (c, 0.45, 0.25, C), (d, 3.3, 2.0, P)],
            [(c, 0.4, 0.0, L), (a, 0.7, 1.0, C), (b, 0.2, 3.0, C)],               # an inactive layer first
            [(a, 0.7, 1.0, P), (c, 0.4, 0.0, C), (d, 0.2, 1.0, L), (b, 0.3, 0.5, C)],   # in the middle
            [(b, 0.25, 0.5, C), (a, 2.5, 0.5, L), (c, 0.4, 0.0, P)],              # last
            [(c, 0.1, 0.0, C), (d, 0.62, 0.3, L)]]                                # one active layer behind an inactive one
    return skeleton, sets


def wraps():
    """anim_cases.arm's clip (keys from 0 to 1.5) under every wrap mode at t < begin, t = begin, inside, t = end, many periods out and
    negative, blended with a second clip whose range is another"""
    skeleton, clip, _ = arm()
    other = clip_for(skeleton[2], 5, cover=0.8, swing=60.0, start=0.3)
    begin, end = clip_range(clip)
    assert (begin, end) == (np.float32(0), np.float32(1.5))
    sets = []
    for mode in (C, L, P):
        for t in (-0.4, 0.0, 0.8, 1.5, 1.5 * 4097 + 0.3, -1.5 * 1001 - 0.7, 2.25, 3.0):
            sets.append([(clip, t, 1.0, mode)])
            sets.append([(clip, t, 0.6, mode), (other, 0.5 * t, 0.4, mode)])
    return skeleton, sets


def degenerate():
    """d = 0: a clip of one key and a clip without channels, under LOOP and PINGPONG (the time passes as given), alone and blended"""
    skeleton, clip, _ = arm()
    one_key = ClipBuilder(3).add(1, PATH_R, LINEAR, [0.75], [quat((0, 1, 0), 50.0)]).add(2, PATH_T, STEP, [0.75], [[0.3, 0.1, 0.0]]).clip()
    none = EMPTY(3)
    sets = [[(one_key, 5.0, 1.0, L)], [(none, -2.0, 1.0, P)], [(one_key, 0.75, 1.0, P), (none, 9.0, 1.0, L)],
            [(none, 0.0, 0.5, L), (clip, 0.3, 0.5, P), (one_key, -1.0, 1.0, L)]]
    return skeleton, sets


CASES = {
    "wraps": wraps,
    "degenerate": degenerate,
    "one": lambda: blends(1, 1, "chain"),
    "three": lambda: blends(3, 2, "reversed", root=True),
    "j255": lambda: blends(255, 5),
    "j256": lambda: blends(256, 6, root=True),
    "j257": lambda: blends(257, 7, "chain"),
    "j1024": lambda: blends(1024, 8, root=True),
}
