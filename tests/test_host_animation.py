"""The host mirror of the animation kernel (cgpth_animate_joints; csrc/host/animation.cpp) against tests/anim_ref.py's float32 statement
of csrc/host/animation.h, bit for bit, and every refusal of CheckSkeleton and CheckClip.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from anim_cases import CASES, IDENTITY, ClipBuilder, overflow
from anim_ref import CUBICSPLINE, LINEAR, PATH_R, PATH_S, PATH_T, STEP, joint_matrices


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_binding_declares_the_animation_calls():
    for name in ("cgpth_animate_joints", "cgpt_scene_set_skeleton", "cgpt_clip_create", "cgpt_clip_destroy", "cgpt_scene_animate_objects",
                 "cgpt_scene_get_joint_matrices"):
        assert name in N.PROTOTYPES and hasattr(N.lib(), name)
    assert N.lib().cgpt_abi_version() == 2 and "animate_joints" in P.__all__
    assert all(hasattr(P.Renderer, f) for f in ("set_skeleton", "create_clip", "destroy_clip", "animate_objects", "joint_matrices"))
    assert C.sizeof(N.SkeletonDesc) == 40 and C.sizeof(N.ClipChannel) == 24 and C.sizeof(N.ClipDesc) == 48 and C.sizeof(N.Animation) == 24
    assert (N.ANIM_PATH_TRANSLATION, N.ANIM_PATH_ROTATION, N.ANIM_PATH_SCALE) == (PATH_T, PATH_R, PATH_S)
    assert (N.ANIM_STEP, N.ANIM_LINEAR, N.ANIM_CUBICSPLINE) == (STEP, LINEAR, CUBICSPLINE)


@pytest.mark.parametrize("name", CASES)
def test_the_mirror_equals_the_float32_statement_bit_for_bit(name):
    skeleton, clip, times = CASES[name]()
    for t in times:
        got = P.animate_joints(skeleton, clip, t)
        want = joint_matrices(skeleton, clip, t, np.float32)
        assert got.shape == want.shape == (len(skeleton[0]), 12)
        assert np.array_equal(bits(got), bits(want)), (name, t)
    if skeleton[3] is not None:                                               # the root is one more product, and its absence none at all
        without = P.animate_joints(skeleton[:3] + (None,), clip, times[2])
        assert np.array_equal(bits(without), bits(joint_matrices(skeleton[:3] + (None,), clip, times[2]))) and not np.array_equal(bits(without), bits(got))


def test_an_overflow_is_computed_not_refused():
    skeleton, clip, times = overflow()
    got = P.animate_joints(skeleton, clip, 0.0)
    assert np.array_equal(bits(got), bits(joint_matrices(skeleton, clip, 0.0))) and not np.isfinite(got[2]).all() and np.isfinite(got[0]).all()


def refused(skeleton, clip, t=0.0):
    with pytest.raises(P.HostError) as e:
        P.animate_joints(skeleton, clip, t)
    return e.value.code, str(e.value)


def test_every_refusal_of_a_skeleton():
    (parents, ib, rest, root), clip, _ = CASES["two_roots"]()
    n = len(parents)
    def with_parents(**kw):
        p = parents.copy()
        for j, v in kw.items():
            p[int(j[1:])] = v
        return (p, ib, rest, root)
    leaf = int([j for j in np.setdiff1d(np.arange(n), parents) if parents[j] >= 0][0])   # a joint that is nobody's parent and has one
    up = int(parents[leaf])
    cases = [(with_parents(**{f"j{leaf}": leaf}), f"joint {leaf}: its parents form a cycle"),        # a self-parent
             (with_parents(**{f"j{up}": leaf}), "its parents form a cycle"),                          # a 2-cycle: leaf -> up -> leaf
             (with_parents(j0=n), f"joint 0: parent {n} outside [-1, {n})"),
             (with_parents(j1=-2), f"joint 1: parent -2 outside [-1, {n})")]
    bad = ib.copy(); bad[2, 7] = np.inf
    cases.append(((parents, bad, rest, root), "joint 2: inverse bind entry 7 is not finite"))
    bad = rest.copy(); bad[3, 9] = np.nan
    cases.append(((parents, ib, bad, root), "joint 3: rest float 9 is not finite"))
    bad = root.copy(); bad[11] = -np.inf
    cases.append(((parents, ib, rest, bad), "root entry 11 is not finite"))
    for skeleton, text in cases:
        code, msg = refused(skeleton, clip)
        assert code == N.CGPT_ERR_INVALID and text in msg, (text, msg)
    # counts and NULL arrays, through the C call
    L = N.lib()
    from cpugpupathtracing_amd.scene import _clip_desc, _skeleton_desc
    cd, keep_c = _clip_desc(*clip)
    out = np.empty((n, 12), np.float32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    for field, text in (("parents", "parents is null"), ("inverse_bind", "inverse_bind is null"), ("rest", "rest is null")):
        sd, keep_s = _skeleton_desc(parents, ib, rest, root)
        setattr(sd, field, None)
        assert L.cgpth_animate_joints(C.byref(sd), C.byref(cd), 0.0, fp, n) == N.CGPT_ERR_INVALID and text in L.cgpth_last_error().decode()
    for joints, text in ((0, "n_joints 0 outside [1, 1024]"), (1025, "n_joints 1025 outside [1, 1024]")):
        sd, keep_s = _skeleton_desc(parents, ib, rest, root)
        sd.n_joints = joints
        assert L.cgpth_animate_joints(C.byref(sd), C.byref(cd), 0.0, fp, n) == N.CGPT_ERR_INVALID and text in L.cgpth_last_error().decode()
    sd, keep_s = _skeleton_desc(parents, ib, rest, root)
    assert L.cgpth_animate_joints(None, C.byref(cd), 0.0, fp, n) == N.CGPT_ERR_INVALID and "skeleton is null" in L.cgpth_last_error().decode()
    assert L.cgpth_animate_joints(C.byref(sd), None, 0.0, fp, n) == N.CGPT_ERR_INVALID and "clip is null" in L.cgpth_last_error().decode()
    assert L.cgpth_animate_joints(C.byref(sd), C.byref(cd), 0.0, None, n) == N.CGPT_ERR_INVALID and "out is null" in L.cgpth_last_error().decode()
    assert L.cgpth_animate_joints(C.byref(sd), C.byref(cd), 0.0, fp, n - 1) == N.CGPT_ERR_INVALID and "got room for" in L.cgpth_last_error().decode()
    for t in (np.nan, np.inf, -np.inf):
        assert L.cgpth_animate_joints(C.byref(sd), C.byref(cd), t, fp, n) == N.CGPT_ERR_INVALID and "time is not finite" in L.cgpth_last_error().decode()
    assert L.cgpth_animate_joints(C.byref(sd), C.byref(cd), 0.25, fp, n) == N.CGPT_OK


def test_every_refusal_of_a_clip():
    skeleton, _, _ = CASES["two_roots"]()
    n = len(skeleton[0])
    q = [0, 0, 0, 1]
    def one(joint=1, path=PATH_T, interpolation=LINEAR, times=(0.0, 1.0), values=((0, 0, 0), (1, 1, 1)), n_joints=n):
        b = ClipBuilder(n_joints).add(0, PATH_S, STEP, [0.0], [[1, 1, 1]])
        width = 4 if path == PATH_R else 3
        b.channels.append((joint, path, interpolation, len(times), len(b.times), len(b.values)))
        b.times += list(times)
        need = width * len(times)
        b.values += ([float(x) for v in values for x in v] + [0.0] * need)[:need]
        return b
    inval, unsup = N.CGPT_ERR_INVALID, N.CGPT_ERR_UNSUPPORTED
    cases = [(one(joint=n).clip(), inval, f"channel 1: joint {n} >= n_joints {n}"),
             (one(path=3).clip(), inval, "channel 1: path 3 is none of translation, rotation, scale"),
             (one(interpolation=CUBICSPLINE).clip(), unsup, "channel 1: CUBICSPLINE interpolation is not built"),
             (one(interpolation=7).clip(), inval, "channel 1: interpolation 7 is neither STEP nor LINEAR"),
             (one(times=(), values=()).clip(), inval, "channel 1: n_keys is 0"),
             (one(joint=0, path=PATH_S).clip(), inval, "channel 1: joint 0 already has a channel of path 2 (channel 0)"),     # a duplicate (joint, path)
             (one(times=(0.5, 0.5)).clip(), inval, "channel 1: time 1 does not lie after time 0"),                         # equal times
             (one(times=(0.5, 0.25)).clip(), inval, "channel 1: time 1 does not lie after time 0"),
             (one(times=(0.0, np.nan)).clip(), inval, "channel 1: time 1 is not finite"),
             (one(times=(0.0, np.inf)).clip(), inval, "channel 1: time 1 is not finite"),
             (one(values=((0, 0, 0), (1, np.nan, 1))).clip(), inval, "channel 1: key 1: value 1 is not finite"),           # a NaN key
             (one(path=PATH_R, values=(q, (0, np.inf, 0, 1))).clip(), inval, "channel 1: key 1: value 1 is not finite"),
             (one(n_joints=n + 1).clip(), inval, f"the clip animates {n + 1} joints, the skeleton has {n}")]
    for clip, code, text in cases:
        got, msg = refused(skeleton, clip)
        assert got == code and text in msg, (text, msg)
    # an overrun of either array
    nj, ch, t, v = one().clip()
    for clip, text in (((nj, ch, t[:-1], v), "overrun the 2 times"), ((nj, ch, t, v[:-1]), "keys overrun the 8 values")):
        got, msg = refused(skeleton, clip)
        assert got == inval and "channel 1: " in msg and text in msg, (text, msg)
    ch2 = ch.copy(); ch2[1, 4] = 0xFFFFFFFF                                   # first_time + n_keys wraps in 32 bits
    got, msg = refused(skeleton, (nj, ch2, t, v))
    assert got == inval and "overrun" in msg
    many = np.tile(ch[:1], (3 * n + 1, 1))
    got, msg = refused(skeleton, (nj, many, t, v))
    assert got == inval and "at most one per joint and path" in msg
    assert P.animate_joints(skeleton, one().clip(), 0.5).shape == (n, 12)     # and the clip they were derived from is accepted
    assert P.animate_joints(skeleton, (n, np.zeros((0, 6), np.uint32), [], []), 0.5).shape == (n, 12)   # no channel at all: the rest pose


def test_the_rest_pose_of_an_inverse_bound_skeleton_is_close_to_the_identity():
    (parents, ib, rest, _), _, _ = CASES["j255"]()
    m = P.animate_joints((parents, ib, rest, None), (len(parents), np.zeros((0, 6), np.uint32), [], []), 0.0)
    assert np.abs(m - IDENTITY).max() < 1e-5
