"""tests/anim_layer_ref.py against itself: the float32 statement of the layer blend (csrc/host/animation.h) within a
tolerance of its float64 model, and the properties the wrap and the blend are specified by.  numpy only."""
import numpy as np
import pytest

from anim_layer_cases import CASES, clips_of
from anim_layer_ref import (WRAP_CLAMP, WRAP_LOOP, WRAP_PINGPONG, active_layers, blend_joints, clip_range, joint_matrices_layers, sample_joints,
                            wrap_time)
from anim_ref import joint_matrices

# The largest deviation of the float32 statement from the float64 model over CASES, relative to the case's largest matrix entry, was
# measured at 1.36e-5 (the 257-joint chain, as in tests/test_anim_reference.py: the chain depth drives it).  Allowed: four times that.
# Every case keeps the first active layer's normalised weight at 0.05 or above (tests/anim_layer_cases.py).
MEASURED = 1.36e-5
TOLERANCE = 4 * MEASURED


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", CASES)
def test_the_float32_statement_stays_close_to_the_float64_model(name):
    skeleton, sets = CASES[name]()
    for k, layers in enumerate(sets):
        assert active_layers(layers, np.float64)[0][2] >= 0.05
        got = joint_matrices_layers(skeleton, layers, np.float32)
        want = joint_matrices_layers(skeleton, layers, np.float64)
        assert got.dtype == np.float32 and want.dtype == np.float64
        rel = np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()
        print(name, k, rel)
        assert rel <= TOLERANCE, (name, k, rel)


def test_wrapped_times_lie_in_the_range_and_pingpong_is_loop_of_the_mirrored_time():
    rng = np.random.default_rng(5)
    n = 30000
    begin = (rng.uniform(-100, 100, n) * rng.choice([0.0, 1e-3, 1.0], n)).astype(np.float32)
    end = begin + (10.0 ** rng.uniform(-6, 4, n)).astype(np.float32)
    t = (rng.uniform(-1, 1, n) * 10.0 ** rng.uniform(-3, 9, n)).astype(np.float32)
    t[::5] = end[::5]; t[1::5] = begin[1::5]
    for a, b, e in zip(t, begin, end):
        assert wrap_time(a, b, e, WRAP_CLAMP).view(np.uint32) == a.view(np.uint32)       # the same bits
        if not e > b:                                                         # begin + a tiny d rounded back to begin: d = 0, the time as given
            assert wrap_time(a, b, e, WRAP_LOOP) == a == wrap_time(a, b, e, WRAP_PINGPONG)
            continue
        for mode in (WRAP_LOOP, WRAP_PINGPONG):
            w = wrap_time(a, b, e, mode)
            assert w.dtype == np.float32 and np.isfinite(w) and b <= w <= e, (a, b, e, mode, w)
    f = np.float32
    assert wrap_time(1.5, 0.0, 1.5, WRAP_LOOP) == 0 and wrap_time(1.5, 0.0, 1.5, WRAP_PINGPONG) == f(1.5)       # t = end: begin under LOOP
    assert wrap_time(0.0, 0.0, 1.5, WRAP_LOOP) == 0 == wrap_time(3.0, 0.0, 1.5, WRAP_PINGPONG)
    assert wrap_time(-0.5, 0.0, 1.5, WRAP_LOOP) == f(1.0) and wrap_time(-0.5, 0.0, 1.5, WRAP_PINGPONG) == f(0.5)
    assert wrap_time(2.0, 0.0, 1.5, WRAP_PINGPONG) == f(1.0) and wrap_time(3.5, 1.0, 2.0, WRAP_LOOP) == f(1.5)
    for a, b, e in ((5.0, 2.0, 2.0), (5.0, 3.0, 2.0), (7.0, -3e38, 3e38)):    # begin = end, end < begin, end - begin overflows
        assert wrap_time(a, b, e, WRAP_LOOP) == f(a) == wrap_time(a, b, e, WRAP_PINGPONG)
    assert wrap_time(0.3, -1e38, 2e38, WRAP_PINGPONG) == f(0.3) and np.isfinite(wrap_time(0.3, -1e38, 2e38, WRAP_LOOP))   # d + d overflows
    assert 0 <= wrap_time(5.0, 0.0, 1e-45, WRAP_LOOP) <= f(1e-45)             # d denormal
    for mode in (WRAP_LOOP, WRAP_PINGPONG):                                   # t - begin overflows: r is reset to 0
        assert wrap_time(3e38, -3e38, -2e38, mode) == f(-3e38)
    # PINGPONG over [0, d] is LOOP over [0, 2 d] mirrored about d: exact where every step is (dyadic times)
    for k in range(-40, 41):
        a, d = f(0.125 * k), f(1.5)
        r = wrap_time(a, 0.0, 2 * d, WRAP_LOOP)
        assert wrap_time(a, 0.0, d, WRAP_PINGPONG) == (r if r <= d else 2 * d - r)
        assert wrap_time(-a, 0.0, d, WRAP_PINGPONG) == wrap_time(a, 0.0, d, WRAP_PINGPONG)    # and even in t


def test_the_blend_is_specified_by_its_single_layers():
    skeleton, (a, b, c, d) = clips_of(6, 3, "two_roots", True)
    rest = skeleton[2]
    for dt in (np.float32, np.float64):
        one = joint_matrices_layers(skeleton, [(a, 0.3, 0.7, WRAP_CLAMP)], dt)
        assert np.array_equal(one, joint_matrices(skeleton, a, 0.3, dt))      # one active layer: no blend arithmetic, whatever its weight
        assert np.array_equal(joint_matrices_layers(skeleton, [(a, 0.3, 1.0, WRAP_CLAMP), (b, 0.6, 0.0, WRAP_LOOP)], dt), one)
        assert np.array_equal(joint_matrices_layers(skeleton, [(b, 0.6, 0.0, WRAP_LOOP), (a, 0.3, 1.0, WRAP_CLAMP)], dt), one)
    # q and -q are one rotation: a clip blended with its negated twin at the same time is that clip, up to the blend's roundings
    got = joint_matrices_layers(skeleton, [(a, 0.3, 0.5, WRAP_CLAMP), (d, 0.3, 0.5, WRAP_CLAMP)], np.float64)
    assert np.abs(got - joint_matrices(skeleton, a, 0.3, np.float64)).max() < 1e-12
    Ta, qa, Sa = sample_joints(a, rest, np.float32(0.3), np.float64)
    Td, qd, Sd = sample_joints(d, rest, np.float32(0.3), np.float64)
    animated = np.asarray(a[1]).reshape(-1, 6)
    animated = np.unique(animated[animated[:, 1] == 1, 0])
    assert animated.size and np.all((qa[animated] * qd[animated]).sum(1) < 0)   # the layers do meet with a negative dot
    # weights enter through their ratios only, and the blended rotation is a unit quaternion no shorter than a_l0 before normalising
    T1, q1, S1 = blend_joints([(a, 0.3, 1.0, WRAP_CLAMP), (c, 0.5, 3.0, WRAP_CLAMP)], rest, np.float64)
    T2, q2, S2 = blend_joints([(a, 0.3, 0.5, WRAP_CLAMP), (c, 0.5, 1.5, WRAP_CLAMP)], rest, np.float64)
    assert np.allclose(T1, T2, rtol=0, atol=1e-15) and np.allclose(q1, q2, rtol=0, atol=1e-15) and np.allclose(np.linalg.norm(q1, axis=1), 1.0)
    Tc, qc, Sc = sample_joints(c, rest, np.float32(0.5), np.float64)
    assert np.allclose(T1, 0.25 * Ta + 0.75 * Tc) and np.allclose(S1, 0.25 * Sa + 0.75 * Sc)
    # a layer without a channel for a (joint, path) takes rest there
    empty = (6, np.zeros((0, 6), np.uint32), np.zeros(0, np.float32), np.zeros(0, np.float32))
    T3, q3, S3 = blend_joints([(a, 0.3, 1.0, WRAP_CLAMP), (empty, 0.0, 1.0, WRAP_LOOP)], rest, np.float64)
    assert np.allclose(T3, 0.5 * Ta + 0.5 * rest[:, 0:3]) and clip_range(empty) == (0, 0)
