"""tests/anim_ref.py against itself: the float32 statement of csrc/host/animation.h within a tolerance of its float64 model, the
nlerp / slerp table the header and DESIGN.md 5.33 quote, and the properties the sampler is specified by.  numpy only."""
import os
import re

import numpy as np
import pytest

from anim_cases import CASES, IDENTITY, ClipBuilder
from anim_ref import LINEAR, PATH_R, PATH_T, STEP, find_key, joint_matrices, local_matrices, nlerp_slerp_table, sample_channel

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The largest deviation of the float32 statement from the float64 model over CASES, relative to the case's largest matrix entry, was
# measured at 2.83e-6 (the 257-joint chain: only the chain depth and the scales of the cases drive it).  Allowed: four times that.
MEASURED = 2.83e-6
TOLERANCE = 4 * MEASURED


@pytest.mark.parametrize("name", CASES)
def test_the_float32_statement_stays_close_to_the_float64_model(name):
    skeleton, clip, times = CASES[name]()
    for t in times:
        got = joint_matrices(skeleton, clip, t, np.float32)
        want = joint_matrices(skeleton, clip, t, np.float64)
        assert got.dtype == np.float32 and want.dtype == np.float64
        rel = np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()
        print(name, t, rel)
        assert rel <= TOLERANCE, (name, t, rel)


def test_the_nlerp_slerp_table_is_the_one_the_header_and_the_design_quote():
    table = nlerp_slerp_table()
    assert [round(table[a], 4) for a in (15.0, 30.0, 60.0, 90.0)] == [0.0041, 0.0331, 0.2675, 0.9188]
    row = "0.0041 deg  0.0331 deg  0.2675 deg  0.9188 deg"
    with open(os.path.join(REPO, "cpugpupathtracing_amd", "csrc", "host", "animation.h")) as f:
        assert row in f.read()
    with open(os.path.join(REPO, "DESIGN.md")) as f:
        assert re.search(r"0\.0041.*0\.0331.*0\.2675.*0\.9188", f.read())
    assert 0.9 < table[90.0] < 1.2 and 0.02 < table[30.0] < 0.05               # about 1 degree at 90, a few hundredths at 30


def test_the_key_search_and_the_sampler_at_every_edge():
    times = np.float32([0.25, 0.5, 1.0, 1.5])
    assert [find_key(times, np.float32(t)) for t in (-1, 0.25, 0.3, 0.5, 0.99, 1.0, 1.5, 9)] == [0, 0, 0, 1, 1, 2, 3, 3]
    assert find_key(times[:1], np.float32(-3)) == 0 == find_key(times[:1], np.float32(3))
    v = np.float32([[0, 0, 0], [1, 2, 4], [3, 3, 3], [5, 5, 5]])
    s = lambda t, i=LINEAR: sample_channel(times, v, i, np.float32(t), False, np.float32)
    assert np.array_equal(s(-1), v[0]) and np.array_equal(s(0.25), v[0]) and np.array_equal(s(0.5), v[1])      # before the first key, on a key
    assert np.array_equal(s(1.5), v[3]) and np.array_equal(s(7), v[3])                                          # on and after the last
    assert np.array_equal(s(0.375), np.float32([0.5, 1, 2]))                                                    # between: u = 0.5 exactly
    assert np.array_equal(s(0.375, STEP), v[0]) and np.array_equal(s(0.99, STEP), v[1])
    a, b = np.float32([0, 0, 0, 1]), np.float32([0.6, 0, 0, -0.8])            # a negative dot: b is negated first
    q = sample_channel(np.float32([0, 1]), np.stack([a, b]), LINEAR, np.float32(0.5), True, np.float32)
    assert np.array_equal(q, a + np.float32(0.5) * (-b - a))


def test_rotations_are_normalised_and_a_rotation_without_length_is_the_identity():
    rest = np.float32([[1, 2, 3, 0, 0, 0, 0, 2, 2, 2], [0, 0, 0, 0, 0, 3, 4, 1, 1, 1]])
    L = local_matrices((2, np.zeros((0, 6), np.uint32), [], []), rest, 0.0, np.float32)
    assert np.array_equal(L[0], np.float32([2, 0, 0, 1, 0, 2, 0, 2, 0, 0, 2, 3]))                               # (0, 0, 0, 0) -> (0, 0, 0, 1)
    q = np.float32([0, 0, 3, 4]) * (np.float32(1) / np.sqrt(np.float32(25)))
    assert np.array_equal(L[1, [0, 1, 4, 5]], np.float32([1 - 2 * q[2] * q[2], -2 * (q[3] * q[2]), 2 * (q[3] * q[2]), 1 - 2 * q[2] * q[2]]))
    clip = ClipBuilder(2).add(1, PATH_R, STEP, [0.0], [[0, 0, 0, 0]]).add(0, PATH_T, LINEAR, [0.0, 2.0], [[0, 0, 0], [2, 4, 6]]).clip()
    L = local_matrices(clip, rest, 1.0, np.float32)
    assert np.array_equal(L[1], IDENTITY) and np.array_equal(L[0, [3, 7, 11]], np.float32([1, 2, 3]))           # a zero key, a sampled T


def test_the_walk_is_bottom_up_and_the_order_of_the_joints_does_not_matter():
    skeleton, clip, times = CASES["two_roots"]()
    parents, ib, rest, root = skeleton
    n = len(parents)
    want = joint_matrices(skeleton, clip, times[2])
    perm = np.random.default_rng(3).permutation(n)                            # new index of every joint
    inv = np.argsort(perm)
    p2 = np.where(parents[inv] >= 0, perm[np.maximum(parents[inv], 0)], -1).astype(np.int32)
    nj, ch, t, v = clip
    ch2 = ch.copy(); ch2[:, 0] = perm[ch[:, 0]]
    got = joint_matrices((p2, ib[inv], rest[inv], root), (nj, ch2, t, v), times[2])
    assert np.array_equal(got.view(np.uint32), want[inv].view(np.uint32))
