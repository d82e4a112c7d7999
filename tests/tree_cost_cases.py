"""What the tree-cost tests share (tests/test_host_tree_cost.py, test_gpu_tree_cost.py, test_gpu_rebuild_degraded.py).

The pinned pose.  The policy test needs a pose under which the refitted tree of the 1 280-triangle strip costs clearly more than the
bind tree AND a rebuild clearly lowers the cost again.  bend_case's 120 degrees does not qualify: the cost is relative to the root box,
which the bend shrinks, so the refitted tree costs 4.97 x the bind tree's but the binned rebuild 5.05 x -- the rebuild does not lower it
(the interval build does, to 4.31 x; at 90, 150, 180 and 240 degrees the binned build is within 2 % of the refit either way).  Of the
poses the helpers offer, skin_cases.make_case("wide") -- 1 024 joints with random small rotations, which scatters neighbouring triangles
-- does: 2.92 x refitted, 2.68 x rebuilt binned, 2.70 x rebuilt with intervals.  test_host_tree_cost.py pins it with 2 % margins."""
import functools

import numpy as np

import cpugpupathtracing_amd as P
from skin_cases import make_case
from test_gpu_rebuild_mesh import GROUND, STRIP, make_scene

N_STRIP = 1280
PINNED_POSE = "wide"
MARGIN = 1.02


def pinned_case(bind):
    """(joints, weights, n_joints, matrices) of the pinned pose for the strip's bind triangles"""
    return make_case(PINNED_POSE, bind, seed=5)


@functools.lru_cache(maxsize=None)
def pinned_costs():
    """(bind, refitted, rebuilt) costs of the strip on the host mirror under the pinned pose and the binned rebuild, computed once"""
    s, binds = make_scene(N_STRIP)
    bind = s.tree_cost(STRIP).cost
    j, w, _, m = pinned_case(binds[STRIP])
    s.skin_mesh(STRIP, binds[STRIP], j, w, m)
    refitted = s.tree_cost(STRIP).cost
    s.rebuild_bvh(STRIP, P.BUILD_SAH_BINNED)
    rebuilt = s.tree_cost(STRIP).cost
    s.close()
    return bind, refitted, rebuilt


def f_refit():
    bind, refitted, _ = pinned_costs()
    return refitted / bind


def midpoint_ratio():
    """the policy test's threshold: halfway between an unposed tree (1) and the pinned pose's refitted one (f_refit)"""
    return 0.5 * (1.0 + f_refit())


# a 12-triangle cube and two far-apart triangles (the SAH splits them: a 3-node tree in the small-mesh class)
CUBE_P = np.float32([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)])
CUBE_I = np.uint32([0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3])


def cube(origin=(0.0, 0.0, 0.0)):
    n = CUBE_P / np.linalg.norm(CUBE_P, axis=1, keepdims=True)
    return np.hstack([CUBE_P + np.float32(origin), n]).astype(np.float32), CUBE_I


TWO = (np.float32([[-2.5, 2.0, 0.0, 0, 0, 1], [-2.0, 2.0, 0.0, 0, 0, 1], [-2.2, 2.5, 0.1, 0, 0, 1],
                   [2.0, 2.0, 0.0, 0, 0, 1], [2.5, 2.0, 0.0, 0, 0, 1], [2.2, 2.5, 0.1, 0, 0, 1]]), np.uint32([0, 1, 2, 3, 4, 5]))
