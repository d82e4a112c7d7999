"""The ray sets of the trace probe's tests: scenes built twice (oracle and host mirror, tests/scenes.py) and the rays that
reach the paths of the production traversal a render never reaches on purpose.  Plain numpy and the CPU oracle; no GPU.
tests/test_trace_cases.py checks against the oracle alone that every set does what it is for; tests/test_gpu_trace_probe.py fires them
through Renderer.trace_rays / trace_first_hits.  Every direction is finite and not zero.
A set is (o, d) or (o, d, tmax), float32; the cached scenes and sets are built once per process and never changed
(round0_pair, whose camera differs per frame, is built anew for every frame)."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import oracle as O
import cpugpupathtracing_amd as P
import replay_ref as RP
import tlas_ref as TL
from scenes import forty_object_pair, pair_from, quad_stack, reference_layout_pair, standin_mesh

NO_HIT = 0xFFFFFFFF
F = np.float32
T_FAR = F(1e34)


# ---- parity: the 20 000 rays of test_gpu_parity.test_intersect_rays_bit_exact ------------------------------------------------------------------
@lru_cache(maxsize=None)
def parity_pair(level):
    """(oracle scene, host scene): the reference layout around the stand-in at `level`, diffuse."""
    return reference_layout_pair(*standin_mesh(level), 1)


@lru_cache(maxsize=None)
def parity_rays():
    rng = np.random.default_rng(7)
    n = 20000
    origins = np.tile(np.array([0, 0, 8], np.float32), (n, 1)) + rng.normal(0, 0.5, (n, 3)).astype(np.float32)
    target = np.stack([rng.uniform(-8, 8, n), rng.uniform(-4, 4, n), rng.uniform(-10, 0, n)], 1).astype(np.float32)
    d = target - origins
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d[:6] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)   # the inf / NaN slab cases (SURVEY A-18)
    origins[:6] = np.array([0, 0, -4.97], np.float32)
    return origins, d


@lru_cache(maxsize=None)
def parity_hits(level):
    """The oracle's (t, obj, tri, bvh_depth) of the parity rays."""
    return parity_pair(level)[0].intersect_rays(*parity_rays())


# ---- zero components: the NaN-exact slab form, and origins on a root box's face ---------------------------------------------------------------
def root_box(scene, obj_index=0):
    nodes, _ = scene.bvh_export(obj_index)
    w = np.asarray(nodes).view(np.uint32).reshape(-1, 8)[0]
    return w[0:3].view(np.float32).copy(), w[4:7].view(np.float32).copy()


@lru_cache(maxsize=None)
def zero_component_rays(level):
    """768 rays into the stand-in with one or two direction components exactly zero, each zero +0 in one half and -0 in the other, then
    384 whose origin lies exactly on a face of the mesh root's box: a third with the face's axis component zero (0 * inf in the slab
    test), a third pointing in, a third pointing out."""
    lo, hi = root_box(parity_pair(level)[1])
    rng = np.random.default_rng(21)
    n = 768
    target = rng.uniform(lo, hi, (n, 3))
    d = rng.standard_normal((n, 3))
    for k in range(n):
        ax = k % 3
        if k < n // 2:
            d[k, ax] = 0.0                                                     # one zero component
        else:
            d[k] = 0.0; d[k, ax] = 1.0 if k % 2 else -1.0                      # two
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = (target - 6.0 * d).astype(np.float32)
    d = d.astype(np.float32)
    zero = d == 0.0
    neg = zero & (np.arange(n)[:, None] % 4 >= 2)
    d[neg] = F(-0.0)
    assert np.signbit(d[zero]).any() and not np.signbit(d[zero]).all()
    m = 384
    fo = rng.uniform(lo, hi, (m, 3)).astype(np.float32)
    fd = rng.standard_normal((m, 3))
    for k in range(m):
        ax, side = k % 3, (k // 3) % 2
        fo[k, ax] = hi[ax] if side else lo[ax]
        inward = -1.0 if side else 1.0
        fd[k, ax] = (0.0, inward, -inward)[(k // 6) % 3] * (abs(fd[k, ax]) + 0.1)
    fd = (fd / np.linalg.norm(fd, axis=1, keepdims=True)).astype(np.float32)
    return np.concatenate([o, fo]), np.concatenate([d, fd])


# ---- list edges and several blocks per wave ------------------------------------------------------------------------------------------------------
LIST_EXTEND, LIST_SHADOW = (1, 63, 64, 65, 129), (0, 1, 64, 65)


def tiled(o, d, n, step=1e-3):
    """n rays: the set repeated, copy k with its origins moved by k * step along x (new rays, the same population)."""
    reps = (n + o.shape[0] - 1) // o.shape[0]
    shift = np.repeat(np.arange(reps, dtype=np.float32) * F(step), o.shape[0])[:n]
    oo = np.tile(o, (reps, 1))[:n].copy()
    oo[:, 0] += shift
    return oo, np.tile(d, (reps, 1))[:n].copy()


def rays_beyond_one_block_per_wave(n_cus):
    """More rays than 64 x the waves of a trace grid of one block per CU (trace_blocks = 1, four waves a block): 70 000 on a 256-CU part."""
    return 64 * 4 * n_cus + 4464


# ---- deep stack ------------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def deep_pair():
    """test_gpu_parity's stack of 2^17 quads (tree depth >= 18) with a sphere and a plane behind it in the object list."""
    v, i = quad_stack(1 << 17)
    glass, grey, light = P.REFERENCE_MATERIALS[3], P.Material(albedo=(0.6, 0.6, 0.6)), P.Material(emissive=(1, 1, 1), intensity=4.0, is_light=True)
    return pair_from([("mesh", v, i, 0, O.BUILD_SAH_INTERVALS), ("sphere", (0, 12, 4), 4.0, 2), ("plane", (0, 1, 0), (0, -3, 0), 1)],
                     [glass, grey, light], [1], camera=((0, 0, 8), (0, 0, -1), 800.0, 33 / 24))


@lru_cache(maxsize=None)
def deep_rays():
    """300 rays down the stack: the first along the axis itself (two zero components), the others aimed at points of the last quad from
    origins around the axis, from the front and -- the far child first -- from behind."""
    rng = np.random.default_rng(33)
    n = 300
    o = np.concatenate([rng.uniform(-0.9, 0.9, (n, 2)), np.full((n, 1), 8.0)], 1)
    target = np.concatenate([rng.uniform(-0.9, 0.9, (n, 2)), np.full((n, 1), -0.01 * ((1 << 17) - 1))], 1)
    back = np.arange(n) % 3 == 2
    o[back, 2] = target[back, 2] - 8.0
    target[back, 2] = 0.0
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o[0] = (0.25, -0.5, 8.0); d[0] = (0.0, 0.0, -1.0)
    return o.astype(np.float32), d.astype(np.float32)


# ---- more objects than the LDS table, and ties --------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def forty_pair():
    return forty_object_pair()


@lru_cache(maxsize=None)
def forty_rays():
    rng = np.random.default_rng(41)
    n = 4096
    o = np.array([0, 2, 8], np.float32) + rng.normal(0, 1.0, (n, 3)).astype(np.float32)
    target = np.stack([rng.uniform(-9, 9, n), rng.uniform(-3, 6, n), rng.uniform(-12, 0, n)], 1).astype(np.float32)
    d = target - o
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _twin_objects(quads):
    grey = P.Material(albedo=(0.8, 0.8, 0.8))
    v, i = TL.quad_mesh((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    objs = [("mesh", v, i, 0, O.BUILD_SAH_INTERVALS) if k in quads else ("sphere", (6.0 + 2.5 * k, 5.0, -3.0), 0.5, 0) for k in range(20)]
    return pair_from(objs, [grey], [], camera=((0, 0, 5), (0, 0, -1), 60.0, 1.0))


@lru_cache(maxsize=None)
def twin_quad_pair(quads=(3, 17)):
    """test_gpu_tlas's scene: the same quad as objects 3 and 17 among 18 spheres off to the side (quads=(3,) or (17,): one of the two,
    for the CPU condition)."""
    return _twin_objects(quads)


@lru_cache(maxsize=None)
def twin_quad_rays():
    rng = np.random.default_rng(4)
    n = 512
    target = np.concatenate([rng.uniform(-0.95, 0.95, (n, 2)), np.zeros((n, 1))], 1)
    o = target + np.array([0.0, 0.0, 4.0]) + rng.uniform(-1.0, 1.0, (n, 3))
    d = target - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


COINCIDENT_COPIES = 300


@lru_cache(maxsize=None)
def coincident_pair(copies=COINCIDENT_COPIES):
    """test_gpu_bvh_build's mesh of 300 copies of one triangle (no plane separates the centroids: the root stays a leaf of 300) in
    front of a plane."""
    v = np.array([[0, 0, 0, 0, 0, 1], [1, 0, 0, 0, 0, 1], [0, 1, 0, 0, 0, 1]], np.float32)
    grey = P.Material(albedo=(0.8, 0.8, 0.8))
    return pair_from([("mesh", v, np.tile(np.array([0, 1, 2], np.uint32), copies), 0, O.BUILD_SAH_INTERVALS), ("plane", (0, 0, 1), (0, 0, -2), 0)], [grey], [])


@lru_cache(maxsize=None)
def coincident_rays():
    rng = np.random.default_rng(9)
    n = 256
    target = np.concatenate([rng.uniform(-0.2, 1.2, (n, 2)), np.zeros((n, 1))], 1)
    o = np.array([0.3, 0.3, 3.0]) + rng.uniform(-0.5, 0.5, (n, 3))
    d = target - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


# ---- tmax edges ------------------------------------------------------------------------------------------------------------------------------------
TMAX_KINDS = ("t", "below", "above", "half", "far")


@lru_cache(maxsize=None)
def tmax_edge_rays(level, n=600):
    """The first n parity rays that hit, five times over: tmax = t (a miss: the test is strict), the float below t (a miss), the float
    above (the hit), t / 2 (a miss) and 1e34: (o, d, tmax), kind-major."""
    o, d = parity_rays()
    t, obj, _, _ = parity_hits(level)
    sel = np.nonzero(obj != NO_HIT)[0][:n]
    th = t[sel]
    tm = np.concatenate([th, np.nextafter(th, F(0.0)), np.nextafter(th, F(np.inf)), (th / F(2.0)).astype(np.float32), np.full(sel.size, T_FAR)])
    return np.tile(o[sel], (5, 1)), np.tile(d[sel], (5, 1)), tm.astype(np.float32)


@lru_cache(maxsize=None)
def nee_shadow_rays(level, n=1500):
    """Shadow rays as next event estimation makes them: from the hit points of parity rays (float32, a ten-thousandth of t short of the
    surface) to points of the two sphere lights of the reference layout, tmax a thousandth short of the distance to the point."""
    o, d = parity_rays()
    t, obj, _, _ = parity_hits(level)
    sel = np.nonzero(obj != NO_HIT)[0][-n:]
    rng = np.random.default_rng(13)
    x = (o[sel] + d[sel] * (t[sel] * F(1.0 - 1e-4))[:, None]).astype(np.float32)       # a little in front of the surface, as the bounce's offset leaves it
    u = rng.standard_normal((sel.size, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    centre = np.where((np.arange(sel.size) % 2 == 0)[:, None], np.array([10.0, 10.0, 10.0]), np.array([-10.0, 10.0, -10.0]))
    w = x - centre
    u = w / np.linalg.norm(w, axis=1, keepdims=True) + 0.7 * u                          # within the cap of the light that the point sees
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    to = (centre + 5.0 * u).astype(np.float32) - x
    dist = np.sqrt((to.astype(np.float32) ** 2).sum(1, dtype=np.float32)).astype(np.float32)
    return x, (to / dist[:, None]).astype(np.float32), (dist * F(0.999)).astype(np.float32)   # short of the light's own surface


# ---- round 0 ---------------------------------------------------------------------------------------------------------------------------------------
ROUND0_FRAMES = ((1, 1, None), (7, 5, None), (45, 37, None), (130, 70, None), (45, 37, (5, 30)))   # W, H, rows
def round0_pair():
    """replay_ref's scene without the glass sphere its second camera sits in (from inside it no primary ray misses) and without the
    stand-alone triangle (the oracle has none): a ground plane, a sphere, the 80-triangle icosphere, the lamp and the two-triangle panel.
    A new pair on every call (it is small): round0_want sets the camera of its own."""
    import smooth_ref as SM
    grey, light = P.Material(albedo=(0.8, 0.7, 0.6)), P.Material(emissive=(1.0, 0.95, 0.8), intensity=10.0, is_light=True)
    v, i = SM.icosphere(1, RP.MESH_CENTER, RP.MESH_RADIUS)
    quad = np.array([[-3.4, 3.0, -4.2, 0, -1, 0], [-1.6, 3.0, -4.2, 0, -1, 0], [-1.6, 3.0, -2.4, 0, -1, 0], [-3.4, 3.0, -2.4, 0, -1, 0]], np.float32)
    return pair_from([("plane", (0, 1, 0), (0, 0, 0), 0), ("sphere", (-1.7, 0.8, -3.0), 0.8, 0),
                      ("mesh", np.asarray(v, np.float32), np.asarray(i, np.uint32), 0, O.BUILD_SAH_INTERVALS), ("sphere", (0.0, 5.0, -2.5), 1.0, 1),
                      ("mesh", quad, np.array([0, 1, 2, 2, 3, 0], np.uint32), 1, O.BUILD_SAH_INTERVALS)], [grey, light], [3])


def round0_camera(view_index, W, H):
    pos, view_dir, fov, _ = RP.VIEWS[view_index]["camera"]
    return pos, view_dir, fov, W / H


def round0_want(view_index, W, H, rows=None):
    """dict(records: the oracle's first hits (obj, tri, bvh_depth, t), each (rows, W), of round0_pair seen from a camera of replay_ref at
    aspect W / H; camera: the host scene's cgpt_camera of that view; counters: the oracle's (traced_rays, inner_steps, tri_tests,
    bvh_depth_sum) of those rays).  A pair of its own: no shared scene is touched."""
    o, s = round0_pair()
    cam = round0_camera(view_index, W, H)
    o.set_camera(*cam); s.set_camera(*cam)
    ro, rd = o.camera_rays(W, H)
    r0, r1 = rows if rows is not None else (0, H)
    o.reset_stats()
    t, obj, tri, dep = o.intersect_rays(ro[r0:r1].reshape(-1, 3), rd[r0:r1].reshape(-1, 3))
    st = o.stats()
    shape = (r1 - r0, W)
    out = dict(records=(obj.reshape(shape), tri.reshape(shape), dep.reshape(shape), t.reshape(shape)), camera=s.camera(),
               counters=(st.traced_rays, st.inner_steps, st.tri_tests, st.bvh_depth_sum))
    s.close(); o.close()
    return out


def padded_tiles(W, rows):
    """(columns, rows) of padding in the 8 x 8 tiles of a band."""
    return (-W) % 8, (-rows) % 8
