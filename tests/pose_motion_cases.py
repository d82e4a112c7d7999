"""The scene, the skins and the pose changes shared by the pose-following tests (test_pose_motion_reference.py on the CPU,
test_gpu_pose_motion.py on the device), at the size of the temporal tests: 97x61.

The scene is motion_cases.py's -- a back wall, a sphere light, a diffuse sphere, a transformed box, a transformed icosphere, two
instanced placements of one icosphere, a glass box -- with a second level-2 icosphere that carries the smooth flag and a stand-alone
triangle object added, and with skins from skin_cases.make_case:
  STATIC  the transformed box under "bend";
  MOVER   the faceted level-2 icosphere (320 triangles) under "bend", in the case "wide" under "wide" (1024 joints);
  INST_A  the instanced icosphere under "bend": a pose moves INST_B, the second placement, too;
  SMOOTH  the smooth icosphere under "four": four influences, a mirrored joint and a non-uniformly scaled joint, the corners
          welded (below);
  TRI     the triangle object under "one_joint".
A case changes every skinned object's pose from the base pose (make_case's matrices) to `varied`: each joint followed by a small
rotation about the bind pose's centre and a shift, another sense per object.  A case without a camera move gets motion_cases.JITTER, a
seventh of a pixel: without it the static hits land on the sample points and float32 names another tap set on half the frame."""
from __future__ import annotations

import numpy as np

import cpugpupathtracing_amd as P
import motion_cases as MC
import skin_cases as SC
import smooth_ref as S
import pose_motion_ref as PM
import transform_ref as TR

W, H, FOV, BASE, CAP = MC.W, MC.H, MC.FOV, MC.BASE, MC.CAP
WALL, LAMP, BALL, STATIC, MOVER, INST_A, INST_B, GLASS, SMOOTH, TRI = range(10)
N_OBJECTS = 10
SKINNED = (STATIC, MOVER, INST_A, SMOOTH, TRI)                                 # the objects that own a skin
POSED = (STATIC, MOVER, INST_A, INST_B, SMOOTH, TRI)                           # the objects a pose moves
DIFFUSE_POSED = POSED
SKIN_OF = {STATIC: STATIC, MOVER: MOVER, INST_A: INST_A, INST_B: INST_A, SMOOTH: SMOOTH, TRI: TRI}
POSE_NAME = {STATIC: "bend", MOVER: "bend", INST_A: "bend", SMOOTH: "four", TRI: "one_joint"}
TRI_P = np.float32([[8.3, 0.1, 0.0], [11.5, 0.6, 0.2], [9.8, 3.5, 0.5]])    # at the right edge, where its pose (-40 degrees about y) faces the camera
TRI_N = np.float32([[0.0, 0.0, 1.0], [0.3, 0.0, 0.95], [0.0, 0.3, 0.95]])
TRI_N /= np.linalg.norm(TRI_N, axis=1, keepdims=True).astype(np.float32)

# name -> (degrees, shift, the camera view after the change, the pose MOVER's skin is made for)
CASES = {
    "nudge": (1.5, (0.05, 0.03, 0.0), MC.JITTER, "bend"),                      # a fraction of a pixel (a pixel is 0.25 world units)
    "swing": (5.0, (0.5, -0.25, 0.1), MC.JITTER, "bend"),                      # whole pixels and a visible turn
    "with_camera": (2.0, (0.1, -0.05, 0.04), MC.CAMERA_MOVE, "bend"),          # a pose and a camera move with parallax in one frame
    "wide": (1.5, (0.04, 0.05, 0.0), MC.JITTER, "wide"),                       # the joint limit on the 320-triangle mesh
}


def base_matrices():
    m = np.tile(np.eye(3, 4, dtype=np.float32), (N_OBJECTS, 1, 1))
    m[:8] = MC.base_matrices()
    m[SMOOTH] = MC.affine(MC.rot(2, 20.0), (2.7, -4.7, 0.0))
    return m


def meshes():
    """object-space geometry of (STATIC, MOVER, INST_A, GLASS, SMOOTH)"""
    box, ico, small, gbox = MC.meshes()
    return box, ico, small, gbox, S.icosphere(2, (0.0, 0.0, 0.0), 2.3)


def bind_triangles():
    """object index -> (n, 18) float32 bind pose, for every object that owns a skin"""
    box, ico, small, _, smooth = meshes()
    out = {STATIC: P.triangles_from_arrays(*box), MOVER: P.triangles_from_arrays(*ico), INST_A: P.triangles_from_arrays(*small),
           SMOOTH: P.triangles_from_arrays(*smooth), TRI: np.concatenate([TRI_P, TRI_N], axis=1).reshape(1, 18)}
    assert len(out[MOVER]) == 320 and len(out[SMOOTH]) == 320 and len(out[STATIC]) == 12
    return out


def product_scene(mats=None, instances=True):
    mats = base_matrices() if mats is None else mats
    s = P.Scene()
    for m in MC.materials():
        s.add_material(m)
    box, ico, small, gbox, smooth = meshes()
    assert s.add_plane((0.0, 0.0, 1.0), (0.0, 0.0, -2.0), MC.M_GROUND) == WALL
    assert s.add_sphere((0.5, 6.5, 3.0), 1.5, MC.M_EMITTER) == LAMP
    assert s.add_sphere((-9.8, -4.6, 0.0), 2.0, MC.M_OTHER) == BALL
    assert s.add_mesh(P.Mesh.from_arrays(*box), MC.M_OTHER, transform=mats[STATIC]) == STATIC
    assert s.add_mesh(P.Mesh.from_arrays(*ico), MC.M_DIFFUSE, transform=mats[MOVER]) == MOVER
    assert s.add_mesh(P.Mesh.from_arrays(*small), MC.M_DIFFUSE, transform=mats[INST_A]) == INST_A
    if instances:
        assert s.add_instance(INST_A, MC.M_OTHER, transform=mats[INST_B]) == INST_B
    else:
        assert s.add_mesh(P.Mesh.from_arrays(*small), MC.M_OTHER, transform=mats[INST_B]) == INST_B
    assert s.add_mesh(P.Mesh.from_arrays(*gbox), MC.M_GLASS, transform=mats[GLASS]) == GLASS
    assert s.add_mesh(P.Mesh.from_arrays(*smooth), MC.M_DIFFUSE, smooth=True, transform=mats[SMOOTH]) == SMOOTH
    assert s.add_triangle(TRI_P, TRI_N, MC.M_OTHER) == TRI
    s.add_light(LAMP)
    s.set_camera(BASE[0], BASE[1], FOV, W / H)
    s.set_settings(P.Settings())
    return s


def skins(mover_pose="bend"):
    """object index -> (bind, joints, weights, n_joints, base matrices) for every object that owns a skin"""
    out = {}
    for o, bind in bind_triangles().items():
        j, w, n_joints, m = SC.make_case(mover_pose if o == MOVER else POSE_NAME[o], bind, seed=o)
        if o == SMOOTH:
            j, w = welded(bind, j, w)
        out[o] = (bind, j, w, n_joints, m)
    return out


def welded(bind, j, w):
    """make_case draws the joints and weights of "four" per corner, which tears the mesh into triangles that each go their own way: a
    sub-pixel shard soup at this frame size.  Every corner takes the draw of the first corner at its bind position, so the surface stays
    connected -- crumpled by the mirror and the scale, four influences a corner as before."""
    pos = bind.reshape(-1, 6)[:, :3]
    _, first, inverse = np.unique(pos.view(np.uint32), axis=0, return_index=True, return_inverse=True)
    pick = first[inverse.reshape(-1)]
    return j.reshape(-1, 4)[pick].reshape(j.shape).copy(), w.reshape(-1, 4)[pick].reshape(w.shape).copy()


def varied(m, bind, deg, shift, sense=1.0):
    """the joint matrices m (n_joints, 12), each followed by a rotation of sense * deg about the bind pose's centre and the shift"""
    centre = bind.reshape(-1, 6)[:, :3].astype(np.float64).mean(axis=0)
    r = SC.rotation((0.3, 1.0, 0.2), sense * deg)
    out = np.empty_like(m)
    for k, row in enumerate(m.reshape(-1, 3, 4).astype(np.float64)):
        a, b = r @ row[:, :3], r @ (row[:, 3] - centre) + centre + sense * np.asarray(shift, np.float64)
        out[k] = np.concatenate([a, b[:, None]], axis=1).astype(np.float32).reshape(12)
    return out


def case_poses(case):
    """(skins, base matrices per skin owner, the case's matrices per skin owner, the view after the change)"""
    deg, shift, view, mover_pose = CASES[case]
    sk = skins(mover_pose)
    base = {o: v[4] for o, v in sk.items()}
    after = {o: varied(v[4], v[0], deg, shift, 1.0 if k % 2 == 0 else -1.0) for k, (o, v) in enumerate(sk.items())}
    return sk, base, after, view


def posed_objects(sk, matrices, mats=None, serial=1, smooth=None):
    """object index -> pose_motion_ref.Posed for every object a pose moves, under the joint matrices `matrices` (per skin owner; None:
    no pose known) and the object-to-world matrices `mats`"""
    mats = base_matrices() if mats is None else mats
    out = {}
    for o in POSED:
        bind, j, w, _, _ = sk[SKIN_OF[o]]
        sm = (o == SMOOTH) if smooth is None else smooth[o]
        out[o] = PM.Posed(bind, j, w, matrices[SKIN_OF[o]], serial, sm, mats[o])
    return out


def extent(o, sk, matrices, mats=None):
    """the largest world coordinate of the posed object's corners, for the tolerance on x_p"""
    mats = base_matrices() if mats is None else mats
    bind, j, w, _, _ = sk[SKIN_OF[o]]
    p = PM.SK.skin_f32(bind, j, w, matrices[SKIN_OF[o]]).reshape(-1, 6)[:, :3].astype(np.float64)
    world = p @ mats[o][:, :3].astype(np.float64).T + mats[o][:, 3].astype(np.float64)
    return float(np.max(np.abs(world)))


def camera(s, view):
    return MC.camera(s, view)


def light_materials():
    return MC.light_materials()


def view_dependent_materials():
    return MC.view_dependent_materials()


# ---- guides made on the host (the CPU tests; the device tests take the device's own) ----------------------------------------------------
def camera_rays(cam):
    """(origin (3,), dirs (H * W, 3) float64) of the pixels' primary rays: u = px / W, v = py / H across the camera's screen"""
    c = PM.T.camera_array(cam).astype(np.float64)
    pos, tl, tr, bl = c[0:3], c[3:6], c[6:9], c[9:12]
    px, py = np.meshgrid(np.arange(W) / W, np.arange(H) / H)
    d = tl + px[..., None] * (tr - tl) + py[..., None] * (bl - tl) - pos
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return pos, d.reshape(-1, 3)


def host_guides(cam, sk, matrices, mats=None):
    """(guides (H, W, 12) float32, tri (H, W) uint32) of the scene with the skinned objects posed by `matrices`: a brute-force float64
    ray-triangle test over the posed triangles (a few hundred), the wall and the two spheres in closed form.  The glass box is left out
    (it owns no skin and covers nothing the tests look at)."""
    mats = base_matrices() if mats is None else mats
    o, d = camera_rays(cam)
    n = d.shape[0]
    best = np.full(n, np.inf)
    obj = np.full(n, D_NO_HIT, np.uint32)
    tri = np.zeros(n, np.uint32)
    nrm = np.zeros((n, 3))
    t = (-2.0 - o[2]) / d[:, 2]                                                 # the wall z = -2
    ok = t > 0
    best[ok], obj[ok], nrm[ok] = t[ok], WALL, (0.0, 0.0, 1.0)
    for idx, (c, r) in ((LAMP, ((0.5, 6.5, 3.0), 1.5)), (BALL, ((-9.8, -4.6, 0.0), 2.0))):
        L = np.asarray(c) - o
        tca = d @ L
        d2 = L @ L - tca * tca
        with np.errstate(invalid="ignore"):
            t = tca - np.sqrt(r * r - d2)
        ok = (d2 <= r * r) & (t > 0) & (t < best)
        best[ok], obj[ok] = t[ok], idx
        x = o + d[ok] * t[ok, None]
        nrm[ok] = (x - np.asarray(c)) / r
    mat_of = {WALL: MC.M_GROUND, LAMP: MC.M_EMITTER, BALL: MC.M_OTHER, STATIC: MC.M_OTHER, MOVER: MC.M_DIFFUSE, INST_A: MC.M_DIFFUSE,
              INST_B: MC.M_OTHER, SMOOTH: MC.M_DIFFUSE, TRI: MC.M_OTHER}
    for k in POSED:
        bind, j, w, _, _ = sk[SKIN_OF[k]]
        rows = PM.SK.skin_f32(bind, j, w, matrices[SKIN_OF[k]])
        inv = TR.invert(mats[k]).astype(np.float64)
        oo = inv[:, :3] @ o + inv[:, 3]
        od = d @ inv[:, :3].T                                                   # not renormalised: t is the same number in both spaces
        t, tau = S.intersect_mesh(rows, oo, od)
        ok = t < best
        best[ok], obj[ok], tri[ok] = t[ok], k, tau[ok]
        r64 = rows.astype(np.float64)[tau[ok]]
        no = r64[:, 3:6]
        if k == SMOOTH:
            u, v, _ = PM.barycentric((oo + od[ok] * t[ok, None]).astype(np.float32), rows[tau[ok]])
            no = (1.0 - u - v)[:, None] * r64[:, 3:6] + u[:, None] * r64[:, 9:12] + v[:, None] * r64[:, 15:18]
        nw = no @ inv[:, :3]                                                    # Ainv^T n
        nrm[ok] = nw / np.linalg.norm(nw, axis=1, keepdims=True)
    g = np.zeros((n, 12), np.float32)
    g[:, 3] = 1e34
    gu = g.view(np.uint32)
    gu[:, 7] = gu[:, 11] = D_NO_HIT
    hit = obj != D_NO_HIT
    g[hit, 0:3] = (o + d[hit] * best[hit, None]).astype(np.float32)
    g[hit, 3] = best[hit].astype(np.float32)
    g[hit, 4:7] = nrm[hit].astype(np.float32)
    gu[hit, 7] = obj[hit]
    mat = np.array([mat_of.get(int(k), 0) for k in obj[hit]], np.uint32)
    g[hit, 8:11] = np.float32([m.albedo for m in MC.materials()])[mat]
    gu[hit, 11] = mat
    tri[~hit] = 0
    return g.reshape(H, W, 12), tri.reshape(H, W)


D_NO_HIT = PM.D.NO_HIT
