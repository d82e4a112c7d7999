"""The host calls of skinning (cgpth_skin_triangles, cgpth_scene_skin_mesh; include/cpugpupt_host.h): every refusal, and
Scene.skin_mesh against Scene.refit_mesh of the mirror's triangles.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from scenes import GROUND_I, GROUND_V, standin_mesh
from skin_cases import POSES, make_case, strip_mesh

MESH, GROUND, LAMP, SUN, WALL, TRI = range(6)
TRI_P = np.float32([[-1, 0, 0], [1, 0, 0], [0, 1.5, 0]])
TRI_N = np.float32([[0, 0, 1], [0.6, 0, 0.8], [0, 0.6, 0.8]])


def make_scene(option=P.BUILD_SAH_INTERVALS):
    s = P.Scene()
    s.add_material(P.Material(albedo=(0.5, 0.5, 0.5)))
    s.add_material(P.Material(emissive=(1, 1, 1), intensity=5.0, is_light=True))
    assert s.add_mesh(P.Mesh.from_arrays(*standin_mesh(2)), 0, option) == MESH
    assert s.add_mesh(P.Mesh.from_arrays(GROUND_V, GROUND_I), 0) == GROUND
    assert s.add_mesh(P.Mesh.from_arrays(*strip_mesh(8)), 1) == LAMP
    s.add_light(LAMP)
    assert s.add_sphere((0, 5, 0), 1.0, 1) == SUN
    assert s.add_plane((0, 0, 1), (0, 0, -9), 0) == WALL
    assert s.add_triangle(TRI_P, TRI_N, 0) == TRI
    return s


BINDS = {MESH: P.triangles_from_arrays(*standin_mesh(2)), GROUND: P.triangles_from_arrays(GROUND_V, GROUND_I),
         LAMP: P.triangles_from_arrays(*strip_mesh(8)), TRI: np.concatenate([TRI_P, TRI_N], axis=1).reshape(1, 18)}


def test_the_binding_declares_the_skinning_calls():
    for name in ("cgpth_skin_triangles", "cgpth_scene_skin_mesh", "cgpt_scene_set_skin", "cgpt_scene_skin_mesh", "cgpt_scene_clear_skin"):
        assert name in N.PROTOTYPES and hasattr(N.lib(), name)
    assert N.lib().cgpt_abi_version() == 2


@pytest.mark.parametrize("pose", POSES)
@pytest.mark.parametrize("option", [P.BUILD_SAH_INTERVALS, P.BUILD_SAH_PRIMITIVES])
def test_scene_skin_mesh_equals_refit_of_the_mirrors_triangles(pose, option):
    a, b = make_scene(option), make_scene(option)
    for obj in (MESH, GROUND, TRI):
        j, w, n_joints, m = make_case(pose, BINDS[obj], seed=obj)
        a.skin_mesh(obj, BINDS[obj], j, w, m)
        b.refit_mesh(obj, P.skin_triangles(BINDS[obj], j, w, m))
    for obj in (MESH, GROUND):
        na, ta = a.bvh_export(obj)
        nb, tb = b.bvh_export(obj)
        assert np.array_equal(na, nb) and np.array_equal(ta, tb)
        assert np.float32(a.bvh_info(obj).total_area).view(np.uint32) == np.float32(b.bvh_info(obj).total_area).view(np.uint32)
    da, db = a.flatten(), b.flatten()
    ta = np.ctypeslib.as_array(C.cast(da.triangles, C.POINTER(C.c_float)), shape=(da.n_triangles, 18))
    tb = np.ctypeslib.as_array(C.cast(db.triangles, C.POINTER(C.c_float)), shape=(db.n_triangles, 18))
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32))            # the triangle object too
    c = make_scene(option)
    assert not np.array_equal(a.bvh_export(MESH)[0], c.bvh_export(MESH)[0])  # it moved
    a.close(); b.close(); c.close()


def test_skin_triangles_refusals_write_nothing():
    tris = BINDS[GROUND]
    j, w, n_joints, m = make_case("bend", tris)
    L = N.lib()
    fp, u16 = C.POINTER(C.c_float), C.POINTER(C.c_uint16)

    def raw(t=tris, jj=j, ww=w, mm=m, n=None, nj=None, out=True):
        o = np.full((2, 18), 7.0, np.float32)
        rc = L.cgpth_skin_triangles(None if t is None else t.ctypes.data_as(C.POINTER(N.Triangle)), None if jj is None else jj.ctypes.data_as(u16),
                                    None if ww is None else ww.ctypes.data_as(fp), tris.shape[0] if n is None else n,
                                    None if mm is None else mm.ctypes.data_as(fp), n_joints if nj is None else nj,
                                    o.ctypes.data_as(C.POINTER(N.Triangle)) if out else None)
        assert (o == 7.0).all() or rc == 0
        return rc, L.cgpth_last_error().decode()

    assert raw()[0] == 0
    bad_j = j.copy(); bad_j[1, 2, 3] = 2
    nan_w = w.copy(); nan_w[0, 1, 2] = np.nan
    inf_b = tris.copy(); inf_b[1, 7] = np.inf
    nan_m = m.copy(); nan_m[1, 11] = np.nan
    cases = [(dict(t=None), "bind_triangles is null"), (dict(jj=None), "joints is null"), (dict(ww=None), "weights is null"),
             (dict(mm=None), "joint_matrices is null"), (dict(out=False), "out_triangles is null"),
             (dict(nj=0), "n_joints 0 outside [1, 1024]"), (dict(nj=1025), "n_joints 1025 outside"),
             (dict(jj=bad_j), "joint index 2 >= n_joints 2"), (dict(ww=nan_w), "triangle 0: weight 6 is not finite"),
             (dict(t=inf_b), "bind triangle 1: float 7 is not finite"), (dict(mm=nan_m), "joint 1: entry 11 is not finite")]
    for kw, msg in cases:
        rc, err = raw(**kw)
        assert rc == N.CGPT_ERR_INVALID and msg in err, (kw.keys(), err)
    with pytest.raises(P.HostError, match="joint index 2"):
        P.skin_triangles(tris, bad_j, w, m)
    with pytest.raises(ValueError, match="12 entries per triangle"):
        P.skin_triangles(tris, j[:1], w, m)
    with pytest.raises(ValueError):
        P.skin_triangles(tris, j, w, m.reshape(-1)[:-1])
    wide = make_case("wide", tris)
    assert P.skin_triangles(tris, wide[0], wide[1], wide[3]).shape == tris.shape   # 1024 joints are accepted


def test_scene_skin_mesh_refusals_leave_the_scene_unchanged():
    s = make_scene()
    before = {obj: s.bvh_export(obj)[0].copy() for obj in (MESH, GROUND, LAMP)}
    tris = BINDS[MESH]
    n = tris.shape[0]
    j, w, n_joints, m = make_case("bend", tris)
    gj, gw, _, gm = make_case("bend", BINDS[GROUND])
    bad_j = j.copy(); bad_j[0, 0, 0] = 9
    nan_m = m.copy(); nan_m[0, 0] = np.inf
    lj, lw, _, lm = make_case("bend", BINDS[LAMP])
    cases = [
        (lambda: s.skin_mesh(9, tris, j, w, m), "object 9 out of range"),
        (lambda: s.skin_mesh(SUN, tris, j, w, m), "is a sphere"),
        (lambda: s.skin_mesh(WALL, tris, j, w, m), "is a plane"),
        (lambda: s.skin_mesh(LAMP, BINDS[LAMP], lj, lw, lm), "is a light"),
        (lambda: s.skin_mesh(MESH, BINDS[GROUND], gj, gw, gm), f"has {n} triangles, got 2"),
        (lambda: s.skin_mesh(TRI, BINDS[GROUND], gj, gw, gm), "has 1 triangles, got 2"),
        (lambda: s.skin_mesh(MESH, tris, bad_j, w, m), "joint index 9 >= n_joints 2"),
        (lambda: s.skin_mesh(MESH, tris, j, w, nan_m), "joint 0: entry 0 is not finite"),
        (lambda: s.skin_mesh(MESH, tris, j, w, np.zeros((0, 12), np.float32)), "n_joints 0 outside"),
    ]
    for call, msg in cases:
        with pytest.raises(P.HostError) as e:
            call()
        assert msg in str(e.value), (msg, str(e.value))
    L = N.lib()
    assert L.cgpth_scene_skin_mesh(None, 0, None, None, None, 0, None, 1) == N.CGPT_ERR_INVALID
    assert L.cgpth_scene_skin_mesh(s._h, MESH, None, None, None, n, None, 2) == N.CGPT_ERR_INVALID and "bind_triangles is null" in L.cgpth_last_error().decode()
    for obj, nodes in before.items():
        assert np.array_equal(s.bvh_export(obj)[0], nodes)
    s.skin_mesh(MESH, tris, j, w, m)                                         # and the accepted call moves it
    assert not np.array_equal(s.bvh_export(MESH)[0], before[MESH])
    s.close()
