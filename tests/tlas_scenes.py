"""The specs of tests/tlas_ref.py as host scenes (cpugpupathtracing_amd.Scene), with every mesh's exported tree attached to the spec so
that tlas_ref.SceneModel walks what the device walks."""
import numpy as np

import cpugpupathtracing_amd as P
import tlas_ref as TL

MATERIALS = (dict(albedo=(0.75, 0.75, 0.75)), dict(albedo=(0.8, 0.4, 0.3)), dict(albedo=(0.9, 0.9, 0.9), specular=0.6),
             dict(albedo=(0.9, 0.95, 1.0), specular=0.1, refractivity=0.8, ior=1.5, absorption=(0.1, 0.2, 0.05)))


def to_scene(spec, lamp=None, camera=((0.0, 2.0, 24.0), (0.0, -0.05, -1.0), 60.0, 64.0 / 48.0), settings=None):
    """(scene, model): spec's objects in order; object `lamp` (a sphere) becomes the light.  The caller closes the scene."""
    s = P.Scene()
    mats = [s.add_material(P.Material(**m)) for m in MATERIALS]
    emitter = s.add_material(P.Material(emissive=(1.0, 0.95, 0.85), intensity=25.0, is_light=True))
    for k, ob in enumerate(spec):
        mat = emitter if k == lamp else mats[k % len(mats)]
        if ob["kind"] == "sphere":
            idx = s.add_sphere(ob["center"], ob["radius"], mat)
        elif ob["kind"] == "plane":
            idx = s.add_plane(ob["normal"], ob["point"], mat)
        elif ob["kind"] == "triangle":
            idx = s.add_triangle(ob["positions"], ob["normal"], mat)
            if ob.get("transform") is not None:
                s.set_transform(idx, ob["transform"])
        else:
            mesh = P.Mesh.from_arrays(ob["vertices"], ob["indices"])
            idx = s.add_mesh(mesh, mat, transform=ob.get("transform"))
            ob["model"] = TL.MeshModel(ob["vertices"], ob["indices"], *s.bvh_export(idx))
            mesh.close()
        assert idx == k
    if lamp is not None:
        s.add_light(lamp)
    s.set_camera(*camera)
    if settings is not None:
        s.set_settings(settings)
    return s, TL.SceneModel(spec)


def all_rays(model):
    """The rays of the tests: 4096 random ones (a quarter with a finite tmax; the first 512 hits' points start 512 more, replacing the
    last 512), and 256 with one or two zero direction components: (o, d, tmax) of 4096 rays, (o, d) of 256."""
    o, d, tmax = TL.random_rays()
    t, obj, _, _, _ = model.walk(o[:2048], d[:2048], tmax[:2048])
    so, sd = TL.surface_rays(o[:2048], d[:2048], t, obj)
    assert so.shape[0] == 512
    o[-512:] = so; d[-512:] = sd; tmax[-512:] = 1e34
    ao, ad = TL.axis_rays()
    return (o, d, tmax), (ao, ad)
