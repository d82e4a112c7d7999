"""cgpt_scene_upload on the device: a scene that the validation refuses leaves the previous scene installed and renderable, on
a one-device context and on every member of a multi-device one.  (What the validation refuses, and the layout an accepted
scene gets, are CPU tests: tests/test_host_scene_layout.py.)"""
import ctypes as C

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N

pytestmark = pytest.mark.gpu

W, H, SPP = 32, 24, 2


@pytest.fixture(params=["single", "group3"])
def renderer(request):
    r = P.Renderer(0) if request.param == "single" else P.Renderer([0, 0, 0], flags=P.CTX_GATHER_PEER_COPY)
    yield r
    r.close()


def test_refused_upload_keeps_the_scene(renderer):
    s = P.Scene.reference_layout(P.Mesh.dragon_standin(1), aspect=W / H)
    renderer.upload(s)
    renderer.render(W, H, SPP, kernel=P.KERNEL_AUTO)
    acc0 = renderer.accumulator().copy()
    assert acc0.any()

    desc = s.flatten()
    mesh = next(desc.objects[k] for k in range(desc.n_objects) if desc.objects[k].kind == N.OBJECT_MESH and desc.objects[k].tri_count == 80)
    tri_indices = np.ctypeslib.as_array(desc.tri_indices, shape=(desc.n_triangles,)).copy()
    tri_indices[mesh.tri_offset] = mesh.tri_count             # the mesh's tri_indices[0] names a triangle it does not have
    bad = N.SceneDesc.from_buffer_copy(desc)
    bad.tri_indices = tri_indices.ctypes.data_as(C.POINTER(C.c_uint32))
    rc = renderer.L.cgpt_scene_upload(renderer._ctx, C.byref(bad))
    msg = renderer.L.cgpt_last_error(renderer._ctx).decode()
    assert rc == N.CGPT_ERR_INVALID and "tri_indices[0] = 80 out of range" in msg, (rc, msg)
    assert msg.startswith("device 0: ") == renderer.is_group, msg

    renderer.reset_accumulator()
    renderer.render(W, H, SPP, kernel=P.KERNEL_AUTO)
    assert np.array_equal(renderer.accumulator().view(np.uint32), acc0.view(np.uint32))
