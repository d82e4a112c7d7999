"""Scenes and camera pairs shared by the temporal tests (test_temporal_reference.py on the CPU, test_gpu_temporal.py on the device)."""
from scenes import reference_layout_pair, standin_mesh
from test_gpu_denoise import all_kinds_pair

W, H = 97, 61
FOV = 60.0
BASE = ((0.0, 0.0, 8.0), (0.0, 0.0, -1.0))
# camera moves whose screen-space shifts are a fraction of a pixel off integers over most of the frame: a translation (the shift depends
# on the depth: parallax, disocclusion behind the small objects) and a rotation (a new view direction; the reference's camera keeps its
# screen plane parallel to the world's xy plane, so this shifts the plane: an off-axis view)
MOVES = {"translation": ((0.31, 0.17, 7.9), (0.0, 0.0, -1.0)), "rotation": ((0.0, 0.0, 8.0), (0.043, -0.027, -1.0))}
REVEAL = ((1.5, 0.0, 8.0), (0.0, 0.0, -1.0))   # far enough to the side to see the wall behind the all-kinds scene's small sphere
SCENES = ("reference", "all_kinds")
CAP = 0.005                       # the share of a frame whose tap validity a float32 run may decide differently


def scene_pair(which):
    """(oracle scene, product scene) with the camera at BASE: the reference layout around the glass stand-in, or every object kind"""
    if which == "reference":
        return reference_layout_pair(*standin_mesh(2), 3, aspect=W / H)
    return all_kinds_pair(W / H)


def set_camera(o, s, view):
    """moves both cameras of a pair; the cgpt_camera of the product scene"""
    if o is not None:
        o.set_camera(view[0], view[1], FOV, W / H)
    s.set_camera(view[0], view[1], FOV, W / H)
    return s.camera()


def view_dependent_materials(s):
    desc = s.flatten()
    return [desc.materials[k].specular > 0 or desc.materials[k].refractivity > 0 for k in range(desc.n_materials)]
