"""The temporal stage's C ABI (include/cpugpupt_abi.h: cgpt_denoise_temporal, cgpt_temporal_reset, cgpt_read_temporal_history) and the
numpy statement of its operations (temporal_ref.py) against closed forms, and how many pixels a float32 run of the statement decides
differently on the scenes and camera moves of the device tests.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cpugpupathtracing_amd import _native as N
import denoise_ref as D
import temporal_ref as T
import temporal_cases as TC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_temporal_calls():
    with open(os.path.join(REPO, "include", "cpugpupt_abi.h")) as f:
        header = f.read()
    for name in ("cgpt_denoise_temporal", "cgpt_temporal_reset", "cgpt_read_temporal_history"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in N.PROTOTYPES
        assert hasattr(N.lib(), name)
    assert "CGPT_TEMPORAL_KEEP_VIEW_DEPENDENT = 1u" in header and N.TEMPORAL_KEEP_VIEW_DEPENDENT == 1
    assert "#define CGPT_ABI_VERSION 2u" in header and N.lib().cgpt_abi_version() == 2
    assert "counts" in header and "twice" in header                          # a second call without a new render
    assert C.sizeof(N.TemporalParams) == 16
    assert [f[0] for f in N.TemporalParams._fields_] == ["max_history", "normal_cos_min", "plane_tolerance", "flags"]


def test_null_context_is_refused_without_a_device():
    L = N.lib()
    cam = N.Camera()
    buf = (C.c_float * 4)()
    assert L.cgpt_denoise_temporal(None, C.byref(cam), None, None, buf, 4, None, 0) == N.CGPT_ERR_INVALID
    assert L.cgpt_temporal_reset(None) == N.CGPT_ERR_INVALID
    assert L.cgpt_read_temporal_history(None, buf, 4) == N.CGPT_ERR_INVALID


# ---- a fronto-parallel plane z = 0 seen from z = 8: one pixel is one world unit ----------------------------------------------------

PW, PH = 16, 8


def plane_camera(cx=0.0):
    return np.float32([cx, 0, 8, cx - 1, 0.5, 7, cx + 1, 0.5, 7, cx - 1, -0.5, 7])


def plane_guides(cx=0.0, obj_edge=None):
    """the guides of the plane from the camera at (cx, 0, 8); obj_edge: world x from which on the object index is 1, not 0"""
    px, py = np.meshgrid(np.arange(PW), np.arange(PH))
    x = np.stack([cx - 8.0 + px, 4.0 - py, np.zeros((PH, PW))], -1)
    g = np.zeros((PH, PW, 12), np.float32)
    g[..., 0:3] = x
    g[..., 3] = np.sqrt(np.sum((x - [cx, 0, 8]) ** 2, -1))
    g[..., 6] = 1.0
    gu = g.view(np.uint32)
    gu[..., 7] = 0 if obj_edge is None else (x[..., 0] >= obj_edge).astype(np.uint32)
    g[..., 8:11] = 0.5
    gu[..., 11] = 1
    return g


def frame(model, acc, n, g, cam, **kw):
    kw.setdefault("iterations", 0)
    kw.setdefault("demodulate", False)
    kw.setdefault("light_materials", [False, False])
    kw.setdefault("view_dependent_materials", [False, False])
    return model.frame(acc, n, g, cam, height=PH, **kw)


def random_acc(rng, n):
    a = np.zeros((PH, PW, 4), np.float32)
    a[..., :3] = rng.uniform(0.0, 2.0, (PH, PW, 3)) * n
    return a


def test_identical_cameras_merge_by_sample_counts_and_cap_as_a_moving_average():
    rng = np.random.default_rng(1)
    g, cam = plane_guides(), plane_camera()
    m = T.Temporal()
    a1, a2, a3 = random_acc(rng, 3), random_acc(rng, 5), random_acc(rng, 2)
    c1, c2, c3 = (D.radiance(a, n).astype(np.float64) for a, n in ((a1, 3), (a2, 5), (a3, 2)))
    out1, _ = frame(m, a1, 3, g, cam)
    assert np.array_equal(out1[..., :3], c1) and np.all(m.history[..., 3] == 3)       # no history: c_0 itself
    out2, px = frame(m, a2, 5, g, cam)
    assert np.allclose(out2[..., :3], (3 * c1 + 5 * c2) / 8, rtol=1e-15, atol=0) and np.all(m.history[..., 3] == 8)
    assert np.all(out2[..., 3] == 1.0) and np.array_equal(px, D.pack_pixels(out2[..., :3]))
    out3, _ = frame(m, a3, 2, g, cam, max_history=6.0)                         # He = min(8, 6): the moving average at H = max_history
    assert np.allclose(out3[..., :3], (6 * out2[..., :3] + 2 * c3) / 8, rtol=1e-15, atol=0) and np.all(m.history[..., 3] == 6)
    m.reset()
    out, _ = frame(m, a3, 2, g, cam)
    assert np.array_equal(out[..., :3], c3) and np.all(m.history[..., 3] == 2)
    out, _ = frame(m, a1, 100, g, cam, max_history=64.0)                       # one frame above the cap
    assert np.all(m.history[..., 3] == 64)


def test_a_key_change_drops_the_history():
    rng = np.random.default_rng(2)
    g, cam = plane_guides(), plane_camera()
    for kw in (dict(generation=1), dict(demodulate=True), dict(first_row=1)):
        m = T.Temporal()
        frame(m, random_acc(rng, 4), 4, g, cam)
        frame(m, random_acc(rng, 4), 4, g, cam, **kw)
        assert np.all(m.history[..., 3] == 4), kw


def test_a_shift_by_two_pixels_moves_the_history_by_two_columns():
    rng = np.random.default_rng(3)
    m = T.Temporal()
    a1, a2 = random_acc(rng, 4), random_acc(rng, 1)
    out1, _ = frame(m, a1, 4, plane_guides(0.0), plane_camera(0.0))
    out2, _ = frame(m, a2, 1, plane_guides(2.0), plane_camera(2.0))           # the camera moved two world units = two pixels to the right
    c2 = D.radiance(a2, 1).astype(np.float64)
    want = (4 * out1[:, 2:, :3] + c2[:, :-2]) / 5
    assert np.allclose(out2[:, :-2, :3], want, rtol=1e-12, atol=0)
    assert np.all(m.history[:, :-2, 3] == 5)
    assert np.all(m.history[:, -2:, 3] == 1) and np.array_equal(out2[:, -2:, :3], c2[:, -2:])   # newly exposed: H' = N, c = c_0


def test_an_object_edge_rejects_the_taps_across_it():
    rng = np.random.default_rng(4)
    m = T.Temporal()
    a1, a2 = random_acc(rng, 4), random_acc(rng, 1)
    edge = 1.5                                                                # between world x = 1 and 2: pixels 9 | 10 of the first frame
    out1, _ = frame(m, a1, 4, plane_guides(0.0, edge), plane_camera(0.0))
    out2, _ = frame(m, a2, 1, plane_guides(2.5, edge), plane_camera(2.5))     # 2.5 pixels: taps at px + 2 and px + 3, half each
    c2 = D.radiance(a2, 1).astype(np.float64)
    h = out1[..., :3]
    # current pixel px sees world x = px - 5.5; its taps are the first frame's pixels px + 2 (world px - 6) and px + 3 (world px - 5)
    for px in range(PW - 3):
        wx_obj = int(px - 5.5 >= edge)
        taps = [q for q in (px + 2, px + 3) if int(q - 8.0 >= edge) == wx_obj]
        assert taps, px
        c_h = np.mean([h[:, q] for q in taps], 0)
        assert np.allclose(out2[:, px, :3], (4 * c_h + c2[:, px]) / 5, rtol=1e-12, atol=0), px
    assert len([q for q in (7 + 2, 7 + 3) if int(q - 8.0 >= edge) == int(7 - 5.5 >= edge)]) == 1   # pixel 7 straddles the edge
    # the last column has one tap in the band with weight 1/2 > 0.01: it is used alone
    assert np.allclose(out2[:, PW - 3, :3], (4 * np.mean([h[:, PW - 1]], 0) + c2[:, PW - 3]) / 5, rtol=1e-12, atol=0)
    assert np.all(m.history[:, PW - 2:, 3] == 1)


def test_normal_and_plane_tests_reject_taps():
    rng = np.random.default_rng(5)
    hist = np.concatenate([rng.uniform(size=(PH, PW, 3)), np.full((PH, PW, 1), 7.0)], -1)
    gp, cam_p = plane_guides(0.0), plane_camera(0.0)
    g = plane_guides(2.0)
    _, H, _ = T.reproject(g, hist, gp, cam_p, PH, 0)
    assert np.all(H[:, :-2] == 7) and np.all(H[:, -2:] == 0)
    tilted = g.copy()
    tilted[..., 4:7] = np.float32([0.6, 0.0, 0.8])                             # n_prev . n = 0.8 < 0.9
    assert np.all(T.reproject(tilted, hist, gp, cam_p, PH, 0)[1] == 0)
    assert np.all(T.reproject(tilted, hist, gp, cam_p, PH, 0, normal_cos_min=0.75, plane_tolerance=10.0)[1][:, :-2] == 7)
    lifted = gp.copy()
    lifted[..., 2] = 0.2                                                      # the history's surface 0.2 off the current tangent plane; t >= 8
    assert np.all(T.reproject(g, hist, lifted, cam_p, PH, 0, plane_tolerance=0.01)[1] == 0)
    assert np.all(T.reproject(g, hist, lifted, cam_p, PH, 0, plane_tolerance=0.03)[1][:, :-2] == 7)
    miss = g.copy()
    miss.view(np.uint32)[..., 7] = D.NO_HIT
    assert np.all(T.reproject(miss, hist, gp, cam_p, PH, 0)[1] == 0)          # a current miss has no history
    prev_miss = gp.copy()
    prev_miss.view(np.uint32)[..., 7] = D.NO_HIT
    assert np.all(T.reproject(g, hist, prev_miss, cam_p, PH, 0)[1] == 0)


def test_a_point_behind_the_previous_camera_has_no_history():
    hist = np.ones((PH, PW, 4))
    gp, cam_p = plane_guides(0.0), plane_camera(0.0)
    g = plane_guides(0.0)
    g[..., 2] = 9.0                                                           # behind the camera at z = 8 that looks down -z: a = -1
    g[..., 0:2] *= -0.125                                                     # ... and mirrored onto the middle of its screen
    lenient = dict(normal_cos_min=-1.0, plane_tolerance=1e6)
    assert np.all(T.reproject(g, hist, gp, cam_p, PH, 0, **lenient)[1] == 0)
    g[..., 2] = 7.5                                                           # in front of it the same points are accepted
    g[..., 0:2] *= -1.0
    assert np.any(T.reproject(g, hist, gp, cam_p, PH, 0, **lenient)[1] > 0)


def test_a_singular_camera_has_no_history():
    cam = plane_camera()
    cam[9:12] = cam[3:6]                                                      # bottom_left = top_left
    assert T.camera_minv(cam) is None
    assert np.all(T.reproject(plane_guides(), np.ones((PH, PW, 4)), plane_guides(), cam, PH, 0)[1] == 0)


def test_view_dependent_materials_drop_the_history_after_a_move_only():
    rng = np.random.default_rng(6)
    a = random_acc(rng, 2)
    for keep, same_camera, want in ((False, False, 2), (True, False, 4), (False, True, 4)):
        m = T.Temporal()
        frame(m, a, 2, plane_guides(0.0), plane_camera(0.0), view_dependent_materials=[False, True])
        cx = 0.0 if same_camera else 2.0
        frame(m, a, 2, plane_guides(cx), plane_camera(cx), view_dependent_materials=[False, True], keep_view_dependent=keep)
        assert np.all(m.history[:, :-2, 3] == want), (keep, same_camera)


# ---- a float32 run of the statement on the device tests' scenes and camera moves ---------------------------------------------------

@pytest.fixture(scope="module")
def oracle_guides():
    out = {}
    for which in TC.SCENES:
        o, s = TC.scene_pair(which)
        for name, view in [("base", TC.BASE)] + list(TC.MOVES.items()):
            cam = TC.set_camera(o, s, view)
            ro, rd = o.camera_rays(TC.W, TC.H)
            ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
            t, obj, tri, _ = o.intersect_rays(ro, rd)
            out[which, name] = (D.guides_from_hits(s.flatten(), ro, rd, t, obj, tri).reshape(TC.H, TC.W, 12), T.camera_array(cam))
    return out


@pytest.mark.parametrize("move", list(TC.MOVES))
@pytest.mark.parametrize("which", TC.SCENES)
def test_a_float32_run_decides_few_pixels_differently(oracle_guides, which, move):
    g_prev, cam_prev = oracle_guides[which, "base"]
    g, _ = oracle_guides[which, move]
    hist = np.ones((TC.H, TC.W, 4))
    taps64 = T.reproject(g, hist, g_prev, cam_prev, TC.H, 0, dtype=np.float64)[2]
    taps32 = T.reproject(g, hist, g_prev, cam_prev, TC.H, 0, dtype=np.float32)[2]
    share = float(np.mean(taps64 != taps32))
    kept = float(np.mean(taps64 >= 0))
    print(f"{which} / {move}: {share:.4%} of the pixels decided differently in float32; {kept:.1%} keep a history")
    assert kept > 0.3                                                          # the move leaves most hits their history
    assert np.mean(taps64 < 0) > 0.02                                          # ... and takes it from some (misses, disocclusion, the frame's edge)
    assert share < TC.CAP
