"""The denoiser's C ABI (include/cpugpupt_abi.h: cgpt_read_guides, cgpt_denoise) and the numpy statement of its filter (denoise_ref.py,
DESIGN.md 5.8).  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np

from cpugpupathtracing_amd import _native as N
import denoise_ref as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _guides(hit, normal=(0.0, 1.0, 0.0), albedo=(0.5, 0.5, 0.5), mat=1, depth=None):
    """guides of a flat frame: hit pixels on the plane y = 0 seen from above, with one normal and one albedo"""
    H, W = hit.shape
    g = np.zeros((H, W, 12), np.float32)
    gu = g.view(np.uint32)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    g[..., 0] = np.where(hit, xs, 0); g[..., 2] = np.where(hit, ys, 0)
    g[..., 3] = np.where(hit, 5.0 if depth is None else depth, 1e34)
    g[..., 4:7] = np.where(hit[..., None], np.float32(normal), 0)
    g[..., 8:11] = np.where(hit[..., None], np.float32(albedo), 0)
    gu[..., 7] = np.where(hit, 1, D.NO_HIT)
    gu[..., 11] = np.where(hit, mat, D.NO_HIT)
    return g


def test_header_declares_and_library_exports_the_denoiser():
    with open(os.path.join(REPO, "include", "cpugpupt_abi.h")) as f:
        header = f.read()
    for name in ("cgpt_denoise", "cgpt_read_guides"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in N.PROTOTYPES
        assert hasattr(N.lib(), name)
    assert "CGPT_DENOISE_DEMODULATE_ALBEDO = 1u" in header
    assert N.DENOISE_DEMODULATE_ALBEDO == 1
    assert N.lib().cgpt_abi_version() == 2


def test_params_struct_is_20_bytes():
    assert C.sizeof(N.DenoiseParams) == 20
    assert [f[0] for f in N.DenoiseParams._fields_] == ["iterations", "flags", "sigma_color", "sigma_normal", "sigma_position"]


def test_null_context_is_refused():
    L = N.lib()
    cam = N.Camera()
    buf = (C.c_float * 12)()
    assert L.cgpt_read_guides(None, C.byref(cam), buf, 12) == N.CGPT_ERR_INVALID
    assert L.cgpt_denoise(None, C.byref(cam), None, buf, 4, None, 0) == N.CGPT_ERR_INVALID


def test_zero_iterations_is_the_identity():
    rng = np.random.default_rng(1)
    acc = rng.uniform(0, 7, (9, 13, 4)).astype(np.float32)
    g = _guides(rng.uniform(size=(9, 13)) < 0.6)
    rgba, px = D.denoise(acc, 7, g, iterations=0, light_materials=[False, False])
    c = acc[..., :3] / np.float32(7)
    assert np.array_equal(rgba[..., :3].astype(np.float32).view(np.uint32), c.view(np.uint32))
    assert np.all(rgba[..., 3] == 1.0)
    assert np.array_equal(px, D.pack_pixels(c))


def test_constant_colour_on_one_surface_is_unchanged():
    hit = np.ones((11, 17), bool)
    g = _guides(hit, albedo=(0.25, 0.5, 0.75))
    acc = np.zeros((11, 17, 4), np.float32)
    acc[..., :3] = np.float32([0.3, 0.6, 0.9]) * 4
    for demod in (False, True):
        rgba, _ = D.denoise(acc, 4, g, iterations=5, demodulate=demod, light_materials=[False, False])
        np.testing.assert_allclose(rgba[..., :3], np.broadcast_to([0.3, 0.6, 0.9], (11, 17, 3)), rtol=1e-6)


def test_hits_and_misses_never_mix():
    hit = np.zeros((12, 12), bool)
    hit[:, :6] = True
    g = _guides(hit)
    acc = np.zeros((12, 12, 4), np.float32)
    acc[..., :3] = np.where(hit[..., None], 0.2, 5.0)
    rgba, _ = D.denoise(acc, 1, g, iterations=4, sigma_color=1e6, demodulate=False, light_materials=[False, False])
    np.testing.assert_allclose(rgba[hit][:, :3], np.float32(0.2), rtol=1e-12)
    np.testing.assert_allclose(rgba[~hit][:, :3], 5.0, rtol=1e-12)


def test_demodulation_rules():
    hit = np.ones((2, 2), bool)
    hit[1, 1] = False
    g = _guides(hit, albedo=(0.5, 1e-4, 1e-3), mat=1)
    g.view(np.uint32)[0, 1, 11] = 0                     # a light material
    m = D.demodulation(g, [True, False])
    np.testing.assert_array_equal(m[0, 0], [0.5, 1.0, np.float32(1e-3)])
    np.testing.assert_array_equal(m[0, 1], [1.0, 1.0, 1.0])
    np.testing.assert_array_equal(m[1, 1], [1.0, 1.0, 1.0])


def test_one_row_band_skips_taps_outside():
    """A band of one row: the vertical taps are skipped, so the result is the 1-D filter along the row, not a clamped 2-D one"""
    rng = np.random.default_rng(3)
    W = 23
    acc = np.zeros((1, W, 4), np.float32)
    acc[..., :3] = rng.uniform(0, 1, (1, W, 3))
    g = _guides(np.ones((1, W), bool))
    got, _ = D.denoise(acc, 1, g, iterations=2, sigma_color=0.5, demodulate=False, light_materials=[False, False])
    # the same row in the middle of a frame of identical rows with the vertical weights removed: the 1-D filter
    c = acc[0, :, :3].astype(np.float64)
    for i in range(2):
        s, sc = 1 << i, 0.5 * 2.0 ** -i
        num = np.zeros_like(c); den = np.zeros(W)
        for dx in range(-2, 3):
            for x in range(W):
                q = x + dx * s
                if 0 <= q < W:
                    w = D.K[abs(dx)] * D.K[0] * np.exp(-np.sum((c[q] - c[x]) ** 2) / (sc * sc))
                    num[x] += w * c[q]; den[x] += w
        c = num / den[:, None]
    np.testing.assert_allclose(got[0, :, :3], c, rtol=1e-12)
    assert got.shape == (1, W, 4)


def test_guides_from_hits_marks_misses():
    desc = N.SceneDesc()
    desc.n_objects = 0; desc.n_triangles = 0
    g = D.guides_from_hits(desc, np.zeros((3, 3), np.float32), np.ones((3, 3), np.float32), np.full(3, 1e34, np.float32),
                           np.full(3, D.NO_HIT, np.uint32), np.zeros(3, np.uint32))
    assert np.all(g[:, 3] == np.float32(1e34))
    assert np.all(g.view(np.uint32)[:, 7] == D.NO_HIT) and np.all(g.view(np.uint32)[:, 11] == D.NO_HIT)
    assert np.all(g[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] == 0)
