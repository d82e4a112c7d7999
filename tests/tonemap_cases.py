"""The images of the display stage's tests (tests/test_tonemap_reference.py, tests/test_gpu_tonemap.py): host arrays of
at most 300 x 217 float4 pixels, each the smallest that reaches one way the stage can go wrong.  Built once; nothing changes them."""
import numpy as np

from tonemap_ref import F, FLT_MAX, index_luminance

DENORMAL = np.float32(1e-41)
BELOW = lambda v: np.nextafter(F(v), F(0.0))
# luminance -> the bin the issue states (-1: not counted)
BIN_OF = [(F(2.0 ** -16), 0), (BELOW(2.0 ** -16), 0), (F(1.0), 128), (BELOW(1.0), 127), (F(2.0 ** 16), 255), (BELOW(2.0 ** 16), 255),
          (FLT_MAX, 255), (F(1e-30), 0), (DENORMAL, 0), (F(0.0), -1), (F(-0.0), -1), (F(-1.0), -1), (F(np.nan), -1), (F(np.inf), -1), (F(-np.inf), -1)]
# pixels whose luminance is one of the above kinds, and channels a curve must survive
SPECIAL_PIXELS = np.array([
    [0, 0, 0, 1], [-1, -1, -1, 1], [np.nan, 0.5, 0.5, 1], [0.5, np.nan, np.nan, 1], [np.inf, 1, 1, 1], [-np.inf, 1, 1, 1], [1e-41, 1e-41, 1e-41, 1],
    [2.0 ** -16, 2.0 ** -16, 2.0 ** -16, 1], [1, 1, 1, 1], [2.0 ** 16, 2.0 ** 16, 2.0 ** 16, 1], [3e38, 3e38, 3e38, 1], [1e-30, 1e-30, 1e-30, 1],
    [-0.0, -0.0, -0.0, 1], [5, -2, 0.25, 1], [0.0031308, 0.0031309, 0.0031307, 1], [1e30, 1e-30, 1, 1]], np.float32)


def hdr(rows, width, seed, octaves=6.0, scale=1.0):
    """log-normal radiance over about +-octaves around `scale`, the channels apart"""
    rng = np.random.default_rng(seed)
    base = np.exp2(rng.normal(0.0, octaves / 3.0, (rows, width, 1))) * scale
    image = (base * rng.uniform(0.2, 1.8, (rows, width, 3))).astype(np.float32)
    return np.concatenate([image, np.ones((rows, width, 1), np.float32)], axis=-1)


def grey(values):
    v = np.asarray(values, np.float32).reshape(1, -1, 1)
    return np.concatenate([v, v, v, np.ones_like(v)], axis=-1)


def one_bin(rows=31, width=67):
    """every luminance in bin 120 ([0.5, 0.5625)): one LDS word takes every atomic of a wave"""
    rng = np.random.default_rng(5)
    v = rng.uniform(0.51, 0.55, (rows, width, 1)).astype(np.float32)
    return np.concatenate([v, v, v, np.ones_like(v)], axis=-1)


def all_bins():
    """1 + (i % 3) pixels at the centre of every bin i"""
    centres = [F(index_luminance(i + 0.5)) for i in range(256) for _ in range(1 + i % 3)]
    return grey(np.random.default_rng(6).permutation(np.array(centres, np.float32)))


def with_specials(rows=37, width=29, seed=7):
    image = hdr(rows, width, seed).reshape(-1, 4)
    at = np.random.default_rng(seed + 1).choice(image.shape[0], 4 * len(SPECIAL_PIXELS), replace=False)
    image[at] = np.tile(SPECIAL_PIXELS, (4, 1))
    return image.reshape(rows, width, 4)


def ramp(n=512, top=16.0):
    """0 .. top, rising, for the curves"""
    return grey(np.concatenate([[0.0], np.geomspace(1e-4, top, n - 1)]))


IMAGES = {
    "1x1": hdr(1, 1, 1),
    "255": hdr(1, 255, 2),
    "256": hdr(1, 256, 3),
    "257": hdr(1, 257, 4),
    "300x217": hdr(217, 300, 8, octaves=10.0),          # several grid-stride passes and a ragged tail
    "one_bin": one_bin(),
    "all_bins": all_bins(),
    "specials": with_specials(),
    "black": np.zeros((5, 7, 4), np.float32),
    "all_nan": np.full((5, 7, 4), np.nan, np.float32),
}
METERED = [k for k in IMAGES if k not in ("black", "all_nan")]
# three frames of different brightness, then one more after a reset; the alphas of the first three
SEQUENCE = [hdr(23, 41, 11, scale=0.05), hdr(23, 41, 12, scale=1.0), hdr(23, 41, 13, scale=20.0), hdr(23, 41, 14, scale=3.0)]
SEQUENCE_ALPHAS = [0.0, 0.5, 1.0, 0.25]
CURVE_NAMES = ("clamp", "reinhard", "aces", "hable")

# ---- the sRGB check's inputs and bound (test_gpu_tonemap.py) ----------------------------------------------------------------------------
SRGB_INPUTS = ("300x217", "specials", "all_bins", "257")


def srgb_deviation(curve):
    """the largest relative deviation of tonemap_ref's float32 statement from its float64 model behind the sRGB transfer over
    SRGB_INPUTS, auto (the defaults) and manual (exposure 1): numpy alone, nothing of the library"""
    import tonemap_ref as R
    worst = 0.0
    for name in SRGB_INPUTS:
        for auto in (True, False):
            rgba, _, info = R.tonemap(IMAGES[name], None, curve=curve, transfer="srgb", auto=auto)
            exposure = info["exposure"] if auto else F(1.0)
            worst = max(worst, R.relative_deviation(rgba[..., :3], R.model(IMAGES[name], exposure, curve=curve, transfer="srgb")))
    return worst


# 4 x srgb_deviation(curve) as measured (numpy 2, x86-64), rounded up to two digits; the factor is the room of the device's powf, a few
# ulp where numpy's is under one.  The deviation is tonemap_ref.relative_deviation's: relative to max(|y|, 2^-8).
#   measured   clamp 2.73e-7   reinhard 3.94e-7   aces 3.71e-7   hable 8.76e-5 (the cancellation of T(x) - E/F near 0, over h(white))
SRGB_BOUND = {"clamp": 1.1e-6, "reinhard": 1.6e-6, "aces": 1.5e-6, "hable": 3.6e-4}
