"""Frames, sizes and the tolerance shared by the variance-guided filter's tests (test_variance_reference.py on the CPU,
test_gpu_variance.py on the device)."""
import numpy as np

import temporal_ref as T
import temporal_cases as TC

W, H = TC.W, TC.H                 # the denoise tests' own size
SMALL = (37, 21)                  # no multiple of the 16-pixel tile and smaller than 4 x 16: pass 4's taps leave the band on both sides
SEED = 0x12345678
# (camera, samples) of the temporal sequence: static, then the translation and the view change of temporal_cases.  The sample counts keep
# Ke + N away from min_history_frames N wherever a reprojected K is an integer up to rounding (the switch itself happens on static
# frames, where K is exact): K = 2, 4, 6, 8 on the static frames, then about 8 + 1 = 9 >= 2, 4 and about 9 + 2 = 11 >= 4, 8, and
# 0 + 1 < 2, 1 + 2 < 4 on revealed pixels.
SEQUENCE = (("base", 2), ("base", 2), ("base", 2), ("base", 2), ("translation", 1), ("rotation", 2))
MIN_HISTORY = (2, 4)              # the switch to var_t happens at frame 1 and at frame 3
FIRST_TEMPORAL = {2: 1, 4: 3}
CAP = 0.005                       # the share of a frame that may be left out beyond the pixels a float32 run decides differently

# The largest deviation of a float32 run of the statement from the float64 one on these scenes, sizes and frames, in units of
# max(1, |ref|), over the variance map, the stored colour and the output (test_variance_reference.py measures it and holds it under
# this figure): the device, with __expf and another summation order, is held to max(1e-4, 4 x this).
DEV32 = 2.5e-5
TOL = max(1e-4, 4.0 * DEV32)


def rel_err(got, ref):
    ref = np.asarray(ref, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref) / np.maximum(1.0, np.abs(ref))


def carried(tainted, guides, hist_camera, camera, height, taps):
    """the pixels whose history comes through a tainted pixel of the history's frame"""
    if not tainted.any():
        return tainted
    if T.camera_array(hist_camera).tobytes() == T.camera_array(camera).tobytes():
        return tainted
    where = T.previous_position(guides, hist_camera, height, 0)
    if where is None:
        return np.zeros_like(tainted)
    fx, fy, _ = where
    rows, width = tainted.shape
    x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    out = np.zeros_like(tainted)
    for j in (0, 1):
        for i in (0, 1):
            out |= tainted[np.clip(y0 + j, 0, rows - 1), np.clip(x0 + i, 0, width - 1)]
    return out & (taps >= 0)
