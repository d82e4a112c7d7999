"""The display stage's Python side: the parameter block of cgpt_tonemap / cgpth_tonemap, the host mirror
tonemap_host and the adaptation helper.  Renderer.tonemap (renderer.py) is the device call."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import numpy as np

from . import _native as N

SOURCES = {"accumulator": N.TONEMAP_ACCUMULATOR, "denoised": N.TONEMAP_DENOISED, "host": N.TONEMAP_HOST}
CURVES = {"clamp": N.CURVE_CLAMP, "reinhard": N.CURVE_REINHARD, "aces": N.CURVE_ACES, "hable": N.CURVE_HABLE}
TRANSFERS = {"linear": N.TRANSFER_LINEAR, "srgb": N.TRANSFER_SRGB}


def adaptation_alpha(dt: float, speed: float) -> float:
    """The `alpha` of an auto-exposure call dt seconds after the last one: 1 - exp(-dt speed), the step of an exponential approach
    with time constant 1 / speed.  The library takes only the number."""
    return 1.0 - math.exp(-float(dt) * float(speed))


def tonemap_params(source="accumulator", curve="aces", transfer="srgb", auto: bool = True, exposure_scale: float = 1.0, ev_bias: int = 0,
                   white: float = 4.0, key: float = 0.18, low_fraction: float = 0.5, high_fraction: float = 0.02, alpha: float = 1.0,
                   image: Optional[np.ndarray] = None, flags: Optional[int] = None):
    """cgpt_tonemap_params and what must outlive it.  source / curve / transfer: a name of SOURCES / CURVES / TRANSFERS or the ABI's
    number; image: (rows, width, 4) float32 for the host source; flags overrides `auto`.  The defaults are those of a NULL block."""
    p = N.TonemapParams()
    p.source = SOURCES[source] if isinstance(source, str) else int(source)
    p.curve = CURVES[curve] if isinstance(curve, str) else int(curve)
    p.transfer = TRANSFERS[transfer] if isinstance(transfer, str) else int(transfer)
    p.flags = int(flags) if flags is not None else (N.TONEMAP_AUTO_EXPOSURE if auto else 0)
    p.exposure_scale, p.ev_bias, p.white = float(exposure_scale), int(ev_bias), float(white)
    p.key, p.low_fraction, p.high_fraction, p.alpha = float(key), float(low_fraction), float(high_fraction), float(alpha)
    keep = None
    if image is not None:
        keep = np.ascontiguousarray(image, np.float32)
        if keep.ndim != 3 or keep.shape[2] != 4:
            raise ValueError("image must be (rows, width, 4) float32")
        p.src_rgba = keep.ctypes.data_as(C.POINTER(C.c_float))
        p.src_height, p.src_width = keep.shape[0], keep.shape[1]
    return p, keep


def tonemap_host(image: np.ndarray, state: Optional[N.ExposureState] = None, **params) -> Tuple[np.ndarray, np.ndarray, Optional[N.ExposureInfo]]:
    """cgpth_tonemap: the display stage on the host, with no GPU -- bit for bit what Renderer.tonemap(source="host", image=...) returns
    except behind transfer="srgb" (the two powf differ by a few ulp).  image: (rows, width, 4) float32 linear radiance.  state: an
    ExposureState (cpugpupathtracing_amd.ExposureState(); the adaptation a Renderer keeps inside), updated in place by an auto-exposure
    call; None: a fresh one each call.  params: as tonemap_params.  Returns (rgba (rows, width, 4) float32, pixels (rows, width)
    uint32, the reading or None in manual mode)."""
    from .scene import HostError
    p, keep = tonemap_params(source="host", image=image, **params)
    rows, width = keep.shape[0], keep.shape[1]
    rgba = np.empty((rows, width, 4), np.float32)
    px = np.empty((rows, width), np.uint32)
    info = N.ExposureInfo()
    if state is None:
        state = N.ExposureState()
    L = N.lib()
    if L.cgpth_tonemap(C.byref(p), C.byref(state), rgba.ctypes.data_as(C.POINTER(C.c_float)), rgba.size, px.ctypes.data_as(C.POINTER(C.c_uint32)),
                       px.size, C.byref(info)) != 0:
        raise HostError(L.cgpth_last_error().decode())
    return rgba, px, (info if p.flags & N.TONEMAP_AUTO_EXPOSURE else None)
