"""The surface of the variance-guided filter: the C ABI's new symbols cgpt_denoise_variance_guided and cgpt_read_variance,
the struct cgpt_variance_params, their ctypes counterparts and the Renderer's methods.  No GPU needed: nothing here creates a context."""
import ctypes as C
import inspect
import os
import re

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _fp, _up = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)


def header():
    with open(os.path.join(REPO, "include", "cpugpupt_abi.h")) as f:
        return f.read()


def test_header_declares_and_library_exports_both_calls():
    abi = header()
    assert re.search(r"int cgpt_denoise_variance_guided\(cgpt_ctx\* ctx, const cgpt_camera\* camera, const cgpt_denoise_params\* params,\s*"
                     r"const cgpt_temporal_params\* temporal, const cgpt_variance_params\* variance,\s*"
                     r"float\* dst_rgba, size_t n_floats, uint32_t\* dst_pixels, size_t n_pixels\);", abi)
    assert re.search(r"int cgpt_read_variance\(cgpt_ctx\* ctx, float\* dst, size_t n_floats\);", abi)
    L = N.lib()
    assert hasattr(L, "cgpt_denoise_variance_guided") and hasattr(L, "cgpt_read_variance")


def test_prototypes_are_registered():
    want = {"cgpt_denoise_variance_guided": [_vp, C.POINTER(N.Camera), C.POINTER(N.DenoiseParams), C.POINTER(N.TemporalParams),
                                             C.POINTER(N.VarianceParams), _fp, C.c_size_t, _up, C.c_size_t],
            "cgpt_read_variance": [_vp, _fp, C.c_size_t]}
    for name, argtypes in want.items():
        restype, got = N.PROTOTYPES[name]
        assert restype is C.c_int and got == argtypes, name
        assert getattr(N.lib(), name).argtypes == argtypes and getattr(N.lib(), name).restype is C.c_int


def test_struct_layout_and_flag():
    abi = header()
    body = re.search(r"typedef struct cgpt_variance_params \{(.*?)\} cgpt_variance_params;", abi, re.S).group(1)
    assert re.findall(r"(float|uint32_t)\s+(\w+);", body) == [("float", "sigma_luminance"), ("uint32_t", "min_history_frames"), ("uint32_t", "flags")]
    assert C.sizeof(N.VarianceParams) == 12
    assert [(f[0], getattr(N.VarianceParams, f[0]).offset) for f in N.VarianceParams._fields_] == \
        [("sigma_luminance", 0), ("min_history_frames", 4), ("flags", 8)]
    assert N.VarianceParams._fields_[0][1] is C.c_float and N.VarianceParams._fields_[1][1] is C.c_uint32
    assert "CGPT_VARIANCE_TEMPORAL = 1u" in abi and N.VARIANCE_TEMPORAL == 1
    assert "the defaults: 4.0, 4, 0" in abi


def test_abi_version_and_older_layouts_are_unchanged():
    abi = header()
    assert "#define CGPT_ABI_VERSION 2u" in abi and N.lib().cgpt_abi_version() == 2
    assert re.search(r"added\s+new\s+symbols\s+\(cgpt_denoise_variance_guided,\s+cgpt_read_variance\)", abi)
    assert (C.sizeof(N.DenoiseParams), C.sizeof(N.TemporalParams)) == (20, 16)   # the feature has a struct of its own
    for struct in ("cgpt_denoise_params", "cgpt_temporal_params"):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", abi, re.S)
        assert body and "luminance" not in body.group(1), struct


def test_null_context_is_refused_without_a_device():
    L = N.lib()
    cam = N.Camera()
    buf = (C.c_float * 4)()
    assert L.cgpt_denoise_variance_guided(None, C.byref(cam), None, None, None, buf, 4, None, 0) == N.CGPT_ERR_INVALID
    assert L.cgpt_read_variance(None, buf, 4) == N.CGPT_ERR_INVALID


def test_renderer_has_the_methods_with_the_documented_defaults():
    sig = inspect.signature(P.Renderer.denoise_variance_guided)
    defaults = {k: p.default for k, p in sig.parameters.items() if k != "self"}
    assert list(defaults)[:8] == ["iterations", "sigma_luminance", "sigma_normal", "sigma_position", "demodulate", "temporal",
                                  "min_history_frames", "camera"]
    assert defaults == dict(iterations=5, sigma_luminance=4.0, sigma_normal=0.2, sigma_position=0.3, demodulate=True, temporal=False,
                            min_history_frames=4, camera=None, max_history=64.0, normal_cos_min=0.9, plane_tolerance=0.01,
                            keep_view_dependent=False)
    temporal = inspect.signature(P.Renderer.denoise_temporal).parameters
    for k in ("max_history", "normal_cos_min", "plane_tolerance", "keep_view_dependent"):   # denoise_temporal's keywords and defaults
        assert defaults[k] == temporal[k].default
    assert callable(getattr(P.Renderer, "variance"))
