"""The surface of resampled light sampling: the C ABI's new symbol cgpt_set_nee_candidates, its ctypes prototype and the
Renderer's method and property.  No GPU needed: nothing here creates a context."""
import os
import re

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES_AT_ABI_2 = (24, 48, 192)      # bytes of cgpt_settings, cgpt_render_params, cgpt_stats


def test_header_declares_and_library_exports_the_call():
    abi = open(os.path.join(REPO, "include", "cpugpupt_abi.h")).read()
    assert re.search(r"int cgpt_set_nee_candidates\(cgpt_ctx\* ctx, uint32_t candidates\);", abi)
    L = N.lib()
    assert hasattr(L, "cgpt_set_nee_candidates")


def test_prototype_is_registered():
    import ctypes as C
    restype, argtypes = N.PROTOTYPES["cgpt_set_nee_candidates"]
    assert restype is C.c_int and argtypes == [C.c_void_p, C.c_uint32]
    assert N.lib().cgpt_set_nee_candidates.argtypes == argtypes


def test_abi_version_and_layouts_are_unchanged():
    import ctypes as C
    abi = open(os.path.join(REPO, "include", "cpugpupt_abi.h")).read()
    assert "#define CGPT_ABI_VERSION 2u" in abi and re.search(r"one\s+new\s+symbol\s+only\s*\(\s*cgpt_set_nee_candidates\s*\)", abi)
    assert N.lib().cgpt_abi_version() == 2
    # the value is context state: no public struct grew to carry it
    assert (C.sizeof(N.Settings), C.sizeof(N.RenderParams), C.sizeof(N.Stats)) == SIZES_AT_ABI_2
    for struct in ("cgpt_settings", "cgpt_render_params", "cgpt_stats"):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", abi, re.S)
        assert body and "candidates" not in body.group(1), struct


def test_null_context_is_refused():
    assert N.lib().cgpt_set_nee_candidates(None, 4) == N.CGPT_ERR_INVALID


def test_renderer_has_the_method_and_the_read_only_property():
    assert callable(getattr(P.Renderer, "set_nee_candidates"))
    prop = getattr(P.Renderer, "nee_candidates")
    assert isinstance(prop, property) and prop.fset is None
