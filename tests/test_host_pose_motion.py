"""CGPT_TEMPORAL_FOLLOW_POSES as the header, the binding and the Python surface declare it.  No GPU."""
import inspect
import os

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from cpugpupathtracing_amd import build as B


def test_header_declares_the_flag_and_the_library_exports_the_read_back():
    with open(os.path.join(B.REPO_DIR, "include", "cpugpupt_abi.h")) as f:
        header = f.read()
    assert "CGPT_TEMPORAL_FOLLOW_POSES = 16u" in header and N.TEMPORAL_FOLLOW_POSES == 16
    assert "CGPT_TEMPORAL_KEEP_VIEW_DEPENDENT = 1u" in header and "CGPT_TEMPORAL_FOLLOW_TRANSFORMS = 4u" in header   # the ABI only grows
    assert "int cgpt_read_previous_hits(cgpt_ctx* ctx, float* dst, size_t n_floats);" in header
    assert "#define CGPT_ABI_VERSION 2u" in header
    assert hasattr(N.lib(), "cgpt_read_previous_hits")
    assert N.TEMPORAL_FOLLOW_POSES & (N.TEMPORAL_KEEP_VIEW_DEPENDENT | N.TEMPORAL_FOLLOW_TRANSFORMS | 2 | 8) == 0


def test_python_defaults():
    params = list(inspect.signature(P.Renderer.denoise_temporal).parameters.values())
    assert params[-1].name == "follow_poses" and params[-1].default is False       # appended last
    assert params[-2].name == "follow_transforms" and params[-2].default is False
    assert callable(P.Renderer.previous_hits)
    assert "follow_poses" not in inspect.signature(P.Renderer.denoise_variance_guided).parameters   # that keyword set is pinned; the ABI takes the flag
