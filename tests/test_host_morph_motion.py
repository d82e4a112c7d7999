"""CGPT_TEMPORAL_FOLLOW_MORPHS as the header, the binding and the Python surface declare it.  No GPU."""
import inspect
import os

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from cpugpupathtracing_amd import build as B


def test_header_declares_the_flag_and_keeps_the_older_ones():
    with open(os.path.join(B.REPO_DIR, "include", "cpugpupt_abi.h")) as f:
        header = f.read()
    assert "CGPT_TEMPORAL_FOLLOW_MORPHS = 32u" in header and N.TEMPORAL_FOLLOW_MORPHS == 32
    assert "#define CGPT_ABI_VERSION 2u" in header                              # a new enum value only
    for older in ("CGPT_TEMPORAL_KEEP_VIEW_DEPENDENT = 1u", "CGPT_TEMPORAL_FOLLOW_TRANSFORMS = 4u", "CGPT_TEMPORAL_FOLLOW_POSES = 16u"):
        assert older in header
    assert (N.TEMPORAL_KEEP_VIEW_DEPENDENT, N.TEMPORAL_FOLLOW_TRANSFORMS, N.TEMPORAL_FOLLOW_POSES) == (1, 4, 16)
    assert N.TEMPORAL_FOLLOW_MORPHS & (1 | 2 | 4 | 8 | 16) == 0
    assert "int cgpt_read_previous_hits(cgpt_ctx* ctx, float* dst, size_t n_floats);" in header   # the records keep their call and format


def test_python_surface():
    following = inspect.signature(P.Renderer.denoise_temporal_following).parameters
    assert [(k, following[k].default) for k in list(following)[-3:]] == [("transforms", False), ("poses", False), ("morphs", False)]
    temporal = inspect.signature(P.Renderer.denoise_temporal).parameters
    assert list(temporal)[-1] == "follow_poses" and temporal["follow_poses"].default is False      # that signature is pinned
    shared = [k for k in temporal if k not in ("follow_transforms", "follow_poses")]
    assert list(following)[:len(shared)] == shared                             # denoise_temporal's other keywords, in its order
    assert all(following[k].default == temporal[k].default for k in shared if k != "self")
    assert "morphs" not in inspect.signature(P.Renderer.denoise_variance_guided).parameters        # that keyword set is pinned; the ABI takes the flag
    assert callable(P.Renderer.previous_hits)
