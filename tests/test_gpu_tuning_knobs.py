"""The tuning-knob surface of cgpt_set_tuning and the CGPT_* environment: every knob's name and range, the error messages,
the routing (pt_* knobs, then the wavefront table) and the clamping of environment values."""
import json
import os
import subprocess
import sys

import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (lo, hi); environment CGPT_<NAME>
PT_KNOBS = {
    "pt_budget_gib": (1, 256), "pt_max_paths_mi": (1, 2047), "pt_refill": (1, 64), "pt_inner_repeat": (1, 65),
    "pt_leaf_repeat": (1, 65), "pt_obj_shift": (0, 6), "pt_shade_shift": (0, 6), "pt_top_records": (0, 4096),
    "pt_blocks": (1, 64), "pt_streams": (1, 2), "pt_path_order": (0, 2), "pt_lds_tris": (0, 1), "pt_tail_lanes": (0, 64),
    "pt_tail_samples": (0, 4096), "pt_chunk": (0, 4096), "pt_fine_rounds": (0, 1024),
}
# name: (lo, hi); environment CGPT_WF_<NAME>
WF_KNOBS = {
    "pools": (1, 8), "batch": (0, 4096), "max_batch": (1, 4096), "pool_paths_mi": (1, 1024), "budget_gib": (1, 256),
    "refill": (1, 64), "leaf_repeat": (1, 65), "inner_repeat": (1, 65), "obj_repeat": (1, 65), "obj_shift": (0, 6),
    "top_records": (0, 4096), "trace_blocks": (1, 64), "shade_chunk": (1, 256), "shade_chunk_banded": (1, 256),
    "shadow_any_hit": (0, 1), "trace_events": (0, 1), "path_order": (0, 2),
    "retire_misses": (0, 1), "lds_tris": (0, 1), "first_lean": (0, 1), "bands": (1, 128), "bands_min_paths": (0, 0x7FFFFFFF),
    "spec_dedupe": (0, 1), "spec_keys": (1, 16), "spec_epochs": (1, 0xFFFF),
}


@pytest.fixture(scope="module")
def renderer():
    r = P.Renderer(0)
    yield r
    r.close()


def _rejects(r, name, value, message):
    with pytest.raises(P.DeviceError) as e:
        r.set_tuning(**{name: value})
    assert e.value.code == N.CGPT_ERR_INVALID
    assert str(e.value) == f"[cgpt status {N.CGPT_ERR_INVALID}] {message}"


@pytest.mark.parametrize("name", sorted(PT_KNOBS) + sorted(WF_KNOBS))
def test_knob_range(renderer, name):
    lo, hi = PT_KNOBS.get(name) or WF_KNOBS[name]
    renderer.set_tuning(**{name: lo})
    renderer.set_tuning(**{name: hi})
    _rejects(renderer, name, hi + 1, f"tuning knob {name}: {hi + 1} outside [{lo}, {hi}]")
    if lo > 0:
        _rejects(renderer, name, lo - 1, f"tuning knob {name}: {lo - 1} outside [{lo}, {hi}]")


@pytest.mark.parametrize("name", ["no_such_knob", "pt_no_such_knob", "band_rows", "sort", "trace_chunk"])
def test_unknown_knob(renderer, name):
    """band_rows is a knob of multi-device contexts only; sort and trace_chunk were removed"""
    _rejects(renderer, name, 1, f"unknown tuning knob '{name}'")


_CHILD = r"""
import json, sys
sys.path.insert(0, {repo!r})
import cpugpupathtracing_amd as P
r = P.Renderer(0)
r.upload(P.Scene.reference_layout(P.Mesh.dragon_standin(2), 3, 1.0, P.BUILD_SAH_INTERVALS))
knobs = {knobs!r}
if knobs:
    r.set_tuning(**knobs)
out = []
for k in (P.KERNEL_PERSISTENT, P.KERNEL_WAVEFRONT):
    r.render(32, 32, 2, kernel=k)
    out.append(r.stats().dominant_waves_per_simd)
print(json.dumps(out))
"""


def _waves(env, knobs):
    e = {k: v for k, v in os.environ.items() if not k.startswith("CGPT_")}
    e.update(env)
    p = subprocess.run([sys.executable, "-c", _CHILD.format(repo=REPO, knobs=knobs)], capture_output=True, text=True, timeout=300, env=e)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_environment_matches_set_tuning():
    """CGPT_PT_* / CGPT_WF_* values are read when the context first needs the launcher's state, clamped into the knob's range,
    and act as set_tuning of the same values would"""
    default = _waves({}, {})
    want = _waves({}, {"pt_blocks": 1, "trace_blocks": 2})
    assert want != default                                       # the knobs bind at the default occupancy
    assert _waves({"CGPT_PT_BLOCKS": "1", "CGPT_WF_TRACE_BLOCKS": "2"}, {}) == want
    clamped = _waves({}, {"pt_blocks": 1, "trace_blocks": 1})
    assert _waves({"CGPT_PT_BLOCKS": "0", "CGPT_WF_TRACE_BLOCKS": "-5"}, {}) == clamped
