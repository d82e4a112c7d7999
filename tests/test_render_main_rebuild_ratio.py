"""examples/render_main.cpp --rebuild-ratio R: the option is parsed, and a ratio the device call would refuse is refused, before a
context exists -- so this much runs without a GPU.  What the option does on the device is in tests/test_gpu_rebuild_degraded.py
(test_the_example_rebuilds_only_where_the_call_says_so: --rebuild-ratio 1e9 prints no rebuild line)."""
import os
import subprocess

from cpugpupathtracing_amd import build as B


def test_a_ratio_that_is_not_finite_and_positive_is_refused_before_the_device_is_touched(tmp_path):
    exe = str(tmp_path / "render_main")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(B.REPO_DIR, "include"), "-I" + os.path.join(B.CSRC, "host"),
                           os.path.join(B.REPO_DIR, "examples", "render_main.cpp"), "-L" + B.LIB_DIR, "-lcpugpupt", "-Wl,-rpath," + B.LIB_DIR, "-o", exe])
    for ratio in ("0", "-2", "nan", "inf", "many"):
        out = subprocess.run([exe, "--bend", "15", "--rebuild-ratio", ratio, "64", "48", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "--rebuild-ratio needs a finite ratio > 0" in out.stderr, (ratio, out.returncode, out.stderr)
        assert "rebuilt" not in out.stdout
    out = subprocess.run([exe, "--rebuild-ratio"], cwd=tmp_path, capture_output=True, text=True, timeout=60)   # no value: not an option
    assert out.returncode == 2 and "unknown option" in out.stderr
