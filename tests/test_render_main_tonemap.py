"""examples/render_main.cpp --tonemap / --srgb / --exposure / --adapt: the options are parsed, and values the device call
would refuse are refused, before a context exists -- so this much runs without a GPU.  What they do on the device is in
tests/test_gpu_tonemap.py (test_the_example_presents_through_the_stage)."""
import os
import subprocess

from cpugpupathtracing_amd import build as B


def build_example(tmp_path):
    exe = str(tmp_path / "render_main")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(B.REPO_DIR, "include"), "-I" + os.path.join(B.CSRC, "host"),
                           os.path.join(B.REPO_DIR, "examples", "render_main.cpp"), "-L" + B.LIB_DIR, "-lcpugpupt", "-Wl,-rpath," + B.LIB_DIR, "-o", exe])
    return exe


def test_bad_display_options_are_refused_before_the_device_is_touched(tmp_path):
    exe = build_example(tmp_path)
    for args, message in ((["--tonemap", "filmic"], "--tonemap needs clamp, reinhard, aces or hable"), (["--exposure", "bright"], "--exposure needs auto or an EV"),
                          (["--exposure", "65"], "--exposure needs auto or an EV"), (["--exposure", "nan"], "--exposure needs auto or an EV"),
                          (["--adapt", "1.5"], "--adapt needs an alpha in [0, 1]"), (["--adapt", "-0.1"], "--adapt needs an alpha in [0, 1]"),
                          (["--adapt", "nan"], "--adapt needs an alpha in [0, 1]")):
        out = subprocess.run([exe] + args + ["64", "48", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and message in out.stderr, (args, out.returncode, out.stderr)
    for args in (["--tonemap"], ["--exposure"], ["--adapt"]):                  # no value: not an option
        out = subprocess.run([exe] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "unknown option" in out.stderr
