#!/usr/bin/env python3
"""Kernel by kernel: does one device source compile to the instruction streams it had at PARENT (default HEAD)?  For a change that adds
kernels to a unit and means to leave the others alone (scripts/device_asm_identical.sh compares whole units).  No GPU needed.
  python3 scripts/kernel_streams_identical.py cpugpupathtracing_amd/csrc/device/<file>.hip [PARENT] > profiles/rNN/<file>_kernels_identical.txt
Both versions are compiled with the flags of build.py plus --offload-device-only -S.  Of every kernel the instructions are compared:
comments, directives and the numbering of local labels are dropped, and a template argument that a kernel gained with its default value
(<..., false>) is dropped from its mangled name.  Exit status 1 if a kernel of the parent is missing or differs."""
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cpugpupathtracing_amd.build import COMMON_FLAGS, DEVICE_FLAGS, HIPCC

src = sys.argv[1]
parent = sys.argv[2] if len(sys.argv) > 2 else "HEAD"


def kernels(path, include_root):
    flags = [f.replace(REPO, include_root) if f.startswith("-I") else f for f in COMMON_FLAGS + DEVICE_FLAGS]
    asm = subprocess.run([HIPCC] + flags + ["--offload-device-only", "-S", path, "-o", "-"], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur is not None:
            if line.strip().startswith(".Lfunc_end"):
                cur = None
                continue
            t = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].rstrip())
            if t.strip() and not t.strip().startswith("."):
                out[cur].append(t)
    return out


with tempfile.TemporaryDirectory() as tmp:
    subprocess.run(f"git -C {REPO} archive {parent} cpugpupathtracing_amd/csrc include | tar -x -C {tmp}", shell=True, check=True)
    before = kernels(os.path.join(tmp, os.path.relpath(os.path.abspath(src), REPO)), tmp)
after = kernels(os.path.abspath(src), REPO)
by_old_name = {re.sub(r"(I(?:Lb[01]E)+)Lb0EE", r"\1E", k): k for k in after}
by_old_name.update({k: k for k in after})
status = 0
for name, stream in before.items():
    now = after.get(by_old_name.get(name, ""))
    verdict = "identical" if now == stream else ("MISSING" if now is None else "DIFFERS")
    status |= verdict != "identical"
    print(f"{name[:72]:72s} {len(stream):5d} instructions  {verdict}")
for name in after:
    if name not in before.keys() and name not in (by_old_name.get(b) for b in before):
        print(f"{name[:72]:72s} {len(after[name]):5d} instructions  new")
sys.exit(status)
