#!/bin/sh
# Is the device code of every csrc/device/*.hip what it was at PARENT (default HEAD)?  For a change that means to touch host code only.
#   scripts/device_asm_identical.sh [PARENT] > profiles/rNN/device_asm_identical.txt
# Both trees are compiled with the flags of build.py plus --offload-device-only -S; the lines that hold __hip_cuid_ (a hash of the
# whole file, host lines included) are dropped.  Exit status 1 if any file differs.
set -e
cd "$(git rev-parse --show-toplevel)" && tmp=$(mktemp -d) && mkdir "$tmp/parent" "$tmp/asm" && status=0
git archive "${1:-HEAD}" cpugpupathtracing_amd/csrc include | tar -x -C "$tmp/parent"
flags=$(python3 -c "from cpugpupathtracing_amd.build import COMMON_FLAGS, DEVICE_FLAGS, REPO_DIR; print(' '.join(f.replace(REPO_DIR, '.') for f in COMMON_FLAGS + DEVICE_FLAGS))")
for f in cpugpupathtracing_amd/csrc/device/*.hip; do
    for tree in . "$tmp/parent"; do
        (cd "$tree" && "${HIPCC:-/opt/rocm/bin/hipcc}" $flags --offload-device-only -S "$f" -o - | grep -v __hip_cuid_ > "$tmp/asm/$(basename "$f").$(basename "$tree")") &
    done
done
wait
for f in cpugpupathtracing_amd/csrc/device/*.hip; do
    b=$tmp/asm/$(basename "$f")
    if [ -s "$b.." ] && cmp -s "$b.." "$b.parent"; then echo "$f identical"; else echo "$f DIFFERS"; status=1; fi
done
rm -rf "$tmp"
exit $status
