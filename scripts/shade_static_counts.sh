#!/bin/bash
# Here (no GPU needed): static instruction counts of every kernel of one device source, from the gfx950 assembly that the flags of
# kernel_resource_usage.sh give.  Per kernel body: vector-ALU instructions, lane moves (v_readlane_b32 + v_writelane_b32: on this
# architecture a spilled scalar register lives in a VGPR lane and every spill or reload is one of them), v_mov_b32, scalar-ALU
# instructions, vector-memory instructions and IEEE divisions (one v_div_fixup each).  Static: what the body holds, not what a wave runs.
# usage: bash scripts/shade_static_counts.sh cpugpupathtracing_amd/csrc/device/<file>.hip [kernel-name filter] [extra hipcc flags]
F=$1; shift
FILTER=""
case "$1" in -*|"") ;; *) FILTER=$1; shift ;; esac
R=$(cd "$(dirname "$0")/.." && pwd)
ASM=$(mktemp)
/opt/rocm/bin/hipcc -O3 -std=c++17 -ffp-contract=off -fPIC -I$R/include -I$R/cpugpupathtracing_amd/csrc/host -I$R/cpugpupathtracing_amd/csrc/device --offload-arch=gfx950 -fno-slp-vectorize "$@" -S --cuda-device-only $F -o "$ASM" || { echo "shade_static_counts.sh: hipcc failed on $F" >&2; rm -f "$ASM"; exit 1; }
c++filt < "$ASM" | python3 -c "
import re, sys
flt = sys.argv[1]
cur = None; rows = []
for l in sys.stdin:
    head = l.split(' ; @')[0].rstrip()
    if l[0] not in ' \t.;#\n' and head.endswith(':'):                      # a symbol: a kernel's body runs from here to its s_endpgm
        name = head[:-1]
        if name.startswith('void '): name = name[5:]
        cur = [name.split('(')[0].replace(', ', ','), 0, 0, 0, 0, 0, 0]; continue
    if cur is None: continue
    s = l.strip()
    if not s or s[0] in ';.' or s.endswith(':'): continue
    op = s.split()[0]
    if op.startswith('v_'):
        cur[1] += 1
        if op in ('v_readlane_b32', 'v_writelane_b32'): cur[2] += 1
        if op.startswith('v_mov_b32'): cur[3] += 1
        if op.startswith('v_div_fixup'): cur[6] += 1
    elif op.startswith('s_') and not re.match(r's_(load|buffer_load|waitcnt|nop|branch|cbranch|endpgm|barrier|sleep|setprio|setpc|swappc|getpc|sendmsg|code_end|inst_prefetch|clause|ttrace)', op): cur[4] += 1
    elif re.match(r'(global|flat|buffer|scratch)_', op): cur[5] += 1
    if op == 's_endpgm':
        rows.append(cur); cur = None
print('kernel'.ljust(64), 'VALU'.rjust(6), 'lane_mv'.rjust(7), 'v_mov'.rjust(6), 'SALU'.rjust(6), 'VMEM'.rjust(6), 'div'.rjust(4))
for r in rows:
    if flt in r[0]: print(r[0][:64].ljust(64), *(str(x).rjust(w) for x, w in zip(r[1:], (6, 7, 6, 6, 6, 4))))
" "$FILTER"
rm -f "$ASM"
