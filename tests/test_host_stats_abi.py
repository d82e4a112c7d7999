"""cgpt_stats in include/cpugpupt_abi.h against its ctypes mirror (_native.Stats): the same fields in the same order, every offset and
the size as the C compiler lays the struct out (natural alignment), and the new 64-bit probe_resolved appended after chain_followers,
so a library and a binding of different ages disagree only about the tail.  No GPU needed."""
import ctypes as C
import os
import re

from cpugpupathtracing_amd import _native as N

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"uint64_t": (8, C.c_uint64), "uint32_t": (4, C.c_uint32), "double": (8, C.c_double)}


def _header_fields():
    """[(name, C type, array length or 0)] of struct cgpt_stats, in declaration order"""
    text = open(os.path.join(REPO, "include", "cpugpupt_abi.h")).read()
    body = re.search(r"typedef struct cgpt_stats \{(.*?)\} cgpt_stats;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        assert ctype in C_TYPES, decl
        for name in names.split(","):
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", name.strip())
            assert m, decl
            fields.append((m.group(1), ctype, int(m.group(2) or 0)))
    return fields


def test_stats_mirror_matches_the_header():
    fields = _header_fields()
    assert [f[0] for f in fields] == [f[0] for f in N.Stats._fields_]
    offset, align = 0, 1
    for (name, ctype, count), (_, mirror) in zip(fields, N.Stats._fields_):
        size, want = C_TYPES[ctype]
        assert mirror == (want * count if count else want), name
        offset = (offset + size - 1) // size * size                # natural alignment of the element type
        align = max(align, size)
        assert getattr(N.Stats, name).offset == offset, (name, getattr(N.Stats, name).offset, offset)
        assert getattr(N.Stats, name).size == size * max(1, count), name
        offset += size * max(1, count)
    assert C.sizeof(N.Stats) == (offset + align - 1) // align * align


def test_probe_resolved_is_appended_as_64_bits():
    names = [f[0] for f in N.Stats._fields_]
    assert names[-2:] == ["chain_followers", "probe_resolved"]
    assert N.Stats.probe_resolved.size == 8
    assert N.Stats.probe_resolved.offset == N.Stats.chain_followers.offset + 4     # no padding: the pair before it fills 8 bytes
    assert C.sizeof(N.Stats) == N.Stats.probe_resolved.offset + 8
    s = N.Stats()
    s.probe_resolved = 7_000_000_000                                                  # a 20-step bench run: past 32 bits
    assert s.probe_resolved == 7_000_000_000
