"""The bookkeeping of cgpt_scene_rebuild_mesh restated in numpy from csrc/device/rebuild_layout.h's header comment (not from its code):
where the records of a rebuilt tree go in an installed layout.  Shared by tests/test_host_rebuild_layout.py and tests/test_gpu_rebuild_mesh.py.

A layout's bookkeeping is kept here as a Book: per object root_code, kind, tri_count, node_count, leaf_base, pair_base, level_begin,
level_offsets, span_base and mesh_group, and for the scene record_perm, n_top_records, n_pair_records, n_refit_levels.
"""
import numpy as np

LEAF_BIT = 0x80000000
NO_SPAN = 0xFFFFFFFF
MESH = 0
STACK = 64
RECORD_LIMIT = 1 << 26
INVALID, UNSUPPORTED = 1, 4                                    # cgpt_status


class Refused(Exception):
    def __init__(self, status, text):
        super().__init__(text)
        self.status, self.text = status, text


class Book:
    def __init__(self, lay, raw, mesh_group=None):
        """from tests/test_host_scene_layout.py's Layout and Raw of one scene"""
        n = len(lay.objects)
        self.kind = [o.kind for o in lay.objects]
        self.root_code = [o.root_code for o in lay.objects]
        self.tri_count = [max(o.n_tris, 0) for o in lay.objects]
        self.node_count = [raw.objects[i].node_count if self.kind[i] == MESH else 0 for i in range(n)]
        self.leaf_base = [int(x) for x in lay.leaf_base]
        self.pair_base = [int(x) for x in lay.pair_base]
        self.level_begin = [int(x) for x in lay.level_begin]
        self.level_offsets = [[int(x) for x in lo] for lo in lay.level_offsets]
        self.span_base = [NO_SPAN] * n
        self.mesh_group = list(range(n)) if mesh_group is None else list(mesh_group)
        self.record_perm = [int(x) for x in lay.record_perm]
        self.n_top_records, self.n_pair_records, self.n_refit_levels = lay.n_top_records, lay.n_pair_records, len(lay.refit_levels)
        self.stack_depth = lay.stack_depth


def record_levels(offsets):
    return max(0, len(offsets) - 1)


def top_slots(book, obj):
    """the names below n_top_records the mesh owns, ascending"""
    pb, pairs = book.pair_base[obj], book.node_count[obj] // 2
    return sorted(r for r in book.record_perm[pb:pb + pairs] if r < book.n_top_records)


def rebuild(book, obj, level_first, top_ranks, assume_pair_records=0):
    """Applies one rebuild to the book and returns what the plan shows: dict(members, top_slots, level_offsets, names, span_base,
    level_begin, pair_base, n_nodes, n_pairs, max_depth, grow, n_pair_records, n_refit_levels, stack_depth).  Raises Refused."""
    level_first = [int(x) for x in level_first]
    n_tris = book.tri_count[obj]
    n_nodes, node_levels = level_first[-1], len(level_first) - 1
    n_pairs, max_depth = n_nodes // 2, node_levels - 1
    if max_depth + 1 > STACK:
        raise Refused(UNSUPPORTED, "exceeds the traversal stack of 64")
    members = [j for j in range(len(book.kind)) if book.mesh_group[j] == book.mesh_group[obj]]
    slots = top_slots(book, obj)
    n_pair_records = assume_pair_records or book.n_pair_records
    room = n_tris - 1
    grow = book.span_base[obj] == NO_SPAN
    if grow:
        if n_pair_records + room >= RECORD_LIMIT:
            raise Refused(INVALID, "scene too large")
        span_base, level_begin, pair_base = n_pair_records, book.n_refit_levels, len(book.record_perm)
        n_pair_records += room
        book.n_refit_levels += room
        book.record_perm += [0xFFFFFFFF] * room
    else:
        span_base, level_begin, pair_base = book.span_base[obj], book.level_begin[obj], book.pair_base[obj]
    book.n_pair_records = n_pair_records
    # the splitting nodes of level d are half the nodes of level d + 1
    offsets = [(level_first[d + 1] - 1) // 2 for d in range(node_levels)] if n_pairs else []
    names = [span_base + k for k in range(n_pairs)]
    used = min(len(slots), n_pairs)
    assert len(top_ranks) == used
    for slot, rank in zip(slots, top_ranks):
        names[int(rank)] = slot
    book.record_perm[pair_base:pair_base + n_pairs] = names
    root = names[0] if n_pairs else LEAF_BIT | book.leaf_base[obj]
    for j in members:
        book.root_code[j], book.node_count[j], book.span_base[j] = root, n_nodes, span_base
        book.level_begin[j], book.pair_base[j], book.level_offsets[j] = level_begin, pair_base, list(offsets)
    deepest = max(record_levels(book.level_offsets[j]) for j in range(len(book.kind)))
    book.stack_depth = deepest + 1
    return dict(members=members, top_slots=slots, level_offsets=offsets, names=names, span_base=span_base, level_begin=level_begin, pair_base=pair_base,
                n_nodes=n_nodes, n_pairs=n_pairs, max_depth=max_depth, grow=int(grow), n_pair_records=n_pair_records, n_refit_levels=book.n_refit_levels,
                stack_depth=book.stack_depth)


def complete_tree(n_levels):
    """level_first of a complete binary tree of n_levels node levels"""
    return [0] + [2 ** (l + 1) - 1 for l in range(n_levels)]


def chain_tree(n_levels):
    """level_first of a tree in which one node a level splits"""
    return [0] + [1 + 2 * l for l in range(n_levels)]
