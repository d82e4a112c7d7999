"""BUILD_SAH_BINNED restated in numpy float32, independent of the C++ (csrc/host/mesh_bvh.cpp: BuildTreeBinned) and of the HIP build.

Per node: centroid bounds -> 16 bins per axis with a positive extent; per bin a count, the union of the triangles' boxes and the bounds of
their centroids; candidates axis-outer, s = 1..15 inner (left = bins [0, s)), empty sides skipped, the reference's cost and leaf test,
first strictly cheaper wins; stable partition; children's bounds from the bins.  Every min / max is taken under the total order in which
-0 < +0 (the sign-flip map to uint32), so no result depends on the order of the fold."""
import numpy as np

F = np.float32


def key(f):
    u = np.ascontiguousarray(f, F).view(np.uint32)
    return u ^ np.where(u >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkey(k):
    k = np.asarray(k, np.uint32)
    return (k ^ np.where(k >> 31, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(F)


def tmin(a):
    return unkey(key(a).min(axis=0))


def tmax(a):
    return unkey(key(a).max(axis=0))


def half_area(lo, hi):
    e = hi.astype(F) - lo.astype(F)
    return F(F(e[0] * e[1]) + F(e[1] * e[2])) + F(e[2] * e[0])


def prepare(pos):
    """pos: [n, 3, 3] float32 -> per-triangle box lo, hi and centroid ((p0 + p1) + p2) * 0.3333f.  A triangle's own box is the mirror's
    cached one: std::min / std::max over v0, v1, v2 in that order (a tie, -0 against +0 included, keeps the earlier vertex)."""
    pos = np.asarray(pos, F)
    p0, p1, p2 = pos[:, 0], pos[:, 1], pos[:, 2]
    std_min = lambda a, b: np.where(b < a, b, a)
    std_max = lambda a, b: np.where(a < b, b, a)
    return std_min(std_min(p0, p1), p2), std_max(std_max(p0, p1), p2), ((p0 + p1) + p2) * F(0.3333)


def bin_of(c, lo, scale):
    with np.errstate(all="ignore"):
        f = (c - lo) * scale
    return np.where(f < F(16), np.where(f < F(16), f, F(0)).astype(np.uint32), np.uint32(15))


def build(pos, order=None):
    """-> nodes [n_nodes, 8] uint32 words (aabb_min, left_first, aabb_max, prim_count), tri_indices [n], max_depth"""
    lo, hi, cen = prepare(pos)
    n_all = lo.shape[0]
    idx = np.arange(n_all, dtype=np.uint32) if order is None else np.array(order, np.uint32)
    nodes = []          # [lo, hi, left_first, prim_count]
    nodes.append([tmin(lo[idx]), tmax(hi[idx]), 0, n_all])
    todo = [(0, 0, tmin(cen[idx]), tmax(cen[idx]))]
    max_depth = 0
    while todo:
        node, depth, cmin, cmax = todo.pop()
        max_depth = max(max_depth, depth)
        nlo, nhi, first, n = nodes[node]
        tris = idx[first:first + n]
        best = None
        with np.errstate(all="ignore"):
            for a in range(3):
                if not cmax[a] > cmin[a]:
                    continue
                scale = F(16) / F(cmax[a] - cmin[a])
                b = bin_of(cen[tris, a], cmin[a], scale)
                count = np.cumsum(np.bincount(b, minlength=16))               # count[s - 1]: triangles in bins [0, s)
                klo = np.full((16, 3), 0xFFFFFFFF, np.uint32)
                khi = np.zeros((16, 3), np.uint32)
                np.minimum.at(klo, b, key(lo[tris]))                          # per-bin box, as keys (an empty bin: the identity)
                np.maximum.at(khi, b, key(hi[tris]))
                left_lo, left_hi = np.minimum.accumulate(klo, axis=0), np.maximum.accumulate(khi, axis=0)                  # bins [0, b]
                right_lo, right_hi = np.minimum.accumulate(klo[::-1], axis=0)[::-1], np.maximum.accumulate(khi[::-1], axis=0)[::-1]  # bins [b, 16)
                for s in range(1, 16):
                    lc, rc = int(count[s - 1]), n - int(count[s - 1])
                    if lc == 0 or rc == 0:
                        continue
                    cost = F(F(lc) * half_area(unkey(left_lo[s - 1]), unkey(left_hi[s - 1]))) + F(F(rc) * half_area(unkey(right_lo[s]), unkey(right_hi[s])))
                    if best is None or cost < best[0]:
                        best = (cost, b < s)
            if best is None or not best[0] < F(half_area(nlo, nhi) * F(n)):
                continue
        L, R = tris[best[1]], tris[~best[1]]                             # the children's bounds below are folded from the triangles, not the bins
        idx[first:first + n] = np.concatenate([L, R])                   # boolean masks keep the order: a stable partition
        left = len(nodes)
        nodes.append([tmin(lo[L]), tmax(hi[L]), first, L.size])
        nodes.append([tmin(lo[R]), tmax(hi[R]), first + L.size, R.size])
        nodes[node][2], nodes[node][3] = left, 0
        todo.append((left + 1, depth + 1, tmin(cen[R]), tmax(cen[R])))  # the left subtree is numbered first
        todo.append((left, depth + 1, tmin(cen[L]), tmax(cen[L])))
    words = np.zeros((len(nodes), 8), np.uint32)
    for i, (nlo, nhi, lf, pc) in enumerate(nodes):
        words[i, 0:3] = np.asarray(nlo, F).view(np.uint32)
        words[i, 3] = lf
        words[i, 4:7] = np.asarray(nhi, F).view(np.uint32)
        words[i, 7] = pc
    return words, idx, max_depth


def sah_cost(words):
    """(sum of inner-node half areas + sum of leaf half area x count) / the root's half area, in float64"""
    w = np.asarray(words).view(np.uint32).reshape(-1, 8)
    lo, hi = w[:, 0:3].copy().view(F).astype(np.float64), w[:, 4:7].copy().view(F).astype(np.float64)
    e = hi - lo
    area = e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0]
    count = w[:, 7].astype(np.float64)
    return float((area * np.where(count > 0, count, 1.0)).sum() / area[0])
