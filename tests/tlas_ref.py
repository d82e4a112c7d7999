"""The top-level tree over the scene's objects (cgpt_set_top_level, scene_layout.h: LayoutTopLevel, rt_device.hpp: intersect_scene<.., TREE>,
trace_steps.hpp: object_step<.., TREE>) restated in numpy.  This file is the specification: the host builds these boxes
and this tree, the device walks it this way.

Boxes, in world space, 6 floats {lo.xyz, hi.xyz}, float32:
    mesh               the bounds of its root node; a leaf root or a stand-alone triangle: min / max of its vertex positions; after a refit
                       the min / max of the new vertex positions
    transformed object the 8 corners of that box under world = A p + b, each row ((a0 x + a1 y) + a2 z) + b in float64 from the float32
                       entries, min / max over the corners, lo rounded down and hi rounded up to float32
    sphere             centre - radius, centre + radius (float32 operations)
    plane              (-inf, +inf) on every axis; so is an object with a bound that is not finite
Every leaf box is then padded outward (PAD; the walk widens every box once more for the ray it tests: FAR_PAD), per axis: pad = PAD * max(|lo|, |hi|, hi - lo) in float32, lo' = nextafter(lo - pad, -inf),
hi' = nextafter(hi + pad, +inf); a result that is not finite makes the box unbounded.

PAD.  For an untransformed mesh with an inner root the skip is exact without any padding (the child boxes are subsets of the root box and
the slab arithmetic is monotone).  A leaf-rooted mesh, a triangle, a sphere and a transformed object are tested by arithmetic that no box
bounds: Moeller-Trumbore accepts u, v within rounding of the edges, the sphere test compares d2 = L.L - tca^2 with r^2 after a cancellation
whose absolute error grows with |L|^2, a transformed mesh is walked with a rounded (o', d').  The first proposal was 1e-5; measured on the 40
objects and 4352 rays of test_tlas_reference.py it gives zero differing rays (so does no padding at all, on these rays), and 1e-4 is what
is built: ten times the proposal, i.e. about a thousand float32 ulps of the box's largest coordinate, which covers a sphere grazed from about thirty radii away
(error of d2 about 4 |L|^2 2^-24, half of that over r as a lateral distance).

FAR_PAD.  No fixed padding bounds those errors for every ray: they grow with the distance of the ray's origin.  A path that lands on an
infinite ground plane 10^4 to 10^6 units out sends its shadow ray at the lamp from there, and the list walk's sphere test, whose d2 carries
an error of about 13 |L|^2 2^-24 (L.L, tca^2 with a direction normalised in float32, the subtraction), then reports hits on spheres the ray
passes up to sqrt(13) 2^-12 |L| = 2^-10.2 |L| from -- a hundred units at 10^5.  So the node test widens the box for the ray it tests: with
a = lo - o, b = hi - o (float32, the slab test's own first step), far = FAR_PAD * max(|a.x|, |a.y|, |a.z|, |b.x|, |b.y|, |b.z|), the slab
test runs on a - far and b + far.  The box holds the sphere's centre, so |L| <= sqrt(3) * that maximum and far >= 2^-8.8 |L|: 2.6 times the
bound above, and the widened box holds the ball of radius r + far around the centre, hence the whole chord the sphere test can report.
Moeller-Trumbore and a transformed ray err by a few 2^-24 |L|, far inside that.  The maximum grows from a child's box to its parent's, so a
widened parent still holds its widened children.  Seen from the origin the pad is an angle of 2^-8 rad (0.22 degrees): it costs the tree
next to nothing.  far_rays() are such shadow rays: the list walk reports a sphere other than the lamp on more than half of them, and
without FAR_PAD the tree walk skips those spheres.

Tree.  Balanced over the object index ranges: the root covers [0, n); a node over [i, j) with j - i > 1 has the children [i, m) and [m, j),
m = i + (j - i + 1) // 2; a leaf is one object.  2 n - 1 nodes in depth-first preorder, left child first.  A node is 8 words,
{lo.xyz, skip | hi.xyz, object}: skip = the first node behind the node's subtree, object = the leaf's object index or INNER.  An inner
node's box is the union of its children's.  entry[j] = the highest node whose range starts at object j (the first such node in preorder),
entry[n] = 2 n - 1: a lane that comes back from object o resumes at entry[o + 1].

Walk.  In preorder, never reordered by distance.  At node k: unless the ray is axis-parallel (1 / d has an infinite component: such a ray
skips nothing), slab-test the node's box, widened by the ray's FAR_PAD, against the world ray with the ray's current t --
t1 = ((lo - o) - far) * (1 / d), t2 = ((hi - o) + far) * (1 / d),
tmax = min over the axes of max(t1, t2), tmin = max over the axes of min(t1, t2), hit when tmax >= tmin and tmin < t and tmax > 0
(slab_dist_finite's arithmetic and rule; evaluated as not (tmax < tmin or tmin >= t or tmax <= 0), so that a NaN -- an unbounded box times
a 1 / d that underflowed to zero -- skips nothing).  Miss: continue at skip.  Hit of an inner node: continue at k + 1.  Hit of a leaf: test its object
exactly as the list walk does, continue at k + 1.  Objects are therefore visited in index order; the tree only skips.
"""
from __future__ import annotations

import numpy as np

import transform_ref as T

PAD = np.float32(1e-4)
FAR_PAD = np.float32(2.0 ** -8)
INNER = 0xFFFFFFFF
NO_HIT = 0xFFFFFFFF
F = np.float32
INF = np.float32(np.inf)


# ---- boxes --------------------------------------------------------------------------------------------------------------------------------
def unbounded():
    return np.array([-np.inf] * 3 + [np.inf] * 3, np.float32)


def float_below(v):
    f = np.asarray(v, np.float64).astype(np.float32)
    return np.where(f.astype(np.float64) > v, np.nextafter(f, -INF), f).astype(np.float32)


def float_above(v):
    f = np.asarray(v, np.float64).astype(np.float32)
    return np.where(f.astype(np.float64) < v, np.nextafter(f, INF), f).astype(np.float32)


def transform_box(m, local):
    m = np.ascontiguousarray(m, np.float32).reshape(3, 4).astype(np.float64)
    local = np.asarray(local, np.float32).astype(np.float64)
    corners = np.array([[local[3 if c & 1 else 0], local[4 if c & 2 else 1], local[5 if c & 4 else 2]] for c in range(8)])
    w = ((m[None, :, 0] * corners[:, None, 0] + m[None, :, 1] * corners[:, None, 1]) + m[None, :, 2] * corners[:, None, 2]) + m[None, :, 3]
    return np.concatenate([float_below(w.min(0)), float_above(w.max(0))]).astype(np.float32)


def pad_box(box):
    box = np.asarray(box, np.float32)
    if not np.all(np.isfinite(box)):
        return unbounded()
    lo, hi = box[:3], box[3:]
    with np.errstate(all="ignore"):
        m = np.maximum(np.maximum(np.abs(lo), np.abs(hi)), (hi - lo).astype(np.float32)).astype(np.float32)
        pad = (PAD * m).astype(np.float32)
        out = np.concatenate([np.nextafter((lo - pad).astype(np.float32), -INF), np.nextafter((hi + pad).astype(np.float32), INF)]).astype(np.float32)
    return out if np.all(np.isfinite(out)) else unbounded()


def vertex_bounds(positions):
    p = np.asarray(positions, np.float32).reshape(-1, 3)
    if not np.all(np.isfinite(p)):
        return unbounded()
    return np.concatenate([p.min(0), p.max(0)]).astype(np.float32)


def leaf_box(obj):
    """The padded world box of one object of a spec (see forty_objects): 'local' is a mesh's object-space box (its root node's bounds)."""
    kind = obj["kind"]
    if kind == "sphere":
        c, r = np.asarray(obj["center"], np.float32), np.float32(obj["radius"])
        box = np.concatenate([c - r, c + r]).astype(np.float32)
        if not np.all(box[:3] <= box[3:]):
            box = unbounded()
    elif kind == "plane":
        box = unbounded()
    else:
        box = np.asarray(obj["local"], np.float32)
        m = obj.get("transform")
        if np.all(np.isfinite(box)) and m is not None and not T.is_identity(m):
            box = transform_box(m, box)
    return pad_box(box)


# ---- tree ---------------------------------------------------------------------------------------------------------------------------------
def build_tree(leaf_boxes):
    """(nodes (2 n - 1, 8) float32 whose words 3 and 7 are uint32 bits, entry (n + 1,) uint32) over the padded leaf boxes (n, 6)."""
    leaf_boxes = np.asarray(leaf_boxes, np.float32).reshape(-1, 6)
    n = leaf_boxes.shape[0]
    nodes = np.zeros((2 * n - 1, 8), np.float32)
    words = nodes.view(np.uint32)
    entry = np.full(n + 1, 0xFFFFFFFF, np.uint32)
    count = [0]

    def build(i, j):
        k = count[0]; count[0] += 1
        if entry[i] == 0xFFFFFFFF:
            entry[i] = k
        if j - i == 1:
            box, obj = leaf_boxes[i], i
        else:
            m = i + (j - i + 1) // 2
            a, b = build(i, m), build(m, j)
            box, obj = np.concatenate([np.minimum(a[:3], b[:3]), np.maximum(a[3:], b[3:])]), INNER
        nodes[k, 0:3] = box[:3]; nodes[k, 4:7] = box[3:]
        words[k, 3] = count[0]; words[k, 7] = obj
        return box

    build(0, n)
    entry[n] = 2 * n - 1
    return nodes, entry


def morton_order(boxes):
    """Scene.sort_objects_spatially's order: unbounded boxes first, then a 30-bit Morton code of the box centres, ties in the old order."""
    boxes = np.asarray(boxes, np.float64)
    finite = np.isfinite(boxes).all(-1)
    key = np.zeros(boxes.shape[0], np.uint64)
    if finite.any():
        c = 0.5 * (boxes[finite, :3] + boxes[finite, 3:])
        lo, hi = c.min(0), c.max(0)
        q = np.floor((c - lo) / np.where(hi > lo, hi - lo, 1.0) * 1023.0 + 0.5).astype(np.uint64)
        code = np.zeros(q.shape[0], np.uint64)
        for bit in range(10):
            for axis in range(3):
                code |= ((q[:, axis] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + axis)
        key[finite] = code + np.uint64(1)
    return np.argsort(key, kind="stable").astype(np.uint32)


# ---- the device's intersectors, float32, vectorised over rays ---------------------------------------------------------------------------------
def _dot(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(np.float32)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(np.float32)


def box_hit(lo, hi, o, inv, t):
    """slab_dist_finite's rule for rays (n, 3) against one box widened by each ray's FAR_PAD (v_min / v_max return the other operand for a
    NaN: fmin / fmax)."""
    with np.errstate(all="ignore"):
        a = (lo[None] - o).astype(np.float32); b = (hi[None] - o).astype(np.float32)
        pad = (FAR_PAD * np.fmax(np.abs(a).max(-1), np.abs(b).max(-1))).astype(np.float32)[:, None]
        t1 = ((a - pad).astype(np.float32) * inv).astype(np.float32); t2 = ((b + pad).astype(np.float32) * inv).astype(np.float32)
        tmax = np.fmin(np.fmin(np.fmax(t1[:, 0], t2[:, 0]), np.fmax(t1[:, 1], t2[:, 1])), np.fmax(t1[:, 2], t2[:, 2]))
        tmin = np.fmax(np.fmax(np.fmin(t1[:, 0], t2[:, 0]), np.fmin(t1[:, 1], t2[:, 1])), np.fmin(t1[:, 2], t2[:, 2]))
        return ~(tmax < tmin) & ~(tmin >= t) & ~(tmax <= 0)                    # the same rule for numbers; a NaN skips nothing


def hit_sphere(c, r2, o, d, t):
    with np.errstate(all="ignore"):
        L = (c[None] - o).astype(np.float32)
        tca = _dot(L, d)
        d2 = (_dot(L, L) - tca * tca).astype(np.float32)
        thc = np.sqrt((r2 - d2).astype(np.float32))
        a, b = (tca - thc).astype(np.float32), (tca + thc).astype(np.float32)
        t0, t1 = np.where(a > b, b, a), np.where(a > b, a, b)
        ok = ~(tca < 0) & ~(d2 > r2)
        t0 = np.where(t0 < 0, t1, t0)
        ok &= ~(t0 < 0) & (t0 < t)
    return ok, t0.astype(np.float32)


def hit_plane(n, p, o, d, t):
    with np.errstate(all="ignore"):
        denom = _dot(d, n[None])
        tt = (_dot((p[None] - o).astype(np.float32), n[None]) / denom).astype(np.float32)
        ok = (np.abs(denom).astype(np.float64) > 1e-6) & (tt > 0) & (tt < t)
    return ok, tt


def hit_triangle(v0, e1, e2, o, d, t):
    with np.errstate(all="ignore"):
        H = _cross(d, e2[None]); a = _dot(e1[None], H)
        f = (np.float32(1.0) / a).astype(np.float32)
        S = (o - v0[None]).astype(np.float32)
        u = (f * _dot(S, H)).astype(np.float32)
        Q = _cross(S, e1[None])
        v = (f * _dot(d, Q)).astype(np.float32)
        tt = (f * _dot(e2[None], Q)).astype(np.float32)
        ok = ~(np.abs(a) < np.float32(0.001)) & ~((u < 0) | (u > 1)) & ~((v < 0) | ((u + v).astype(np.float32) > 1)) & (tt > 0) & (tt < t)
    return ok, tt


def _slab_dist(lo, hi, o, inv, t, exact):
    """One ray against one child box: rt_device.hpp's slab_dist_finite, or slab_dist_exact (the NaN behaviour of the compare-and-select form)."""
    with np.errstate(all="ignore"):
        t1 = ((lo - o) * inv).astype(np.float32); t2 = ((hi - o) * inv).astype(np.float32)
        if not exact:
            tmax = np.fmin(np.fmin(np.fmax(t1[0], t2[0]), np.fmax(t1[1], t2[1])), np.fmax(t1[2], t2[2]))
            tmin = np.fmax(np.fmax(np.fmin(t1[0], t2[0]), np.fmin(t1[1], t2[1])), np.fmin(t1[2], t2[2]))
        else:
            vmax = [t1[k] if t1[k] > t2[k] else t2[k] for k in range(3)]
            vmin = [t1[k] if t1[k] < t2[k] else t2[k] for k in range(3)]
            mn = lambda a, b: b if b < a else a                               # std::min / std::max
            mx = lambda a, b: b if a < b else a
            tmax = mn(vmax[0], mn(vmax[1], vmax[2]))
            tmin = mx(vmin[0], mx(vmin[1], vmin[2]))
        return tmin if (tmax >= tmin and tmin < t and tmax > 0) else np.float32(1e30)


class MeshModel:
    """A mesh as the device walks it: the exported tree (Scene.bvh_export: nodes (n, 8) words, tri_indices) over its triangles."""

    def __init__(self, vertices, indices, nodes, tri_indices):
        v = np.asarray(vertices, np.float32)[:, :3]
        i = np.asarray(indices).reshape(-1, 3)
        self.v0 = v[i[:, 0]]
        self.e1 = (v[i[:, 1]] - self.v0).astype(np.float32)
        self.e2 = (v[i[:, 2]] - self.v0).astype(np.float32)
        raw = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8)
        self.words = raw
        self.bounds = raw.view(np.float32)
        self.tidx = np.asarray(tri_indices, np.int64)
        self.inner_root = raw[0, 7] == 0
        self.local = np.concatenate([self.bounds[0, 0:3], self.bounds[0, 4:7]]) if self.inner_root else vertex_bounds(v[i.ravel()])

    def _leaf(self, node, o, d, t, tri, counts):
        first, n = int(self.words[node, 3]), int(self.words[node, 7])
        hit = False
        for s in range(first, first + n):
            k = self.tidx[s]
            counts[1] += 1
            ok, tt = hit_triangle(self.v0[k], self.e1[k], self.e2[k], o[None], d[None], t)
            if ok[0]:
                t, tri, hit = tt[0], k, True
        return hit, t, tri

    def traverse(self, o, d, t, tri, depth, counts):
        """traverse_mesh for one ray: (hit, t, tri, depth); counts = [inner steps, triangle tests]."""
        with np.errstate(all="ignore"):
            inv = (np.float32(1.0) / d).astype(np.float32)
        exact = bool(np.isinf(inv).any())
        node, stack, result = 0, [], False
        while True:
            if self.words[node, 7] > 0:
                hit, t, tri = self._leaf(node, o, d, t, tri, counts)
                result = result or hit
                if not stack:
                    break
                node = stack.pop()
                continue
            L = int(self.words[node, 3])
            counts[0] += 1
            dl = _slab_dist(self.bounds[L, 0:3], self.bounds[L, 4:7], o, inv, t, exact)
            dr = _slab_dist(self.bounds[L + 1, 0:3], self.bounds[L + 1, 4:7], o, inv, t, exact)
            a, b = L, L + 1
            if dl > dr:
                dl, dr, a, b = dr, dl, b, a
            if dl == np.float32(1e30):
                if not stack:
                    break
                node = stack.pop()
            else:
                depth += 1
                node = a
                if dr != np.float32(1e30):
                    stack.append(b)
        return result, t, tri, depth


class SceneModel:
    """IntersectScene over a spec (forty_objects' format; a mesh carries 'model': MeshModel): the list walk and the tree walk."""

    def __init__(self, spec):
        self.spec = spec
        self.n = len(spec)
        for ob in spec:
            if ob["kind"] == "mesh":
                ob["local"] = ob["model"].local
            elif ob["kind"] == "triangle":
                ob["local"] = vertex_bounds(ob["positions"])
        self.leaf_boxes = np.stack([leaf_box(ob) for ob in spec])
        self.nodes, self.entry = build_tree(self.leaf_boxes)

    def _test(self, k, idx, o, d, st):
        """Object k against the rays idx, as the list walk tests it."""
        ob = self.spec[k]
        t = st["t"][idx]
        if ob["kind"] == "sphere":
            r = np.float32(ob["radius"])
            ok, tt = hit_sphere(np.asarray(ob["center"], np.float32), np.float32(r * r), o[idx], d[idx], t)
        elif ob["kind"] == "plane":
            ok, tt = hit_plane(np.asarray(ob["normal"], np.float32), np.asarray(ob["point"], np.float32), o[idx], d[idx], t)
        else:
            oo, od = o[idx], d[idx]
            m = ob.get("transform")
            if m is not None and not T.is_identity(m):
                oo, od = T.ray_to_object(T.invert(m), oo, od)
            if ob["kind"] == "triangle":
                p = np.asarray(ob["positions"], np.float32).reshape(3, 3)
                ok, tt = hit_triangle(p[0], (p[1] - p[0]).astype(np.float32), (p[2] - p[0]).astype(np.float32), oo, od, t)
            else:
                mm = ob["model"]
                ok = np.zeros(idx.size, bool); tt = t.copy()
                for j in range(idx.size):
                    counts = [0, 0]
                    hit, tj, tri, depth = mm.traverse(oo[j], od[j], t[j], int(st["tri"][idx[j]]), int(st["depth"][idx[j]]), counts)
                    st["depth"][idx[j]] = depth; st["inner"] += counts[0]; st["tris"] += counts[1]
                    if hit:
                        ok[j] = True; tt[j] = tj; st["tri"][idx[j]] = tri
        hit = idx[ok]
        st["t"][hit] = tt[ok]; st["obj"][hit] = k

    def walk(self, o, d, tmax=None, tree=False):
        """(t, obj, tri, depth, info): info['inner'] mesh inner steps, info['tris'] mesh triangle tests, info['leaves'] objects tested
        per ray, info['nodes'] tree nodes met per ray, info['skipped_inner_roots'] meshes with an inner root that the tree skipped, summed over the rays."""
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32)
        n = o.shape[0]
        st = {"t": np.full(n, 1e34, np.float32) if tmax is None else np.array(tmax, np.float32, copy=True),
              "obj": np.full(n, NO_HIT, np.uint32), "tri": np.zeros(n, np.int64), "depth": np.zeros(n, np.int64), "inner": 0, "tris": 0}
        leaves = np.zeros(n, np.int64)
        tested = np.zeros(self.n, np.int64)                                    # rays that reached each object
        boxes = np.zeros(n, np.int64)                                          # nodes met per ray
        with np.errstate(all="ignore"):
            inv = (np.float32(1.0) / d).astype(np.float32)
        no_skip = np.isinf(inv).any(-1) | (not tree)
        words = self.nodes.view(np.uint32)
        cursor = np.zeros(n, np.int64)
        for k in range(2 * self.n - 1):
            idx = np.nonzero(cursor == k)[0]
            if idx.size == 0:
                continue
            boxes[idx] += 1
            hit = no_skip[idx] | box_hit(self.nodes[k, 0:3], self.nodes[k, 4:7], o[idx], inv[idx], st["t"][idx])
            cursor[idx[~hit]] = words[k, 3]
            cursor[idx[hit]] = k + 1
            obj = words[k, 7]
            if obj == INNER:
                continue
            leaves[idx[hit]] += 1
            tested[obj] = int(hit.sum())
            if hit.any():
                self._test(int(obj), idx[hit], o, d, st)
        skipped = sum(n - int(tested[k]) for k, ob in enumerate(self.spec) if ob["kind"] == "mesh" and ob["model"].inner_root)
        info = {"inner": st["inner"], "tris": st["tris"], "leaves": leaves, "nodes": boxes, "skipped_inner_roots": skipped}
        return st["t"], st["obj"], st["tri"].astype(np.uint32), st["depth"].astype(np.uint32), info


# ---- the 40 objects and the rays of the tests ---------------------------------------------------------------------------------------------------
def box_mesh(center, half):
    """(vertices (24, 6), indices (36,)): an axis-aligned box, 12 triangles, face normals."""
    c = np.asarray(center, np.float64); h = np.asarray(half, np.float64) * np.ones(3)
    verts, idx = [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            u, v = (axis + 1) % 3, (axis + 2) % 3
            n = np.zeros(3); n[axis] = sign
            base = len(verts)
            for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = c.copy(); p[axis] += sign * h[axis]; p[u] += su * h[u]; p[v] += sv * h[v]
                verts.append(np.concatenate([p, n]))
            idx += [base, base + 1, base + 2, base, base + 2, base + 3]
    return np.array(verts, np.float32), np.array(idx, np.uint32)


def quad_mesh(center, ex, ey):
    """(vertices (4, 6), indices (6,)): the parallelogram centre +- ex +- ey, two triangles."""
    c, ex, ey = (np.asarray(a, np.float64) for a in (center, ex, ey))
    n = np.cross(ex, ey); n /= np.linalg.norm(n)
    verts = [np.concatenate([c + a * ex + b * ey, n]) for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    return np.array(verts, np.float32), np.array([0, 1, 2, 0, 2, 3], np.uint32)


def forty_objects(seed=11):
    """The 40 objects of the tests, in a cube of side 20: 2 planes (objects 0 and 20), 10 spheres (object 1 is the lamp), 8 stand-alone
    triangles, 10 two-triangle quads and 10 boxes; 13 of the 28 triangles / quads / boxes stand under random affine transforms (rotation
    times scale, among them a mirror and a 1:5 non-uniform scale) that bring them from a frame at the origin to their place."""
    rng = np.random.default_rng(seed)
    kinds = ["sphere"] * 9 + ["triangle"] * 8 + ["quad"] * 10 + ["box"] * 10
    rng.shuffle(kinds)
    kinds = ["plane", "sphere"] + kinds[:18] + ["plane"] + kinds[18:]
    assert len(kinds) == 40
    movable = [k for k, kind in enumerate(kinds) if kind in ("triangle", "quad", "box")]
    moved = set(int(k) for k in rng.choice(movable, 13, replace=False))
    special = iter([np.diag([1.0, 1.0, -1.0]), np.diag([1.0, 5.0, 1.0]) * 0.5])       # a mirror; 1:5 non-uniform
    spec = []
    for k, kind in enumerate(kinds):
        centre = rng.uniform(-9.0, 9.0, 3)
        if kind == "plane":
            spec.append({"kind": "plane", "normal": (0.0, 1.0, 0.0), "point": (0.0, -11.0, 0.0)} if k == 0 else
                        {"kind": "plane", "normal": (0.0, 0.0, 1.0), "point": (0.0, 0.0, -12.0)})
            continue
        if kind == "sphere":
            spec.append({"kind": "sphere", "center": tuple(np.float32(centre)) if k != 1 else (0.0, 9.0, 6.0), "radius": float(np.float32(rng.uniform(0.4, 1.2)))})
            continue
        transform = None
        place = centre
        if k in moved:
            A = T.rotation(rng.standard_normal(3), rng.uniform(0.2, 2.8)) @ next(special, np.diag(rng.uniform(0.6, 1.6, 3)))
            transform = T.affine(A, centre)
            place = np.zeros(3)                                                # stored at the origin, placed by the transform
        if kind == "triangle":
            p = place + rng.uniform(-1.2, 1.2, (3, 3))
            nrm = np.cross(p[1] - p[0], p[2] - p[0]); nrm /= np.linalg.norm(nrm)
            spec.append({"kind": "triangle", "positions": p.astype(np.float32), "normal": nrm.astype(np.float32), "transform": transform})
        elif kind == "quad":
            ex = rng.standard_normal(3); ex *= rng.uniform(0.5, 1.3) / np.linalg.norm(ex)
            ey = np.cross(ex, rng.standard_normal(3)); ey *= rng.uniform(0.5, 1.3) / np.linalg.norm(ey)
            v, i = quad_mesh(place, ex, ey)
            spec.append({"kind": "mesh", "vertices": v, "indices": i, "transform": transform, "shape": "quad"})
        else:
            v, i = box_mesh(place, rng.uniform(0.4, 1.1, 3))
            spec.append({"kind": "mesh", "vertices": v, "indices": i, "transform": transform, "shape": "box"})
    return spec


def forest_of_boxes(n=64, spacing=6.0, seed=3):
    """n well-separated boxes on a cubic grid of the given spacing, in a shuffled order (untransformed meshes)."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    cells = np.array([(x, y, z) for x in range(side) for y in range(side) for z in range(side)][:n], np.float64)
    rng.shuffle(cells)
    return [dict(kind="mesh", vertices=v, indices=i, transform=None, shape="box")
            for v, i in (box_mesh(spacing * (c - 0.5 * (side - 1)), 0.5) for c in cells)]


def random_rays(n=4096, seed=5, radius=26.0, target=11.0):
    """n rays from a sphere of the given radius aimed into the ball of radius `target` around the origin; a quarter of them carry a
    finite tmax: (o, d, tmax) float32."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3)); u /= np.linalg.norm(u, axis=-1, keepdims=True)
    o = radius * u
    w = rng.standard_normal((n, 3)); w /= np.linalg.norm(w, axis=-1, keepdims=True)
    d = target * w * rng.random((n, 1)) ** (1.0 / 3.0) - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    tmax = np.full(n, 1e34, np.float32)
    tmax[::4] = rng.uniform(10.0, 40.0, tmax[::4].size).astype(np.float32)
    return o.astype(np.float32), d.astype(np.float32), tmax


def surface_rays(o, d, t, obj, n=512, seed=6):
    """n rays that start on a surface: the hit points o + d t of earlier rays (float32), with fresh directions."""
    rng = np.random.default_rng(seed)
    hit = np.nonzero(obj != NO_HIT)[0][:n]
    so = (o[hit] + d[hit] * t[hit][:, None]).astype(np.float32)
    w = rng.standard_normal((hit.size, 3)); w /= np.linalg.norm(w, axis=-1, keepdims=True)
    return so, w.astype(np.float32)


def axis_rays(n=256, seed=8, extent=9.0):
    """n rays with one or two direction components exactly zero, through the cube of the objects."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-extent, extent, (n, 3))
    d = rng.standard_normal((n, 3))
    for k in range(n):
        ax = k % 3
        if k < n // 2:
            d[k] = 0.0; d[k, ax] = 1.0 if k % 2 else -1.0
        else:
            d[k, ax] = 0.0
        d[k] /= np.linalg.norm(d[k])
        o[k] -= 20.0 * d[k]
    return o.astype(np.float32), d.astype(np.float32)


def far_rays(n=2048, seed=12, height=-11.0, target=(0.0, 9.0, 6.0), radius=1.0):
    """n shadow rays as a path on an infinite ground plane sends them: from points of the plane y = height 10^4 to 10^6 units out, aimed at
    points of a sphere (the lamp of forty_objects), tmax the distance to the point: (o, d, tmax) float32.  From there the list walk's
    sphere test reports hits on spheres that the ray passes a hundred units from (see FAR_PAD)."""
    rng = np.random.default_rng(seed)
    rad = 10.0 ** rng.uniform(4.0, 6.0, n); ang = rng.uniform(0.0, 2.0 * np.pi, n)
    o = np.stack([rad * np.cos(ang), np.full(n, height), rad * np.sin(ang)], -1)
    u = rng.standard_normal((n, 3)); u /= np.linalg.norm(u, axis=-1, keepdims=True)
    d = np.asarray(target, np.float64) + radius * u - o
    dist = np.linalg.norm(d, axis=-1, keepdims=True)
    return o.astype(np.float32), (d / dist).astype(np.float32), dist[:, 0].astype(np.float32)
