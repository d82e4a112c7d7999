// bvh_build.hip -- GPU BVH::Build / BVH::Rebuild for the reference's three BuildOptions, bit-identical to the host build,
// and for CGPT_BUILD_SAH_BINNED (not in the reference; see "BuildOption_SAHBinned" below), word for word the host mirror's tree.
//
// Options (ref: Source/BVH.cpp:204-297): SAH split intervals (the default, BVH.h:43-44; described below), naive split (midpoint of the
// longest axis, stop at <= 2 triangles, :208-224 -- the same level kernels with the 24-candidate sweep replaced by one plane), and
// SAH split primitives, whose cheapest_cost is never updated (SURVEY A-5), so the root stays a leaf: no kernel at all.
// Rebuild (ref: BVH.cpp:47-59) re-splits over the CURRENT triangle order (m_tri_indices is not reset), so it is the same build
// started from a caller-provided permutation instead of the identity.
//
// Reproduces ref: Source/BVH.cpp:11-45 (Build), :204-259 (Subdivide, SAH with 8 planes x 3 axes on the node bounds),
// :299-327 (EvaluateSAH), :329-366 (Split) -- same split decisions, same node numbering, same triangle order:
//   * levels run one after the other, all nodes of a level are independent.  Deep levels (many small nodes): one workgroup per
//     node does everything (subdivide_level).  The top levels (few, huge nodes -- the root alone is the whole mesh) are cut into
//     kWideBlocks-ish position-ordered pieces, one workgroup each, and run as six short kernels (wide_*) whose per-piece partial
//     results are combined IN PIECE ORDER by one workgroup per node: with one workgroup per node the first ten levels of a
//     1.31 M-triangle mesh kept one CU busy for 0.5 s;
//   * a candidate plane's cost is the reference's float expression on exact counts and exact (min/max) bounds.  Bounds are
//     reduced in triangle order (each thread owns a contiguous chunk, partial results are combined in thread order), so
//     even the sign of a zero bound is the one the sequential std::min/std::max chain leaves;
//   * the in-place swap partition (BVH.cpp:334-344) is order-sensitive; its result has a closed form (see partition_slot
//     below, checked against the sequential loop in tests/test_host.py) that is evaluated in parallel from one prefix
//     sum of the "left" flags;
//   * nodes are created in breadth-first order with an atomic counter and renumbered at the end into the reference's
//     allocation order (children of the k-th splitting node in depth-first preorder get indices 2k+1, 2k+2).
// cgpt_scene_rebuild_mesh (at the end of this file) runs the same level loop over a mesh of the uploaded scene, fed from
// the scene's own triangle arrays, and writes the tree as the scene's child-pair and leaf-triangle records: a Rebuild in place.
#include <hip/hip_runtime.h>

#include <exception>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cpugpupt_abi.h"
#include "ctx_internal.h"
#include "device_memory.h"
#include "minmax_std.h"
#include "rebuild_layout.h"

namespace cgpt {

hipStream_t CtxStream(cgpt_ctx* ctx);
int CtxDevice(cgpt_ctx* ctx);
cgpt_ctx* GroupFirstMemberOrNull(cgpt_ctx* ctx);
int GroupForwarded(cgpt_ctx* ctx, int rc);

namespace {

constexpr uint32_t kBuildThreads = 256;

struct F3 { float x, y, z; };
__device__ inline F3 f3min(F3 a, F3 b) { return { min_std(a.x, b.x), min_std(a.y, b.y), min_std(a.z, b.z) }; }
__device__ inline F3 f3max(F3 a, F3 b) { return { max_std(a.x, b.x), max_std(a.y, b.y), max_std(a.z, b.z) }; }
__device__ inline float axis_of(F3 v, uint32_t a) { return a == 0 ? v.x : (a == 1 ? v.y : v.z); }
__device__ inline float half_area(F3 lo, F3 hi)                               // GetAABBVolume, ref: Primitives.cpp:280-284
{
    const float ex = hi.x - lo.x, ey = hi.y - lo.y, ez = hi.z - lo.z;
    return ex * ey + ey * ez + ez * ex;
}

struct BuildNode {              // breadth-first working node
    F3 lo, hi;
    uint32_t first, count;      // segment of tri_indices
    uint32_t left;              // breadth-first id of the left child (right = left + 1); 0 = leaf
    uint32_t depth;
    uint32_t splits;            // splitting nodes in this subtree (renumbering)
    uint32_t rank;              // preorder rank among splitting nodes (renumbering)
    uint32_t new_id;            // index in the reference's numbering
};

struct Bounds { F3 lo, hi; };
struct WidePartial { Bounds lb, rb; uint32_t lc, rc; };
struct WideDecision { uint32_t split, axis; float pos; uint32_t n_left; };
struct WideChild { Bounds lb, rb; };

struct BuildArrays {
    const F3* tri_lo; const F3* tri_hi; const F3* centroid;   // per triangle
    uint32_t* tri_indices; uint32_t* scratch_idx;              // n_tris each
    uint32_t* sel_a; uint32_t* sel_b;                           // n_tris each: hole / tail-left position tables of the partition
    BuildNode* nodes;                                            // 2 n_tris - 1
    uint32_t* counters;                                          // [0] nodes allocated, [1] max depth
    uint32_t naive;                                              // BuildOption_NaiveSplit: one plane per node instead of the SAH sweep
    // wide levels only (index j = node of the level, b = piece of the node)
    WidePartial* partial;                                        // [j][b][24]: candidate sums of one piece
    WideDecision* decision;                                      // [j]
    uint32_t* piece_left;                                        // [j][b]: lefts before the piece (exclusive prefix over the pieces)
    uint32_t* piece_front;                                       // [j][b]: lefts of the piece that lie in the front [0, n_left)
    WideChild* piece_child;                                      // [j][b]: child bounds of the piece, new triangle order
};

// ---- per-triangle preparation: bounds and centroid (ref: Primitives.cpp:232-243, 255-258) ------------------------------------
__global__ void prepare_triangles(const cgpt_triangle* tris, uint32_t n, F3* lo, F3* hi, F3* centroid, uint32_t* idx, uint32_t identity)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const cgpt_triangle& t = tris[i];
    const F3 p0 = { t.v0.pos[0], t.v0.pos[1], t.v0.pos[2] }, p1 = { t.v1.pos[0], t.v1.pos[1], t.v1.pos[2] }, p2 = { t.v2.pos[0], t.v2.pos[1], t.v2.pos[2] };
    lo[i] = f3min(f3min(p0, p1), p2);
    hi[i] = f3max(f3max(p0, p1), p2);
    centroid[i] = { ((p0.x + p1.x) + p2.x) * 0.3333f, ((p0.y + p1.y) + p2.y) * 0.3333f, ((p0.z + p1.z) + p2.z) * 0.3333f };
    if (identity) idx[i] = i;                                              // Build: ref BVH.cpp:25-29; Rebuild keeps the order it is given
}

// ---- ordered block reductions ------------------------------------------------------------------------------------------------
// Threads own contiguous chunks in position order, so "the earlier operand" is always the lower lane / lower wave:
// combining with a = earlier, b = later keeps std::min / std::max's left-most-of-equals result.
__device__ inline Bounds empty_bounds() { return { { 1e30f, 1e30f, 1e30f }, { -1e30f, -1e30f, -1e30f } }; }
__device__ inline Bounds merge(Bounds a, Bounds b) { return { f3min(a.lo, b.lo), f3max(a.hi, b.hi) }; }

__device__ inline float shfl_down_f(float v, int off) { return __shfl_down(v, off, 64); }
__device__ inline Bounds shfl_down_bounds(Bounds v, int off)
{
    return { { shfl_down_f(v.lo.x, off), shfl_down_f(v.lo.y, off), shfl_down_f(v.lo.z, off) },
             { shfl_down_f(v.hi.x, off), shfl_down_f(v.hi.y, off), shfl_down_f(v.hi.z, off) } };
}
// result valid in thread 0
__device__ inline Bounds block_reduce_bounds(Bounds v, Bounds* lds /* [4] */)
{
    for (int off = 1; off < 64; off <<= 1) {          // lane l absorbs lane l + off: earlier operand first
        const Bounds o = shfl_down_bounds(v, off);
        if ((threadIdx.x & 63) + off < 64) v = merge(v, o);
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) v = merge(merge(lds[0], lds[1]), merge(lds[2], lds[3]));
    __syncthreads();
    return v;
}
__device__ inline uint32_t block_reduce_sum(uint32_t v, uint32_t* lds /* [4] */)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) v = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return v;
}
// exclusive prefix over the block of one value per thread; *total gets the block sum (all threads)
__device__ inline uint32_t block_exclusive_scan(uint32_t v, uint32_t* lds /* [5] */, uint32_t* total)
{
    uint32_t incl = v;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off, 64);
        if ((int)(threadIdx.x & 63) >= off) incl += o;
    }
    if ((threadIdx.x & 63) == 63) lds[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) base += lds[w];
    *total = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return base + incl - v;
}

// ---- group-wide primitives: a group is a whole 256-thread block (G = 256), one wavefront (G = 64) or a quarter of one (G = 16);
//      the sub-block groups use neither LDS nor barriers ------------------------------------------------------------------------
__device__ inline Bounds shfl_down_bounds_w(Bounds v, int off, int width)
{
    return { { __shfl_down(v.lo.x, off, width), __shfl_down(v.lo.y, off, width), __shfl_down(v.lo.z, off, width) },
             { __shfl_down(v.hi.x, off, width), __shfl_down(v.hi.y, off, width), __shfl_down(v.hi.z, off, width) } };
}
template <uint32_t G> __device__ inline void group_sync()                       // orders the group's global-memory writes before its reads
{
    if (G == kBuildThreads) __syncthreads();
    else { __threadfence_block(); __builtin_amdgcn_wave_barrier(); }
}
template <uint32_t G> __device__ inline Bounds group_reduce_bounds(Bounds v, Bounds* lds)       // result valid in thread 0 of the group
{
    if (G == kBuildThreads) return block_reduce_bounds(v, lds);
    for (int off = 1; off < (int)G; off <<= 1) {      // lane l absorbs lane l + off: earlier operand first
        const Bounds o = shfl_down_bounds_w(v, off, (int)G);
        if ((threadIdx.x % G) + off < G) v = merge(v, o);
    }
    return v;
}
template <uint32_t G> __device__ inline uint32_t group_reduce_sum(uint32_t v, uint32_t* lds)    // result valid in thread 0 of the group
{
    if (G == kBuildThreads) return block_reduce_sum(v, lds);
    for (int off = 1; off < (int)G; off <<= 1) {
        const uint32_t o = __shfl_down(v, off, (int)G);
        if ((threadIdx.x % G) + off < G) v += o;
    }
    return v;
}
template <uint32_t G> __device__ inline uint32_t group_exclusive_scan(uint32_t v, uint32_t* lds, uint32_t* total)
{
    if (G == kBuildThreads) return block_exclusive_scan(v, lds, total);
    uint32_t incl = v;
    for (int off = 1; off < (int)G; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off, (int)G);
        if ((int)(threadIdx.x % G) >= off) incl += o;
    }
    *total = __shfl(incl, (int)G - 1, (int)G);
    return incl - v;
}
template <uint32_t G> __device__ inline uint32_t group_broadcast(uint32_t v, uint32_t* lds_word)     // thread 0's value to the group
{
    if (G == kBuildThreads) {
        if (threadIdx.x == 0) *lds_word = v;
        __syncthreads();
        const uint32_t r = *lds_word;
        __syncthreads();
        return r;
    }
    return __shfl(v, 0, (int)G);
}

// ---- one tree level, one GROUP per node (ref: BVH.cpp:225-259 + Split :329-366) --------------------------------------------------
// G = 256: a workgroup per node.  G = 64 / 16: a wavefront / a quarter wavefront per node -- the deep levels, where a level is hundreds
// of thousands of nodes of a few triangles each and a workgroup's two hundred barriers per node were the whole cost (17 ms per level).
// Groups of one wavefront diverge at the leaf / no-split exits; a group's lanes always leave together, and no lane reads another
// group's registers.
// NaiveSplit's plane: the midpoint of the longest axis of the node bounds (ref: BVH.cpp:214-223)
__device__ inline void naive_plane(const BuildNode& node, uint32_t& axis, float& pos)
{
    const F3 extent = { node.hi.x - node.lo.x, node.hi.y - node.lo.y, node.hi.z - node.lo.z };
    axis = 0u;
    if (extent.y > extent.x) axis = 1u;
    if (extent.z > axis_of(extent, axis)) axis = 2u;
    pos = axis_of(node.lo, axis) + axis_of(extent, axis) * 0.5f;
}

template <uint32_t G>
__global__ void __launch_bounds__(kBuildThreads) subdivide_level(BuildArrays A, uint32_t level_first, uint32_t level_count)
{
    __shared__ Bounds s_bounds[4];
    __shared__ uint32_t s_u32[5];
    __shared__ uint32_t s_word;

    constexpr uint32_t groups = kBuildThreads / G;
    const uint32_t in_level = blockIdx.x * groups + threadIdx.x / G, t = threadIdx.x % G;
    if (in_level >= level_count) return;                                       // group-uniform
    const uint32_t node_id = level_first + in_level;
    BuildNode node = A.nodes[node_id];
    const uint32_t n = node.count, first = node.first;
    uint32_t* const idx = A.tri_indices + first;

    // contiguous chunk of this thread, in position order
    const uint32_t chunk = (n + G - 1) / G;
    const uint32_t c0 = min(t * chunk, n), c1 = min(c0 + chunk, n);

    // ---- SAH over 8 planes x 3 axes (split_idx outer, axis inner: the first strictly cheaper candidate wins) ----
    float cheapest_cost = 1e30f; uint32_t cheapest_axis = 0; float cheapest_pos = 0.0f;      // meaningful in thread 0
    float parent_cost = half_area(node.lo, node.hi) * (float)n;
    if (A.naive) {                                                              // ref: BVH.cpp:208-224
        naive_plane(node, cheapest_axis, cheapest_pos);
        cheapest_cost = 0.0f; parent_cost = n <= 2u ? 0.0f : 1.0f;              // "split unless <= 2 triangles" in the test below
    }
    for (uint32_t split_idx = 0; split_idx < (A.naive ? 0u : 8u); ++split_idx) {
        for (uint32_t axis = 0; axis < 3; ++axis) {
            const float axis_width = axis_of(node.hi, axis) - axis_of(node.lo, axis);
            const float split_pos = axis_width * ((float)split_idx / 8) + axis_of(node.lo, axis);
            Bounds lb = empty_bounds(), rb = empty_bounds();
            uint32_t lc = 0, rc = 0;
            for (uint32_t i = c0; i < c1; ++i) {
                const uint32_t tri = idx[i];
                const Bounds tb = { A.tri_lo[tri], A.tri_hi[tri] };
                if (axis_of(A.centroid[tri], axis) < split_pos) { ++lc; lb = merge(lb, tb); }
                else { ++rc; rb = merge(rb, tb); }
            }
            lb = group_reduce_bounds<G>(lb, s_bounds);
            rb = group_reduce_bounds<G>(rb, s_bounds);
            lc = group_reduce_sum<G>(lc, s_u32);
            rc = group_reduce_sum<G>(rc, s_u32);
            if (t == 0) {
                // an empty side has extent -2e30 -> +inf area -> 0 * inf = NaN, which the "<" rejects (ref: BVH.cpp:325)
                const float split_cost = (float)lc * half_area(lb.lo, lb.hi) + (float)rc * half_area(rb.lo, rb.hi);
                if (split_cost < cheapest_cost) { cheapest_cost = split_cost; cheapest_axis = axis; cheapest_pos = split_pos; }
            }
        }
    }
    if (t == 0) atomicMax(&A.counters[1], node.depth);                                          // m_max_depth, ref: BVH.cpp:206
    const uint32_t do_split = group_broadcast<G>((cheapest_cost >= parent_cost) ? 0u : 1u, &s_word);   // ref: BVH.cpp:253-256
    if (do_split == 0u) return;                                                                 // leaf
    const uint32_t axis = group_broadcast<G>(cheapest_axis, &s_word);
    const float split_pos = __uint_as_float(group_broadcast<G>(__float_as_uint(cheapest_pos), &s_word));

    // ---- Split: the reference's in-place swap partition (BVH.cpp:331-344), evaluated in closed form ----
    // L(p) = lefts before p.  n_left = L(n).  Front [0, n_left): a left element stays; the k-th hole (right element,
    // k = p - L(p)) receives the k-th tail-left counted from the end.  Tail [n_left, n): position q receives a[q+1] when a[q+1]
    // is a right element, otherwise (q = n-1 or a[q+1] is a left element) the k-th hole's element with k = lefts behind q, and
    // once the holes are used up the first tail element a[n_left] (the final rotation).
    uint32_t my_left = 0;
    for (uint32_t i = c0; i < c1; ++i) my_left += (axis_of(A.centroid[idx[i]], axis) < split_pos) ? 1u : 0u;
    uint32_t n_left = 0;
    const uint32_t left_before_chunk = group_exclusive_scan<G>(my_left, s_u32, &n_left);
    uint32_t* const hole_pos = A.sel_a + first;          // k-th hole -> position
    uint32_t* const tail_left_pos = A.sel_b + first;     // k-th tail-left from the end -> position
    uint32_t* const out = A.scratch_idx + first;
    uint32_t front_left = 0;
    {
        uint32_t L = left_before_chunk;
        for (uint32_t p = c0; p < c1; ++p) {
            const bool is_left = axis_of(A.centroid[idx[p]], axis) < split_pos;
            if (p < n_left) { if (is_left) ++front_left; else hole_pos[p - L] = p; }
            else if (is_left) tail_left_pos[n_left - L - 1u] = p;       // lefts at positions > p: n_left - (L + 1)
            L += is_left ? 1u : 0u;
        }
    }
    front_left = group_reduce_sum<G>(front_left, s_u32);
    group_sync<G>();                                                    // publishes the two tables
    const uint32_t holes = n_left - group_broadcast<G>(front_left, &s_word);    // rights in the front = lefts in the tail
    {
        uint32_t L = left_before_chunk;
        for (uint32_t p = c0; p < c1; ++p) {
            const bool is_left = axis_of(A.centroid[idx[p]], axis) < split_pos;
            L += is_left ? 1u : 0u;                                     // now: lefts at positions <= p
            uint32_t value;
            if (p < n_left) {
                value = is_left ? idx[p] : idx[tail_left_pos[p - L]];                  // hole number = rights before p
            } else if (p + 1u == n || axis_of(A.centroid[idx[p + 1u]], axis) < split_pos) {
                const uint32_t k = n_left - L;                                              // lefts at positions > p
                value = k < holes ? idx[hole_pos[k]] : idx[n_left];
            } else {
                value = idx[p + 1u];
            }
            out[p] = value;
        }
    }
    group_sync<G>();                                                    // every read of the old order is done
    for (uint32_t p = c0; p < c1; ++p) idx[p] = out[p];
    group_sync<G>();

    if (n_left == 0u || n_left == n) return;                                                // ref: BVH.cpp:346-348 (stays a leaf)

    // ---- children (ref: BVH.cpp:350-362): bounds in the NEW triangle order (CalculateNodeBounds) ----
    Bounds lb = empty_bounds(), rb = empty_bounds();
    for (uint32_t p = c0; p < c1; ++p) {
        const uint32_t tri = idx[p];
        const Bounds tb = { A.tri_lo[tri], A.tri_hi[tri] };
        if (p < n_left) lb = merge(lb, tb); else rb = merge(rb, tb);
    }
    lb = group_reduce_bounds<G>(lb, s_bounds);
    rb = group_reduce_bounds<G>(rb, s_bounds);
    if (t == 0) {
        const uint32_t left_id = atomicAdd(&A.counters[0], 2u);
        BuildNode l{}, r{};
        l.lo = lb.lo; l.hi = lb.hi; l.first = first; l.count = n_left; l.depth = node.depth + 1u;
        r.lo = rb.lo; r.hi = rb.hi; r.first = first + n_left; r.count = n - n_left; r.depth = node.depth + 1u;
        A.nodes[left_id] = l; A.nodes[left_id + 1u] = r;
        A.nodes[node_id].left = left_id;
    }
}

// ---- the top levels: a node's index range cut into `pieces` position-ordered pieces, one workgroup each --------------------------
// Same arithmetic as subdivide_level, split where that kernel has a block-wide dependency: candidate sums per piece ->
// (wide_decide) combine in piece order, choose the plane, prefix of the left counts -> partition tables per piece -> the closed-form
// partition per piece -> copy back + child bounds per piece -> (wide_children) combine in piece order, create the children.
// min_std / max_std keep the EARLIER operand on ties and every combination below has the earlier piece on the left, so the result is
// the one the sequential chain over the node's triangles leaves (same argument as for the thread-ordered block reduction).
constexpr uint32_t kWideBlocks = 1024;      // pieces of a level at most (nodes x pieces per node)
constexpr uint32_t kCandidates = 24;        // 8 planes x 3 axes, split_idx outer (ref: BVH.cpp:229-251)

struct Piece { uint32_t j, b, n, first, c0, c1; };       // node of the level, piece; node size / first index; this thread's positions
__device__ inline Piece piece_of(const BuildArrays& A, uint32_t level_first, uint32_t pieces, BuildNode& node)
{
    Piece q;
    q.j = blockIdx.x / pieces; q.b = blockIdx.x - q.j * pieces;
    node = A.nodes[level_first + q.j];
    q.n = node.count; q.first = node.first;
    const uint32_t per_piece = (q.n + pieces - 1u) / pieces;
    const uint32_t p0 = min(q.b * per_piece, q.n), p1 = min(p0 + per_piece, q.n);
    const uint32_t chunk = (p1 - p0 + kBuildThreads - 1u) / kBuildThreads;
    q.c0 = min(p0 + threadIdx.x * chunk, p1); q.c1 = min(q.c0 + chunk, p1);
    return q;
}
__device__ inline float candidate_pos(const BuildNode& node, uint32_t split_idx, uint32_t axis)      // ref: BVH.cpp:233-234
{
    const float axis_width = axis_of(node.hi, axis) - axis_of(node.lo, axis);
    return axis_width * ((float)split_idx / 8) + axis_of(node.lo, axis);
}

__global__ void __launch_bounds__(kBuildThreads) wide_sah_partial(BuildArrays A, uint32_t level_first, uint32_t pieces)
{
    __shared__ Bounds s_bounds[4];
    __shared__ uint32_t s_u32[5];
    BuildNode node;
    const Piece q = piece_of(A, level_first, pieces, node);
    const uint32_t* const idx = A.tri_indices + q.first;
    WidePartial* const out = A.partial + ((size_t)q.j * pieces + q.b) * kCandidates;
    uint32_t naive_axis = 0; float naive_pos = 0.0f;
    if (A.naive) naive_plane(node, naive_axis, naive_pos);                      // one candidate, kept in slot 0
    for (uint32_t split_idx = 0; split_idx < (A.naive ? 1u : 8u); ++split_idx) {
        for (uint32_t axis = (A.naive ? naive_axis : 0u); axis < (A.naive ? naive_axis + 1u : 3u); ++axis) {
            const float split_pos = A.naive ? naive_pos : candidate_pos(node, split_idx, axis);
            Bounds lb = empty_bounds(), rb = empty_bounds();
            uint32_t lc = 0, rc = 0;
            for (uint32_t i = q.c0; i < q.c1; ++i) {
                const uint32_t tri = idx[i];
                const Bounds tb = { A.tri_lo[tri], A.tri_hi[tri] };
                if (axis_of(A.centroid[tri], axis) < split_pos) { ++lc; lb = merge(lb, tb); }
                else { ++rc; rb = merge(rb, tb); }
            }
            lb = block_reduce_bounds(lb, s_bounds);
            rb = block_reduce_bounds(rb, s_bounds);
            lc = block_reduce_sum(lc, s_u32);
            rc = block_reduce_sum(rc, s_u32);
            if (threadIdx.x == 0) out[A.naive ? 0u : split_idx * 3u + axis] = { lb, rb, lc, rc };
        }
    }
}

__global__ void __launch_bounds__(64) wide_decide(BuildArrays A, uint32_t level_first, uint32_t pieces)
{
    __shared__ WidePartial s_c[kCandidates];
    const uint32_t j = blockIdx.x;
    const BuildNode node = A.nodes[level_first + j];
    if (threadIdx.x < (A.naive ? 1u : kCandidates)) {
        WidePartial acc = { empty_bounds(), empty_bounds(), 0u, 0u };
        for (uint32_t b = 0; b < pieces; ++b) {                                 // piece order = position order
            const WidePartial w = A.partial[((size_t)j * pieces + b) * kCandidates + threadIdx.x];
            acc.lb = merge(acc.lb, w.lb); acc.rb = merge(acc.rb, w.rb); acc.lc += w.lc; acc.rc += w.rc;
        }
        s_c[threadIdx.x] = acc;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float cheapest_cost = 1e30f; uint32_t cheapest = 0;
    for (uint32_t c = 0; c < (A.naive ? 0u : kCandidates); ++c) {               // split_idx outer, axis inner: the first strictly cheaper wins
        const WidePartial& w = s_c[c];
        const float split_cost = (float)w.lc * half_area(w.lb.lo, w.lb.hi) + (float)w.rc * half_area(w.rb.lo, w.rb.hi);
        if (split_cost < cheapest_cost) { cheapest_cost = split_cost; cheapest = c; }
    }
    const float parent_cost = half_area(node.lo, node.hi) * (float)node.count;
    WideDecision d;
    d.split = (cheapest_cost >= parent_cost) ? 0u : 1u;                         // ref: BVH.cpp:253-256
    d.axis = cheapest % 3u;
    d.pos = candidate_pos(node, cheapest / 3u, d.axis);
    if (A.naive) { d.split = node.count <= 2u ? 0u : 1u; naive_plane(node, d.axis, d.pos); }   // ref: BVH.cpp:211-223
    uint32_t run = 0;
    for (uint32_t b = 0; b < pieces; ++b) {                                     // lefts before each piece, for the partition
        A.piece_left[(size_t)j * pieces + b] = run;
        run += A.partial[((size_t)j * pieces + b) * kCandidates + cheapest].lc;
    }
    d.n_left = run;
    A.decision[j] = d;
    atomicMax(&A.counters[1], node.depth);                                      // m_max_depth, ref: BVH.cpp:206
}

// the partition's position tables (see subdivide_level); leaves every piece's count of front lefts
__global__ void __launch_bounds__(kBuildThreads) wide_tables(BuildArrays A, uint32_t level_first, uint32_t pieces)
{
    __shared__ uint32_t s_u32[5];
    BuildNode node;
    const Piece q = piece_of(A, level_first, pieces, node);
    const WideDecision d = A.decision[q.j];
    if (d.split == 0u) return;
    const uint32_t* const idx = A.tri_indices + q.first;
    uint32_t my_left = 0;
    for (uint32_t i = q.c0; i < q.c1; ++i) my_left += (axis_of(A.centroid[idx[i]], d.axis) < d.pos) ? 1u : 0u;
    uint32_t piece_total = 0;
    uint32_t L = block_exclusive_scan(my_left, s_u32, &piece_total) + A.piece_left[(size_t)q.j * pieces + q.b];
    uint32_t* const hole_pos = A.sel_a + q.first;
    uint32_t* const tail_left_pos = A.sel_b + q.first;
    uint32_t front_left = 0;
    for (uint32_t p = q.c0; p < q.c1; ++p) {
        const bool is_left = axis_of(A.centroid[idx[p]], d.axis) < d.pos;
        if (p < d.n_left) { if (is_left) ++front_left; else hole_pos[p - L] = p; }
        else if (is_left) tail_left_pos[d.n_left - L - 1u] = p;
        L += is_left ? 1u : 0u;
    }
    front_left = block_reduce_sum(front_left, s_u32);
    if (threadIdx.x == 0) A.piece_front[(size_t)q.j * pieces + q.b] = front_left;
}

__global__ void __launch_bounds__(kBuildThreads) wide_write(BuildArrays A, uint32_t level_first, uint32_t pieces)
{
    __shared__ uint32_t s_u32[5];
    BuildNode node;
    const Piece q = piece_of(A, level_first, pieces, node);
    const WideDecision d = A.decision[q.j];
    if (d.split == 0u) return;
    const uint32_t n = q.n, n_left = d.n_left;
    const uint32_t* const idx = A.tri_indices + q.first;
    uint32_t fronts = 0;
    for (uint32_t b = threadIdx.x; b < pieces; b += kBuildThreads) fronts += A.piece_front[(size_t)q.j * pieces + b];
    fronts = block_reduce_sum(fronts, s_u32);
    if (threadIdx.x == 0) s_u32[4] = fronts;
    __syncthreads();
    const uint32_t holes = n_left - s_u32[4];                                   // rights in the front = lefts in the tail
    __syncthreads();
    uint32_t my_left = 0;
    for (uint32_t i = q.c0; i < q.c1; ++i) my_left += (axis_of(A.centroid[idx[i]], d.axis) < d.pos) ? 1u : 0u;
    uint32_t piece_total = 0;
    uint32_t L = block_exclusive_scan(my_left, s_u32, &piece_total) + A.piece_left[(size_t)q.j * pieces + q.b];
    const uint32_t* const hole_pos = A.sel_a + q.first;
    const uint32_t* const tail_left_pos = A.sel_b + q.first;
    uint32_t* const out = A.scratch_idx + q.first;
    for (uint32_t p = q.c0; p < q.c1; ++p) {
        const bool is_left = axis_of(A.centroid[idx[p]], d.axis) < d.pos;
        L += is_left ? 1u : 0u;                                                 // lefts at positions <= p
        uint32_t value;
        if (p < n_left) {
            value = is_left ? idx[p] : idx[tail_left_pos[p - L]];
        } else if (p + 1u == n || axis_of(A.centroid[idx[p + 1u]], d.axis) < d.pos) {
            const uint32_t k = n_left - L;
            value = k < holes ? idx[hole_pos[k]] : idx[n_left];
        } else {
            value = idx[p + 1u];
        }
        out[p] = value;
    }
}

// new order back into tri_indices; the piece's share of the children's bounds (CalculateNodeBounds in the NEW order, ref: BVH.cpp:350-362)
__global__ void __launch_bounds__(kBuildThreads) wide_finish_piece(BuildArrays A, uint32_t level_first, uint32_t pieces)
{
    __shared__ Bounds s_bounds[4];
    BuildNode node;
    const Piece q = piece_of(A, level_first, pieces, node);
    const WideDecision d = A.decision[q.j];
    if (d.split == 0u) return;
    uint32_t* const idx = A.tri_indices + q.first;
    const uint32_t* const out = A.scratch_idx + q.first;
    for (uint32_t p = q.c0; p < q.c1; ++p) idx[p] = out[p];
    if (d.n_left == 0u || d.n_left == q.n) return;                              // ref: BVH.cpp:346-348 (stays a leaf, in the new order)
    Bounds lb = empty_bounds(), rb = empty_bounds();
    for (uint32_t p = q.c0; p < q.c1; ++p) {
        const uint32_t tri = idx[p];
        const Bounds tb = { A.tri_lo[tri], A.tri_hi[tri] };
        if (p < d.n_left) lb = merge(lb, tb); else rb = merge(rb, tb);
    }
    lb = block_reduce_bounds(lb, s_bounds);
    rb = block_reduce_bounds(rb, s_bounds);
    if (threadIdx.x == 0) A.piece_child[(size_t)q.j * pieces + q.b] = { lb, rb };
}

__global__ void __launch_bounds__(64) wide_children(BuildArrays A, uint32_t level_first, uint32_t pieces)
{
    const uint32_t j = blockIdx.x, node_id = level_first + j;
    if (threadIdx.x != 0) return;
    const BuildNode node = A.nodes[node_id];
    const WideDecision d = A.decision[j];
    if (d.split == 0u || d.n_left == 0u || d.n_left == node.count) return;
    Bounds lb = empty_bounds(), rb = empty_bounds();
    for (uint32_t b = 0; b < pieces; ++b) {
        const WideChild w = A.piece_child[(size_t)j * pieces + b];
        lb = merge(lb, w.lb); rb = merge(rb, w.rb);
    }
    const uint32_t left_id = atomicAdd(&A.counters[0], 2u);
    BuildNode l{}, r{};
    l.lo = lb.lo; l.hi = lb.hi; l.first = node.first; l.count = d.n_left; l.depth = node.depth + 1u;
    r.lo = rb.lo; r.hi = rb.hi; r.first = node.first + d.n_left; r.count = node.count - d.n_left; r.depth = node.depth + 1u;
    A.nodes[left_id] = l; A.nodes[left_id + 1u] = r;
    A.nodes[node_id].left = left_id;
}

// ---- BuildOption_SAHBinned (not in the reference; specification: csrc/host/mesh_bvh.cpp BuildTreeBinned, include/cpugpupt_abi.h) ----------
// One read of a node's triangles per level: each goes into one of 16 centroid bins per axis; a bin keeps a count, the union of its
// triangles' boxes and the bounds of their centroids.  The 45 candidates (axis outer, s = 1..15 inner, left = bins [0, s)), the leaf
// test, the children's boxes and the children's centroid bounds all come from the bins; the triangles are read once more by the
// stable partition.  Every bound is folded as a KEY under the total order on floats in which -0 < +0 (negative floats: all bits
// flipped, the others: the sign bit), with integer atomicMin / atomicMax in LDS: the fold does not depend on the order of the
// operands, down to the sign of a zero, so there is no ordered reduction and no piece-ordered combination anywhere below.  (Float LDS
// min / max treat -0 and +0 as equal: not this order.)
// Level shapes as for the other options: a workgroup / a wavefront / a quarter wavefront per node (binned_level<G>), and for the few
// huge nodes at the top many workgroups per node (binned_wide_*): each bins its piece in LDS and issues one global atomic per word
// of a non-empty bin; one wavefront per node then sweeps, decides, creates the children and prefixes the pieces' left counts.
// The node counter is taken once per wavefront for all the children it creates (binned_sweep), and the tree's depth is the number of
// levels, read off by the driver: no per-node atomic on a single word.
constexpr uint32_t kBins = 16;
constexpr uint32_t kBinWords = 13;                           // count, box lo[3], box hi[3], centroid lo[3], centroid hi[3]
constexpr uint32_t kNodeBinWords = 3 * kBins * kBinWords;    // 624 words = 2496 bytes per node
constexpr uint32_t kBinnedCandidates = 3 * (kBins - 1);

__device__ inline uint32_t order_key(float f)
{
    const uint32_t u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ inline float key_float(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }
// a product that is not below 16 (the last bin's upper edge, an overflowed scale) is bin 15; c >= lo always
__device__ inline uint32_t bin_of(float c, float lo, float scale)
{
    const float f = (c - lo) * scale;
    return f < 16.0f ? (uint32_t)f : kBins - 1u;
}
__device__ inline bool bin_word_is_min(uint32_t field) { return (field >= 1u && field <= 3u) || (field >= 7u && field <= 9u); }

struct BinnedDecision { uint32_t split, axis, s, n_left; float lo, scale; };
struct BinnedArrays {
    Bounds* cbounds;             // per BuildNode: the bounds of its triangles' centroids
    uint32_t* root_keys;         // [12]: root box and centroid bounds as keys, the lower bounds complemented (every word folds with max from 0)
    // wide levels only (index j = node of the level, b = piece of the node)
    uint32_t* gbins;             // [j][kNodeBinWords]
    uint32_t* piece_count;       // [j][b][3 * kBins]: the piece's bin counts
    uint32_t* piece_left;        // [j][b]: lefts before the piece
    BinnedDecision* decision;    // [j]
};
struct BinScale { F3 lo; F3 scale; uint32_t usable; };       // usable: bit a = axis a has a positive centroid extent
__device__ inline BinScale bin_scale(const Bounds& cb)
{
    BinScale q;
    q.lo = cb.lo; q.usable = 0u; q.scale = { 0.0f, 0.0f, 0.0f };
    if (cb.hi.x > cb.lo.x) { q.usable |= 1u; q.scale.x = 16.0f / (cb.hi.x - cb.lo.x); }
    if (cb.hi.y > cb.lo.y) { q.usable |= 2u; q.scale.y = 16.0f / (cb.hi.y - cb.lo.y); }
    if (cb.hi.z > cb.lo.z) { q.usable |= 4u; q.scale.z = 16.0f / (cb.hi.z - cb.lo.z); }
    return q;
}
__device__ inline void bins_clear(uint32_t* bins, uint32_t t, uint32_t stride)
{
    for (uint32_t w = t; w < kNodeBinWords; w += stride) bins[w] = bin_word_is_min(w % kBinWords) ? 0xFFFFFFFFu : 0u;
}
// one triangle into its bin of every usable axis (LDS atomics)
__device__ inline void bins_add(uint32_t* bins, const BuildArrays& A, uint32_t tri, const BinScale& q)
{
    const F3 lo = A.tri_lo[tri], hi = A.tri_hi[tri], c = A.centroid[tri];
    const uint32_t k[12] = { order_key(lo.x), order_key(lo.y), order_key(lo.z), order_key(hi.x), order_key(hi.y), order_key(hi.z),
                             order_key(c.x), order_key(c.y), order_key(c.z), order_key(c.x), order_key(c.y), order_key(c.z) };
#pragma unroll
    for (uint32_t a = 0; a < 3; ++a) {
        if (!(q.usable & (1u << a))) continue;
        uint32_t* const w = bins + (a * kBins + bin_of(axis_of(c, a), axis_of(q.lo, a), axis_of(q.scale, a))) * kBinWords;
        atomicAdd(w, 1u);
#pragma unroll
        for (uint32_t f = 0; f < 12; ++f) {
            if (bin_word_is_min(f + 1u)) atomicMin(w + 1u + f, k[f]); else atomicMax(w + 1u + f, k[f]);
        }
    }
}

struct BinSide { uint32_t count; uint32_t k[12]; };          // k: a bin's twelve bound words
__device__ inline void side_add(BinSide& s, const uint32_t* w)
{
    s.count += w[0];
#pragma unroll
    for (uint32_t f = 0; f < 12; ++f) s.k[f] = bin_word_is_min(f + 1u) ? min(s.k[f], w[1u + f]) : max(s.k[f], w[1u + f]);
}
__device__ inline BinSide side_empty()
{
    BinSide s; s.count = 0u;
#pragma unroll
    for (uint32_t f = 0; f < 12; ++f) s.k[f] = bin_word_is_min(f + 1u) ? 0xFFFFFFFFu : 0u;
    return s;
}
__device__ inline float side_half_area(const BinSide& s)
{
    return half_area({ key_float(s.k[0]), key_float(s.k[1]), key_float(s.k[2]) }, { key_float(s.k[3]), key_float(s.k[4]), key_float(s.k[5]) });
}

// The sweep of one node by the W lanes t = 0 .. W-1 of one wavefront (W = 64 or 16): lane t evaluates candidates t, t + W, ...; the
// cheapest (lowest candidate number among equals = the first strictly cheaper in axis-outer, s-inner order) is found with a butterfly.
// Costs are sums of non-negative products, never NaN, so their bit patterns compare as the floats do.  Every lane returns the
// decision; the lane that evaluated the winner creates the children from its two sides.
template <uint32_t W>
__device__ inline BinnedDecision binned_sweep(const uint32_t* bins, uint32_t t, const BuildArrays& A, const BinnedArrays& Bn, uint32_t node_id,
                                              const BuildNode& node, const BinScale& q)
{
    BinSide best_l = side_empty(), best_r = side_empty();
    uint32_t best_cost = 0x7F800000u, best_c = 0xFFFFFFFFu;                     // +inf, none
    for (uint32_t c = t; c < kBinnedCandidates; c += W) {
        const uint32_t a = c / (kBins - 1u), s = c % (kBins - 1u) + 1u;
        const uint32_t* const w = bins + a * kBins * kBinWords;
        BinSide l = side_empty(), r = side_empty();
        for (uint32_t b = 0; b < s; ++b) side_add(l, w + b * kBinWords);        // an empty bin is the identity
        for (uint32_t b = s; b < kBins; ++b) side_add(r, w + b * kBinWords);
        if (l.count == 0u || r.count == 0u) continue;
        const float cost = (float)l.count * side_half_area(l) + (float)r.count * side_half_area(r);
        if (cost < __uint_as_float(best_cost)) { best_cost = __float_as_uint(cost); best_c = c; best_l = l; best_r = r; }
    }
    uint32_t win_cost = best_cost, win_c = best_c;
    for (int off = (int)W / 2; off > 0; off >>= 1) {
        const uint32_t o_cost = __shfl_xor(win_cost, off, (int)W), o_c = __shfl_xor(win_c, off, (int)W);
        if (o_cost < win_cost || (o_cost == win_cost && o_c < win_c)) { win_cost = o_cost; win_c = o_c; }
    }
    BinnedDecision d{};
    d.split = (__uint_as_float(win_cost) < half_area(node.lo, node.hi) * (float)node.count) ? 1u : 0u;     // ref: BVH.cpp:253; no candidate: +inf
    if (d.split == 0u) return d;
    d.axis = win_c / (kBins - 1u); d.s = win_c % (kBins - 1u) + 1u;
    d.lo = axis_of(q.lo, d.axis); d.scale = axis_of(q.scale, d.axis);
    d.n_left = __shfl(best_l.count, (int)(win_c % W), (int)W);
    if (best_c == win_c) {                                                      // exactly one lane per node: candidate numbers are distinct
        // One returning atomic on the node counter per wavefront, not per node: the lanes in this branch are the winners of the
        // wavefront's splitting nodes (four nodes per wavefront in the deepest levels, where a level creates hundreds of thousands of
        // nodes and a single word takes some 90 returning atomics per microsecond).  Ids inside a level are in no particular order anyway.
        const uint64_t winners = __ballot(1);
        const uint32_t lane = threadIdx.x & 63u;
        uint32_t base = 0;
        if (lane == (uint32_t)__ffsll((long long)winners) - 1u) base = atomicAdd(&A.counters[0], 2u * (uint32_t)__popcll(winners));
        base = __builtin_amdgcn_readfirstlane(base);                            // the first active lane is the one that asked
        const uint32_t left_id = base + 2u * (uint32_t)__popcll(winners & ((1ull << lane) - 1ull));
        BuildNode l{}, r{};
        l.lo = { key_float(best_l.k[0]), key_float(best_l.k[1]), key_float(best_l.k[2]) }; l.hi = { key_float(best_l.k[3]), key_float(best_l.k[4]), key_float(best_l.k[5]) };
        r.lo = { key_float(best_r.k[0]), key_float(best_r.k[1]), key_float(best_r.k[2]) }; r.hi = { key_float(best_r.k[3]), key_float(best_r.k[4]), key_float(best_r.k[5]) };
        l.first = node.first; l.count = best_l.count; l.depth = node.depth + 1u;
        r.first = node.first + best_l.count; r.count = best_r.count; r.depth = node.depth + 1u;
        A.nodes[left_id] = l; A.nodes[left_id + 1u] = r;
        Bn.cbounds[left_id] = { { key_float(best_l.k[6]), key_float(best_l.k[7]), key_float(best_l.k[8]) }, { key_float(best_l.k[9]), key_float(best_l.k[10]), key_float(best_l.k[11]) } };
        Bn.cbounds[left_id + 1u] = { { key_float(best_r.k[6]), key_float(best_r.k[7]), key_float(best_r.k[8]) }, { key_float(best_r.k[9]), key_float(best_r.k[10]), key_float(best_r.k[11]) } };
        A.nodes[node_id].left = left_id;
    }
    return d;
}

// One tile of the stable partition: position p of the node (valid lanes only) goes to the front in the order of the lefts, or behind
// the n_left lefts in the order of the rights.  `run`: lefts before the tile.
template <uint32_t G>
__device__ inline void binned_scatter_tile(const BuildArrays& A, const BinnedDecision& d, const uint32_t* idx, uint32_t* out, uint32_t p, bool valid,
                                           uint32_t& run, uint32_t* s_u32)
{
    const uint32_t tri = valid ? idx[p] : 0u;
    const uint32_t is_left = (valid && bin_of(axis_of(A.centroid[tri], d.axis), d.lo, d.scale) < d.s) ? 1u : 0u;
    uint32_t total = 0;
    const uint32_t lefts_before = run + group_exclusive_scan<G>(is_left, s_u32, &total);
    if (valid) out[is_left ? lefts_before : d.n_left + (p - lefts_before)] = tri;
    run += total;
}

template <uint32_t G>
__global__ void __launch_bounds__(kBuildThreads) binned_level(BuildArrays A, BinnedArrays Bn, uint32_t level_first, uint32_t level_count)
{
    constexpr uint32_t groups = kBuildThreads / G, W = G < 64u ? G : 64u;
    __shared__ uint32_t s_bins[groups * kNodeBinWords];
    __shared__ uint32_t s_u32[5];
    __shared__ BinnedDecision s_decision;

    const uint32_t group = threadIdx.x / G, in_level = blockIdx.x * groups + group, t = threadIdx.x % G;
    if (in_level >= level_count) return;                                       // group-uniform
    const uint32_t node_id = level_first + in_level;
    const BuildNode node = A.nodes[node_id];
    const uint32_t n = node.count;
    if (n == 1u) return;                                                        // one centroid: no axis has an extent, no candidate
    const BinScale q = bin_scale(Bn.cbounds[node_id]);
    if (q.usable == 0u) return;
    uint32_t* const bins = s_bins + group * kNodeBinWords;
    uint32_t* const idx = A.tri_indices + node.first;

    bins_clear(bins, t, G);
    group_sync<G>();
    for (uint32_t i = t; i < n; i += G) bins_add(bins, A, idx[i], q);
    group_sync<G>();

    BinnedDecision d{};
    if (G == kBuildThreads) {                                                   // the first wavefront sweeps
        if (t < W) { d = binned_sweep<W>(bins, t, A, Bn, node_id, node, q); if (t == 0) s_decision = d; }
        __syncthreads();
        d = s_decision;
    } else {
        d = binned_sweep<W>(bins, t, A, Bn, node_id, node, q);
    }
    if (d.split == 0u) return;                                                  // leaf

    uint32_t* const out = A.scratch_idx + node.first;
    uint32_t run = 0;
    for (uint32_t base = 0; base < n; base += G) binned_scatter_tile<G>(A, d, idx, out, base + t, base + t < n, run, s_u32);
    group_sync<G>();                                                            // every read of the old order is done
    for (uint32_t p = t; p < n; p += G) idx[p] = out[p];
}

__device__ inline void binned_piece(const BuildNode& node, uint32_t pieces, uint32_t b, uint32_t& p0, uint32_t& p1)
{
    const uint32_t per_piece = (node.count + pieces - 1u) / pieces;
    p0 = min(b * per_piece, node.count); p1 = min(p0 + per_piece, node.count);
}

__global__ void binned_wide_clear(uint32_t* gbins, uint32_t n_words)
{
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w < n_words) gbins[w] = bin_word_is_min(w % kBinWords) ? 0xFFFFFFFFu : 0u;
}

__global__ void __launch_bounds__(kBuildThreads) binned_wide_hist(BuildArrays A, BinnedArrays Bn, uint32_t level_first, uint32_t pieces)
{
    __shared__ uint32_t s_bins[kNodeBinWords];
    const uint32_t j = blockIdx.x / pieces, b = blockIdx.x - j * pieces;
    const BuildNode node = A.nodes[level_first + j];
    const BinScale q = bin_scale(Bn.cbounds[level_first + j]);
    uint32_t p0, p1;
    binned_piece(node, pieces, b, p0, p1);
    const uint32_t* const idx = A.tri_indices + node.first;
    bins_clear(s_bins, threadIdx.x, kBuildThreads);
    __syncthreads();
    for (uint32_t p = p0 + threadIdx.x; p < p1; p += kBuildThreads) bins_add(s_bins, A, idx[p], q);
    __syncthreads();
    uint32_t* const g = Bn.gbins + (size_t)j * kNodeBinWords;
    for (uint32_t w = threadIdx.x; w < kNodeBinWords; w += kBuildThreads) {
        const uint32_t bin = w / kBinWords, field = w - bin * kBinWords;
        const uint32_t count = s_bins[bin * kBinWords];
        if (field == 0u) Bn.piece_count[((size_t)j * pieces + b) * (3u * kBins) + bin] = count;
        if (count == 0u) continue;                                              // one global atomic per word of a non-empty bin
        if (field == 0u) atomicAdd(g + w, count);
        else if (bin_word_is_min(field)) atomicMin(g + w, s_bins[w]);
        else atomicMax(g + w, s_bins[w]);
    }
}

__global__ void __launch_bounds__(64) binned_wide_decide(BuildArrays A, BinnedArrays Bn, uint32_t level_first, uint32_t pieces)
{
    __shared__ uint32_t s_bins[kNodeBinWords];
    const uint32_t j = blockIdx.x, node_id = level_first + j, t = threadIdx.x;
    const BuildNode node = A.nodes[node_id];
    const BinScale q = bin_scale(Bn.cbounds[node_id]);
    for (uint32_t w = t; w < kNodeBinWords; w += 64u) s_bins[w] = Bn.gbins[(size_t)j * kNodeBinWords + w];
    __syncthreads();
    const BinnedDecision d = binned_sweep<64>(s_bins, t, A, Bn, node_id, node, q);
    if (t == 0) Bn.decision[j] = d;
    if (d.split == 0u) return;
    uint32_t run = 0;                                                           // lefts before each piece, for the partition
    for (uint32_t base = 0; base < pieces; base += 64u) {
        const uint32_t b = base + t;
        uint32_t lefts = 0;
        if (b < pieces) for (uint32_t k = 0; k < d.s; ++k) lefts += Bn.piece_count[((size_t)j * pieces + b) * (3u * kBins) + d.axis * kBins + k];
        uint32_t total = 0;
        const uint32_t before = group_exclusive_scan<64>(lefts, nullptr, &total);
        if (b < pieces) Bn.piece_left[(size_t)j * pieces + b] = run + before;
        run += total;
    }
}

__global__ void __launch_bounds__(kBuildThreads) binned_wide_scatter(BuildArrays A, BinnedArrays Bn, uint32_t level_first, uint32_t pieces)
{
    __shared__ uint32_t s_u32[5];
    const uint32_t j = blockIdx.x / pieces, b = blockIdx.x - j * pieces;
    const BinnedDecision d = Bn.decision[j];
    if (d.split == 0u) return;
    const BuildNode node = A.nodes[level_first + j];
    uint32_t p0, p1;
    binned_piece(node, pieces, b, p0, p1);
    const uint32_t* const idx = A.tri_indices + node.first;
    uint32_t* const out = A.scratch_idx + node.first;
    uint32_t run = Bn.piece_left[(size_t)j * pieces + b];
    for (uint32_t base = p0; base < p1; base += kBuildThreads) binned_scatter_tile<kBuildThreads>(A, d, idx, out, base + threadIdx.x, base + threadIdx.x < p1, run, s_u32);
}

__global__ void __launch_bounds__(kBuildThreads) binned_wide_copy(BuildArrays A, BinnedArrays Bn, uint32_t level_first, uint32_t pieces)
{
    const uint32_t j = blockIdx.x / pieces, b = blockIdx.x - j * pieces;
    if (Bn.decision[j].split == 0u) return;
    const BuildNode node = A.nodes[level_first + j];
    uint32_t p0, p1;
    binned_piece(node, pieces, b, p0, p1);
    for (uint32_t p = p0 + threadIdx.x; p < p1; p += kBuildThreads) A.tri_indices[node.first + p] = A.scratch_idx[node.first + p];
}

// root box and centroid bounds over all triangles (any order): per thread in registers, per wavefront with shuffles, then one global
// atomicMax per word and wavefront on root_keys (zeroed; the lower bounds are complemented so that every word folds with max)
__global__ void __launch_bounds__(kBuildThreads) binned_root_fold(BuildArrays A, BinnedArrays Bn, uint32_t n)
{
    uint32_t k[12];
#pragma unroll
    for (uint32_t f = 0; f < 12; ++f) k[f] = 0u;
    for (uint32_t i = blockIdx.x * kBuildThreads + threadIdx.x; i < n; i += gridDim.x * kBuildThreads) {
        const F3 lo = A.tri_lo[i], hi = A.tri_hi[i], c = A.centroid[i];
        const uint32_t v[12] = { ~order_key(lo.x), ~order_key(lo.y), ~order_key(lo.z), order_key(hi.x), order_key(hi.y), order_key(hi.z),
                                 ~order_key(c.x), ~order_key(c.y), ~order_key(c.z), order_key(c.x), order_key(c.y), order_key(c.z) };
#pragma unroll
        for (uint32_t f = 0; f < 12; ++f) k[f] = max(k[f], v[f]);
    }
#pragma unroll
    for (uint32_t f = 0; f < 12; ++f) {
        for (int off = 32; off > 0; off >>= 1) k[f] = max(k[f], (uint32_t)__shfl_xor(k[f], off, 64));
        if ((threadIdx.x & 63u) == 0u) atomicMax(&Bn.root_keys[f], k[f]);
    }
}
__global__ void binned_root_node(BuildArrays A, BinnedArrays Bn, uint32_t n)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint32_t* const k = Bn.root_keys;
    BuildNode root{};
    root.lo = { key_float(~k[0]), key_float(~k[1]), key_float(~k[2]) }; root.hi = { key_float(k[3]), key_float(k[4]), key_float(k[5]) };
    root.first = 0; root.count = n; root.depth = 0; root.rank = 0; root.new_id = 0;
    A.nodes[0] = root;
    Bn.cbounds[0] = { { key_float(~k[6]), key_float(~k[7]), key_float(~k[8]) }, { key_float(k[9]), key_float(k[10]), key_float(k[11]) } };
    A.counters[0] = 1u; A.counters[1] = 0u;
}

// ---- renumbering into the reference's allocation order --------------------------------------------------------------------------
__global__ void count_splits_level(BuildNode* nodes, uint32_t level_first, uint32_t level_count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= level_count) return;
    BuildNode& n = nodes[level_first + i];
    n.splits = n.left ? 1u + nodes[n.left].splits + nodes[n.left + 1u].splits : 0u;
}
__global__ void assign_ids_level(BuildNode* nodes, uint32_t level_first, uint32_t level_count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= level_count) return;
    const BuildNode& n = nodes[level_first + i];
    if (!n.left) return;
    BuildNode& l = nodes[n.left]; BuildNode& r = nodes[n.left + 1u];
    l.new_id = 1u + 2u * n.rank; r.new_id = l.new_id + 1u;       // children of the k-th splitting node: 2k+1, 2k+2
    l.rank = n.rank + 1u;                                         // preorder: the left subtree's splits come first
    r.rank = n.rank + 1u + l.splits;
}
__global__ void emit_nodes(const BuildNode* nodes, uint32_t n_nodes, cgpt_bvh_node* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    const BuildNode& n = nodes[i];
    cgpt_bvh_node o;
    o.aabb_min[0] = n.lo.x; o.aabb_min[1] = n.lo.y; o.aabb_min[2] = n.lo.z;
    o.aabb_max[0] = n.hi.x; o.aabb_max[1] = n.hi.y; o.aabb_max[2] = n.hi.z;
    if (n.left) { o.left_first = nodes[n.left].new_id; o.prim_count = 0u; }
    else { o.left_first = n.first; o.prim_count = n.count; }
    out[n.new_id] = o;
}

// root bounds (CalculateNodeBounds over all triangles in index order, ref: BVH.cpp:43,188-202): one block, ordered
__global__ void __launch_bounds__(kBuildThreads) root_bounds(BuildArrays A, uint32_t n)
{
    __shared__ Bounds s_bounds[4];
    const uint32_t chunk = (n + kBuildThreads - 1) / kBuildThreads;
    const uint32_t c0 = min(threadIdx.x * chunk, n), c1 = min(c0 + chunk, n);
    Bounds b = empty_bounds();
    for (uint32_t i = c0; i < c1; ++i) { const uint32_t tri = A.tri_indices[i]; b = merge(b, Bounds{ A.tri_lo[tri], A.tri_hi[tri] }); }   // index order (a Rebuild starts from a permutation)
    b = block_reduce_bounds(b, s_bounds);
    if (threadIdx.x == 0) {
        BuildNode root{};
        root.lo = b.lo; root.hi = b.hi; root.first = 0; root.count = n; root.depth = 0; root.rank = 0; root.new_id = 0;
        A.nodes[0] = root;
        A.counters[0] = 1u; A.counters[1] = 0u;
    }
}

// ---- cgpt_scene_rebuild_mesh: the builder fed from the device scene, and its tree written as the scene's own records (device_scene.h;
//      the names of the records: rebuild_layout.h) ------------------------------------------------------------------------------------
// report words the host reads back: {flags, root lo.xyz, root hi.xyz, top slots used, then the rank that took each used top slot}
constexpr uint32_t kReportRanks = 8;
constexpr uint32_t kTopScan = 2u * kTopRecords;              // the K-th splitting node of a level-ordered array sits at position 2 (K - 1) at most
constexpr uint32_t kFlagDomain = 1u;                         // a position that is not finite or exceeds 1e30 in magnitude (the binned build's domain)
constexpr uint32_t kFlagSlot = 2u;                           // a leaf slot that names no triangle of the mesh
constexpr uint32_t kFlagEmit = 4u;                           // an emit kernel met a node or an index that the checks in front of the first write rule out:
                                                             // it skipped the write, and the host drops the half-written scene

// The front end: index i is leaf slot i and triangle i at once.  Slot i's tri_leaf tail gives the Rebuild's starting order; triangle i's
// box and centroid come from tri_orig with prepare_triangles' arithmetic.  Both reads are consecutive across a wave: no gather.
__global__ void __launch_bounds__(256) prepare_from_scene(const float4* __restrict__ tri_leaf, const float4* __restrict__ tri_orig, uint32_t leaf_base, uint32_t tri_base,
                                                          uint32_t n, F3* lo, F3* hi, F3* centroid, uint32_t* idx, uint32_t* flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t t = __float_as_uint(tri_leaf[3 * (size_t)(leaf_base + i) + 2].z);
    uint32_t flag = 0u;
    if (t >= n) { flag |= kFlagSlot; t = 0u; }                // validated at upload; the kernels index with it
    idx[i] = t;
    const float4* o = tri_orig + 3 * (size_t)(tri_base + i);
    const float4 a = o[0], b = o[1], c = o[2];
    const F3 p0 = { a.x, a.y, a.z }, p1 = { b.x, b.y, b.z }, p2 = { c.x, c.y, c.z };
    lo[i] = f3min(f3min(p0, p1), p2);
    hi[i] = f3max(f3max(p0, p1), p2);
    centroid[i] = { ((p0.x + p1.x) + p2.x) * 0.3333f, ((p0.y + p1.y) + p2.y) * 0.3333f, ((p0.z + p1.z) + p2.z) * 0.3333f };
    const float m = fmaxf(fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(b.x))), fmaxf(fmaxf(fabsf(b.y), fabsf(b.z)), fmaxf(fmaxf(fabsf(c.x), fabsf(c.y)), fabsf(c.z))));
    const bool nan = a.x != a.x || a.y != a.y || a.z != a.z || b.x != b.x || b.y != b.y || b.z != b.z || c.x != c.x || c.y != c.y || c.z != c.z;   // fmaxf drops a NaN
    if (nan || !(m <= 1e30f)) flag |= kFlagDomain;
    if (flag) atomicOr(flags, flag);
}

// The first K splitting nodes of the level-ordered array take the mesh's top slots (rebuild_layout.h).  One block over the first kTopScan
// nodes, a thread a run of consecutive nodes, so the prefix of the splitting flags is the array's order.  top_name[i] = the slot of node
// i, 0xFFFFFFFF for every other node below kTopScan; the report gets the ranks in slot order and the root's bounds.
__global__ void __launch_bounds__(kBuildThreads) assign_top_slots(const BuildNode* __restrict__ nodes, uint32_t n_nodes, const uint32_t* __restrict__ top_slots, uint32_t K,
                                                                  uint32_t* top_name, uint32_t* report)
{
    __shared__ uint32_t s_u32[5];
    constexpr uint32_t per = (kTopScan + kBuildThreads - 1u) / kBuildThreads;
    const uint32_t i0 = threadIdx.x * per;
    uint32_t mine = 0;
    for (uint32_t k = 0; k < per; ++k) { const uint32_t i = i0 + k; if (i < kTopScan && i < n_nodes && nodes[i].left != 0u) ++mine; }
    uint32_t total = 0;
    uint32_t j = block_exclusive_scan(mine, s_u32, &total);
    for (uint32_t k = 0; k < per; ++k) {
        const uint32_t i = i0 + k;
        if (i >= kTopScan) break;
        uint32_t name = 0xFFFFFFFFu;
        if (i < n_nodes && nodes[i].left != 0u) {
            if (j < K) { name = top_slots[j]; report[kReportRanks + j] = nodes[i].rank; }
            ++j;
        }
        top_name[i] = name;
    }
    if (threadIdx.x == 0) {
        const BuildNode root = nodes[0];
        report[1] = __float_as_uint(root.lo.x); report[2] = __float_as_uint(root.lo.y); report[3] = __float_as_uint(root.lo.z);
        report[4] = __float_as_uint(root.hi.x); report[5] = __float_as_uint(root.hi.y); report[6] = __float_as_uint(root.hi.z);
        report[7] = min(total, K);
    }
}

// One thread per leaf slot: PackLeafTri (scene_layout.h) of the triangle the new order puts there, last_in_leaf cleared -- emit_pair_records
// sets it on every leaf's last slot.  The one gather of the call: neighbouring slots name scattered tri_orig records.
__global__ void __launch_bounds__(256) emit_leaf_triangles(const uint32_t* __restrict__ idx, const float4* __restrict__ tri_orig, float4* __restrict__ tri_leaf,
                                                           uint32_t leaf_base, uint32_t tri_base, uint32_t n, uint32_t* flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = idx[i];
    if (t >= n) { atomicOr(flags, kFlagEmit); return; }
    const float4* o = tri_orig + 3 * (size_t)(tri_base + t);
    const float4 a = o[0], b = o[1], c = o[2];
    const float e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z;            // ref: Primitives.cpp:9
    const float e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;            // ref: Primitives.cpp:10
    float4* leaf = tri_leaf + 3 * (size_t)(leaf_base + i);
    leaf[0] = make_float4(a.x, a.y, a.z, e1x);
    leaf[1] = make_float4(e1y, e1z, e2x, e2y);
    leaf[2] = make_float4(0.0f, e2z, __uint_as_float(t), __uint_as_float(0u));
}

__device__ inline uint32_t record_name(const BuildNode& n, uint32_t id, const uint32_t* __restrict__ top_name, uint32_t span_base)
{
    if (id < kTopScan) { const uint32_t slot = top_name[id]; if (slot != 0xFFFFFFFFu) return slot; }
    return span_base + n.rank;
}

// One thread per node of the builder's array.  A leaf ends its slot range (last_in_leaf).  A splitting node writes its 64-byte record --
// the two children's bounds straight from their BuildNodes, interleaved per component, and their traversal codes -- and its name into
// the mesh's slice of refit_levels: the children of level L are level L + 1 and were allocated in pairs, so (left - 1) / 2 is the node's
// place among the splitting nodes in level order, depth by depth (rebuild_layout.h: level_offsets).
__global__ void __launch_bounds__(256) emit_pair_records(const BuildNode* __restrict__ nodes, uint32_t n_nodes, const uint32_t* __restrict__ top_name, uint32_t span_base,
                                                         uint32_t span_room, uint32_t leaf_base, uint32_t n_tris, float4* __restrict__ node_pairs,
                                                         float4* __restrict__ tri_leaf, uint32_t* __restrict__ levels, uint32_t* flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    const BuildNode n = nodes[i];
    if (n.left == 0u) {
        if (n.count == 0u || (uint64_t)n.first + n.count > n_tris) { atomicOr(flags, kFlagEmit); return; }
        reinterpret_cast<uint32_t*>(tri_leaf + 3 * (size_t)(leaf_base + n.first + n.count - 1u) + 2)[3] = 1u;
        return;
    }
    if (n.left + 1u >= n_nodes || n.rank >= span_room) { atomicOr(flags, kFlagEmit); return; }
    const BuildNode l = nodes[n.left], r = nodes[n.left + 1u];
    if ((l.left != 0u && l.rank >= span_room) || (r.left != 0u && r.rank >= span_room)) { atomicOr(flags, kFlagEmit); return; }
    const uint32_t name = record_name(n, i, top_name, span_base);
    const uint32_t lc = l.left ? record_name(l, n.left, top_name, span_base) : (kLeafBit | (leaf_base + l.first));
    const uint32_t rc = r.left ? record_name(r, n.left + 1u, top_name, span_base) : (kLeafBit | (leaf_base + r.first));
    float4* rec = node_pairs + 4 * (size_t)name;
    rec[0] = make_float4(l.lo.x, r.lo.x, l.lo.y, r.lo.y);                     // device_scene.h: node_pairs
    rec[1] = make_float4(l.lo.z, r.lo.z, l.hi.x, r.hi.x);
    rec[2] = make_float4(l.hi.y, r.hi.y, l.hi.z, r.hi.z);
    rec[3] = make_float4(0.0f, 0.0f, __uint_as_float(lc), __uint_as_float(rc));
    levels[(n.left - 1u) / 2u] = name;
}

// Morph targets in leaf-slot order (MorphBuffers): the rebuild permutes the slots.  from[i] = the old slot of the triangle now at slot i,
// and the triangle's slot_of_tri entry moves to i; then every set's nine planes are gathered through `from` into a scratch and copied back.
__global__ void __launch_bounds__(256) morph_slot_map(const uint32_t* __restrict__ idx, uint32_t* slot_of_tri, uint32_t* from, uint32_t n, uint32_t* flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = idx[i];
    if (t >= n) { from[i] = i; atomicOr(flags, kFlagEmit); return; }
    const uint32_t old = slot_of_tri[t];                      // every thread reads and writes its own triangle's entry only
    if (old >= n) atomicOr(flags, kFlagEmit);
    from[i] = old < n ? old : i;
    slot_of_tri[t] = i;
}
__global__ void __launch_bounds__(256) morph_gather_set(const float2* __restrict__ set, const uint32_t* __restrict__ from, float2* __restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = from[i];
#pragma unroll
    for (uint32_t p = 0; p < 9u; ++p) out[(size_t)p * n + i] = set[(size_t)p * n + s];
}

}  // namespace

float HostTriangleArea(const cgpt_triangle& t)                                // Heron, ref: Primitives.cpp:270-278 (also refit.hip)
{
    auto len = [](const float a[3], const float b[3]) { const float x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2]; return sqrtf(x * x + y * y + z * z); };
    const float a = len(t.v1.pos, t.v0.pos), b = len(t.v2.pos, t.v0.pos), c = len(t.v2.pos, t.v1.pos);
    const float s = (a + b + c) / 2.0f;
    return sqrtf(s * (s - a) * (s - b) * (s - c));
}

}  // namespace cgpt

using namespace cgpt;

// ---- the driver in three parts: the work arrays, the level loop with the renumbering passes, and an emit.  cgpt_bvh_build_ex emits the
//      reference's node array to the host; cgpt_scene_rebuild_mesh (below) writes the device scene's own records instead ------------------
struct BuildWork {
    DevBuf<F3> lo, hi, c;
    DevBuf<uint32_t> idx, scratch, sa, sb, counters;
    DevBuf<BuildNode> nodes;
    DevBuf<WidePartial> partial; DevBuf<WideDecision> decision; DevBuf<uint32_t> piece_left, piece_front; DevBuf<WideChild> piece_child;
    DevBuf<Bounds> cbounds; DevBuf<uint32_t> root_keys, gbins, piece_count; DevBuf<BinnedDecision> bdecision;
    BuildArrays A{};
    BinnedArrays Bn{};
    uint32_t n_tris = 0, build_option = 0;
    bool binned = false;
    uint32_t quarter_tris = 32;                                               // ... and one quarter wavefront per node
    uint32_t wave_tris = 2048;                                                // average triangles per node up to which a level runs one wavefront per node
    uint32_t piece_tris = 512;                                                // average triangles per piece below which a level goes to one workgroup per node
    std::vector<uint32_t> level_first;                                        // breadth-first ranges of the levels; after the loop closed by n_nodes
    uint32_t counters_h[2] = { 0, 0 };
    uint32_t n_nodes = 0;
};

static int AllocBuildWork(cgpt_ctx* ctx, uint32_t n_tris, uint32_t build_option, BuildWork& w)
{
    w.n_tris = n_tris; w.build_option = build_option; w.binned = build_option == CGPT_BUILD_SAH_BINNED;
    const bool binned = w.binned;
    const uint32_t max_nodes = 2u * n_tris - 1u;
    HIP_TRY(ctx, w.lo.Alloc(n_tris));
    HIP_TRY(ctx, w.hi.Alloc(n_tris));
    HIP_TRY(ctx, w.c.Alloc(n_tris));
    HIP_TRY(ctx, w.idx.Alloc(n_tris)); HIP_TRY(ctx, w.scratch.Alloc(n_tris));
    if (!binned) { HIP_TRY(ctx, w.sa.Alloc(n_tris)); HIP_TRY(ctx, w.sb.Alloc(n_tris)); }
    HIP_TRY(ctx, w.counters.Alloc(2));
    HIP_TRY(ctx, w.nodes.Alloc(max_nodes));
    HIP_TRY(ctx, w.piece_left.Alloc(kWideBlocks));
    if (!binned) {
        HIP_TRY(ctx, w.partial.Alloc((size_t)kWideBlocks * kCandidates));
        HIP_TRY(ctx, w.decision.Alloc(kWideBlocks));
        HIP_TRY(ctx, w.piece_front.Alloc(kWideBlocks));
        HIP_TRY(ctx, w.piece_child.Alloc(kWideBlocks));
    } else {
        HIP_TRY(ctx, w.cbounds.Alloc(max_nodes));
        HIP_TRY(ctx, w.root_keys.Alloc(12));
        HIP_TRY(ctx, w.gbins.Alloc((size_t)kWideBlocks * kNodeBinWords));
        HIP_TRY(ctx, w.piece_count.Alloc((size_t)kWideBlocks * 3 * kBins));
        HIP_TRY(ctx, w.bdecision.Alloc(kWideBlocks));
    }
    if (const char* e = getenv("CGPT_BVH_WAVE_TRIS")) w.wave_tris = (uint32_t)std::max(0l, strtol(e, nullptr, 10));     // tests: 0 = workgroups only
    if (const char* e = getenv("CGPT_BVH_QUARTER_TRIS")) w.quarter_tris = (uint32_t)std::max(0l, strtol(e, nullptr, 10));
    if (const char* e = getenv("CGPT_BVH_PIECE_TRIS")) w.piece_tris = (uint32_t)std::max(1l, strtol(e, nullptr, 10));   // tests: the wide path on small meshes
    BuildArrays& A = w.A; BinnedArrays& Bn = w.Bn;
    A.naive = build_option == CGPT_BUILD_NAIVE_SPLIT ? 1u : 0u;
    A.tri_lo = w.lo.p; A.tri_hi = w.hi.p; A.centroid = w.c.p; A.tri_indices = w.idx.p; A.scratch_idx = w.scratch.p; A.sel_a = w.sa.p; A.sel_b = w.sb.p;
    A.nodes = w.nodes.p; A.counters = w.counters.p;
    A.partial = w.partial.p; A.decision = w.decision.p; A.piece_left = w.piece_left.p; A.piece_front = w.piece_front.p; A.piece_child = w.piece_child.p;
    Bn.cbounds = w.cbounds.p; Bn.root_keys = w.root_keys.p; Bn.gbins = w.gbins.p; Bn.piece_count = w.piece_count.p; Bn.piece_left = w.piece_left.p; Bn.decision = w.bdecision.p;
    return CGPT_OK;
}

// The root's bounds, the level loop and the renumbering passes over triangles prepared in w (bounds, centroids, starting order).
static int RunBuildLevels(cgpt_ctx* ctx, BuildWork& w, hipStream_t stream)
{
    const uint32_t n_tris = w.n_tris, build_option = w.build_option;
    const bool binned = w.binned;
    const uint32_t quarter_tris = w.quarter_tris, wave_tris = w.wave_tris, piece_tris = w.piece_tris;
    BuildArrays& A = w.A; BinnedArrays& Bn = w.Bn;
    DevBuf<BuildNode>& d_nodes = w.nodes; DevBuf<uint32_t>& d_counters = w.counters; DevBuf<uint32_t>& d_root_keys = w.root_keys; DevBuf<uint32_t>& d_gbins = w.gbins;
    std::vector<uint32_t>& level_first = w.level_first;
    uint32_t (&counters)[2] = w.counters_h;
    level_first.clear(); counters[0] = counters[1] = 0;
    if (binned) {
        HIP_TRY(ctx, hipMemsetAsync(d_root_keys.p, 0, 12 * 4, stream));
        hipLaunchKernelGGL(binned_root_fold, dim3(std::min(1024u, (n_tris + kBuildThreads - 1u) / kBuildThreads)), dim3(kBuildThreads), 0, stream, A, Bn, n_tris);
        hipLaunchKernelGGL(binned_root_node, dim3(1), dim3(1), 0, stream, A, Bn, n_tris);
    } else {
        hipLaunchKernelGGL(root_bounds, dim3(1), dim3(kBuildThreads), 0, stream, A, n_tris);
    }
    // SAH split primitives (ref: BVH.cpp:260-297): cheapest_cost stays 1e30 because the loop never assigns it (SURVEY A-5), so
    // "cheapest_cost >= parent_cost" ends the build at the root whenever the root's cost is an ordinary number.  A root cost
    // of NaN or beyond 1e30 (bounds near the float limit) would take the reference into Split with the last candidate plane:
    // that corner is left to the host build.
    bool root_only = false;
    if (build_option == CGPT_BUILD_SAH_SPLIT_PRIMITIVES) {
        BuildNode root{};
        HIP_TRY(ctx, hipMemcpyAsync(&root, d_nodes.p, sizeof(root), hipMemcpyDeviceToHost, stream));
        HIP_TRY(ctx, hipStreamSynchronize(stream));
        const float ex = root.hi.x - root.lo.x, ey = root.hi.y - root.lo.y, ez = root.hi.z - root.lo.z;
        const float parent_cost = (ex * ey + ey * ez + ez * ex) * (float)n_tris;
        if (!(1e30f >= parent_cost)) return CtxFail(ctx, CGPT_ERR_UNSUPPORTED, "cgpt_bvh_build: SAH-split-primitives on bounds whose cost is not below 1e30: use the host build");
        root_only = true;
    }

    // level by level: the nodes created while level L is processed are exactly level L + 1
    uint32_t first = 0, count = 1;
    if (root_only) { level_first.push_back(0); counters[0] = 1; counters[1] = 0; count = 0; }
    while (count > 0) {
        level_first.push_back(first);
        // few, big nodes: pieces of ~piece_tris triangles or more, at most kWideBlocks of them per level
        const uint32_t pieces = std::min(kWideBlocks / std::min(count, kWideBlocks), std::max(1u, n_tris / count / piece_tris));
        if (binned) {
            if (count <= kWideBlocks && pieces >= 2u) {
                const dim3 grid(count * pieces), per_node(count), block(kBuildThreads);
                hipLaunchKernelGGL(binned_wide_clear, dim3((count * kNodeBinWords + 255u) / 256u), dim3(256), 0, stream, d_gbins.p, count * kNodeBinWords);
                hipLaunchKernelGGL(binned_wide_hist, grid, block, 0, stream, A, Bn, first, pieces);
                hipLaunchKernelGGL(binned_wide_decide, per_node, dim3(64), 0, stream, A, Bn, first, pieces);
                hipLaunchKernelGGL(binned_wide_scatter, grid, block, 0, stream, A, Bn, first, pieces);
                hipLaunchKernelGGL(binned_wide_copy, grid, block, 0, stream, A, Bn, first, pieces);
            } else if ((uint64_t)count * wave_tris < n_tris) {
                hipLaunchKernelGGL(binned_level<kBuildThreads>, dim3(count), dim3(kBuildThreads), 0, stream, A, Bn, first, count);
            } else if ((uint64_t)count * quarter_tris < n_tris) {
                hipLaunchKernelGGL(binned_level<64>, dim3((count + 3u) / 4u), dim3(kBuildThreads), 0, stream, A, Bn, first, count);
            } else {
                hipLaunchKernelGGL(binned_level<16>, dim3((count + 15u) / 16u), dim3(kBuildThreads), 0, stream, A, Bn, first, count);
            }
        } else if (count <= kWideBlocks && pieces >= 2u) {
            const dim3 grid(count * pieces), per_node(count), block(kBuildThreads);
            hipLaunchKernelGGL(wide_sah_partial, grid, block, 0, stream, A, first, pieces);
            hipLaunchKernelGGL(wide_decide, per_node, dim3(64), 0, stream, A, first, pieces);
            hipLaunchKernelGGL(wide_tables, grid, block, 0, stream, A, first, pieces);
            hipLaunchKernelGGL(wide_write, grid, block, 0, stream, A, first, pieces);
            hipLaunchKernelGGL(wide_finish_piece, grid, block, 0, stream, A, first, pieces);
            hipLaunchKernelGGL(wide_children, per_node, dim3(64), 0, stream, A, first, pieces);
        } else if ((uint64_t)count * wave_tris < n_tris) {                  // big nodes on average: a workgroup per node
            hipLaunchKernelGGL(subdivide_level<kBuildThreads>, dim3(count), dim3(kBuildThreads), 0, stream, A, first, count);
        } else if ((uint64_t)count * quarter_tris < n_tris) {               // the deep levels: a wavefront per node
            hipLaunchKernelGGL(subdivide_level<64>, dim3((count + 3u) / 4u), dim3(kBuildThreads), 0, stream, A, first, count);
        } else {                                                          // the deepest: a handful of triangles per node, 16 lanes each
            hipLaunchKernelGGL(subdivide_level<16>, dim3((count + 15u) / 16u), dim3(kBuildThreads), 0, stream, A, first, count);
        }
        HIP_TRY(ctx, hipMemcpyAsync(counters, d_counters.p, sizeof(counters), hipMemcpyDeviceToHost, stream));
        HIP_TRY(ctx, hipStreamSynchronize(stream));
        first += count;
        count = counters[0] - first;
        if (level_first.size() > 4096) return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_bvh_build: tree deeper than 4096 levels");
    }
    const uint32_t n_nodes = w.n_nodes = counters[0];
    if (n_nodes == 0u || n_nodes > 2u * n_tris - 1u) return CtxFail(ctx, CGPT_ERR_HIP, "cgpt_bvh_build: the node counter reads %u for %u triangles", n_nodes, n_tris);
    level_first.push_back(n_nodes);
    // splitting-node counts bottom-up, preorder ranks and final ids top-down
    for (size_t l = level_first.size() - 1; l-- > 0;) {
        const uint32_t c = level_first[l + 1] - level_first[l];
        hipLaunchKernelGGL(count_splits_level, dim3((c + 255u) / 256u), dim3(256), 0, stream, d_nodes.p, level_first[l], c);
    }
    for (size_t l = 0; l + 1 < level_first.size(); ++l) {
        const uint32_t c = level_first[l + 1] - level_first[l];
        hipLaunchKernelGGL(assign_ids_level, dim3((c + 255u) / 256u), dim3(256), 0, stream, d_nodes.p, level_first[l], c);
    }
    return CGPT_OK;
}

static int BuildOnDevice(cgpt_ctx* ctx, const cgpt_triangle* triangles, uint32_t n_tris, uint32_t build_option, const uint32_t* initial_tri_indices,
                         cgpt_bvh_node* nodes_out, uint32_t* n_nodes_out, uint32_t* tri_indices_out, uint32_t* max_depth_out, float* total_area_out);

extern "C" int cgpt_bvh_build_ex(cgpt_ctx* ctx, const cgpt_triangle* triangles, uint32_t n_tris, uint32_t build_option, const uint32_t* initial_tri_indices,
                                 cgpt_bvh_node* nodes_out, uint32_t* n_nodes_out, uint32_t* tri_indices_out, uint32_t* max_depth_out, float* total_area_out)
{
    if (!ctx) return CGPT_ERR_INVALID;
    cgpt_ctx* const first = GroupFirstMemberOrNull(ctx);                       // a multi-device context builds on its first device
    cgpt_ctx* const target = first ? first : ctx;
    const int rc = Guarded(target, "cgpt_bvh_build", [&] {                    // host vectors
        return BuildOnDevice(target, triangles, n_tris, build_option, initial_tri_indices, nodes_out, n_nodes_out, tri_indices_out, max_depth_out, total_area_out);
    });
    return first ? GroupForwarded(ctx, rc) : rc;
}

extern "C" int cgpt_bvh_build(cgpt_ctx* ctx, const cgpt_triangle* triangles, uint32_t n_tris, cgpt_bvh_node* nodes_out, uint32_t* n_nodes_out,
                              uint32_t* tri_indices_out, uint32_t* max_depth_out, float* total_area_out)
{
    return cgpt_bvh_build_ex(ctx, triangles, n_tris, CGPT_BUILD_SAH_SPLIT_INTERVALS, nullptr, nodes_out, n_nodes_out, tri_indices_out, max_depth_out, total_area_out);
}

static int BuildOnDevice(cgpt_ctx* ctx, const cgpt_triangle* triangles, uint32_t n_tris, uint32_t build_option, const uint32_t* initial_tri_indices,
                         cgpt_bvh_node* nodes_out, uint32_t* n_nodes_out, uint32_t* tri_indices_out, uint32_t* max_depth_out, float* total_area_out)
{
    if (!triangles || n_tris == 0 || !nodes_out || !n_nodes_out || !tri_indices_out || !max_depth_out || !total_area_out)
        return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_bvh_build: null argument or empty mesh");
    if (n_tris > 0x3FFFFFFFu) return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_bvh_build: too many triangles");
    if (build_option > CGPT_BUILD_SAH_BINNED) return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_bvh_build: unknown build option %u", build_option);
    const bool binned = build_option == CGPT_BUILD_SAH_BINNED;
    if (binned) {                                                             // its input domain (include/cpugpupt_abi.h): the bin index must stay defined
        for (uint32_t i = 0; i < n_tris; ++i) {
            const cgpt_vertex* const v[3] = { &triangles[i].v0, &triangles[i].v1, &triangles[i].v2 };
            for (int k = 0; k < 3; ++k)
                for (int a = 0; a < 3; ++a)
                    if (!(fabsf(v[k]->pos[a]) <= 1e30f))
                        return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_bvh_build: the binned build needs finite positions of magnitude <= 1e30 (triangle %u)", i);
        }
    }
    if (initial_tri_indices) {                                                // a Rebuild's starting order must be a permutation: the kernels index with it
        std::vector<uint8_t> seen(n_tris, 0);
        for (uint32_t i = 0; i < n_tris; ++i) {
            const uint32_t t = initial_tri_indices[i];
            if (t >= n_tris || seen[t]) return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_bvh_build: initial_tri_indices[%u] = %u: not a permutation of 0..%u", i, t, n_tris - 1u);
            seen[t] = 1;
        }
    }
    hipStream_t stream = CtxStream(ctx);
    if (hipSetDevice(CtxDevice(ctx)) != hipSuccess) return CtxFail(ctx, CGPT_ERR_HIP, "cgpt_bvh_build: hipSetDevice failed");

    DevBuf<cgpt_triangle> d_tris; DevBuf<cgpt_bvh_node> d_out;
    BuildWork w;
    int rc = AllocBuildWork(ctx, n_tris, build_option, w);
    if (rc != CGPT_OK) return rc;
    HIP_TRY(ctx, d_tris.Alloc(n_tris));
    HIP_TRY(ctx, d_out.Alloc(2u * n_tris - 1u));
    HIP_TRY(ctx, hipMemcpyAsync(d_tris.p, triangles, (size_t)n_tris * sizeof(cgpt_triangle), hipMemcpyHostToDevice, stream));
    if (initial_tri_indices) HIP_TRY(ctx, hipMemcpyAsync(w.idx.p, initial_tri_indices, (size_t)n_tris * 4, hipMemcpyHostToDevice, stream));   // Rebuild: the current order
    hipLaunchKernelGGL(prepare_triangles, dim3((n_tris + 255u) / 256u), dim3(256), 0, stream, d_tris.p, n_tris, w.lo.p, w.hi.p, w.c.p, w.idx.p, initial_tri_indices ? 0u : 1u);
    rc = RunBuildLevels(ctx, w, stream);
    if (rc != CGPT_OK) return rc;
    const uint32_t n_nodes = w.n_nodes;
    const std::vector<uint32_t>& level_first = w.level_first;
    const uint32_t* const counters = w.counters_h;
    DevBuf<BuildNode>& d_nodes = w.nodes; DevBuf<uint32_t>& d_idx = w.idx;
    hipLaunchKernelGGL(emit_nodes, dim3((n_nodes + 255u) / 256u), dim3(256), 0, stream, d_nodes.p, n_nodes, d_out.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(nodes_out, d_out.p, (size_t)n_nodes * sizeof(cgpt_bvh_node), hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipMemcpyAsync(tri_indices_out, d_idx.p, (size_t)n_tris * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    *n_nodes_out = n_nodes;
    *max_depth_out = binned ? (uint32_t)level_first.size() - 2u : counters[1];   // binned: level L holds the nodes of depth L (no atomicMax per node)
    float area = 0.0f;                                                    // m_total_area: a sequential float sum (ref: BVH.cpp:22)
    for (uint32_t i = 0; i < n_tris; ++i) area += HostTriangleArea(triangles[i]);
    *total_area_out = area;
    return CGPT_OK;
}

// ---- cgpt_scene_rebuild_mesh -----------------------------------------------------------------------------------------
// The three parts above around the device scene: prepare_from_scene instead of an upload, the level loop, and the emit kernels instead of
// the host emit.  Everything up to the plan runs in scratch buffers; the scene is written after the last refusal.
static int RebuildLost(cgpt_ctx* ctx, const char* what, hipError_t e)        // refit.hip: SceneLost
{
    ctx->has_scene = false;
    return CtxFail(ctx, CGPT_ERR_HIP, "%s failed: %s (the device scene is dropped; upload it again)", what, hipGetErrorString(e));
}
#define REBUILD_HIP_WRITING(ctx, expr)                                                                                  \
    do {                                                                                                                \
        hipError_t e_ = (expr);                                                                                         \
        if (e_ != hipSuccess) return RebuildLost((ctx), #expr, e_);                                                     \
    } while (0)

static int RebuildMesh(cgpt_ctx* ctx, uint32_t obj_index, uint32_t build_option, uint32_t* n_nodes_out, uint32_t* max_depth_out)
{
    if (!ctx->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "no scene uploaded");
    if (obj_index >= ctx->h_objects.size()) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u out of range (%zu objects)", obj_index, ctx->h_objects.size());
    const DevObject d = ctx->h_objects[obj_index];
    if (d.kind != CGPT_OBJECT_MESH) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u is no mesh: only a mesh has a tree to rebuild", obj_index);
    if (build_option > CGPT_BUILD_SAH_BINNED) return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_scene_rebuild_mesh: unknown build option %u", build_option);
    if (build_option == CGPT_BUILD_SAH_SPLIT_PRIMITIVES)
        return CtxFail(ctx, CGPT_ERR_UNSUPPORTED, "cgpt_scene_rebuild_mesh: SAH-split-primitives never splits (SURVEY A-5): nothing to rebuild with");
    const RefitObject old = ctx->refit_objects[obj_index];
    const uint32_t n_tris = old.tri_count, tri_base = d.tri_base, leaf_base = old.leaf_base;
    if (n_tris == 0u || n_tris != d.n_tris) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u: the layout's triangle counts disagree", obj_index);
    hipStream_t stream = ctx->stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(stream));

    // ---- in scratch: the build ----
    BuildWork w;
    int rc = AllocBuildWork(ctx, n_tris, build_option, w);
    if (rc != CGPT_OK) return rc;
    DevBuf<uint32_t> d_report, d_top_name, d_top_slots;
    HIP_TRY(ctx, d_report.Alloc(kReportRanks + kTopRecords));
    HIP_TRY(ctx, d_top_name.Alloc(kTopScan));
    HIP_TRY(ctx, d_top_slots.Alloc(kTopRecords));
    HIP_TRY(ctx, hipMemsetAsync(d_report.p, 0, sizeof(uint32_t) * (kReportRanks + kTopRecords), stream));
    const dim3 per_tri((n_tris + 255u) / 256u), block(256);
    hipLaunchKernelGGL(prepare_from_scene, per_tri, block, 0, stream, ctx->sb.tri_leaf.p, ctx->sb.tri_orig.p, leaf_base, tri_base, n_tris, w.lo.p, w.hi.p, w.c.p, w.idx.p, d_report.p);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t flags = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&flags, d_report.p, sizeof(flags), hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));                               // before a level kernel sees a position outside its domain
    if (flags & kFlagSlot) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u: a leaf slot names a triangle outside the mesh", obj_index);
    if (w.binned && (flags & kFlagDomain))
        return CtxFail(ctx, CGPT_ERR_INVALID, "cgpt_scene_rebuild_mesh: the binned build needs finite positions of magnitude <= 1e30 (object %u)", obj_index);
    rc = RunBuildLevels(ctx, w, stream);
    if (rc != CGPT_OK) return rc;

    // ---- on the host: where the records go (rebuild_layout.h) ----
    RebuildPlan plan;
    std::string why;
    rc = PlanRebuild(ctx->h_objects, ctx->refit_objects, ctx->record_perm, ctx->mesh_group, ctx->scene.n_top_records, ctx->footprint.n_pair_records, ctx->n_refit_levels,
                     obj_index, w.level_first, plan, why);
    if (rc != CGPT_OK) return CtxFail(ctx, rc, "%s", why.c_str());
    const uint32_t K = (uint32_t)plan.top_slots.size(), room = n_tris - 1u;
    if (K > kTopRecords) return CtxFail(ctx, CGPT_ERR_INVALID, "object %u owns %u top records", obj_index, K);
    if (K) HIP_TRY(ctx, hipMemcpyAsync(d_top_slots.p, plan.top_slots.data(), sizeof(uint32_t) * K, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(assign_top_slots, dim3(1), dim3(kBuildThreads), 0, stream, w.nodes.p, w.n_nodes, d_top_slots.p, K, d_top_name.p, d_report.p);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<uint32_t> report(kReportRanks + kTopRecords);
    HIP_TRY(ctx, hipMemcpyAsync(report.data(), d_report.p, sizeof(uint32_t) * report.size(), hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    const uint32_t n_ranks = report[7];
    const uint32_t* const ranks = report.data() + kReportRanks;
    if (n_ranks > K || !CheckTopRanks(plan, ranks, n_ranks)) return CtxFail(ctx, CGPT_ERR_HIP, "object %u: the builder's ranks do not fit the plan", obj_index);

    // the top-level box: the new root's bounds, or TriangleBounds for a root that stays a leaf (LayoutScene)
    TopLevelState top = ctx->top_state;
    float* box = top.local_box.data() + 6 * (size_t)obj_index;
    if (plan.n_pairs == 0u) {
        uint32_t fold[8];
        HIP_TRY(ctx, FoldObjectBoxToHost(ctx, tri_base, n_tris, fold));
        if (fold[7] != 0u) UnboundedBox(box); else memcpy(box, fold + 1, 24);
    } else {
        memcpy(box, report.data() + 1, 24);
    }
    for (const uint32_t j : plan.members)
        if (j != obj_index) memcpy(top.local_box.data() + 6 * (size_t)j, box, 24);

    // the room: grown copies of the two record tables at a first rebuild, the scratch of the morph targets' permutation
    DevBuf<float4> grown_pairs; DevBuf<uint32_t> grown_levels;
    if (plan.grow && room != 0u) {
        HIP_TRY(ctx, grown_pairs.Alloc(4 * (size_t)plan.n_pair_records));
        HIP_TRY(ctx, grown_levels.Alloc(plan.n_refit_levels));
        if (ctx->footprint.n_pair_records) HIP_TRY(ctx, hipMemcpyAsync(grown_pairs.p, ctx->sb.node_pairs.p, sizeof(float4) * 4 * (size_t)ctx->footprint.n_pair_records, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(ctx, hipMemsetAsync(grown_pairs.p + 4 * (size_t)ctx->footprint.n_pair_records, 0, sizeof(float4) * 4 * (size_t)room, stream));
        if (ctx->n_refit_levels) HIP_TRY(ctx, hipMemcpyAsync(grown_levels.p, ctx->sb.refit_levels.p, sizeof(uint32_t) * ctx->n_refit_levels, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(ctx, hipMemsetAsync(grown_levels.p + ctx->n_refit_levels, 0, sizeof(uint32_t) * room, stream));
        HIP_TRY(ctx, hipStreamSynchronize(stream));
    }
    std::vector<uint32_t> leaf_morphs;                                         // the members whose targets are stored in leaf-slot order
    for (const uint32_t j : plan.members)
        if (j < ctx->morphs.size() && ctx->morphs[j].n_targets != 0u && ctx->morphs[j].leaf_order != 0u) leaf_morphs.push_back(j);
    DevBuf<float2> d_planes; DevBuf<uint32_t> d_from;
    if (!leaf_morphs.empty()) { HIP_TRY(ctx, d_planes.Alloc(9 * (size_t)n_tris)); HIP_TRY(ctx, d_from.Alloc(n_tris)); }
    ctx->record_perm.reserve(plan.n_record_perm);                              // may throw: before the first write (the slice is then written in place)
    std::vector<DevObject> new_objects = ctx->h_objects;                       // a word and a RefitObject an object: not by the record
    std::vector<RefitObject> new_refit = ctx->refit_objects;
    ApplyRebuildObjects(plan, RebuildRootCode(plan, ranks, n_ranks), new_objects, new_refit);

    // ---- from here on the scene changes ----
    ctx->scene_generation++; ctx->shape_generation++;                          // as a refit: the guides are stale and the temporal history is dropped
    if (plan.grow && room != 0u) {
        const uint64_t before = sizeof(float4) * (uint64_t)ctx->sb.node_pairs.n + sizeof(uint32_t) * (uint64_t)ctx->sb.refit_levels.n;
        ctx->sb.node_pairs = std::move(grown_pairs); ctx->sb.refit_levels = std::move(grown_levels);
        ctx->scene.node_pairs = ctx->sb.node_pairs.p;
        ctx->footprint.device_bytes += sizeof(float4) * (uint64_t)ctx->sb.node_pairs.n + sizeof(uint32_t) * (uint64_t)ctx->sb.refit_levels.n - before;
    }
    ctx->footprint.n_pair_records = plan.n_pair_records; ctx->n_refit_levels = plan.n_refit_levels;
    hipLaunchKernelGGL(emit_leaf_triangles, per_tri, block, 0, stream, w.idx.p, ctx->sb.tri_orig.p, ctx->sb.tri_leaf.p, leaf_base, tri_base, n_tris, d_report.p);
    REBUILD_HIP_WRITING(ctx, hipGetLastError());
    hipLaunchKernelGGL(emit_pair_records, dim3((w.n_nodes + 255u) / 256u), block, 0, stream, w.nodes.p, w.n_nodes, d_top_name.p, plan.refit.span_base, room, leaf_base, n_tris,
                       ctx->sb.node_pairs.p, ctx->sb.tri_leaf.p, ctx->sb.refit_levels.p + plan.refit.level_begin, d_report.p);
    REBUILD_HIP_WRITING(ctx, hipGetLastError());
    for (const uint32_t j : leaf_morphs) {
        MorphBuffers& mb = ctx->morphs[j];
        hipLaunchKernelGGL(morph_slot_map, per_tri, block, 0, stream, w.idx.p, mb.slot_of_tri.p, d_from.p, n_tris, d_report.p);
        REBUILD_HIP_WRITING(ctx, hipGetLastError());
        for (uint32_t s = 0; s <= mb.n_targets; ++s) {                         // one set of nine planes at a time through the scratch
            float2* set = mb.data.p + 9 * (size_t)n_tris * s;
            hipLaunchKernelGGL(morph_gather_set, per_tri, block, 0, stream, set, d_from.p, d_planes.p, n_tris);
            REBUILD_HIP_WRITING(ctx, hipGetLastError());
            REBUILD_HIP_WRITING(ctx, hipMemcpyAsync(set, d_planes.p, sizeof(float2) * 9 * (size_t)n_tris, hipMemcpyDeviceToDevice, stream));
        }
    }
    for (const uint32_t j : plan.members) {                                    // every placement of the copy: its root code, where a kernel reads it
        REBUILD_HIP_WRITING(ctx, hipMemcpyAsync(&ctx->sb.objects.p[j].root_code, &new_objects[j].root_code, sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        REBUILD_HIP_WRITING(ctx, hipMemcpyAsync(reinterpret_cast<uint32_t*>(ctx->sb.obj_trace.p + 2 * (size_t)j) + 1, &new_objects[j].root_code, sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    }
    REBUILD_HIP_WRITING(ctx, hipMemcpyAsync(&flags, d_report.p, sizeof(flags), hipMemcpyDeviceToHost, stream));
    REBUILD_HIP_WRITING(ctx, hipStreamSynchronize(stream));
    if (flags & kFlagEmit) {                                                   // an emit kernel skipped a write: the tree on the device is not whole
        ctx->has_scene = false;
        return CtxFail(ctx, CGPT_ERR_HIP, "cgpt_scene_rebuild_mesh: object %u: the builder's node array is inconsistent (the device scene is dropped; upload it again)", obj_index);
    }
    ctx->h_objects.swap(new_objects); ctx->refit_objects.swap(new_refit);
    ApplyRebuildPerm(plan, ranks, n_ranks, ctx->record_perm);                  // the one host pass over the mesh's own records: n_pairs names
    ctx->scene.stack_depth = plan.stack_depth;
    REBUILD_HIP_WRITING(ctx, WriteTopLevel(ctx, ctx->h_objects, top));
    ctx->top_state.local_box.swap(top.local_box);
    if (n_nodes_out) *n_nodes_out = plan.n_nodes;
    if (max_depth_out) *max_depth_out = plan.max_depth;
    return CGPT_OK;
}

extern "C" int cgpt_scene_rebuild_mesh(cgpt_ctx* ctx, uint32_t obj_index, uint32_t build_option, uint32_t* n_nodes_out, uint32_t* max_depth_out)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return Guarded(ctx, __func__, [&] { return GroupRebuildMesh(ctx, obj_index, build_option, n_nodes_out, max_depth_out); });
    return Guarded(ctx, __func__, [&] { return RebuildMesh(ctx, obj_index, build_option, n_nodes_out, max_depth_out); });   // bumps the generations once the call is accepted
}
