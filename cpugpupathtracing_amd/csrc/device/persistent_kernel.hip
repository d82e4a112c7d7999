// persistent_kernel.hip -- whole paths in ONE persistent launch (gfx950): K6 of SURVEY 2.2 done the wavefront way.
//
// The wavefront pipeline (wavefront_kernels.hip) synchronises every bounce round through HBM: per round a trace launch, a shade
// launch and two list kernels, ~150 bytes of ray / path state streamed per path, and a drain at the end of every launch in which a
// few long rays keep a handful of waves busy (a launch never takes less than ~0.2 ms, so a 1-sample frame of seven rounds costs
// 2.6 ms however few rays it has).  Here a lane owns a PATH: the same voted traversal steps (trace_steps.hpp) trace its rays,
// a fourth voted state runs shade_bounce() (ref: Main.cpp:404-573) on the hit -- same device function as the other two render
// paths, so the image is bit-identical -- and the lane goes straight on to the NEE shadow ray and the next extend ray without
// leaving the kernel.  A lane whose path ends takes the next path id from the launch's work counters (trace_steps.hpp:
// WorkFetch).  What reaches HBM is 16 bytes per path: the path's radiance, which pt_accumulate adds to the float4 accumulator in
// sample order (ref: Main.cpp:735-746).  Measured against the other two paths: DESIGN.md 5.2, profiles/r02/.
// Rays that miss everything are retired where the miss is found (no shade step), brute-force / comparison paths
// (TracePath, ref: Main.cpp:581-689) keep their per-level operations in a per-lane HBM stack and apply them innermost-first.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <new>

#include "cpugpupt_abi.h"
#include "device_scene.h"
#include "fast_div.h"
#include "rt_device.hpp"
#include "shade_device.hpp"
#include "trace_steps.hpp"
#include "accumulate.hpp"
#include "launch_common.h"

namespace cgpt {

using namespace dev;

hipStream_t CtxStream(cgpt_ctx* ctx);
void** CtxPersistentSlot(cgpt_ctx* ctx);
hipEvent_t CtxStartEvent(cgpt_ctx* ctx);
void PersistentFree(void* state);

extern __shared__ uint32_t pt_lds[];

static constexpr uint32_t kShade = 0x40000002u;          // traversal code: the extend ray is done, shade its hit

struct PtDev {
    float4* st_en;                     // [n_paths] {energy.xyz, bits(final depth)}: the finished paths' radiance
    float4* brute;                     // [level][thread][2] BruteLevel records of the brute-force paths (BRUTE kernels only)
    uint32_t* stack_overflow;          // [level - kLdsStackLevels][thread]: the rarely used deep end of the traversal stack
    uint32_t n_paths;                  // path ids 0 .. n_paths-1 of this batch
    PathGrid g;
    uint32_t* work;                    // the launch's kWorkCounters work counters, 32 bytes apart (zeroed before the launch)
    uint32_t coarse;                   // path ids a wave takes per fetch while plenty are left
    uint32_t fine_below;               // once a counter has fewer ids than this left, a wave takes only as many as it has idle lanes
    uint32_t shade_shift;              // lanes waiting to shade count 2^shift times in the vote
};

enum : uint32_t {                      // per-lane path flags
    kPfDepthMask = 0xFFu,              // TracePathAdvanced's ray_depth (ref: Main.cpp:401)
    kPfSpecular = 0x100u,              // is_specular_ray (ref: Main.cpp:402)
    kPfShadow = 0x200u,                // the ray in flight is the NEE shadow ray
    kPfDead = 0x400u,                  // the path ends once the shadow ray in flight is resolved
    kPfBrute = 0x800u,                 // this path runs TracePath (brute force)
    kPfSameRay = 0x1000u               // the parked extend ray is the one just shaded (total internal reflection, SURVEY A-3): not walked again
};

// TAIL: the instantiation for small calls (few samples per call -- the reference's own main loop renders ONE per Render(), ref:
// Main.cpp:702,825-942), which are mostly drain: once nothing is left to fetch, a wave with few busy lanes runs their rays in the lean
// per-lane loop (trace_steps.hpp: lean_traverse) instead of voted steps, because the call ends when its longest chain does (1080p, one
// sample: 2.47 -> 2.21 ms).  Kept out of the throughput instantiations, which it costs registers and SGPR spills (profiles/r03/one_sample.md).
// LEVEL: the kernel level, kernel_variant.h.  RIS: shade_device.hpp, above shade_bounce.
template <bool COUNT, bool BRUTE, bool TAIL, int LEVEL, bool RIS>
__global__ void __launch_bounds__(kTraceBlock, 1) pt_persistent(const DevRenderArgs args, const PtDev pt, uint32_t batch_first, const TraceTune tune)
{
    constexpr bool TREE = ThroughTree(LEVEL);                                 // the objects are reached through the top-level tree, at the scene's own lobe level
    constexpr int LOBES = LobeOf(LEVEL);
    constexpr bool XFORM = HonoursTransforms(LOBES);                          // the scene has a transformed object (trace_steps.hpp)
    constexpr bool STEP = XFORM || TREE;
    const DevScene& sc = args.scene;
    const DevSettings& st = args.settings;
    const uint32_t grid_threads = gridDim.x * kTraceBlock;
    const TravCtx ctx = trav_setup(sc, pt_lds, tune.top_records, pt.stack_overflow, grid_threads, tune.lds_tris);
    const uint32_t tid = blockIdx.x * kTraceBlock + threadIdx.x;

    // Work distribution: path ids from the launch's work counters (trace_steps.hpp: WorkFetch) -- consecutive ids, i.e. with the
    // default pixel-major ids the samples of one pixel and of its neighbours in the 8x8 tile; coarse fetches first and one id per
    // idle lane near the end
    WorkFetch work = work_begin(blockIdx.x * (kTraceBlock / 64u) + (threadIdx.x >> 6));

    Trav r;
    r.d = mk(0.0f); r.rs = make_ray_slab(r.d, r.d); r.t = 0.0f;
    r.obj = kNoHit; r.tri = 0; r.depth = 0; r.cur_obj = 0; r.code = kIdle; r.sp = 0; r.fast_levels = kLdsStackLevels;
    if (XFORM) { r.wo = mk(0.0f); r.wd = mk(0.0f); trav_set_ray(r, r.wo, r.wd); }   // d, 1 / d and the slab operands of one ray, as object_step keeps them
    // the path this lane owns
    uint32_t pid = 0, rng = 0, pf = 0;
    V3 tp = mk(0.0f), en = mk(0.0f), pending = mk(0.0f);
    V3 park_o = mk(0.0f), park_d = mk(0.0f);                                  // the next extend ray, parked while the shadow ray is traced
    float park_t = 0.0f;
    uint32_t park_obj = kNoHit, park_tri = 0, park_depth = 0;                 // its payload: a ray traced again after total internal reflection keeps its hit (SURVEY A-3)
    Counters cnt = { 0, 0, 0, 0, 0, 0 };

    auto finish_path = [&](V3 energy) {                                       // ref: Main.cpp:575-578: the path's radiance leaves the kernel
        float4 o4; o4.x = energy.x; o4.y = energy.y; o4.z = energy.z; o4.w = __uint_as_float(pf & kPfDepthMask);
        st_stream(&pt.st_en[pid], o4);
        r.code = kIdle;
    };

    // a finished ray is dispatched on the spot: the lanes for which object_step() returned true
    auto ray_done = [&]() {
        if (pf & kPfShadow) {                                     // NEE connection resolved, ref: Main.cpp:454-463
            if (r.obj == kNoHit) en = en + pending;
            pf &= ~kPfShadow;
            if (pf & kPfDead) {
                finish_path(en);
            } else if (!COUNT && (pf & kPfSameRay)) {             // the parked ray is the one just shaded: its parked hit is the answer
                r.t = park_t; r.obj = park_obj; r.tri = park_tri; r.depth = park_depth;   // (DESIGN.md 5.1); only what shade_hit reads is restored
                if (XFORM) { r.wo = park_o; r.wd = park_d; }
                else trav_set_ray(r, park_o, park_d);
                r.code = kShade;
                cnt.rays++; cnt.unwalked++;
            } else {
                trav_start<XFORM, TREE>(ctx, r, park_o, park_d, park_t, park_obj, park_tri, park_depth);
                cnt.rays++;
            }
        } else if (r.obj == kNoHit && !(BRUTE && (pf & kPfBrute)) && !(st.debug_mode == 2u && (pf & kPfDepthMask) == 0u)) {
            finish_path(en);                                      // the extend ray left the scene, ref: Main.cpp:415-416
        } else {
            r.code = kShade;
        }
    };
    // one bounce of the path on the hit of its extend ray: the lanes with r.code == kShade
    auto shade_hit = [&]() {
        Ray ray;
        ray.o = trav_world_origin<XFORM>(r); ray.d = trav_world_dir<XFORM>(r); ray.t = r.t; ray.obj = r.obj; ray.tri = r.tri; ray.bvh_depth = trav_depth(r);
        if (BRUTE && (pf & kPfBrute)) {
            // one TracePath level (shade_device.hpp: brute_level), the chain in this thread's column of pt.brute
            uint32_t depth = pf & kPfDepthMask;
            V3 L;
            const bool done = brute_level<COUNT, LOBES>(sc, st, ray, rng, depth,
                [&](uint32_t k, const BruteLevel& lv) {
                    float4* rec = pt.brute + ((size_t)k * grid_threads + tid) * 2u;
                    float4 r0, r1;
                    brute_pack(lv, r0, r1);
                    rec[0] = r0; rec[1] = r1;
                },
                [&](uint32_t k) { const float4* rec = pt.brute + ((size_t)k * grid_threads + tid) * 2u; return brute_unpack(rec[0], rec[1]); }, L, cnt);
            pf = (pf & ~kPfDepthMask) | (depth & kPfDepthMask);
            if (done) {
                finish_path(L);
            } else {
                trav_start<XFORM, TREE>(ctx, r, ray.o, ray.d, ray.t, ray.obj, ray.tri, ray.bvh_depth);
                cnt.rays++;
            }
        } else {
            PathState ps;
            ps.throughput = tp; ps.energy = en; ps.rng = rng; ps.depth = pf & kPfDepthMask; ps.is_specular = (pf & kPfSpecular) != 0u;
            Ray shadow = ray;
            V3 pend = mk(0.0f);
            const uint32_t flags = shade_bounce<COUNT, LOBES, RIS>(sc, st, ray, ps, shadow, pend, cnt);
            tp = ps.throughput; en = ps.energy; rng = ps.rng;
            pf = (ps.depth & kPfDepthMask) | (ps.is_specular ? kPfSpecular : 0u);   // every other flag starts clear: kPfSameRay is this bounce's or none
            const bool dead = (flags & kBounceTerminate) != 0u;
            // The same ray again: IntersectScene accepts only t < ray.t and ray.t is this ray's closest hit, so the call returns the hit it
            // starts from.  It is counted and the lane shades again; the counting kernels walk it, as the oracle does.
            const bool same_ray = !COUNT && !dead && ((flags >> kBounceChainShift) & 3u) == kChainTir;
            if (same_ray) pf |= kPfSameRay;
            if (flags & kBounceShadow) {                          // the shadow ray first: its contribution precedes the next bounce's
                pending = pend;
                pf |= kPfShadow | (dead ? kPfDead : 0u);
                park_o = ray.o; park_d = ray.d; park_t = ray.t; park_obj = ray.obj; park_tri = ray.tri; park_depth = ray.bvh_depth;
                trav_start<XFORM, TREE>(ctx, r, shadow.o, shadow.d, shadow.t, kNoHit, 0u, 0u);
                cnt.rays++;
            } else if (same_ray) {                                // r still holds the ray and its hit: r.code stays kShade
                cnt.rays++; cnt.unwalked++;
            } else if (!dead) {
                trav_start<XFORM, TREE>(ctx, r, ray.o, ray.d, ray.t, ray.obj, ray.tri, ray.bvh_depth);
                cnt.rays++;
            } else {
                finish_path(en);
            }
        }
    };

    for (;;) {
        // ---- idle lanes take new paths: consecutive ids from the wave's fetched range ----
        const unsigned long long need = __builtin_amdgcn_ballot_w64(r.code == kIdle);
        uint32_t n_need = (uint32_t)__popcll(need);
        if (n_need) {
            work_fetch(work, pt.work, pt.n_paths, pt.coarse, pt.fine_below, n_need);
            const uint32_t take = min(n_need, work.loc_end - work.loc_next);
            const uint32_t rank = rank_in_mask(need);
            if (r.code == kIdle && rank < take) {
                pid = work.loc_next + rank;
                Ray pr; uint32_t px = 0;
                if (primary_ray(args, pt.g, pid, batch_first, pr, rng, px)) {  // false: padding of an edge tile, the lane stays idle
                    tp = mk(1.0f); en = mk(0.0f); pf = 0u;                    // ref: Main.cpp:398-402
                    if (BRUTE && (st.render_mode == 1u || (st.render_mode == 0u && px < args.width / 2u))) pf = kPfBrute;   // ref: Main.cpp:719-729
                    trav_start<XFORM, TREE>(ctx, r, pr.o, pr.d, pr.t, kNoHit, 0u, 0u);
                    cnt.rays++;
                }
            }
            work.loc_next += take;
        }
        // Done when nothing is in flight and nothing is left to fetch (nothing in flight alone is not enough: every id just handed out
        // may have been padding of an edge tile; the step loop below then falls straight through and the wave fetches on)
        if (__builtin_amdgcn_ballot_w64(r.code != kIdle) == 0ull && work.exhausted && work.loc_next == work.loc_end) break;
        const bool can_refill = !work.exhausted;

        // ---- run the most popular state's step until enough lanes are idle ----
        for (;;) {
            const uint32_t n_inner = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(r.code < kStartObject));
            const uint32_t n_leaf = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((int32_t)r.code < 0));
            const uint32_t n_obj = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(r.code == kStartObject));
            const uint32_t n_shade = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(r.code == kShade));
            const uint32_t n_busy = n_inner + n_leaf + n_obj + n_shade;
            if (n_busy == 0u) break;
            if (can_refill && 64u - n_busy >= tune.refill_idle) break;
            const uint32_t w_obj = n_obj << tune.obj_shift, w_shade = n_shade << pt.shade_shift;
            // ---- the tail of the launch: a few rays left in this wave and no path to hand to the idle lanes: every lane runs its ray to
            //      the next object boundary in the lean loop (trace_steps.hpp: lean_traverse) -- the launch ends when its longest chain does
            if (TAIL && !can_refill && n_busy <= tune.tail_lanes && n_inner + n_leaf != 0u) {
                if (r.code < kStartObject || (int32_t)r.code < 0) lean_traverse<COUNT, false, STEP>(ctx, r, cnt);
                continue;
            }

            if (n_inner >= n_leaf && n_inner >= w_obj && n_inner >= w_shade) {
                do {
                    if (r.code < kStartObject) inner_step<COUNT, STEP>(ctx, r, cnt);
                } while ((uint32_t)__popcll(__builtin_amdgcn_ballot_w64(r.code < kStartObject)) >= tune.inner_repeat);
            } else if (n_leaf >= w_obj && n_leaf >= w_shade) {
                do {
                    if ((int32_t)r.code < 0) leaf_step<COUNT, false, STEP>(ctx, r, cnt);
                } while ((uint32_t)__popcll(__builtin_amdgcn_ballot_w64((int32_t)r.code < 0)) >= tune.leaf_repeat);
            } else if (w_obj >= w_shade) {
                // ---- object step; a finished ray is dispatched on the spot ----
                if (r.code == kStartObject && object_step<COUNT, false, XFORM, TREE>(ctx, r, cnt)) ray_done();
            } else {
                // ---- shade step: one bounce of the path on the hit of its extend ray ----
                if (r.code == kShade) shade_hit();
            }
        }
    }

    wave_add_u64(&args.counters->traced_rays, cnt.rays);
    if (!COUNT) wave_add_u64(&args.counters->retrace_unwalked, cnt.unwalked);
    if (COUNT) {
        wave_add_u64(&args.counters->inner_steps, cnt.inner);
        wave_add_u64(&args.counters->tri_tests, cnt.tris);
        wave_add_u64(&args.counters->bvh_depth_sum, cnt.depth);
        wave_add_u64(&args.counters->closest_hits, cnt.hits);
    }
}

// ---- accumulate + pack: the batch's samples in order (ref: Main.cpp:735-746, MathLib.h:144-152) ---------------------------------
__global__ void __launch_bounds__(256) pt_accumulate(const DevRenderArgs args, const float4* __restrict__ st_en, const PathGrid g, uint32_t batch_first, uint32_t batch_n)
{
    accumulate_batch(args, st_en, g, batch_first, batch_n);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct PtTuning {
    uint32_t budget_gib = 24;     // HBM for the finished paths' radiance (16 bytes per path of a batch; also at most half of what is free)
    uint32_t max_paths_mi = 1536; // most paths per batch, in Mi (path ids are 32-bit)
    uint32_t refill_idle = 16, inner_repeat = 20, leaf_repeat = 4, obj_shift = 0, shade_shift = 0;
    uint32_t top_records = kLdsTopMax;
    uint32_t blocks_per_cu = 64;  // cap on resident blocks per CU (occupancy experiments)
    uint32_t streams = 2;         // batches in flight (the drain of one overlaps the start of the next)
    uint32_t path_order = 2;      // PathOrder of the path ids = the order work items are handed out (trace_steps.hpp PathGrid)
    uint32_t chunk = 0;           // 64-path tiles per coarse work-counter fetch (0 = auto)
    uint32_t lds_tris = 1;        // the small meshes' triangles (the ground quad) are read from an LDS copy
    uint32_t tail_samples = 8;    // calls of at most this many samples run the TAIL instantiation
    uint32_t tail_lanes = 16;     // small calls: with nothing left to fetch, a wave of at most this many busy lanes runs the lean per-lane loop (0 = never)
    uint32_t fine_rounds = 2;     // fine fetches (one id per idle lane) once fewer than this many ids per lane of the grid are left
};

// every instantiation, [RIS][LEVEL][COUNT][BRUTE][TAIL]
#define CGPT_PT_LEVEL(G, R) \
    { { { pt_persistent<false, false, false, G, R>, pt_persistent<false, false, true, G, R> }, { pt_persistent<false, true, false, G, R>, pt_persistent<false, true, true, G, R> } }, \
      { { pt_persistent<true, false, false, G, R>, pt_persistent<true, false, true, G, R> }, { pt_persistent<true, true, false, G, R>, pt_persistent<true, true, true, G, R> } } }
static decltype(&pt_persistent<false, false, false, 0, false>) const kPtKernels[2][kKernelLevels][2][2][2] = {   // the second half of the levels: the first through the top-level tree
    { CGPT_PT_LEVEL(0, false), CGPT_PT_LEVEL(1, false), CGPT_PT_LEVEL(2, false), CGPT_PT_LEVEL(3, false), CGPT_PT_LEVEL(4, false), CGPT_PT_LEVEL(5, false), CGPT_PT_LEVEL(6, false), CGPT_PT_LEVEL(7, false), CGPT_PT_LEVEL(8, false), CGPT_PT_LEVEL(9, false) },
    { CGPT_PT_LEVEL(0, true), CGPT_PT_LEVEL(1, true), CGPT_PT_LEVEL(2, true), CGPT_PT_LEVEL(3, true), CGPT_PT_LEVEL(4, true), CGPT_PT_LEVEL(5, true), CGPT_PT_LEVEL(6, true), CGPT_PT_LEVEL(7, true), CGPT_PT_LEVEL(8, true), CGPT_PT_LEVEL(9, true) },
};
#undef CGPT_PT_LEVEL
static constexpr size_t kPtKernelCount = TableCount(kPtKernels);
static constexpr size_t kPtListKernelCount = kLobeLevels * TableCount(kPtKernels[0][0]);   // per RIS: the levels without the tree, and as many with it

struct PtHost {
    PtTuning tune;
    DevBuf<float4> st_en[2];                  // [stream]
    DevBuf<float4> brute;
    DevBuf<uint32_t> overflow;
    DevBuf<uint32_t> work_counters;           // kWorkCounters counters of 8 words per launch of a render, zeroed before it
    hipStream_t streams[2] = { nullptr, nullptr };
    hipEvent_t begin = nullptr, acc_done[2] = { nullptr, nullptr };
    EventPairs ev;
    uint32_t n_cus = 0;
    uint32_t blocks_per_cu[2][kKernelLevels][2][2][2] = {}; // [RIS][LEVEL][COUNT][BRUTE][TAIL]; the tree levels are queried at the first launch with the tree on
    static_assert(sizeof(blocks_per_cu) / sizeof(uint32_t) == kPtKernelCount && 2 * 2 * kPtListKernelCount == kPtKernelCount, "one occupancy entry per instantiation");
    size_t occupancy_lds = 0, tree_occupancy_lds = 0;
};

static const Knob<PtTuning> kPtKnobs[] = {
    { "pt_budget_gib", &PtTuning::budget_gib, 1, 256 },   { "pt_max_paths_mi", &PtTuning::max_paths_mi, 1, 2047 },
    { "pt_refill", &PtTuning::refill_idle, 1, 64 },       { "pt_inner_repeat", &PtTuning::inner_repeat, 1, 65 },
    { "pt_leaf_repeat", &PtTuning::leaf_repeat, 1, 65 },  { "pt_obj_shift", &PtTuning::obj_shift, 0, 6 },
    { "pt_shade_shift", &PtTuning::shade_shift, 0, 6 },   { "pt_top_records", &PtTuning::top_records, 0, 4096 },
    { "pt_blocks", &PtTuning::blocks_per_cu, 1, 64 },     { "pt_streams", &PtTuning::streams, 1, 2 },
    { "pt_path_order", &PtTuning::path_order, 0, 2 },
    { "pt_lds_tris", &PtTuning::lds_tris, 0, 1 },            { "pt_tail_lanes", &PtTuning::tail_lanes, 0, 64 },
    { "pt_tail_samples", &PtTuning::tail_samples, 0, 4096 },
    { "pt_chunk", &PtTuning::chunk, 0, 4096 },            { "pt_fine_rounds", &PtTuning::fine_rounds, 0, 1024 },
};

static PtHost* PtGetHost(cgpt_ctx* ctx)
{
    void** slot = CtxPersistentSlot(ctx);
    if (*slot) return static_cast<PtHost*>(*slot);
    PtHost* h = new (std::nothrow) PtHost;
    if (!h) { CtxFail(ctx, CGPT_ERR_INVALID, "out of host memory"); return nullptr; }
    LoadKnobsFromEnv(kPtKnobs, "CGPT_", h->tune);
    hipError_t e = hipEventCreateWithFlags(&h->begin, hipEventDisableTiming);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        e = hipStreamCreateWithFlags(&h->streams[i], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&h->acc_done[i], hipEventDisableTiming);
    }
    if (e != hipSuccess) {                                                    // a half-built state is never left in the context
        CtxFail(ctx, CGPT_ERR_HIP, "persistent kernel streams: %s", hipGetErrorString(e));
        PersistentFree(h);
        return nullptr;
    }
    *slot = h;
    return h;
}

int PersistentSetTuning(cgpt_ctx* ctx, const char* name, uint32_t value, bool* known)
{
    const Knob<PtTuning>* k = FindKnob(kPtKnobs, name);
    *known = k != nullptr;
    if (!k) return CGPT_OK;
    PtHost* h = PtGetHost(ctx);
    return h ? SetKnob(ctx, k, h->tune, name, value) : CGPT_ERR_HIP;
}

void PersistentFree(void* state)
{
    if (!state) return;
    PtHost* h = static_cast<PtHost*>(state);
    for (int i = 0; i < 2; ++i) {
        if (h->streams[i]) (void)hipStreamDestroy(h->streams[i]);
        if (h->acc_done[i]) (void)hipEventDestroy(h->acc_done[i]);
    }
    if (h->begin) (void)hipEventDestroy(h->begin);
    FreeEvents(h->ev);
    delete h;                                                                 // and its buffers
}

void PersistentCollectTiming(void* state, ShadeVariant v, double* ms, uint32_t* launches, uint32_t* waves_per_simd)
{
    *ms = 0.0; *launches = 0; *waves_per_simd = 0;
    if (!state) return;
    PtHost* h = static_cast<PtHost*>(state);
    ForEachPair(h->ev, [&](uint32_t, float t) { *ms += t; *launches += 1; });
    *waves_per_simd = std::min(h->tune.blocks_per_cu, h->blocks_per_cu[v.ris][KernelLevel(v)][0][0][0]) * (kTraceBlock / 256u);
}

int LaunchPersistent(cgpt_ctx* ctx, const DevRenderArgs& args_in, ShadeVariant v)
{
    hipStream_t stream = CtxStream(ctx);
    PtHost* h = PtGetHost(ctx);
    if (!h) return -1;

    const bool brute = args_in.settings.render_mode != 2u;
    LAUNCH_TRY(QueryCuCount(h->n_cus));
    const uint32_t top_records = std::min(h->tune.top_records, args_in.scene.n_top_records);
    const size_t lds = trace_lds_bytes(top_records);
    if (h->occupancy_lds != lds) {
        for (uint32_t ris = 0; ris < 2u; ++ris)                               // the list kernels: what mode 0 always queried
            LAUNCH_TRY(QueryOccupancy(&kPtKernels[ris][0][0][0][0], &h->blocks_per_cu[ris][0][0][0][0], kPtListKernelCount, kTraceBlock, lds));
        h->occupancy_lds = lds;
    }
    if (v.tree && h->tree_occupancy_lds != lds) {
        for (uint32_t ris = 0; ris < 2u; ++ris)
            LAUNCH_TRY(QueryOccupancy(&kPtKernels[ris][KernelLevel(kLobesMirror, true)][0][0][0], &h->blocks_per_cu[ris][KernelLevel(kLobesMirror, true)][0][0][0], kPtListKernelCount, kTraceBlock, lds));
        h->tree_occupancy_lds = lds;
    }
    const bool tail = args_in.n_samples <= h->tune.tail_samples;              // a small call: mostly drain
    const uint32_t level = KernelLevel(v);                                    // cgpt_set_top_level(1): the scene's own level through the tree
    const uint32_t blocks_per_cu = std::min(h->tune.blocks_per_cu, h->blocks_per_cu[v.ris][level][v.count][brute][tail]);
    // the resident capacity of the chip, or fewer blocks when there are fewer than 64 paths per wave (a small call ends sooner when
    // its paths are spread thin than when the tail of a launch waits for 4 096 waves to find out that there is nothing to do)
    const uint32_t n_tiles = ((args_in.width + 7u) / 8u) * ((args_in.n_rows + 7u) / 8u);
    const uint64_t paths_in_call = (uint64_t)n_tiles * 64u * args_in.n_samples;
    const uint32_t blocks_wanted = (uint32_t)std::min<uint64_t>(h->n_cus * blocks_per_cu, std::max<uint64_t>(1, paths_in_call / (16u * (kTraceBlock / 64u))));
    const dim3 grid(blocks_wanted), block(256), trace_block(kTraceBlock);
    uint32_t max_blocks = 1;
    // every instantiation (the loop used to stop after lobe level 1; levels 2 and 3 and RIS never have the higher occupancy, so the sizes below are what they were)
    for (size_t i = 0; i < kPtKernelCount; ++i) max_blocks = std::max(max_blocks, (&h->blocks_per_cu[0][0][0][0][0])[i]);
    const uint32_t max_threads = h->n_cus * max_blocks * kTraceBlock;

    const uint32_t tiles_x = (args_in.width + 7u) / 8u;
    const uint64_t n_pixels64 = (uint64_t)n_tiles * 64u;
    const uint64_t max_paths = (uint64_t)h->tune.max_paths_mi << 20;
    if (n_pixels64 > max_paths) { CtxFail(ctx, CGPT_ERR_UNSUPPORTED, "band of %llu pixels exceeds the path-id range", (unsigned long long)n_pixels64); return -1; }
    const uint32_t n_pixels = (uint32_t)n_pixels64;

    // ---- samples per batch: as many as the radiance buffers hold; two buffers when there is more than one batch ----
    size_t free_b = 0, total_b = 0;
    LAUNCH_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t held = (h->st_en[0].n + h->st_en[1].n) * sizeof(float4);
    const size_t budget = std::min<size_t>((size_t)h->tune.budget_gib << 30, (free_b + held) / 2);
    uint32_t batch = (uint32_t)std::min<uint64_t>(args_in.n_samples, std::min<uint64_t>(max_paths / n_pixels, budget / sizeof(float4) / n_pixels));
    if (batch == 0) { CtxFail(ctx, CGPT_ERR_HIP, "not enough free HBM for one sample of %u pixels", n_pixels); return -1; }
    uint32_t n_batches = (args_in.n_samples + batch - 1u) / batch;
    uint32_t n_streams = 1;
    if (n_batches > 1 && h->tune.streams > 1) {                               // two half-size buffers: batch k's drain overlaps batch k+1
        n_streams = 2;
        batch = std::max(1u, (uint32_t)std::min<uint64_t>(batch, budget / 2 / sizeof(float4) / n_pixels));
        n_batches = (args_in.n_samples + batch - 1u) / batch;
    }
    const size_t cap = (size_t)n_pixels * batch;
    LAUNCH_TRY(Grow(h->st_en[0], cap));
    if (n_streams == 2) LAUNCH_TRY(Grow(h->st_en[1], cap));
    const uint32_t deep_levels = args_in.scene.stack_depth > kLdsStackLevels ? args_in.scene.stack_depth - kLdsStackLevels : 0u;
    LAUNCH_TRY(Grow(h->overflow, std::max<size_t>(1, (size_t)deep_levels * max_threads) * n_streams));
    if (brute) LAUNCH_TRY(Grow(h->brute, (size_t)(args_in.settings.max_ray_depth + 1) * max_threads * 2u * n_streams));
    if (ReserveEvents(ctx, h->ev, 2u * n_batches) != 0) return -1;
    const size_t work_words = (size_t)n_batches * kWorkCounters * 8u;
    LAUNCH_TRY(Grow(h->work_counters, work_words));
    LAUNCH_TRY(hipEventRecord(CtxStartEvent(ctx), stream));                   // one-time host setup is over: the render's device time starts here
    LAUNCH_TRY(hipMemsetAsync(h->work_counters.p, 0, work_words * sizeof(uint32_t), stream));   // before `begin`: ordered ahead of both streams
    const TraceTune tt = { h->tune.refill_idle, h->tune.inner_repeat, h->tune.leaf_repeat, 1u, h->tune.obj_shift, top_records, 0u, h->tune.lds_tris, h->tune.tail_lanes, 0u };   // shadow rays to the end here: stopping them early (wf_trace does) cost this kernel 2 % in registers

    if (n_streams == 2) {
        LAUNCH_TRY(hipEventRecord(h->begin, stream));
        for (int i = 0; i < 2; ++i) LAUNCH_TRY(hipStreamWaitEvent(h->streams[i], h->begin, 0));
    }
    int launches = 0;
    uint32_t k = 0;
    for (uint32_t done = 0; done < args_in.n_samples; done += batch, ++k) {
        const uint32_t s = n_streams == 2 ? k & 1u : 0u;
        hipStream_t st = n_streams == 2 ? h->streams[s] : stream;
        const uint32_t bn = std::min(batch, args_in.n_samples - done);
        const uint32_t bfirst = args_in.first_sample + done;
        PtDev pt{};
        pt.st_en = h->st_en[s].p;
        pt.brute = brute ? h->brute.p + (size_t)s * (h->brute.n / n_streams) : nullptr;
        pt.stack_overflow = h->overflow.p + (size_t)s * (h->overflow.n / n_streams);
        pt.n_paths = n_pixels * bn;
        pt.g.n_pixels = n_pixels; pt.g.tiles_x = tiles_x; pt.g.div_tiles_x = MakeFastDiv(tiles_x); pt.g.div_n_pixels = MakeFastDiv(n_pixels);
        pt.shade_shift = h->tune.shade_shift;
        pt.g.order = h->tune.path_order; pt.g.n_samples = bn; pt.g.div_samples = MakeFastDiv(bn);
        pt.work = h->work_counters.p + (size_t)k * kWorkCounters * 8u;
        work_sizes(pt.n_paths, grid.x * (kTraceBlock / 64u), h->tune.fine_rounds, h->tune.chunk, pt.coarse, pt.fine_below);
        // the buffer's previous batch must have been accumulated (same stream: implicit)
        LAUNCH_TRY(hipEventRecord(NextEvent(h->ev), st));
        hipLaunchKernelGGL(kPtKernels[v.ris][level][v.count][brute][tail], grid, trace_block, lds, st, args_in, pt, bfirst, tt);
        LAUNCH_TRY(hipEventRecord(NextEvent(h->ev), st));
        // accumulate in sample order: batch k after batch k-1
        if (n_streams == 2 && k > 0) LAUNCH_TRY(hipStreamWaitEvent(st, h->acc_done[(k - 1u) & 1u], 0));
        hipLaunchKernelGGL(pt_accumulate, dim3(std::min((n_pixels + 255u) / 256u, h->n_cus * 8u)), block, 0, st, args_in, (const float4*)pt.st_en, pt.g, bfirst, bn);
        if (n_streams == 2) LAUNCH_TRY(hipEventRecord(h->acc_done[s], st));
        LAUNCH_TRY(hipGetLastError());
        launches += 2;
    }
    if (n_streams == 2 && k > 0) LAUNCH_TRY(hipStreamWaitEvent(stream, h->acc_done[(k - 1u) & 1u], 0));
    return launches;
}

}  // namespace cgpt
