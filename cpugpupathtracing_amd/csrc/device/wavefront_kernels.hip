// wavefront_kernels.hip -- the wavefront pipeline (gfx950): per bounce [trace -> shade -> plan -> gather] -> accumulate.
//
// Why: in the megakernel a wave's traversal loop runs until its slowest lane is done (max-vs-mean ray length) and a tile
// runs until its most expensive pixel is done; PMC showed ~10 % active lanes per VALU instruction.  Here
//   * trace<>  is a PERSISTENT kernel: every wave keeps its 64 lanes filled from the round's ray list, each lane runs the
//     reference's ordered stack traversal (ref: Source/BVH.cpp:61-127) on a per-wavefront LDS stack, and a lane that
//     finishes its ray is refilled while its neighbours keep going.  Extend rays and NEE shadow rays are traced by the
//     same kernel (both are closest-hit IntersectScene calls, ref: Source/Main.cpp:299-316,452-453); a shadow ray's
//     epilogue adds its pending contribution to the path's energy.
//   * shade<>  runs shade_bounce() (ref: Main.cpp:404-573) for every extend hit, rewrites the path's slot with its next ray
//     (and its shadow slot with the NEE connection) and appends the surviving path ids / shadow ids to this wave's own
//     output segment with __ballot + mbcnt (active-lane compaction, no atomics).
//   * plan + gather turn the per-wave segments into one dense list per kind (exclusive scan of the segment counts, then a copy).
//   * accumulate adds the finished samples to the float4 accumulator IN SAMPLE ORDER, so the image is bit-identical to
//     the megakernel's and the oracle's (ref: Main.cpp:735-746).
// Work distribution: consumers take 64-item blocks of the dense list strided over the persistent grid (wave w: blocks w,
// w + n_waves, ...).  Every wave therefore gets the same number of rays (+-64) sampled from the whole image, which balances
// cost as well as count with no atomics at all.  Rejected on measurements: (1) compaction through global atomic counters,
// one per wave -- 10.6 M waves/step serialise on one L2 word at ~88 atomics/us and cost more than the tracing; (2) a liveness
// byte per slot scanned by strided waves -- correct but waves own unequal numbers of live rays (59 % wave residency);
// (3) the same with 64 partitioned head counters -- the atomics cost more than the imbalance they removed.
// Slot entry (48 B, three float4 planes, extend slot = path id, shadow slot = cap + path id):
//   A = {o.xyz, t_max}  B = {d.xyz, bits(depth | spec << 8 | brute << 9 | chain << 10 | same ray << 30 | follower << 31)}  C = extend: hit record
//   {bits obj, tri, bvh_depth, t} written by trace (a ray traced again after total internal reflection, SURVEY A-3, keeps it: the counting
//   kernels walk that ray with it as payload, the others take it as the answer -- DESIGN.md 5.1) | shadow: {pending.xyz, -}.  A follower's A.w is its leader's path id instead of t_max (see wf_shade).
// Round 0 has no generate kernel and no slot traffic for the rays: trace and shade both recompute the primary ray (ref: Main.cpp:713-716,
// Camera::GetRay :133-140).  The reference does not jitter (SURVEY A-14), so trace walks the band's pixels, not the paths: one ray per
// pixel, its 16-byte hit record in px_hit[pixel], counted once per sample.  Shade reads the record of the path's pixel and initialises
// the path state.
// TracePath (brute force, ref: Main.cpp:581-689) paths -- RENDER_MODE_BRUTE_FORCE, or the left half of the image in the reference's default
// RENDER_MODE_COMPARISON (ref: Main.cpp:215,719-725) -- run through the same rounds: shade<BRUTE> records the level's operation in
// brute[level][path] instead of updating a throughput, and folds the recorded chain over the leaf's radiance, innermost level first
// (float multiplication is not associative), when the path ends.  They have no shadow rays; flag bit 9 of B.w marks them.
// Path state (path id = sample_in_batch * n_pixels + pixel index): {throughput.xyz, bits(rng)} rewritten every bounce while the path
// lives; {energy.xyz, bits(final depth)} touched only when radiance arrives (emissive hit, unoccluded shadow ray).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "cpugpupt_abi.h"
#include "ctx_internal.h"
#include "device_scene.h"
#include "fast_div.h"
#include "rt_device.hpp"
#include "shade_device.hpp"
#include "shade_items.h"
#include "trace_steps.hpp"
#include "accumulate.hpp"
#include "launch_common.h"

namespace cgpt {

using namespace dev;

hipStream_t CtxStream(cgpt_ctx* ctx);
void** CtxWavefrontSlot(cgpt_ctx* ctx);
hipEvent_t CtxStartEvent(cgpt_ctx* ctx);

extern __shared__ uint32_t lds_dyn[];

static constexpr uint32_t kMaxBands = 128;  // most runs per segment (image bands) the count / prefix tables are sized for

struct WfDev {
    float4* A; float4* B; float4* C;   // 2 * cap slots each: [0, cap) extend, [cap, 2 cap) shadow
    float4* st_tp; float4* st_en;      // cap paths
    float4* px_hit;                    // n_pixels: round 0's hit record {bits obj, tri, bvh_depth, t} per pixel of the band, shared by all samples of the batch
    float4* brute;                     // TracePath / COMPARISON renders only: [level][path][2] BruteLevel records (shade_device.hpp), max_ray_depth + 1 levels
    uint8_t* hit_flag;                 // cap paths: did the path's extend ray of this round hit anything (retire_misses only; written by trace)
    uint32_t* list_ext; uint32_t* list_sh;     // dense lists of path ids for the next trace / shade (cap entries each)
    uint32_t* seg_ext; uint32_t* seg_sh;       // per-wave output segments of shade (n_segs * seg_cap entries each)
    uint32_t* seg_count;               // [kind][band][segment]: extend counts, then shadow counts (plain lists: [2 * n_segs])
    uint32_t* seg_prefix;              // exclusive prefix of the above, per kind, band-major: where each (band, segment) run starts in the list
    uint32_t n_bands;                  // runs per segment: > 1, the next round's lists are ordered by image band (see wf_shade); 1: plain lists
    uint32_t band_magic;               // band of path id p = min(n_bands - 1, umulhi(p, band_magic))
    uint32_t* plan;                    // {n_ext, n_sh}
    uint32_t* stack_overflow;          // [level - kLdsStackLevels][thread of the trace grid]: the rarely used deep end of the stack
    uint32_t cap;                      // slots per kind
    uint32_t n_paths;                  // paths of this batch (path ids 0 .. n_paths-1, all valid)
    PathGrid g;                        // path id <-> pixel of the band (trace_steps.hpp)
    uint32_t n_segs, seg_cap;
    uint32_t shade_chunk;              // most consecutive 64-path blocks a shade wave takes at a time (shorter lists: shade_items.h)
    uint32_t retire_misses;            // later rounds: trace leaves one byte per extend ray (hit or not) and shade takes only the hits (off for the debug views)
    uint32_t rot_trace[2], rot_shade;  // rotation of the wave order from one row of blocks to the next ([FIRST] for trace): see next_block()
    unsigned long long* spec_tab;      // specular-chain election (wf_shade): spec_keys entries {bits(epoch << 16 | chain), leader path id << 32} per
                                       // pixel of the band; null: no election (the COUNT and TracePath renders, spec_dedupe 0)
    uint32_t spec_keys;                // entries per pixel
    uint32_t spec_epoch;               // 1..0xFFFF, new for every shade launch: entries of other epochs are free
    uint32_t probe;                    // wf_shade resolves the rays that probe_scene() decides itself (wf_shade: "Probe")
    uint32_t probe_lights;             // ... and ends the path of a fresh extend ray that it decides as a hit on a light (wf_shade: "Probe")
};

// Specular chains.  The reference does not jitter (SURVEY A-14), so all samples of a pixel share the primary ray and its hit, and
// after a mirror or dielectric bounce the next ray is a function of the traced ray and its hit alone: the RNG only picks WHICH of
// reflect (the mirror lobe and the dielectric's reflection make the same ray), refract or total internal reflection (the same ray
// again) follows.  So within a batch the ray of a path whose bounces were all specular is fixed by (pixel, chain): the base-3 code of
// its choices with a leading 1 (1 at the primary hit; 0 = not a chain: a diffuse bounce, a code past 16 bits).  wf_shade elects one
// leader per (pixel, chain) among the rays it emits; the followers stay in the extend list (lists, plans and bands are unchanged),
// trace skips them, and the next shade reads the leader's hit record (C and hit_flag of the leader's slot: neither changes between
// that trace and the next).  Each follower still shades with its own RNG stream, throughput and Beer factor.
static constexpr uint32_t kChainShift = 10u, kChainMax = 0xFFFFu, kFollowerBit = 0x80000000u, kNoLeader = 0xFFFFFFFFu;
static constexpr uint32_t kSameRayBit = 0x40000000u;   // B.w: shade_bounce left the ray as it was (total internal reflection): A.w is its hit's t, C its hit record

// Called by the lanes that emit an extend ray; `chain` = 0: no election for this lane.  Returns the path id of the leader of the
// lane's (pixel, chain) -- the lane's own when it leads -- or kNoLeader when the pixel's entries are all taken (traced as usual).
// Inside the wave the first lane of every distinct key probes for all lanes of that key (with pixel-major ids a wave holds a few
// keys); across waves one load + CAS per probed entry.
__device__ __forceinline__ uint32_t elect_chain_leader(const WfDev& wf, uint32_t chain, uint32_t pid)
{
    const bool want = chain != 0u;
    uint32_t pixel = 0;
    if (want) { uint32_t sample_unused; path_split(wf.g, pid, sample_unused, pixel); }
    uint32_t src = lane_id();                                                 // the lane that probes for this lane's key
    for (unsigned long long pend = __builtin_amdgcn_ballot_w64(want); pend != 0ull;) {
        const uint32_t f = (uint32_t)__builtin_ctzll(pend);
        const bool m = want && pixel == __builtin_amdgcn_readlane(pixel, f) && chain == __builtin_amdgcn_readlane(chain, f);
        if (m) src = f;
        pend &= ~__builtin_amdgcn_ballot_w64(m);
    }
    uint32_t leader = kNoLeader;
    if (want && src == lane_id()) {
        unsigned long long* const row = wf.spec_tab + (size_t)pixel * wf.spec_keys;
        const uint32_t tag = (wf.spec_epoch << 16) | chain;
        const unsigned long long mine = ((unsigned long long)pid << 32) | tag;
        for (uint32_t k = 0; k < wf.spec_keys; ++k) {
            unsigned long long cur = __hip_atomic_load(&row[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            while (((uint32_t)cur >> 16) != wf.spec_epoch) {                  // free: claim it (an entry changes once per epoch)
                const unsigned long long prev = atomicCAS(&row[k], cur, mine);
                cur = prev == cur ? mine : prev;
            }
            if ((uint32_t)cur == tag) { leader = (uint32_t)(cur >> 32); break; }
        }
    }
    return __shfl(leader, (int)src);
}

// ---- K2/K4 trace: persistent closest-hit traversal with per-lane refill ------------------------------------------------
// `first_round`: the list is the identity over the PIXELS of the band (not the paths) and there are no shadow rays yet.  The reference
// does not jitter (SURVEY A-14): every sample of a pixel traces the same primary ray to the same hit, so round 0 traces it once, stores
// the hit record to px_hit[pixel] and counts it as the batch's n_samples IntersectScene calls.
// The traversal states, their voted steps and the LDS layout are in trace_steps.hpp.

// FIRST (round 0) is a separate instantiation so the later rounds carry neither its code nor its registers.
// XFORM: the scene has an object with a transform (trace_steps.hpp: the lane also keeps its world ray, six registers that only these
// instantiations carry).  TREE: the objects are reached through the top-level tree (trace_steps.hpp: object_step<.., TREE>).
template <bool COUNT, bool FIRST, bool XFORM = false, bool TREE = false>
__global__ void __launch_bounds__(kTraceBlock, 1) wf_trace(const DevRenderArgs args, const WfDev wf, uint32_t batch_first, const TraceTune tune)
{
    constexpr bool first_round = FIRST;
    constexpr bool STEP = XFORM || TREE;                                      // every object boundary goes through object_step: no fold
    const DevScene& sc = args.scene;
    DevCounters* const counters = args.counters;
    const TravCtx ctx = trav_setup(sc, lds_dyn, tune.top_records, wf.stack_overflow, gridDim.x * kTraceBlock, tune.lds_tris);
    lds_u32* const ring = ctx.ring;

    const uint32_t n_ext = first_round ? wf.g.n_pixels : wf.plan[0];
    const uint32_t n_sh = first_round ? 0u : wf.plan[1];
    const uint32_t blocks_ext = (n_ext + 63u) / 64u, n_blocks = blocks_ext + (n_sh + 63u) / 64u;
    const uint32_t n_waves = gridDim.x * (kTraceBlock / 64u);
    // wave-uniform: the wave's next 64-item block of the dense list
    BlockWalk walk = first_block(blockIdx.x * (kTraceBlock / 64u) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6));   // wave-uniform: scalar registers
    uint32_t block = block_of(walk);
    const uint32_t rot = wf.rot_trace[first_round ? 1 : 0];
    uint32_t ring_count = 0;

    Trav r;
    r.d = mk(0.0f); r.rs = make_ray_slab(r.d, r.d); r.t = 0.0f;
    r.obj = kNoHit; r.tri = 0; r.depth = 0; r.cur_obj = 0; r.code = kIdle; r.sp = 0; r.fast_levels = kLdsStackLevels;
    if (XFORM) { r.wo = mk(0.0f); r.wd = mk(0.0f); trav_set_ray(r, r.wo, r.wd); }   // d, 1 / d and the slab operands of one ray, as object_step keeps them
    uint32_t slot_of_lane = 0;
    uint32_t wave_rays = 0;                                                   // wave-uniform: rays this wave started (later rounds)
    uint32_t wave_followers = 0;                                              // wave-uniform: of those, followers of a specular chain (not traced)
    uint32_t wave_unwalked = 0;                                               // wave-uniform: of those, traced again after total internal reflection (not walked)
    Counters cnt = { 0, 0, 0, 0, 0, 0 };

    auto finish_ray = [&]() {                                                 // the ray of this lane has seen every object of the scene
        // The slot's addresses are formed here, when the ray ends: left to the optimiser they are hoisted to where the slot is assigned
        // (loop-invariant for the whole traversal) and six 64-bit addresses ride along through every step -- ten registers of the budget.
        uint32_t slot = slot_of_lane;
        asm volatile("" : "+v"(slot));
        if (first_round) {                                                    // slot = pixel index: the hit record of all its samples
            float4 c; c.x = __uint_as_float(r.obj); c.y = __uint_as_float(r.tri); c.z = __uint_as_float(trav_depth(r)); c.w = r.t;
            st_stream(&wf.px_hit[slot], c);
        } else if (slot >= wf.cap) {                                                 // connect epilogue, ref: Main.cpp:454-463
            if (r.obj == kNoHit) {
                const float4 pe = ld_stream(&wf.C[slot]);
                const uint32_t pid = slot - wf.cap;
                float4 en = ld_stream(&wf.st_en[pid]);
                en.x += pe.x; en.y += pe.y; en.z += pe.z;
                st_stream(&wf.st_en[pid], en);
            }
        } else {
            // A later-round extend ray that left the scene ends its path with nothing to add (ref: Main.cpp:415-416; the debug views
            // read the last depth, so they take the full path): ~40 % of the later rounds' rays.  Shade never sees them: it reads
            // this byte per ray and queues only the hits.
            const bool hit = r.obj != kNoHit;
            if (wf.retire_misses) wf.hit_flag[slot] = hit ? (uint8_t)1 : (uint8_t)0;
            if (!wf.retire_misses || hit) {
                float4 c; c.x = __uint_as_float(r.obj); c.y = __uint_as_float(r.tri); c.z = __uint_as_float(trav_depth(r)); c.w = r.t;
                st_stream(&wf.C[slot], c);                                    // hit record
            }
        }
        r.code = kIdle;
    };

    for (;;) {
        // ---- refill idle lanes from the ring; top the ring up with this wave's next blocks of the dense list ----
        const unsigned long long need = __builtin_amdgcn_ballot_w64(r.code == kIdle);
        const uint32_t n_need = (uint32_t)__popcll(need);
        while (ring_count < n_need && block < n_blocks) {
            uint32_t s = 0; bool valid;
            if (block < blocks_ext) {
                const uint32_t i = block * 64u + lane_id();
                valid = i < n_ext;
                if (valid) s = first_round ? i : ld_stream(&wf.list_ext[i]);
            } else {
                const uint32_t i = (block - blocks_ext) * 64u + lane_id();
                valid = i < n_sh;
                if (valid) s = wf.cap + ld_stream(&wf.list_sh[i]);
            }
            const unsigned long long m = __builtin_amdgcn_ballot_w64(valid);
            if (valid) ring[ring_count + rank_in_mask(m)] = s;
            ring_count += (uint32_t)__popcll(m);
            next_block(walk, n_waves, rot);
            block = block_of(walk);
            __builtin_amdgcn_wave_barrier();
        }
        if (n_need && ring_count) {
            const uint32_t take = min(n_need, ring_count);
            const uint32_t rank = rank_in_mask(need);
            bool followed = false, unwalked = false;
            if (r.code == kIdle && rank < take) {
                const uint32_t slot = ring[ring_count - 1u - rank];
                slot_of_lane = slot;
                bool ok = true;
                V3 o, d; float t; uint32_t obj = kNoHit, tri = 0, depth = 0;      // fresh ray (extend or shadow, ref: Primitives.h:79-81)
                if (first_round) {                                            // primary ray from the pixel index, nothing to load
                    Ray pr;
                    ok = pixel_ray(args, wf.g, slot, pr);                     // false: padding of an edge tile
                    o = pr.o; d = pr.d; t = pr.t;
                } else {
                    const float4 a = ld_stream(&wf.A[slot]), b = ld_stream(&wf.B[slot]);
                    o = mk(a.x, a.y, a.z); t = a.w; d = mk(b.x, b.y, b.z);
                    // Not walked: a follower -- its leader traces this ray (wf_shade: specular chains) and shade reads the leader's hit or miss --
                    // and the same ray again after total internal reflection (SURVEY A-3; wf_shade marks it): that walk can only return the hit
                    // it starts from.  C[slot] holds it, and hit_flag[slot] is 1 since that hit was found (round 0: wf_shade set it).
                    if (!COUNT && slot < wf.cap && (__float_as_uint(b.w) & (kFollowerBit | kSameRayBit))) {
                        ok = false;
                        followed = (__float_as_uint(b.w) & kFollowerBit) != 0u; unwalked = !followed;
                        if (followed && wf.retire_misses) wf.hit_flag[slot] = 1;
                    } else if (slot < wf.cap && t != 1e34f) {                 // the counting kernels walk it, as the oracle does:
                        const float4 c = ld_stream(&wf.C[slot]);              // it keeps its previous hit as payload
                        obj = __float_as_uint(c.x); tri = __float_as_uint(c.y); depth = __float_as_uint(c.z);
                    }
                }
                if (ok) {
                    trav_start<XFORM, TREE>(ctx, r, o, d, t, obj, tri, depth);
                    if (!first_round && tune.shadow_any_hit != 0u && slot >= wf.cap) r.depth |= kAnyHitBit;
                    if (first_round) cnt.rays++;                              // later rounds: every id of the lists is a ray, counted per wave below
                }
            }
            __builtin_amdgcn_wave_barrier();
            ring_count -= take;
            if (!first_round) wave_rays += take;
            if (!COUNT && !first_round) {
                wave_followers += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(followed));
                wave_unwalked += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(unwalked));
            }
        }
        // Done when nothing is in flight and nothing is left to fetch.  Nothing in flight alone is not enough: every id just handed
        // out may have been padding of an edge tile (round 0: a padded row of a tile; later rounds never list one); the step loop below
        // then falls straight through and the wave fetches on.
        if (__builtin_amdgcn_ballot_w64(r.code != kIdle) == 0ull && ring_count == 0u && block >= n_blocks) break;
        const bool can_refill = ring_count != 0u || block < n_blocks;

        // ---- run the most popular state's step until enough lanes are idle ----
        for (;;) {
            const uint32_t n_inner = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(r.code < kStartObject));
            const uint32_t n_leaf = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((int32_t)r.code < 0));
            const uint32_t n_obj = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(r.code == kStartObject));
            const uint32_t n_busy = n_inner + n_leaf + n_obj;
            if (n_busy == 0u) break;
            if (can_refill && 64u - n_busy >= tune.refill_idle) break;        // enough idle lanes: go refill them
            const uint32_t w_obj = n_obj << tune.obj_shift;
            // Round 0: the 64 lanes of a wave carry the primary rays of one 8x8 tile -- neighbouring rays that walk nearly the same
            // nodes, so there is little divergence for the voted branch-free steps to buy off; every lane walks its meshes in the lean
            // loop (the reference's own control flow, trace_steps.hpp: lean_traverse -- ~50 instructions per node instead of ~75 and no
            // votes), then takes the object step.  Same results, same counters.
            if (FIRST && tune.first_lean) {
                if (r.code < kStartObject || (int32_t)r.code < 0) lean_traverse<COUNT, !FIRST, STEP>(ctx, r, cnt);
                if (r.code == kStartObject && object_step<COUNT, !FIRST, XFORM, TREE>(ctx, r, cnt)) finish_ray();
                continue;
            }

            if (n_inner >= n_leaf && n_inner >= w_obj) {
                do {
                    if (r.code < kStartObject) inner_step<COUNT, STEP>(ctx, r, cnt);
                } while ((uint32_t)__popcll(__builtin_amdgcn_ballot_w64(r.code < kStartObject)) >= tune.inner_repeat);
            } else if (n_leaf >= w_obj) {
                do {
                    if ((int32_t)r.code < 0) leaf_step<COUNT, !FIRST, STEP>(ctx, r, cnt);
                } while ((uint32_t)__popcll(__builtin_amdgcn_ballot_w64((int32_t)r.code < 0)) >= tune.leaf_repeat);
            } else {
                do {
                    if (r.code == kStartObject && object_step<COUNT, !FIRST, XFORM, TREE>(ctx, r, cnt)) finish_ray();
                } while ((uint32_t)__popcll(__builtin_amdgcn_ballot_w64(r.code == kStartObject)) >= tune.obj_repeat);
            }
        }
    }

    // round 0: every traced pixel ray is the IntersectScene call of each of the batch's samples (the reference's counts); the lanes'
    // 32-bit sums are of per-pixel counts and the product is formed in 64 bits
    const uint32_t per_ray = first_round ? wf.g.n_samples : 1u;
    if (first_round) wave_add_u64(&counters->traced_rays, cnt.rays, per_ray);
    else if (lane_id() == 0u && wave_rays) atomicAdd(&counters->traced_rays, (unsigned long long)wave_rays);
    if (!COUNT && !first_round && lane_id() == 0u && wave_followers) atomicAdd(&counters->chain_followers, (unsigned long long)wave_followers);
    if (!COUNT && !first_round && lane_id() == 0u && wave_unwalked) atomicAdd(&counters->retrace_unwalked, (unsigned long long)wave_unwalked);
    if (COUNT) {
        wave_add_u64(&counters->inner_steps, cnt.inner, per_ray);
        wave_add_u64(&counters->tri_tests, cnt.tris, per_ray);
        wave_add_u64(&counters->bvh_depth_sum, cnt.depth, per_ray);
    }
}

// ---- K3 shade: one bounce per extend hit; survivors compacted into this wave's output segment ---------------------------
// BRUTE: the render has TracePath paths (RENDER_MODE_BRUTE_FORCE / COMPARISON); a separate instantiation, so the TracePathAdvanced
// renders carry neither its code nor its registers.  LOBES: the lobe level, kernel_variant.h.  RIS: shade_device.hpp, above shade_bounce.
// A rough bounce reports lobe choice 0, so its ray is never elected or followed as a specular chain.
// Registers.  The kernel's arguments are two structs of ~100 dwords together, nearly all of them read once per pass: as by-value arguments
// they are loaded at the kernel's entry, and what does not fit beside the probe's scalar records is parked in VGPR lanes and fetched back
// with a vector instruction at every use -- in a kernel whose limit is vector issue.  So wf_shade names its arguments only
// for the launch: each part of a pass reads the fields it needs from the kernel-argument segment itself, through shade_kernargs() -- a
// scalar load where the field is used, with no register held across the probes.  The view's address passes through an empty asm
// statement, as the slot addresses of wf_trace's finish_ray do: to the optimiser every call is a new pointer, so nothing read through
// one is hoisted out of the pass loop or kept for the next part.
// ShadeKernArgs IS wf_shade's parameter list, field for field, as the argument segment lays it out: change both together (the
// static_assert behind the kernel holds the signature to these three types in this order).  The view is returned as a generic reference
// because shade_bounce, probe_scene and the other shared helpers take generic ones; after inlining the address space is inferred back
// from the constant-address-space pointer the view starts from, and the reads are scalar loads (scripts/shade_static_counts.sh shows it).
struct ShadeKernArgs { DevRenderArgs args; WfDev wf; uint32_t batch_first; };
static_assert(alignof(DevRenderArgs) == 8 && alignof(WfDev) == 8 && sizeof(DevRenderArgs) % 8 == 0, "ShadeKernArgs mirrors the argument segment: every parameter at its natural alignment");
__device__ __forceinline__ const ShadeKernArgs& shade_kernargs()
{
    const CGPT_UNIFORM ShadeKernArgs* p = (const CGPT_UNIFORM ShadeKernArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const ShadeKernArgs*)p;
}

template <bool COUNT, bool FIRST, bool BRUTE = false, int LOBES = 0, bool RIS = false>
__global__ void __launch_bounds__(256, 1) wf_shade(const DevRenderArgs, const WfDev, uint32_t)   // read through shade_kernargs(): "Registers" above
{
    constexpr bool first_round = FIRST;
    constexpr bool kChains = !COUNT && !BRUTE;                                // specular chains are tracked (and elected when wf.spec_tab is set)
    uint32_t n_ext;
    { const WfDev& wf = shade_kernargs().wf; n_ext = first_round ? wf.n_paths : wf.plan[0]; }
    const uint32_t n_blocks = (n_ext + 63u) / 64u;
    const uint32_t n_waves = gridDim.x * 4u;
    const uint32_t wave = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // = this wave's segment (wave-uniform: a scalar register)
    uint32_t count_ext = 0, count_sh = 0;                                     // wave-uniform
    // Image bands: a wave walks its chunks in ascending list order and the lists are band-major (round 0: path ids in image order), so
    // the entries it appends are already grouped by the band of their pixel -- contiguous runs inside its segment, with no per-entry key.
    // The wave only notes where each band's run ends; plan + gather then put all segments' runs of band 0 first, then band 1, ...
    // The rays trace works on at any one time (a contiguous piece of the list) then come from ONE strip of the image instead of from all
    // over it, and the part of the tree they walk stays in the 4 MB L2 of every XCD.
    uint32_t cur_band = 0, band_start_ext = 0, band_start_sh = 0;             // wave-uniform
    Counters cnt = { 0, 0, 0, 0, 0, 0 };
    // Probe.  More than half of the later rounds' rays of the reference scene are decided by the top of IntersectScene alone: they miss both
    // halves of the mesh's box, the ground quad and the light spheres -- shadow rays of ground pixels towards the lights, their bounce
    // rays into the sky.  probe_scene() (rt_device.hpp) answers those here, from the registers that hold the ray, with the trace kernels'
    // own intersectors: a decided shadow ray is never listed (unoccluded: its pending radiance goes to st_en now, the connect epilogue's
    // read-modify-write moved; occluded: dropped), an extend ray decided as a miss ends its path now instead of in the next round, and so
    // does one decided as a hit whose closest object is a light (probe_lights; the emission the next round would add is added here).  Each
    // is still one IntersectScene call of the reference and is counted as one.  Not probed: the counting kernels (they walk as the oracle
    // walks), TracePath lanes, the debug views (they read the last depth), rays of a specular chain (the election and its followers stay
    // as they are) and a ray re-traced after total internal reflection (wf_trace does not walk it at all: its hit is known).
    uint32_t wave_probed = 0;                                                 // wave-uniform: rays this wave decided
    uint32_t wave_absorbed = 0;                                               // wave-uniform: stuck iterations shade_bounce ran in place

    // The order in which a wave appends its survivors is the order of the next round's ray list.  Taking runs of `chunk`
    // consecutive blocks (the samples of one pixel and of its neighbours in round 0, and their descendants later) keeps the rays of
    // a 64-ray block of every later round from one neighbourhood of the image rather than from unrelated ones (measured +1.3 % with
    // sample-major ids; flat between 1 and 16 blocks with the pixel-major ones, profiles/r02/experiments.md).
    // Wave-uniform loop state: the walk and the block.  The chunk's end and "the list has a block left for this wave" follow from them.
    // wf.shade_chunk is the most a work item takes: a list too short to give every wave a whole one is dealt in shorter items, down to four
    // blocks, so that a late round's few thousand blocks spread over the waves instead of sitting 32 deep in a few dozen (shade_items.h,
    // with the bound that keeps a wave inside its segment).  What a wave appends is still in ascending list order.
    BlockWalk walk = first_block(wave);
    const uint32_t chunk = shade_item_blocks(n_blocks, n_waves, shade_kernargs().wf.shade_chunk);   // wave-uniform
    uint32_t block = wave * chunk;
    auto more = [&]() { return block < n_blocks; };                           // chunks start at whole multiples of the chunk: past the last one, past the list
    auto advance = [&]() {
        if (++block >= min((block_of(walk) + 1u) * chunk, n_blocks)) {
            next_block(walk, n_waves, shade_kernargs().wf.rot_shade);
            block = block_of(walk) * chunk;
        }
    };
    // Later rounds with retire_misses: the wave reads one hit byte per ray of its blocks and queues the path ids of the hits (in list
    // order: the queue is first in, first out, so what the wave appends to its segments is in the order it would have been anyway);
    // every pass below then has 64 hits to shade instead of the ~38 a block of the list holds.
    __shared__ uint32_t s_queue[4][128];
    uint32_t* const queue = s_queue[threadIdx.x >> 6];
    uint32_t queued = 0;                                                      // wave-uniform
    const bool hits_only = !first_round && shade_kernargs().wf.retire_misses != 0u;

    for (;;) {
        bool active = false;
        bool emit_ext = false, emit_sh = false;
        bool decided_sh = false, decided_ext = false;                         // probe: the ray is resolved here and not listed
        uint32_t pid = 0;
        uint32_t absorbed = 0;                                                // at most the depth limit: eight bits
        if (!hits_only) {
            if (!more()) break;
            const uint32_t i = block * 64u + lane_id();
            active = i < n_ext;
            if (active) pid = first_round ? i : ld_stream(&shade_kernargs().wf.list_ext[i]);
            advance();
        } else {
            while (queued < 64u && more()) {
                const WfDev& wf = shade_kernargs().wf;
                const uint32_t i = block * 64u + lane_id();
                uint32_t p = 0; bool hit = false;
                if (i < n_ext) { p = ld_stream(&wf.list_ext[i]); hit = wf.hit_flag[p] != 0; }
                const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
                if (hit) queue[queued + rank_in_mask(m)] = p;
                queued += (uint32_t)__popcll(m);
                advance();
            }
            if (queued == 0u) break;
            __builtin_amdgcn_wave_barrier();
            const uint32_t take = min(queued, 64u), rest = queued - take;
            active = lane_id() < take;
            if (active) pid = queue[lane_id()];
            const uint32_t moved = queue[64u + lane_id()];
            __builtin_amdgcn_wave_barrier();
            if (lane_id() < rest) queue[lane_id()] = moved;
            __builtin_amdgcn_wave_barrier();
            queued = rest;
        }
        float4 c;                                                             // hit record written by trace
        bool brute_path = false;                                              // this path runs TracePath
        uint32_t sample = 0, px = 0, py = 0;                                  // round 0: the path's sample of the batch and its pixel
        if (first_round && active) {
            // Round 0 begins with the hit record of the path's pixel (one record for all its samples, cached: with pixel-major ids a wave's
            // lanes share a few records).  A pixel whose primary ray left the scene ends all its paths here with the zero energy record that
            // the pass below would write: shade_bounce returns on a miss before it reads the ray or draws a number, so such a lane needs no
            // camera ray and no RNG seed, emits nothing and elects nothing -- with pixel-major ids whole waves are such lanes.  Not taken by
            // the BVH-depth view (it colours the misses too) and by TracePath lanes; a padded index still writes nothing.
            const ShadeKernArgs& ka = shade_kernargs();
            const DevRenderArgs& args = ka.args;
            uint32_t pixel, local_row;
            path_split(ka.wf.g, pid, sample, pixel);
            active = pixel_of_index(args, ka.wf.g, pixel, px, py, local_row);
            if (active) {
                c = ka.wf.px_hit[pixel];
                if (BRUTE) brute_path = args.settings.render_mode == 1u || (args.settings.render_mode == 0u && px < args.width / 2u);   // ref: Main.cpp:719-729
                if (__float_as_uint(c.x) == kNoHit && args.settings.debug_mode != 2u && !(BRUTE && brute_path)) {
                    if (!pixel_adds_nothing(args, c, px)) {                   // (the ray-depth view: its record is read)
                        float4 en; en.x = 0.0f; en.y = 0.0f; en.z = 0.0f; en.w = __uint_as_float(0u);   // {no energy, depth 0}
                        st_stream(&ka.wf.st_en[pid], en);
                    }                                                         // else wf_accumulate supplies the record itself and reads nothing: accumulate.hpp
                    active = false;
                }
            }
        }
        if (active) {
            Ray ray, shadow;
            PathState ps;
            constexpr bool is_pixel = true;                                   // (round 0's padded indices have left above; later rounds list none)
            uint32_t chain = 0;                                               // kChains: the specular-chain code of the path's ray
            bool followed = false;                                            // c is the leader's: this path's own C slot is stale
            if (first_round) {                                                // primary ray and fresh path state (ref: Main.cpp:713-716, Camera::GetRay :133-140)
                const ShadeKernArgs& ka = shade_kernargs();
                const DevRenderArgs& args = ka.args;
                ps.rng = pcg_seed(py * args.width + px, ka.batch_first + sample, args.seed);
                ray = camera_ray(args.camera, (float)px * (1.0f / (float)args.width), (float)py * (1.0f / (float)args.height));
                ps.throughput = mk(1.0f); ps.energy = mk(0.0f); ps.depth = 0; ps.is_specular = false;
                chain = 1u;
            } else {
                const WfDev& wf = shade_kernargs().wf;
                const float4 a = ld_stream(&wf.A[pid]), b = ld_stream(&wf.B[pid]);
                ray.o = mk(a.x, a.y, a.z); ray.d = mk(b.x, b.y, b.z);
                const float4 tp = ld_stream(&wf.st_tp[pid]);
                ps.throughput = mk(tp.x, tp.y, tp.z); ps.rng = __float_as_uint(tp.w);
                ps.energy = mk(0.0f);                                         // the bounce's own addition; folded into st_en below
                const uint32_t fl = __float_as_uint(b.w);
                ps.depth = fl & 0xFFu; ps.is_specular = (fl & 0x100u) != 0u;
                if (BRUTE) brute_path = (fl & 0x200u) != 0u;
                if (kChains) chain = (fl >> kChainShift) & kChainMax;
                if (kChains && (fl & kFollowerBit)) {                         // the leader's hit is this ray's
                    const uint32_t lead = __float_as_uint(a.w);
                    followed = true;
                    if (!wf.retire_misses || wf.hit_flag[lead]) c = ld_stream(&wf.C[lead]);
                    else { c.x = __uint_as_float(kNoHit); c.y = 0.0f; c.z = 0.0f; c.w = 0.0f; }   // the leader left the scene: a miss
                } else c = ld_stream(&wf.C[pid]);
            }
            ray.t = c.w; ray.obj = __float_as_uint(c.x); ray.tri = __float_as_uint(c.y); ray.bvh_depth = __float_as_uint(c.z);
            shadow = ray;
            V3 pending = mk(0.0f);

            uint32_t flags = kBounceTerminate;
            if (BRUTE && brute_path) {
                // one TracePath level (shade_device.hpp: brute_level), the chain in this path's column of wf.brute
                if (is_pixel) {
                    const ShadeKernArgs& ka = shade_kernargs();
                    const DevScene& sc = ka.args.scene;
                    const DevRenderArgs& args = ka.args;
                    const WfDev& wf = ka.wf;
                    const bool done = brute_level<COUNT, LOBES>(sc, args.settings, ray, ps.rng, ps.depth,
                        [&](uint32_t k, const BruteLevel& lv) {
                            float4* rec = wf.brute + ((size_t)k * wf.cap + pid) * 2u;
                            float4 r0, r1;
                            brute_pack(lv, r0, r1);
                            st_stream(&rec[0], r0); st_stream(&rec[1], r1);
                        },
                        [&](uint32_t k) { const float4* rec = wf.brute + ((size_t)k * wf.cap + pid) * 2u; return brute_unpack(ld_stream(&rec[0]), ld_stream(&rec[1])); },
                        ps.energy, cnt);
                    flags = done ? kBounceTerminate | kBounceBruteDone : 0u;
                }
            } else if (is_pixel) {
                const DevRenderArgs& args = shade_kernargs().args;
                flags = shade_bounce<COUNT, LOBES, RIS>(args.scene, args.settings, ray, ps, shadow, pending, cnt);
            }
            if (!COUNT) { absorbed = cnt.unwalked; cnt.unwalked = 0; }       // shade_bounce's stuck iterations, each an IntersectScene call of the reference
            emit_ext = (flags & kBounceTerminate) == 0u;
            emit_sh = (flags & kBounceShadow) != 0u;
            if (kChains && emit_ext) {
                const uint32_t choice = (flags >> kBounceChainShift) & 3u;    // 0: diffuse, else 1 + base-3 digit
                chain = choice != 0u && chain != 0u && chain <= (kChainMax - 2u) / 3u ? chain * 3u + choice - 1u : 0u;
            }
            bool connect = false;                                             // the shadow ray is decided and reaches its light
            bool light_added = false;                                         // the extend ray is decided as a hit on a light whose emission counts:
            V3 light_energy = mk(0.0f);                                       // the next round's addition (0 + throughput * emissive * intensity)
            if (!COUNT && shade_kernargs().wf.probe != 0u && !(BRUTE && brute_path)) {
                if (emit_sh) {                                                // (each probe reads the scene through a view of its own: what the shadow probe
                    float t = shadow.t;                                       // holds in scalar registers is dead before the extend probe starts)
                    const uint32_t seen = probe_scene(shade_kernargs().args.scene, shadow.o, shadow.d, t);
                    decided_sh = seen != kProbeUndecided;
                    connect = seen == kProbeMiss;
                }
                if (emit_ext && !(kChains && chain != 0u) && ray.t == 1e34f) {
                    float t = ray.t;
                    ProbeLight pl;
                    const uint32_t seen = probe_scene<true>(shade_kernargs().args.scene, ray.o, ray.d, t, &pl, shade_kernargs().wf.probe_lights != 0u);
                    decided_ext = seen == kProbeMiss;
                    // Decided as a hit on a light: the next round's pass would do nothing for this path but shade_bounce's light branch -- no
                    // number drawn, the emission added or not by ps as this bounce leaves it -- so that happens here and the path ends: no slot,
                    // no state, no list entry.  One case stays with the lists: the emission would be added and this bounce's shadow ray is listed.
                    // The next trace adds that ray's pending radiance before the next shade adds the emission, and the sum keeps that order (a
                    // shadow ray decided here is added below, before the emission).  Only a specular lobe of a material with a diffuse part gets there.
                    if (seen == kProbeHit && pl.is_light) {
                        PathState next = ps;                                      // the state that pass would start from
                        next.energy = mk(0.0f);
                        const bool adds = add_light_hit(shade_kernargs().args.settings, next, pl.emissive, pl.intensity);
                        if (!(adds && emit_sh && !decided_sh)) { decided_ext = true; light_added = adds; light_energy = next.energy; }
                    }
                }
                emit_sh = emit_sh && !decided_sh;
                emit_ext = emit_ext && !decided_ext;
            }

            // radiance added by this bounce (emissive hit / BVH-depth view): energy_old + x, the reference's single addition
            const WfDev& wf = shade_kernargs().wf;                            // the stores: slot and state addresses formed here, not before the probes
            const bool final_depth_needed = shade_kernargs().args.settings.debug_mode == 1u && !emit_ext;      // ray-depth view reads the last depth
            const bool own_energy = is_pixel && (first_round || (flags & (kBounceEnergy | kBounceBruteDone)) || final_depth_needed);
            if (own_energy || connect || light_added) {
                float4 en;
                if (first_round || (BRUTE && (flags & kBounceBruteDone))) { en.x = 0.0f; en.y = 0.0f; en.z = 0.0f; en.w = 0.0f; }
                else en = ld_stream(&wf.st_en[pid]);
                if (BRUTE && (flags & kBounceBruteDone)) { en.x = ps.energy.x; en.y = ps.energy.y; en.z = ps.energy.z; }   // TracePath's return value, as it is
                if (flags & kBounceEnergy) { en.x += ps.energy.x; en.y += ps.energy.y; en.z += ps.energy.z; }
                if (own_energy || light_added) en.w = __uint_as_float(ps.depth & 0xFFu);   // (the next round's pass leaves the depth this bounce ends with)
                if (connect) { en.x += pending.x; en.y += pending.y; en.z += pending.z; }   // ref: Main.cpp:454-463, as wf_trace's connect epilogue adds it
                if (light_added) { en.x += light_energy.x; en.y += light_energy.y; en.z += light_energy.z; }   // the record that pass would have stored
                st_stream(&wf.st_en[pid], en);
            }
            if (emit_ext) {                                                   // the path lives on: state + next extend ray, same slot
                float4 tpo;
                tpo.x = ps.throughput.x; tpo.y = ps.throughput.y; tpo.z = ps.throughput.z; tpo.w = __uint_as_float(ps.rng);
                st_stream(&wf.st_tp[pid], tpo);
                float4 na, nb;
                na.x = ray.o.x; na.y = ray.o.y; na.z = ray.o.z; na.w = ray.t;    // 1e34 for a fresh ray, the hit t for a re-traced one
                nb.x = ray.d.x; nb.y = ray.d.y; nb.z = ray.d.z;
                uint32_t fl = (ps.depth & 0xFFu) | (ps.is_specular ? 0x100u : 0u) | ((BRUTE && brute_path) ? 0x200u : 0u);
                if (((flags >> kBounceChainShift) & 3u) == kChainTir && !(BRUTE && brute_path)) fl |= kSameRayBit;
                if (kChains) {
                    fl |= chain << kChainShift;
                    if (wf.spec_tab) {
                        const uint32_t lead = elect_chain_leader(wf, chain, pid);
                        if (lead != kNoLeader && lead != pid) { na.w = __uint_as_float(lead); fl |= kFollowerBit; }
                    }
                }
                nb.w = __uint_as_float(fl);
                st_stream(&wf.A[pid], na); st_stream(&wf.B[pid], nb);         // C keeps the hit record (payload of a re-traced ray)
                if ((first_round || followed) && ray.t != 1e34f) st_stream(&wf.C[pid], c);   // round 0 kept it per pixel, a follower's came from
                                                                              // its leader: the re-traced ray's hit record goes to its slot (the
                                                                              // counting trace reads C exactly when A.w != 1e34; the others leave it)
                if (first_round && !COUNT && wf.retire_misses && ray.t != 1e34f) wf.hit_flag[pid] = 1;   // and its hit byte, which trace will not write: a
                                                                              // ray traced again is not walked (later rounds: the byte is 1 from its walk)
            }
            if (emit_sh) {                                                    // NEE connection, slot cap + pid
                const uint32_t ss = wf.cap + pid;
                float4 sa, sb, scc;
                sa.x = shadow.o.x; sa.y = shadow.o.y; sa.z = shadow.o.z; sa.w = shadow.t;
                sb.x = shadow.d.x; sb.y = shadow.d.y; sb.z = shadow.d.z; sb.w = 0.0f;
                scc.x = pending.x; scc.y = pending.y; scc.z = pending.z; scc.w = 0.0f;
                st_stream(&wf.A[ss], sa); st_stream(&wf.B[ss], sb); st_stream(&wf.C[ss], scc);
            }
        }
        // active-lane compaction into the wave's own segments: __ballot + mbcnt, no atomics
        const unsigned long long m_ext = __builtin_amdgcn_ballot_w64(emit_ext), m_sh = __builtin_amdgcn_ballot_w64(emit_sh);
        if (!COUNT) wave_probed += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(decided_sh)) + (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(decided_ext));
        if (!COUNT && __builtin_amdgcn_ballot_w64(absorbed != 0u) != 0ull)    // summed over the wave bit by bit: no per-lane total rides through the loop
            for (uint32_t b = 0; b < 8u; ++b) wave_absorbed += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((absorbed >> b) & 1u)) << b;
        const WfDev& wf = shade_kernargs().wf;                                // the appends: segment addresses and band table, formed here
        if (wf.n_bands > 1u) {                                                // close the runs of the bands this pass has left behind
            const uint32_t band = min(wf.n_bands - 1u, __umulhi(pid, wf.band_magic));
            const bool emits = emit_ext | emit_sh;
            while (__builtin_amdgcn_ballot_w64(emits && band > cur_band) != 0ull) {
                const unsigned long long behind = __builtin_amdgcn_ballot_w64(band <= cur_band);
                const uint32_t end_ext = count_ext + (uint32_t)__popcll(m_ext & behind), end_sh = count_sh + (uint32_t)__popcll(m_sh & behind);
                if (lane_id() == 0u) {
                    wf.seg_count[cur_band * wf.n_segs + wave] = end_ext - band_start_ext;
                    wf.seg_count[(wf.n_bands + cur_band) * wf.n_segs + wave] = end_sh - band_start_sh;
                }
                band_start_ext = end_ext; band_start_sh = end_sh;
                ++cur_band;
            }
        }
        if (emit_ext) st_stream(&wf.seg_ext[(size_t)wave * wf.seg_cap + count_ext + rank_in_mask(m_ext)], pid);
        if (emit_sh) st_stream(&wf.seg_sh[(size_t)wave * wf.seg_cap + count_sh + rank_in_mask(m_sh)], pid);
        count_ext += (uint32_t)__popcll(m_ext);
        count_sh += (uint32_t)__popcll(m_sh);
    }
    const ShadeKernArgs& ka = shade_kernargs();
    const WfDev& wf = ka.wf;
    const DevRenderArgs& args = ka.args;
    if (wf.n_bands > 1u) {                                                    // the last band this wave reached takes the rest; later bands are empty
        if (lane_id() == 0u)
            for (uint32_t b = cur_band; b < wf.n_bands; ++b) {
                wf.seg_count[b * wf.n_segs + wave] = b == cur_band ? count_ext - band_start_ext : 0u;
                wf.seg_count[(wf.n_bands + b) * wf.n_segs + wave] = b == cur_band ? count_sh - band_start_sh : 0u;
            }
    } else if (lane_id() == 0) {
        wf.seg_count[wave] = count_ext; wf.seg_count[wf.n_segs + wave] = count_sh;
    }
    if (COUNT) wave_add_u64(&args.counters->closest_hits, cnt.hits);
    if (!COUNT && lane_id() == 0u && wave_probed) {                           // every decided ray is an IntersectScene call of the reference
        atomicAdd(&args.counters->traced_rays, (unsigned long long)wave_probed);
        atomicAdd(&args.counters->probe_resolved, (unsigned long long)wave_probed);
    }
    if (!COUNT && lane_id() == 0u && wave_absorbed) {
        atomicAdd(&args.counters->traced_rays, (unsigned long long)wave_absorbed);
        atomicAdd(&args.counters->retrace_unwalked, (unsigned long long)wave_absorbed);
    }
}

static_assert(std::is_same<decltype(&wf_shade<false, false>), void (*)(DevRenderArgs, WfDev, uint32_t)>::value &&
              offsetof(ShadeKernArgs, args) == 0 && offsetof(ShadeKernArgs, wf) == sizeof(DevRenderArgs) &&
              offsetof(ShadeKernArgs, batch_first) == sizeof(DevRenderArgs) + sizeof(WfDev),
              "wf_shade reads its arguments through ShadeKernArgs: the struct and the parameter list change together");

// ---- plan: exclusive scan of the segment counts -------------------------------------------------------------------------------
// One 256-thread block per (kind, band): the exclusive prefix of that band's n_segs counts (a few thousand) goes to seg_prefix, the
// band's total to plan[2 + kind * n_bands + band]; wf_gather adds the totals of the bands before (and sums them into plan[kind] for the
// next round's kernels).  Plain lists: plan[kind] directly.  Small blocks with 1 KB of LDS start in the wave slots a resident persistent
// kernel of another batch leaves free (a 1024-thread block had to wait for a whole CU to drain: 0.4 ms average in the 8-pool profile);
// one block scanning all runs in turn took 100 us with 8 of them, on the critical path of its batch.
__global__ void __launch_bounds__(256) wf_plan(const WfDev wf)
{
    __shared__ uint32_t partial[256];
    const uint32_t n = wf.n_segs;
    const uint32_t kk = blockIdx.x;                                           // kind * n_bands + band
    const uint32_t* cnt = wf.seg_count + (size_t)kk * n;
    uint32_t* pre = wf.seg_prefix + (size_t)kk * n;
    const uint32_t per = (n + 255u) / 256u;
    const uint32_t begin = min(threadIdx.x * per, n), end = min(begin + per, n);
    uint32_t sum = 0;
    for (uint32_t i = begin; i < end; ++i) sum += cnt[i];
    partial[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 256u; off <<= 1) {                           // Hillis-Steele inclusive scan
        const uint32_t v = threadIdx.x >= off ? partial[threadIdx.x - off] : 0u;
        __syncthreads();
        partial[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = partial[threadIdx.x] - sum;                                // exclusive prefix of this thread's range
    for (uint32_t i = begin; i < end; ++i) { pre[i] = run; run += cnt[i]; }
    if (threadIdx.x == 255u) {
        wf.plan[2u + kk] = partial[255];
        if (wf.n_bands == 1u) wf.plan[kk] = partial[255];
    }
}

// ---- gather: segments -> dense lists -------------------------------------------------------------------------------------------
// 16 bytes per lane: a segment starts on a 16-byte boundary, its place in the list on a 4-byte one (global dwordx4 accesses only
// need dword alignment).  Round 0 moves ~1 GB per batch here while the other batch's shade streams its state.
__global__ void __launch_bounds__(256) wf_gather(const WfDev wf)
{
    typedef uint32_t u4a4 __attribute__((ext_vector_type(4), aligned(4)));
    if (wf.n_bands == 1u) {
        for (uint32_t s = blockIdx.x; s < 2u * wf.n_segs; s += gridDim.x) {
            const bool sh = s >= wf.n_segs;
            const uint32_t seg = sh ? s - wf.n_segs : s;
            const uint32_t n = wf.seg_count[s], base = wf.seg_prefix[s];
            const uint32_t* src = (sh ? wf.seg_sh : wf.seg_ext) + (size_t)seg * wf.seg_cap;
            uint32_t* dst = (sh ? wf.list_sh : wf.list_ext) + base;
            const uint32_t n4 = n & ~3u;
            for (uint32_t i = threadIdx.x * 4u; i < n4; i += blockDim.x * 4u) *reinterpret_cast<u4a4*>(dst + i) = *reinterpret_cast<const u4a4*>(src + i);
            if (threadIdx.x < n - n4) dst[n4 + threadIdx.x] = src[n4 + threadIdx.x];
        }
        return;
    }
    // Band runs: contiguous in the segment, each copied to its place in the list.  One block per segment.  The run table of the
    // segment (where each band's run starts in the segment and in the list) is built once in LDS -- all counts, prefixes and band
    // totals fetched in parallel, then one short serial pass -- and the four waves copy runs side by side; read one after the other
    // from HBM, 32 bands were 32 dependent round trips per segment.
    __shared__ uint32_t s_n[kMaxBands], s_dst[kMaxBands], s_src[kMaxBands];
    const uint32_t lane = threadIdx.x & 63u, wave_in_block = threadIdx.x >> 6;
    for (uint32_t s = blockIdx.x; s < 2u * wf.n_segs; s += gridDim.x) {
        const bool sh = s >= wf.n_segs;
        const uint32_t seg = sh ? s - wf.n_segs : s;
        const uint32_t* cnt = wf.seg_count + (sh ? wf.n_bands * wf.n_segs : 0u);
        const uint32_t* pre = wf.seg_prefix + (sh ? wf.n_bands * wf.n_segs : 0u);
        const uint32_t* band_total = wf.plan + 2u + (sh ? wf.n_bands : 0u);
        __syncthreads();                                                      // the previous segment's table is no longer read
        if (threadIdx.x < wf.n_bands) {
            s_n[threadIdx.x] = cnt[threadIdx.x * wf.n_segs + seg];
            s_dst[threadIdx.x] = pre[threadIdx.x * wf.n_segs + seg];         // + the totals of the bands before, below
            s_src[threadIdx.x] = band_total[threadIdx.x];
        }
        __syncthreads();
        if (threadIdx.x == 0u) {
            uint32_t off = 0, base = 0;                                       // base: entries of the bands before this one, all segments
            for (uint32_t b = 0; b < wf.n_bands; ++b) {
                const uint32_t n = s_n[b], total = s_src[b];
                s_dst[b] += base; s_src[b] = off;
                off += n; base += total;
            }
            if (seg == 0u) wf.plan[sh ? 1 : 0] = base;                        // the list's length, for the next round's kernels
        }
        __syncthreads();
        const uint32_t* src = (sh ? wf.seg_sh : wf.seg_ext) + (size_t)seg * wf.seg_cap;
        uint32_t* const list = sh ? wf.list_sh : wf.list_ext;
        for (uint32_t b = wave_in_block; b < wf.n_bands; b += 4u) {
            const uint32_t n = s_n[b], n4 = n & ~3u;
            uint32_t* dst = list + s_dst[b];
            const uint32_t* run = src + s_src[b];                             // 16 bytes per lane, dword-aligned at both ends
            for (uint32_t i = lane * 4u; i < n4; i += 256u) *reinterpret_cast<u4a4*>(dst + i) = *reinterpret_cast<const u4a4*>(run + i);
            if (lane < n - n4) dst[n4 + lane] = run[n4 + lane];
        }
    }
}

// ---- K5 accumulate + pack: samples of the batch in order (ref: Main.cpp:735-746, MathLib.h:144-152) ------------------------
__global__ void __launch_bounds__(256) wf_accumulate(const DevRenderArgs args, const WfDev wf, uint32_t batch_first, uint32_t batch_n)
{
    accumulate_batch<true>(args, wf.st_en, wf.g, batch_first, batch_n, wf.px_hit);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// Batches of samples are independent until the final accumulate, and every bounce round ends in a tail where a few
// long rays keep a handful of waves busy.  Several batches are therefore in flight at once, each with its own pool on
// its own HIP stream, so one batch's tail overlaps another batch's bulk; the accumulate kernels are chained with events so
// samples are still added in order.
static constexpr uint32_t kMaxPools = 8;

struct WfTuning {               // defaults measured on MI355X (profiles/r01); overridable for sweeps via CGPT_WF_* env vars
    uint32_t pools = 8;         // most sample batches in flight (the memory budget usually allows fewer)
    uint32_t batch = 0;         // samples per batch; 0 = auto (LaunchWavefront: "samples per batch")
    uint32_t max_batch = 512;   // auto: largest batch (a 1080p / 8 band at 1024 spp: 128 -> 54.3 ms, 256 -> 49.4, 512 -> 43.7: fewer, longer rounds)
    uint32_t pool_paths_mi = 512;   // auto: most paths per pool, in Mi (path ids and slot indices are 32-bit: 2 * paths < 2^32)
    uint32_t budget_gib = 96;   // HBM the pools may take (also at most half of what is free)
    uint32_t refill_idle = 16;  // trace leaves its traversal loop to refill once this many lanes are idle
    uint32_t leaf_repeat = 4;         // same for leaf triangles (measured plateau: inner 16-20, leaf 4-8)
    uint32_t inner_repeat = 20;       // trace keeps taking inner steps without re-voting while this many lanes are at inner nodes
    uint32_t obj_repeat = 1;          // same for the object step (1: until no lane is at an object boundary)
    uint32_t obj_shift = 0;           // lanes at an object boundary count 2^shift times in the vote
    uint32_t top_records = kLdsTopMax;   // records of the top of the tree mirrored in LDS
    uint32_t max_trace_blocks = 64;   // cap on trace blocks per CU (occupancy experiments)
    uint32_t max_shade_blocks = 5;    // cap on shade blocks per CU.  Without spilled scalars the production shade kernels take 70 VGPRs and seven blocks would
                                      // fit; five stay: beside five trace waves a SIMD holds two shade waves either way, a larger grid is more segments to plan
                                      // and gather, and 6 / 7 measured 50.2 against 50.8 ms on the default frame but 58.7 against 57.8 ms in COMPARISON and
                                      // 4.16 against 4.06 ms at 8 samples (profiles/r20/ab_shade_diet.txt)
    uint32_t shade_chunk = 4;         // consecutive blocks per shade work item
    uint32_t shade_chunk_banded = 32; // the same when the lists are ordered by image band: a longer piece of one band per work item (C3 86.8-87.3 -> 85.8-86.0 ms,
                                      // C4 rank share 33.7-34.4 -> 33.4-33.6 ms; 8: 86.4-87.0, 16: 86.4-86.9, 64: 86.1, 128: 86.8-87.3, 256: 91.8-92.0).  Plain lists
                                      // lose with it (C3 rank share of 8, 33 M-path batches: 13.07 -> 13.30 ms)
    uint32_t shadow_any_hit = 1;      // shadow rays stop at their first hit (not in the counting kernels)
    uint32_t lds_tris = 1;            // the small meshes' triangles (the ground quad) are read from an LDS copy
    uint32_t first_lean = 1;          // round 0 walks in the lean per-lane loop instead of voted steps (per-pixel rays: 0.68-0.71 ms
                                      // against 0.72-0.74 voted, frame level; profiles/r04)
    uint32_t trace_events = 1;        // time every trace launch with its own hipEvent pair (cgpt_stats.dominant_ms)
    uint32_t path_order = 2;          // PathOrder of the path ids (trace_steps.hpp PathGrid): 2 pixel-major, 1 tile-major, 0 sample-major
    uint32_t retire_misses = 1;       // shade skips the state loads of later-round rays that hit nothing
    uint32_t bands_min_paths = 32u << 20;  // batches of fewer paths keep plain lists (1080p, 8 samples per call: 4.81 ms plain, 5.21 banded; 33 M-path batches: level)
    uint32_t bands = 32;              // > 1: every round's ray lists ordered by image band (wf_shade: "Image bands"); at most kMaxBands.  C3: 1 band 89.1-89.4 ms,
                                      // 8: 87.3-87.6, 16: 88.0-88.2, 32: 87.1-87.5, 64: 87.8-88.4 (profiles/r03/image_bands.md)
    uint32_t spec_dedupe = 1;         // later rounds trace one ray per (pixel, specular chain) and batch (wf_shade: "Specular chains")
    uint32_t spec_keys = 8;           // election entries per pixel; a ray whose pixel has none left is traced as usual
    uint32_t spec_epochs = 0xFFFF;    // shade launches between two clears of a pool's election table (the 16-bit tag's range; fewer: tests)
    uint32_t probe = 1;               // shade resolves the rays that the top of IntersectScene decides (wf_shade: "Probe")
    uint32_t probe_max_objects = 128; // ... in scenes of at most this many objects: the probe walks all of them for every ray, as trace does; with 4 to
                                      // 128 objects (the bench scene + far-away spheres) probe 1 took 0.87-0.91 of probe 0's time at every count
                                      // (profiles/r10/probe_objects.txt), so the default is the largest count measured
    uint32_t probe_lights = 1;        // a fresh extend ray the probe decides as a hit on a light ends its path in that pass (0: listed, traced and shaded)
};

static uint32_t Gcd(uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; }
// smallest rot in [0, n_waves) with gcd(n_waves + rot, n_tiles) == 1 (device: next_block)
static uint32_t CoprimeRotation(uint32_t n_waves, uint32_t n_tiles)
{
    for (uint32_t rot = 0; rot < n_waves && rot < 4096u; ++rot)
        if (Gcd(n_waves + rot, std::max(1u, n_tiles)) == 1u) return rot;
    return 0u;
}

// every instantiation: trace [XFORM][COUNT][FIRST], shade [RIS][LOBES][COUNT][FIRST][BRUTE]
static decltype(&wf_trace<false, false>) const kTraceKernels[2][2][2] = {
    { { wf_trace<false, false>, wf_trace<false, true> }, { wf_trace<true, false>, wf_trace<true, true> } },
    { { wf_trace<false, false, true>, wf_trace<false, true, true> }, { wf_trace<true, false, true>, wf_trace<true, true, true> } },
};
// the same with the top-level tree (cgpt_set_top_level(1)): a table of its own, so that a context that never turns the tree on queries and
// launches what it did before
static decltype(&wf_trace<false, false>) const kTraceTreeKernels[2][2][2] = {
    { { wf_trace<false, false, false, true>, wf_trace<false, true, false, true> }, { wf_trace<true, false, false, true>, wf_trace<true, true, false, true> } },
    { { wf_trace<false, false, true, true>, wf_trace<false, true, true, true> }, { wf_trace<true, false, true, true>, wf_trace<true, true, true, true> } },
};
#define CGPT_SHADE_LEVEL(G, R) \
    { { { wf_shade<false, false, false, G, R>, wf_shade<false, false, true, G, R> }, { wf_shade<false, true, false, G, R>, wf_shade<false, true, true, G, R> } }, \
      { { wf_shade<true, false, false, G, R>, wf_shade<true, false, true, G, R> }, { wf_shade<true, true, false, G, R>, wf_shade<true, true, true, G, R> } } }
static decltype(&wf_shade<false, false>) const kShadeKernels[2][kLobeLevels][2][2][2] = {
    { CGPT_SHADE_LEVEL(0, false), CGPT_SHADE_LEVEL(1, false), CGPT_SHADE_LEVEL(2, false), CGPT_SHADE_LEVEL(3, false), CGPT_SHADE_LEVEL(4, false) },
    { CGPT_SHADE_LEVEL(0, true), CGPT_SHADE_LEVEL(1, true), CGPT_SHADE_LEVEL(2, true), CGPT_SHADE_LEVEL(3, true), CGPT_SHADE_LEVEL(4, true) },
};
#undef CGPT_SHADE_LEVEL

// What a pool's buffers are sized for (one record per render; the pools of a render are alike)
struct WfSizes {
    uint32_t cap = 0, n_pixels = 0, n_segs = 0, seg_cap = 0;
    uint32_t overflow_words = 0;                 // stack_overflow
    uint32_t brute_levels = 0;                   // TracePath levels of `brute` (0: none)
    size_t spec = 0;                             // entries of spec_tab (0: none)
    bool Holds(const WfSizes& n) const
    {
        return cap >= n.cap && n_pixels >= n.n_pixels && n_segs >= n.n_segs && seg_cap >= n.seg_cap && overflow_words >= n.overflow_words &&
               brute_levels >= n.brute_levels && spec >= n.spec;
    }
};

// Every device buffer of a pool with its bytes at the sizes s (0 bytes: not allocated).  Allocation, release and the bytes the pools
// hold in the memory budget all go through this one list.
template <typename F> static void ForEachBuffer(WfDev& d, const WfSizes& s, F&& f)
{
    const size_t slots = 2 * (size_t)s.cap * sizeof(float4), paths = s.cap, segs = (size_t)s.n_segs * s.seg_cap * sizeof(uint32_t);
    const size_t runs = 2 * (size_t)kMaxBands * s.n_segs * sizeof(uint32_t);
    f(d.A, slots); f(d.B, slots); f(d.C, slots);
    f(d.st_tp, paths * sizeof(float4)); f(d.st_en, paths * sizeof(float4)); f(d.hit_flag, paths);
    f(d.px_hit, (size_t)s.n_pixels * sizeof(float4));
    f(d.brute, (size_t)s.brute_levels * paths * 2u * sizeof(float4));
    f(d.list_ext, paths * sizeof(uint32_t)); f(d.list_sh, paths * sizeof(uint32_t));
    f(d.seg_ext, segs); f(d.seg_sh, segs);
    f(d.seg_count, runs); f(d.seg_prefix, runs);
    f(d.plan, (2 + 2 * (size_t)kMaxBands) * sizeof(uint32_t));
    f(d.stack_overflow, (size_t)s.overflow_words * sizeof(uint32_t));
    f(d.spec_tab, s.spec * sizeof(unsigned long long));
}

static size_t PoolBytes(const WfSizes& s)                                 // device memory of one pool at the sizes s
{
    WfDev d{};
    size_t n = 0;
    ForEachBuffer(d, s, [&](auto*&, size_t bytes) { n += bytes; });
    return n;
}

struct WfHost {
    WfTuning tune;
    WfDev dev[kMaxPools] = {};
    hipStream_t streams[kMaxPools] = {};
    hipEvent_t acc_done[kMaxPools] = {};
    hipEvent_t begin = nullptr;
    WfSizes held;                                // what the pools [0, held_pools) are allocated for
    uint32_t held_pools = 0;
    uint32_t spec_epoch[kMaxPools] = {};         // last epoch used in each pool's spec_tab
    uint32_t n_cus = 0;
    uint32_t trace_blocks_per_cu[2][2][2] = {}, shade_blocks_per_cu[2][kLobeLevels][2][2] = {};   // trace: [XFORM][COUNT][FIRST]; shade: [RIS][LOBES][COUNT][BRUTE]
    bool last_xform = false;                     // the last render ran the XFORM trace kernels (WavefrontTraceWavesPerSimd)
    uint32_t trace_tree_blocks_per_cu[2][2][2] = {};   // kTraceTreeKernels: queried by the first render with the tree on
    bool last_tree = false;
    size_t occupancy_lds = 0, tree_occupancy_lds = 0;
    // hipEvent pairs around every trace launch of the last render (roofline accounting: the dominant kernel's own duration)
    EventPairs trace_ev;
    uint32_t trace_rounds = 0;
};

static void WfRelease(WfHost* h)
{
    for (uint32_t p = 0; p < kMaxPools; ++p) {                               // every pointer, whatever its size: also a failed, partial allocation
        ForEachBuffer(h->dev[p], h->held, [](auto*& ptr, size_t) { DevFree(ptr); });
        h->dev[p] = WfDev{};
    }
    h->held = WfSizes{}; h->held_pools = 0;
}

void WavefrontFree(void* state)
{
    if (!state) return;
    WfHost* h = static_cast<WfHost*>(state);
    WfRelease(h);
    for (uint32_t p = 0; p < kMaxPools; ++p) {
        if (h->streams[p]) (void)hipStreamDestroy(h->streams[p]);
        if (h->acc_done[p]) (void)hipEventDestroy(h->acc_done[p]);
    }
    if (h->begin) (void)hipEventDestroy(h->begin);
    FreeEvents(h->trace_ev);
    delete h;
}

// resident waves per SIMD of the later-round trace kernel (one 256-thread block = one wave on each of the CU's four SIMDs)
uint32_t WavefrontTraceWavesPerSimd(void* state)
{
    if (!state) return 0;
    const WfHost* h = static_cast<const WfHost*>(state);
    return std::min(h->tune.max_trace_blocks, (h->last_tree ? h->trace_tree_blocks_per_cu : h->trace_blocks_per_cu)[h->last_xform][0][0]) * (kTraceBlock / 256u);
}

// Sum of the trace launches' durations of the last render (and the round-0 launches' share); call after the render's device work has completed.
void WavefrontCollectTiming(void* state, double* trace_ms, uint32_t* trace_launches, double* round0_ms, uint32_t* round0_launches)
{
    *trace_ms = 0.0; *trace_launches = 0; *round0_ms = 0.0; *round0_launches = 0;
    if (!state) return;
    WfHost* h = static_cast<WfHost*>(state);
    ForEachPair(h->trace_ev, [&](uint32_t i, float ms) {
        *trace_ms += ms; *trace_launches += 1;
        if (h->trace_rounds && i % h->trace_rounds == 0u) { *round0_ms += ms; *round0_launches += 1; }   // launches are recorded batch by batch, round by round
    });
}

// environment: CGPT_WF_<NAME>
static const Knob<WfTuning> kKnobs[] = {
    { "pools", &WfTuning::pools, 1, kMaxPools },           { "batch", &WfTuning::batch, 0, 4096 },
    { "max_batch", &WfTuning::max_batch, 1, 4096 },         { "pool_paths_mi", &WfTuning::pool_paths_mi, 1, 1024 },
    { "budget_gib", &WfTuning::budget_gib, 1, 256 },       { "refill", &WfTuning::refill_idle, 1, 64 },
    { "leaf_repeat", &WfTuning::leaf_repeat, 1, 65 },      { "inner_repeat", &WfTuning::inner_repeat, 1, 65 },
    { "obj_repeat", &WfTuning::obj_repeat, 1, 65 },        { "obj_shift", &WfTuning::obj_shift, 0, 6 },
    { "top_records", &WfTuning::top_records, 0, 4096 },     { "trace_blocks", &WfTuning::max_trace_blocks, 1, 64 },
    { "shade_blocks", &WfTuning::max_shade_blocks, 1, 64 },
    { "shade_chunk", &WfTuning::shade_chunk, 1, 256 },     { "shade_chunk_banded", &WfTuning::shade_chunk_banded, 1, 256 },
    { "shadow_any_hit", &WfTuning::shadow_any_hit, 0, 1 },     { "trace_events", &WfTuning::trace_events, 0, 1 },
    { "path_order", &WfTuning::path_order, 0, 2 },         { "retire_misses", &WfTuning::retire_misses, 0, 1 },
    { "lds_tris", &WfTuning::lds_tris, 0, 1 },             { "first_lean", &WfTuning::first_lean, 0, 1 },                     { "bands", &WfTuning::bands, 1, kMaxBands },             { "bands_min_paths", &WfTuning::bands_min_paths, 0, 0x7FFFFFFF },
    { "spec_dedupe", &WfTuning::spec_dedupe, 0, 1 },       { "spec_keys", &WfTuning::spec_keys, 1, 16 },
    { "spec_epochs", &WfTuning::spec_epochs, 1, 0xFFFF },   { "probe", &WfTuning::probe, 0, 1 },
    { "probe_max_objects", &WfTuning::probe_max_objects, 0, 4096 }, { "probe_lights", &WfTuning::probe_lights, 0, 1 },
};

static WfHost* WfGetHost(cgpt_ctx* ctx)
{
    void** slot = CtxWavefrontSlot(ctx);
    if (*slot) return static_cast<WfHost*>(*slot);
    WfHost* fresh = new (std::nothrow) WfHost;
    if (!fresh) { CtxFail(ctx, CGPT_ERR_INVALID, "out of host memory"); return nullptr; }
    LoadKnobsFromEnv(kKnobs, "CGPT_WF_", fresh->tune);
    hipError_t e = hipEventCreateWithFlags(&fresh->begin, hipEventDisableTiming);
    for (uint32_t p = 0; p < kMaxPools && e == hipSuccess; ++p) {
        e = hipStreamCreateWithFlags(&fresh->streams[p], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&fresh->acc_done[p], hipEventDisableTiming);
    }
    if (e != hipSuccess) {                                                    // a half-built state is never left in the context
        CtxFail(ctx, CGPT_ERR_HIP, "wavefront streams / events: %s", hipGetErrorString(e));
        WavefrontFree(fresh);
        return nullptr;
    }
    *slot = fresh;                                                            // fully initialised: owned by the context from here on (WavefrontFree)
    return fresh;
}

int WavefrontSetTuning(cgpt_ctx* ctx, const char* name, uint32_t value)
{
    WfHost* h = WfGetHost(ctx);                                               // created even for an unknown name
    return h ? SetKnob(ctx, FindKnob(kKnobs, name), h->tune, name, value) : CGPT_ERR_HIP;
}

// ---- what a trace launch is made of: shared by the renders (LaunchWavefront) and the trace probe (cgpt_trace_rays, cgpt_trace_first_hits) ----
// The kernel table, the two persistent grids (round 0 and the later rounds: the resident capacity of the chip for each kernel, capped by the
// trace_blocks knob), the dynamic LDS, the TraceTune of the context's knobs and the words of stack_overflow.
struct TraceLaunch {
    const decltype(&wf_trace<false, false>) (*kernels)[2][2];   // [XFORM][COUNT][FIRST]: kTraceKernels, or kTraceTreeKernels with the tree
    dim3 grid_first, grid_later;
    size_t lds = 0;
    TraceTune tune{};
    uint32_t overflow_words = 0;       // deep end of the traversal stacks: one dword per level beyond the LDS part and per thread of the largest trace grid
};

// Fills `tl` for the scene `sc` and the chosen instantiations; queries (once per LDS size, cached in h) the occupancy of every trace kernel --
// and of the shade kernels, whose cache shares the key.  0, or -1 with the context's error set.
static int PrepareTraceLaunch(cgpt_ctx* ctx, WfHost* h, const DevScene& sc, bool xform, bool count, bool tree, TraceLaunch& tl)
{
    LAUNCH_TRY(QueryCuCount(h->n_cus));
    const uint32_t n_cus = h->n_cus;
    const uint32_t top_records = std::min(h->tune.top_records, sc.n_top_records);
    const size_t trace_lds = trace_lds_bytes(top_records);
    // persistent grids = the resident capacity of the chip for each kernel
    if (h->occupancy_lds != trace_lds) {
        static_assert(TableCount(kTraceKernels) == sizeof(h->trace_blocks_per_cu) / sizeof(uint32_t) && TableCount(kTraceTreeKernels) == sizeof(h->trace_tree_blocks_per_cu) / sizeof(uint32_t), "one occupancy entry per trace kernel");
        LAUNCH_TRY(QueryOccupancy(&kTraceKernels[0][0][0], &h->trace_blocks_per_cu[0][0][0], TableCount(kTraceKernels), kTraceBlock, trace_lds));
        // shade: the round-0 and later-round instantiations share one grid size (one output segment per wave)
        uint32_t shade[2][kLobeLevels][2][2][2];
        static_assert(sizeof(shade) / sizeof(uint32_t) == TableCount(kShadeKernels), "one occupancy entry per shade kernel");
        LAUNCH_TRY(QueryOccupancy(&kShadeKernels[0][0][0][0][0], &shade[0][0][0][0][0], TableCount(kShadeKernels), 256, 0));
        for (int r = 0; r < 2; ++r)
            for (int g = 0; g < kLobeLevels; ++g)
                for (int c = 0; c < 2; ++c)
                    for (int b = 0; b < 2; ++b) h->shade_blocks_per_cu[r][g][c][b] = std::min(shade[r][g][c][0][b], shade[r][g][c][1][b]);
        h->occupancy_lds = trace_lds;
    }
    if (tree && h->tree_occupancy_lds != trace_lds) {
        LAUNCH_TRY(QueryOccupancy(&kTraceTreeKernels[0][0][0], &h->trace_tree_blocks_per_cu[0][0][0], TableCount(kTraceTreeKernels), kTraceBlock, trace_lds));
        h->tree_occupancy_lds = trace_lds;
    }
    const uint32_t (&trace_blocks)[2][2][2] = tree ? h->trace_tree_blocks_per_cu : h->trace_blocks_per_cu;
    tl.kernels = tree ? kTraceTreeKernels : kTraceKernels;
    tl.grid_first = dim3(n_cus * std::min(h->tune.max_trace_blocks, trace_blocks[xform][count][1]));
    tl.grid_later = dim3(n_cus * std::min(h->tune.max_trace_blocks, trace_blocks[xform][count][0]));
    tl.lds = trace_lds;
    tl.tune = TraceTune{ h->tune.refill_idle, h->tune.inner_repeat, h->tune.leaf_repeat, h->tune.obj_repeat, h->tune.obj_shift, top_records, h->tune.shadow_any_hit, h->tune.lds_tris, 0u, h->tune.first_lean };
    const uint32_t max_trace_threads = n_cus * std::max(*std::max_element(&h->trace_blocks_per_cu[0][0][0], &h->trace_blocks_per_cu[0][0][0] + TableCount(h->trace_blocks_per_cu)),
                                                        *std::max_element(&h->trace_tree_blocks_per_cu[0][0][0], &h->trace_tree_blocks_per_cu[0][0][0] + TableCount(h->trace_tree_blocks_per_cu))) * kTraceBlock;   // (the tree's entries are 0 until it is used)
    const uint32_t deep_levels = sc.stack_depth > kLdsStackLevels ? sc.stack_depth - kLdsStackLevels : 0u;
    tl.overflow_words = std::max(1u, deep_levels * max_trace_threads);
    return 0;
}

// path id <-> pixel of a band of n_pixels padded pixel indices in tiles_x tiles per row, for a batch of n_samples samples
static PathGrid MakePathGrid(uint32_t n_pixels, uint32_t tiles_x, uint32_t n_samples, uint32_t order)
{
    PathGrid g{};
    g.n_pixels = n_pixels; g.tiles_x = tiles_x; g.div_tiles_x = MakeFastDiv(tiles_x); g.div_n_pixels = MakeFastDiv(n_pixels);
    g.n_samples = n_samples; g.div_samples = MakeFastDiv(n_samples); g.order = order;
    return g;
}

int LaunchWavefront(cgpt_ctx* ctx, const DevRenderArgs& args_in, ShadeVariant v)
{
    hipStream_t stream = CtxStream(ctx);
    WfHost* h = WfGetHost(ctx);
    if (!h) return -1;
    const bool count = v.count;
    const uint32_t rows = args_in.n_rows;
    const uint32_t tiles_x = (args_in.width + 7u) / 8u, tiles_y = (rows + 7u) / 8u;
    const uint64_t n_pixels64 = (uint64_t)tiles_x * tiles_y * 64u;             // padded to whole 8x8 tiles
    const uint32_t pool_paths = h->tune.pool_paths_mi << 20;
    if (n_pixels64 > pool_paths) { CtxFail(ctx, CGPT_ERR_UNSUPPORTED, "band of %llu pixels exceeds the wavefront pool", (unsigned long long)n_pixels64); return -1; }
    const uint32_t n_pixels = (uint32_t)n_pixels64;
    const uint32_t rounds = (uint32_t)args_in.settings.max_ray_depth + 2u;    // extend rounds 0..max_depth, + the trailing shadow rays

    const bool xform = HonoursTransforms((int)v.lobe_level);                  // the scene has a transformed object: the XFORM trace kernels
    h->last_xform = xform;
    const bool tree = v.tree;                                                 // cgpt_set_top_level(1): the TREE trace kernels
    h->last_tree = tree;
    TraceLaunch tl;
    if (PrepareTraceLaunch(ctx, h, args_in.scene, xform, count, tree, tl) != 0) return -1;
    const uint32_t n_cus = h->n_cus;
    const dim3 block(256);
    const auto& trace_kernels = tl.kernels;
    const size_t trace_lds = tl.lds;
    const dim3 trace_grid_first = tl.grid_first, trace_grid_later = tl.grid_later;
    const bool brute = args_in.settings.render_mode != 2u;                    // the render has TracePath paths (ref: Main.cpp:719-729)
    const uint32_t brute_levels = brute ? (uint32_t)args_in.settings.max_ray_depth + 1u : 0u;
    uint32_t shade_blocks[2][2];                                              // every lobe level's shade kernels, with and without RIS, have grids of their own
    for (int c = 0; c < 2; ++c)
        for (int b = 0; b < 2; ++b) shade_blocks[c][b] = std::min(h->tune.max_shade_blocks, h->shade_blocks_per_cu[v.ris][v.lobe_level][c][b]);
    const dim3 shade_grid(n_cus * shade_blocks[count][brute]);
    // one output segment per shade wave, sized for the most 64-item blocks a wave can be handed
    const uint32_t n_segs = n_cus * std::max({ shade_blocks[0][0], shade_blocks[1][0], shade_blocks[0][1], shade_blocks[1][1] }) * 4u;
    const uint32_t min_shade_waves = n_cus * std::min({ shade_blocks[0][0], shade_blocks[1][0], shade_blocks[0][1], shade_blocks[1][1] }) * 4u;

    const uint32_t overflow_words = tl.overflow_words;

    uint32_t shade_chunk = h->tune.shade_chunk;                              // set with the batch size below (banded lists take longer chunks)
    // ---- samples per batch and batches in flight ----
    // Big batches win: every bounce round is one pass of the persistent kernels over its ray list, the late rounds of a batch
    // are short, and a short list leaves the waves draining most of their life (measured at 1080p / 256 spp: 16 spp per
    // batch x 8 pools 118 ms, 64 x 4 108 ms, 128 x 2 104 ms; one batch of 256 with nothing to overlap its tails 129 ms).  288 GB
    // of HBM is what makes that possible: a pool is ~150 B per path, 128 spp of a 1080p frame is 265 M paths = 40 GB per pool.
    // So: the largest power-of-two batch up to max_batch that fits the pool limit and leaves at least two batches (two
    // pools overlap each other's tails), within a memory budget of half the free HBM (at most budget_gib).
    const bool chains = h->tune.spec_dedupe && !count && !brute;             // specular-chain election (wf_shade)
    const size_t spec_entries = chains ? (size_t)n_pixels * h->tune.spec_keys : 0u;
    const size_t kBytesPerPath = 160 + 32 * (size_t)brute_levels;             // slots 96, state 32, lists 8, segments ~8-16; TracePath levels 32 each
    size_t free_b = 0, total_b = 0;
    LAUNCH_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t held_bytes = (size_t)h->held_pools * PoolBytes(h->held);  // what releasing the pools gives back: counted as free
    const size_t budget = std::min<size_t>((size_t)h->tune.budget_gib << 30, (free_b + held_bytes) / 2);
    uint32_t batch = h->tune.batch;
    if (batch == 0) {
        batch = 1;
        while (batch < h->tune.max_batch && (uint64_t)n_pixels * batch * 2u <= (uint64_t)pool_paths) batch *= 2u;
    }
    batch = std::max(1u, std::min({ batch, std::max(1u, args_in.n_samples / 2u), args_in.n_samples, pool_paths / n_pixels }));
    WfSizes need;
    need.n_pixels = n_pixels; need.n_segs = n_segs; need.overflow_words = overflow_words; need.brute_levels = brute_levels; need.spec = spec_entries;
    uint32_t n_pools = 0, n_batches = 0;
    for (int attempt = 0;; ++attempt) {
        for (;;) {
            need.cap = n_pixels * batch;
            n_batches = (args_in.n_samples + batch - 1u) / batch;
            const uint32_t afford = (uint32_t)std::min<size_t>(kMaxPools, budget / ((size_t)need.cap * kBytesPerPath + spec_entries * sizeof(unsigned long long)));
            n_pools = std::max(1u, std::min({ h->tune.pools, n_batches, afford }));
            if (batch == 1u || (afford >= 1u && n_pools >= std::min({ 2u, n_batches, h->tune.pools }))) break;
            batch /= 2u;                                                      // smaller batches: room for a second pool
        }
        const bool banded = h->tune.bands > 1u && need.cap >= h->tune.bands_min_paths;   // (the last, shorter batch of a render may still fall below: it keeps this chunk)
        shade_chunk = banded ? h->tune.shade_chunk_banded : h->tune.shade_chunk;
        need.seg_cap = shade_segment_blocks((need.cap + 63u) / 64u, min_shade_waves, shade_chunk) * 64u;   // whole chunks per wave; shorter items stay inside (shade_items.h)
        if (h->held_pools >= n_pools && h->held.Holds(need)) break;
        LAUNCH_TRY(hipDeviceSynchronize());
        WfRelease(h);
        hipError_t err = hipSuccess;
        for (uint32_t p = 0; p < n_pools; ++p) {
            WfDev& d = h->dev[p];
            ForEachBuffer(d, need, [&](auto*& ptr, size_t bytes) { if (err == hipSuccess && bytes) err = DevAlloc((void**)&ptr, bytes); });
            if (err == hipSuccess && d.spec_tab) err = hipMemset(d.spec_tab, 0, need.spec * sizeof(unsigned long long));   // epoch 0 is never current: all entries free
            h->spec_epoch[p] = 0;
        }
        if (err == hipSuccess) { h->held = need; h->held_pools = n_pools; break; }
        (void)hipGetLastError();                                              // out of memory: give everything back and ask for half
        WfRelease(h);
        if (batch == 1u || attempt >= 8) { CtxFail(ctx, CGPT_ERR_HIP, "wavefront pools: %s", hipGetErrorString(err)); return -1; }
        batch /= 2u;
    }

    // event pairs for the trace launches of this render
    if (ReserveEvents(ctx, h->trace_ev, 2u * n_batches * rounds) != 0) return -1;
    h->trace_rounds = rounds;

    // one-time host setup is over: the render's device time starts here (cgpt_stats.kernel_ms).  The pool streams start after
    // whatever the caller queued on the context's stream.
    LAUNCH_TRY(hipEventRecord(CtxStartEvent(ctx), stream));
    LAUNCH_TRY(hipEventRecord(h->begin, stream));
    for (uint32_t p = 0; p < n_pools; ++p) LAUNCH_TRY(hipStreamWaitEvent(h->streams[p], h->begin, 0));

    int launches = 0;
    DevRenderArgs args = args_in;
    const TraceTune tt = tl.tune;
    uint32_t k = 0;
    for (uint32_t done = 0; done < args_in.n_samples; done += batch, ++k) {
        const uint32_t p = k % n_pools;
        hipStream_t st = h->streams[p];
        const uint32_t bn = std::min(batch, args_in.n_samples - done);
        const uint32_t bfirst = args_in.first_sample + done;
        WfDev wf = h->dev[p];
        wf.cap = h->held.cap; wf.n_paths = n_pixels * bn;
        wf.rot_trace[0] = CoprimeRotation(trace_grid_later.x * (kTraceBlock / 64u), tiles_x * tiles_y);
        wf.rot_trace[1] = CoprimeRotation(trace_grid_first.x * (kTraceBlock / 64u), tiles_x * tiles_y);
        wf.rot_shade = CoprimeRotation(shade_grid.x * 4u, std::max(1u, tiles_x * tiles_y / shade_chunk));
        wf.shade_chunk = shade_chunk;
        wf.g = MakePathGrid(n_pixels, tiles_x, bn, h->tune.path_order); wf.n_segs = h->held.n_segs; wf.seg_cap = h->held.seg_cap;
        wf.n_bands = h->tune.bands > 1u && wf.n_paths >= h->tune.bands_min_paths ? h->tune.bands : 1u;   // short lists: nothing to order, and every band is a run per segment to plan and copy
        if (wf.n_bands > 1u)
            wf.band_magic = (uint32_t)std::min<uint64_t>(0xFFFFFFFFull, (((uint64_t)wf.n_bands << 32) + wf.n_paths - 1u) / wf.n_paths);   // ceil(2^32 * bands / paths)
        wf.retire_misses = h->tune.retire_misses && args_in.settings.debug_mode == 0u ? 1u : 0u;
        if (!chains) wf.spec_tab = nullptr;
        wf.spec_keys = h->tune.spec_keys;
        // (probe_scene tests mesh roots against the world ray: with a transformed object in the scene the probe is off; it walks the object
        // list, not the tree: off with the tree as well)
        wf.probe = h->tune.probe && !count && !xform && !tree && args_in.settings.debug_mode == 0u && args_in.scene.n_objects <= h->tune.probe_max_objects ? 1u : 0u;
        wf.probe_lights = h->tune.probe_lights;
        // segments of waves that a smaller shade grid does not launch must read as empty
        if (k < n_pools) LAUNCH_TRY(hipMemsetAsync(wf.seg_count, 0, 2 * (size_t)kMaxBands * wf.n_segs * sizeof(uint32_t), st));
        for (uint32_t r = 0; r < rounds; ++r) {
            const bool first = r == 0u;
            if (h->tune.trace_events) LAUNCH_TRY(hipEventRecord(NextEvent(h->trace_ev), st));
            hipLaunchKernelGGL(trace_kernels[xform][count][first], first ? trace_grid_first : trace_grid_later, dim3(kTraceBlock), trace_lds, st, args, wf, bfirst, tt);
            if (h->tune.trace_events) LAUNCH_TRY(hipEventRecord(NextEvent(h->trace_ev), st));
            ++launches;
            if (r + 1u < rounds) {
                if (wf.spec_tab) {                                            // a fresh epoch frees every entry; after spec_epochs of them, clear
                    if (++h->spec_epoch[p] > h->tune.spec_epochs) {           // the whole table: entries past this call's n_pixels * spec_keys
                                                                              // hold tags of the old epochs too, written by larger layouts
                        LAUNCH_TRY(hipMemsetAsync(wf.spec_tab, 0, h->held.spec * sizeof(unsigned long long), st));
                        h->spec_epoch[p] = 1u;
                    }
                    wf.spec_epoch = h->spec_epoch[p];
                }
                hipLaunchKernelGGL(kShadeKernels[v.ris][v.lobe_level][count][first][brute], shade_grid, block, 0, st, args, wf, bfirst);
                hipLaunchKernelGGL(wf_plan, dim3(2u * wf.n_bands), dim3(256), 0, st, wf);
                hipLaunchKernelGGL(wf_gather, dim3(std::min(2u * wf.n_segs, n_cus * 16u)), block, 0, st, wf);
                launches += 3;
            }
        }
        // accumulate in sample order: batch k after batch k-1
        if (k > 0) LAUNCH_TRY(hipStreamWaitEvent(st, h->acc_done[(k - 1u) % n_pools], 0));
        hipLaunchKernelGGL(wf_accumulate, dim3(std::min((n_pixels + 255u) / 256u, n_cus * 8u)), block, 0, st, args, wf, bfirst, bn);
        ++launches;
        LAUNCH_TRY(hipEventRecord(h->acc_done[p], st));
        LAUNCH_TRY(hipGetLastError());
    }
    // the context's stream continues after the last accumulate (which transitively follows all the others)
    if (k > 0) LAUNCH_TRY(hipStreamWaitEvent(stream, h->acc_done[(k - 1u) % n_pools], 0));
    return launches;
}

// ---- the trace probe: the pipeline's own trace launches on rays the host supplies (cgpt_trace_rays, cgpt_trace_first_hits) ---------------
// The trace step's counterpart of cgpt_shade_samples (shade_probe.hip).  No kernel of its own: a private WfDev in allocations of its own
// (never the render pools of WfHost::dev, so a context's held pools and its next render are untouched), filled as wf_shade and wf_gather
// leave a pool before a trace launch, then the launch a render makes -- PrepareTraceLaunch's kernel table, grid, LDS bytes, TraceTune and
// overflow words -- on the context's stream.  Neither kernel_launches nor the timings of cgpt_stats move.
namespace {

constexpr uint32_t kMaxProbeRays = 1u << 22;       // per kind, and padded pixels of a round-0 band
constexpr uint32_t kTraceProbeFlags = CGPT_TRACE_COUNTERS | CGPT_TRACE_REVERSED;

float4 F4(float x, float y, float z, float w) { float4 v; v.x = x; v.y = y; v.z = z; v.w = w; return v; }
float BitsToFloat(uint32_t u) { float f; memcpy(&f, &u, sizeof(f)); return f; }
uint32_t FloatToBits(float f) { uint32_t u; memcpy(&u, &f, sizeof(u)); return u; }

// what both modes start with: the variant a render of this context would run, the launch, and the kernel arguments that name the scene
struct ProbeSetup { WfHost* h; ShadeVariant v; bool xform; TraceLaunch tl; DevRenderArgs args; };
int ProbeBegin(cgpt_ctx* ctx, uint32_t flags, ProbeSetup& s)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    s.h = WfGetHost(ctx);
    if (!s.h) return CGPT_ERR_HIP;
    s.args = DevRenderArgs{};
    s.args.settings.render_mode = CGPT_MODE_ADVANCED;
    s.v = ChooseVariant(ctx, s.args.settings, (flags & CGPT_TRACE_COUNTERS) ? (uint32_t)CGPT_RENDER_COUNTERS : 0u);
    s.xform = HonoursTransforms((int)s.v.lobe_level);
    if (PrepareTraceLaunch(ctx, s.h, ctx->scene, s.xform, s.v.count, s.v.tree, s.tl) != 0) return CGPT_ERR_HIP;
    s.args.scene = ctx->scene;
    s.args.counters = ctx->counters.p;
    return CGPT_OK;
}

int TraceProbeRays(cgpt_ctx* ctx, const float* ext_o, const float* ext_d, const float* ext_tmax, uint32_t n_ext, const float* sh_o, const float* sh_d,
                   const float* sh_tmax, uint32_t n_sh, uint32_t flags, float* out_t, uint32_t* out_obj, uint32_t* out_tri, uint32_t* out_depth, uint8_t* out_occluded)
{
    ProbeSetup s;
    int rc = ProbeBegin(ctx, flags, s);
    if (rc != CGPT_OK) return rc;
    const bool reversed = (flags & CGPT_TRACE_REVERSED) != 0u;
    const uint32_t cap = std::max(n_ext, n_sh);
    auto ext_slot = [&](uint32_t i) { return reversed ? n_ext - 1u - i : i; };           // the slot of extend ray i = entry i of its list
    auto sh_slot = [&](uint32_t j) { return reversed ? n_sh - 1u - j : j; };             // (+ cap)

    // the slots as wf_shade leaves them (the follower and same-ray bits of B.w are pipeline state: 0) and the lists as wf_gather does
    std::vector<float4> A(2 * (size_t)cap, F4(0, 0, 0, 0)), B(A), C(A);
    std::vector<uint32_t> list_ext(cap, 0u), list_sh(cap, 0u);
    for (uint32_t i = 0; i < n_ext; ++i) {
        const uint32_t slot = ext_slot(i);
        const float tm = ext_tmax ? ext_tmax[i] : 1e34f;
        A[slot] = F4(ext_o[3 * (size_t)i], ext_o[3 * (size_t)i + 1], ext_o[3 * (size_t)i + 2], tm);
        B[slot] = F4(ext_d[3 * (size_t)i], ext_d[3 * (size_t)i + 1], ext_d[3 * (size_t)i + 2], 0.0f);
        // "no hit": what a slot that retire_misses leaves unwritten reads as, and the payload a ray with tmax != 1e34f starts from
        C[slot] = F4(BitsToFloat(kNoHit), 0.0f, 0.0f, tm);
        list_ext[i] = slot;
    }
    for (uint32_t j = 0; j < n_sh; ++j) {
        const uint32_t slot = sh_slot(j);
        A[cap + slot] = F4(sh_o[3 * (size_t)j], sh_o[3 * (size_t)j + 1], sh_o[3 * (size_t)j + 2], sh_tmax ? sh_tmax[j] : 1e34f);
        B[cap + slot] = F4(sh_d[3 * (size_t)j], sh_d[3 * (size_t)j + 1], sh_d[3 * (size_t)j + 2], 0.0f);
        C[cap + slot] = F4(1.0f, 1.0f, 1.0f, 0.0f);                                      // the pending energy: arrives in st_en iff the ray is not occluded
        list_sh[j] = slot;
    }
    const uint32_t plan[2] = { n_ext, n_sh };
    std::vector<float4> en(n_sh);                                                        // the host ends of the copies back: declared before the device
    std::vector<uint8_t> flag(n_ext);                                                    // buffers, so that on any return they outlive the frees, which wait for the device

    DevBuf<float4> dA, dB, dC, d_en;
    DevBuf<uint8_t> d_flag;
    DevBuf<uint32_t> d_list_ext, d_list_sh, d_plan, d_overflow;
    HIP_TRY(ctx, dA.Alloc(2 * (size_t)cap)); HIP_TRY(ctx, dB.Alloc(2 * (size_t)cap)); HIP_TRY(ctx, dC.Alloc(2 * (size_t)cap));
    HIP_TRY(ctx, d_en.Alloc(cap)); HIP_TRY(ctx, d_flag.Alloc(cap));
    HIP_TRY(ctx, d_list_ext.Alloc(cap)); HIP_TRY(ctx, d_list_sh.Alloc(cap));
    HIP_TRY(ctx, d_plan.Alloc(2 + 2 * (size_t)kMaxBands)); HIP_TRY(ctx, d_overflow.Alloc(s.tl.overflow_words));
    hipStream_t st = ctx->stream;
    const size_t slot_bytes = 2 * (size_t)cap * sizeof(float4);
    HIP_TRY(ctx, hipMemcpyAsync(dA.p, A.data(), slot_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dB.p, B.data(), slot_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dC.p, C.data(), slot_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(d_en.p, 0, (size_t)cap * sizeof(float4), st));
    HIP_TRY(ctx, hipMemsetAsync(d_flag.p, 0, cap, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_list_ext.p, list_ext.data(), (size_t)cap * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_list_sh.p, list_sh.data(), (size_t)cap * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(d_plan.p, 0, (2 + 2 * (size_t)kMaxBands) * sizeof(uint32_t), st));
    HIP_TRY(ctx, hipMemcpyAsync(d_plan.p, plan, sizeof(plan), hipMemcpyHostToDevice, st));

    WfDev wf{};
    wf.A = dA.p; wf.B = dB.p; wf.C = dC.p; wf.st_en = d_en.p; wf.hit_flag = d_flag.p;
    wf.list_ext = d_list_ext.p; wf.list_sh = d_list_sh.p; wf.plan = d_plan.p; wf.stack_overflow = d_overflow.p;
    wf.cap = cap; wf.n_paths = n_ext; wf.n_bands = 1u;
    wf.g = MakePathGrid(64u, 1u, 1u, s.h->tune.path_order);                              // no frame: never read by a later round's trace
    wf.retire_misses = s.h->tune.retire_misses;                                          // the knob alone: a render also turns it off for the debug views, which the probe has none of
    const uint32_t n_blocks = (n_ext + 63u) / 64u + (n_sh + 63u) / 64u;                  // the lists' 64-ray blocks stand in for the band's tiles
    wf.rot_trace[0] = CoprimeRotation(s.tl.grid_later.x * (kTraceBlock / 64u), n_blocks);
    hipLaunchKernelGGL(s.tl.kernels[s.xform][s.v.count][0], s.tl.grid_later, dim3(kTraceBlock), s.tl.lds, st, s.args, wf, 0u, s.tl.tune);
    HIP_TRY(ctx, hipGetLastError());

    if (n_ext) HIP_TRY(ctx, hipMemcpyAsync(C.data(), dC.p, (size_t)n_ext * sizeof(float4), hipMemcpyDeviceToHost, st));
    if (n_ext) HIP_TRY(ctx, hipMemcpyAsync(flag.data(), d_flag.p, n_ext, hipMemcpyDeviceToHost, st));
    if (n_sh) HIP_TRY(ctx, hipMemcpyAsync(en.data(), d_en.p, (size_t)n_sh * sizeof(float4), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (uint32_t i = 0; i < n_ext; ++i) {
        const float4 c = C[ext_slot(i)];
        out_obj[i] = FloatToBits(c.x); out_tri[i] = FloatToBits(c.y); out_depth[i] = FloatToBits(c.z); out_t[i] = c.w;
        // wf_shade takes the rays whose byte is 1: the byte and the record must tell the same story
        if (wf.retire_misses && (flag[ext_slot(i)] != 0) != (out_obj[i] != kNoHit))
            return CtxFail(ctx, CGPT_ERR_HIP, "extend ray %u: hit_flag %u beside the record of object %u", i, (unsigned)flag[ext_slot(i)], out_obj[i]);
    }
    for (uint32_t j = 0; j < n_sh; ++j) {
        const float4 e = en[sh_slot(j)];
        out_occluded[j] = (e.x != 0.0f || e.y != 0.0f || e.z != 0.0f) ? (uint8_t)0 : (uint8_t)1;
    }
    return CGPT_OK;
}

int TraceProbeFirstHits(cgpt_ctx* ctx, const cgpt_camera* camera, uint32_t width, uint32_t height, uint32_t row_begin, uint32_t row_end, uint32_t flags,
                        uint32_t tiles_x, uint32_t n_pixels, uint32_t* out_obj, uint32_t* out_tri, uint32_t* out_depth, float* out_t)
{
    ProbeSetup s;
    int rc = ProbeBegin(ctx, flags, s);
    if (rc != CGPT_OK) return rc;
    const uint32_t rows = row_end - row_begin;
    memcpy(&s.args.camera, camera, sizeof(DevCamera));
    s.args.width = width; s.args.height = height;
    s.args.n_rows = rows; s.args.band_first = row_begin; s.args.band_h = rows; s.args.band_stride = 0u;
    s.args.n_samples = 1u;

    std::vector<float4> hit(n_pixels);                                                   // before the device buffers: see TraceProbeRays
    DevBuf<float4> d_hit;
    DevBuf<uint32_t> d_overflow;
    HIP_TRY(ctx, d_hit.Alloc(n_pixels)); HIP_TRY(ctx, d_overflow.Alloc(s.tl.overflow_words));
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemsetAsync(d_hit.p, 0, (size_t)n_pixels * sizeof(float4), st));    // (the padded indices stay unwritten)
    WfDev wf{};
    wf.px_hit = d_hit.p; wf.stack_overflow = d_overflow.p;
    wf.cap = n_pixels; wf.n_paths = n_pixels; wf.n_bands = 1u;
    wf.g = MakePathGrid(n_pixels, tiles_x, 1u, s.h->tune.path_order);                    // one sample: every pixel ray counts once
    wf.rot_trace[1] = CoprimeRotation(s.tl.grid_first.x * (kTraceBlock / 64u), n_pixels / 64u);
    hipLaunchKernelGGL(s.tl.kernels[s.xform][s.v.count][1], s.tl.grid_first, dim3(kTraceBlock), s.tl.lds, st, s.args, wf, 0u, s.tl.tune);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(hit.data(), d_hit.p, (size_t)n_pixels * sizeof(float4), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    // pixel indices run over 8x8 tiles in row-major tile order, row-major inside a tile (trace_steps.hpp: pixel_of_index)
    for (uint32_t p = 0; p < n_pixels; ++p) {
        const uint32_t tile = p >> 6, l = p & 63u, ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const uint32_t px = tx * 8u + (l & 7u), row = ty * 8u + (l >> 3);
        if (px >= width || row >= rows) continue;
        const size_t k = (size_t)row * width + px;
        out_obj[k] = FloatToBits(hit[p].x); out_tri[k] = FloatToBits(hit[p].y); out_depth[k] = FloatToBits(hit[p].z); out_t[k] = hit[p].w;
    }
    return CGPT_OK;
}

}  // namespace

}  // namespace cgpt

using namespace cgpt;

extern "C" int cgpt_trace_rays(cgpt_ctx* ctx, const float* ext_origins, const float* ext_dirs, const float* ext_tmax, uint32_t n_extend,
                               const float* sh_origins, const float* sh_dirs, const float* sh_tmax, uint32_t n_shadow, uint32_t flags,
                               float* out_t, uint32_t* out_obj, uint32_t* out_tri, uint32_t* out_depth, uint8_t* out_occluded)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return CtxFail(ctx, CGPT_ERR_UNSUPPORTED, "cgpt_trace_rays: a one-device context only");
    if (!ctx->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "cgpt_trace_rays before cgpt_scene_upload");
    if (flags & ~kTraceProbeFlags) return CtxFail(ctx, CGPT_ERR_INVALID, "unknown flag bits 0x%x", flags & ~kTraceProbeFlags);
    if (n_extend > kMaxProbeRays || n_shadow > kMaxProbeRays) return CtxFail(ctx, CGPT_ERR_INVALID, "%u extend and %u shadow rays: at most %u of each", n_extend, n_shadow, kMaxProbeRays);
    if (n_extend && (!ext_origins || !ext_dirs || !out_t || !out_obj || !out_tri || !out_depth)) return CtxFail(ctx, CGPT_ERR_INVALID, "null argument of the extend rays");
    if (n_shadow && (!sh_origins || !sh_dirs || !out_occluded)) return CtxFail(ctx, CGPT_ERR_INVALID, "null argument of the shadow rays");
    if (n_extend == 0u && n_shadow == 0u) return CGPT_OK;
    return Guarded(ctx, __func__, [&] {
        return TraceProbeRays(ctx, ext_origins, ext_dirs, ext_tmax, n_extend, sh_origins, sh_dirs, sh_tmax, n_shadow, flags, out_t, out_obj, out_tri, out_depth, out_occluded);
    });
}

extern "C" int cgpt_trace_first_hits(cgpt_ctx* ctx, const cgpt_camera* camera, uint32_t width, uint32_t height, uint32_t row_begin, uint32_t row_end,
                                     uint32_t flags, uint32_t* out_obj, uint32_t* out_tri, uint32_t* out_depth, float* out_t)
{
    if (!ctx) return CGPT_ERR_INVALID;
    if (ctx->group) return CtxFail(ctx, CGPT_ERR_UNSUPPORTED, "cgpt_trace_first_hits: a one-device context only");
    if (!ctx->has_scene) return CtxFail(ctx, CGPT_ERR_NO_SCENE, "cgpt_trace_first_hits before cgpt_scene_upload");
    if (flags & ~(uint32_t)CGPT_TRACE_COUNTERS) return CtxFail(ctx, CGPT_ERR_INVALID, "unknown flag bits 0x%x", flags & ~(uint32_t)CGPT_TRACE_COUNTERS);
    if (!camera || !out_obj || !out_tri || !out_depth || !out_t) return CtxFail(ctx, CGPT_ERR_INVALID, "null argument");
    if (width == 0 || height == 0 || row_begin >= row_end || row_end > height)
        return CtxFail(ctx, CGPT_ERR_INVALID, "bad frame/rows: %ux%u rows [%u,%u)", width, height, row_begin, row_end);
    const uint64_t tiles_x = ((uint64_t)width + 7u) / 8u, tiles_y = ((uint64_t)(row_end - row_begin) + 7u) / 8u;
    if ((uint64_t)width * height > 0xFFFFFFFFull || tiles_x * tiles_y * 64u > kMaxProbeRays)
        return CtxFail(ctx, CGPT_ERR_INVALID, "a band of %llu padded pixels: at most %u", (unsigned long long)(tiles_x * tiles_y * 64u), kMaxProbeRays);
    return Guarded(ctx, __func__, [&] {
        return TraceProbeFirstHits(ctx, camera, width, height, row_begin, row_end, flags, (uint32_t)tiles_x, (uint32_t)(tiles_x * tiles_y * 64u), out_obj, out_tri, out_depth, out_t);
    });
}
