// shade_items.h -- how long a work item of wf_shade is, and what that makes of a wave's output segment; host + device.
// A shade wave takes items of `item` consecutive 64-path blocks of the round's list: item k is the blocks [k * item, (k + 1) * item),
// dealt in rows of n_waves items (trace_steps.hpp: next_block).  The configured length `chunk` suits a list that gives every wave at
// least one whole item; a shorter list would leave most waves without work while a few walk `chunk` blocks one after the other, every
// pass a chain of dependent misses.  Such a list gets shorter items -- a power of two, down to kShadeItemMin blocks -- so that its
// blocks spread over the waves.
// The bound the segments depend on: a wave is never dealt more blocks than shade_segment_blocks(cap_blocks, min_waves, chunk), what the
// host sizes a segment for, whenever n_blocks <= cap_blocks and n_waves >= min_waves.
//   * n_blocks >= n_waves * chunk: item = chunk, and shade_wave_blocks() only grows with n_blocks and shrinks with n_waves.
//   * shorter: with the configured chunk the list is at most one row, a wave gets at most `chunk` blocks, and a segment holds at least
//     that many (shade_segment_blocks is a positive multiple of chunk for cap_blocks >= 1).  A shorter item is taken only where its rows
//     times its length stay within `chunk`: rows <= chunk / item, tested as items <= (chunk / item) * n_waves.  An item of one block
//     always passes (n_blocks < n_waves * chunk), so the search ends; an answer below kShadeItemMin is replaced by `chunk` itself.  Flooring n_blocks / n_waves alone would not do: chunk 5,
//     n_blocks = 5 n_waves - 1, item 2 makes three rows, six blocks.
// tests/test_host_shade_items.py sweeps the bound through cgpth_shade_item_blocks / cgpth_shade_segment_blocks and by dealing the blocks.
#pragma once
#include <cstdint>

#include "fast_div.h"

namespace cgpt {

// most blocks a wave is dealt: whole rows of items (the last item of a list may be shorter; the bound does not use that)
CGPT_HD inline uint32_t shade_wave_blocks(uint32_t n_blocks, uint32_t n_waves, uint32_t item)
{
    const uint32_t items = (n_blocks + item - 1u) / item;
    return ((items + n_waves - 1u) / n_waves) * item;
}

// blocks of one output segment (x 64 entries): whole chunks per wave of the smallest shade grid, for a full pool
CGPT_HD inline uint32_t shade_segment_blocks(uint32_t cap_blocks, uint32_t min_waves, uint32_t chunk)
{
    return shade_wave_blocks(cap_blocks, min_waves, chunk);
}

// Items are never shorter than this: the survivors a wave appends from consecutive blocks are neighbours in the image, and that grouping
// is what the plain lists' chunk of 4 was measured for.  Items of one block made the calls with plain lists 3-4 % slower (8 and 16
// samples at 1080p, C2; profiles/r22/ab_batch_tail.txt) -- the next round's trace pays for the mixing -- so a chunk of at most 4 is
// left as it is.
static constexpr uint32_t kShadeItemMin = 4;

// item length for a list of n_blocks blocks walked by n_waves waves, at most `chunk` (>= 1); wave-uniform, shifts and compares only
CGPT_HD inline uint32_t shade_item_blocks(uint32_t n_blocks, uint32_t n_waves, uint32_t chunk)
{
    if ((uint64_t)n_blocks >= (uint64_t)n_waves * chunk) return chunk;
    uint32_t k = 0;                                                           // item = 2^k: at most max(n_blocks / n_waves, kShadeItemMin), at most chunk
    while ((2u << k) <= chunk && (((uint64_t)n_waves << (k + 1u)) <= n_blocks || (2u << k) <= kShadeItemMin)) ++k;
    while (k > 0u && (uint64_t)((n_blocks + (1u << k) - 1u) >> k) > (uint64_t)(chunk >> k) * n_waves) --k;
    return (1u << k) >= kShadeItemMin ? 1u << k : chunk;                      // (one row of whole chunks: what the segments were always sized for)
}

}  // namespace cgpt
