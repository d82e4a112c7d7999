"""The work-item rule of wf_shade (csrc/device/shade_items.h) through the host C API: cgpth_shade_item_blocks is the length the kernel
takes for a list, cgpth_shade_segment_blocks what the launcher sizes a wave's output segment for.

The bound that keeps a wave inside its segment: for every list of n_blocks <= cap_blocks blocks walked by n_waves >= min_waves waves, a wave
is dealt at most cgpth_shade_segment_blocks(cap_blocks, min_waves, chunk) blocks (each appends at most 64 entries per kind).  Swept over
chunks 1..256 (non-powers of two included), grids from one wave to more than the chip holds, and the list lengths at which the rule
changes its answer; then checked once more by dealing the blocks exactly as the kernel's loop does (first_block / next_block /
advance), where also every block must be dealt once and a wave's blocks must ascend (the band runs depend on it)."""
import pytest

from cpugpupathtracing_amd import _native as N

WAVES = (1, 2, 3, 4, 64, 1000, 1024, 5120, 7168)
ITEM_MIN = 4          # shade_items.h: kShadeItemMin


@pytest.fixture(scope="module")
def lib():
    return N.lib()


def _wave_blocks(n_blocks, n_waves, item):
    """most blocks of one wave: whole rows of items"""
    items = -(-n_blocks // item)
    return -(-items // n_waves) * item


def _lengths(n_waves, chunk, cap_blocks):
    """list lengths around every point at which the rule can change: multiples of n_waves * 2^k, of n_waves * chunk, and the ends"""
    out = {0, 1, 2, cap_blocks}
    marks = [n_waves * chunk, 2 * n_waves * chunk, n_waves * chunk // 2]
    k = 1
    while k <= 2 * chunk:
        marks += [n_waves * k, n_waves * k + k, (chunk // k) * k * n_waves, (chunk // k) * n_waves * k - k]
        k *= 2
    for m in marks:
        out.update((m - 1, m, m + 1))
    out.update(range(0, min(cap_blocks, 3 * n_waves) + 1, max(1, n_waves // 3)))
    return sorted(n for n in out if 0 <= n <= cap_blocks)


def test_rule_and_bound(lib):
    checked = 0
    for chunk in range(1, 257):
        for min_waves in WAVES:
            for n_waves in {min_waves, min_waves + 1, 2 * min_waves, 7 * min_waves}:
                for cap_blocks in {1, n_waves, n_waves * chunk - 1, n_waves * chunk + 1, 3 * min_waves * chunk + 5, 4147200}:   # 4147200: 1080p x 128 samples
                    if cap_blocks < 1:
                        continue
                    segment = lib.cgpth_shade_segment_blocks(cap_blocks, min_waves, chunk)
                    assert segment == _wave_blocks(cap_blocks, min_waves, chunk) and segment % chunk == 0 and segment >= chunk
                    for n_blocks in _lengths(n_waves, chunk, cap_blocks):
                        item = lib.cgpth_shade_item_blocks(n_blocks, n_waves, chunk)
                        where = (n_blocks, n_waves, chunk, item)
                        assert 1 <= item <= chunk, where
                        if n_blocks >= n_waves * chunk:
                            assert item == chunk, where                      # walked exactly as with the knob alone
                        elif item != chunk:
                            assert item & (item - 1) == 0 and item >= ITEM_MIN, where
                            assert item == ITEM_MIN or item * n_waves <= n_blocks, where    # never longer than the list gives every wave
                        if chunk <= ITEM_MIN:
                            assert item == chunk, where                      # the plain lists' chunk of 4 and the test knobs below it: untouched
                        elif chunk % ITEM_MIN == 0 and n_blocks < 2 * ITEM_MIN * n_waves:
                            assert item == ITEM_MIN, where
                        assert _wave_blocks(n_blocks, n_waves, item) <= segment, (where, segment)
                        checked += 1
    assert checked > 500000


def test_power_of_two_chunks_halve(lib):
    """chunk 32 on the production grid: the largest power of two a list gives every wave, as the issue's rule, but never below four"""
    n_waves = 5120
    for per, want in ((0, 4), (1, 4), (2, 4), (3, 4), (4, 4), (7, 4), (8, 8), (15, 8), (16, 16), (20, 16), (31, 16), (32, 32), (100, 32)):
        assert lib.cgpth_shade_item_blocks(per * n_waves + 17, n_waves, 32) == want, per
    # flooring alone would take 2: three rows, six blocks in a five-block segment; 1 would be safe and is below the floor: the chunk stays
    assert lib.cgpth_shade_item_blocks(5 * 7 - 1, 7, 5) == 5
    assert lib.cgpth_shade_item_blocks(6 * 7 - 1, 7, 12) == 4
    assert lib.cgpth_shade_item_blocks(10, 0, 4) == 0 and lib.cgpth_shade_item_blocks(10, 4, 0) == 0


def _deal(n_blocks, n_waves, item, rot):
    """the blocks each wave takes, in the order wf_shade's loop takes them"""
    taken = []
    for wave in range(n_waves):
        row_base, pos = 0, wave
        block = wave * item
        mine = []
        while block < n_blocks:
            mine.append(block)
            block += 1
            if block >= min((row_base + pos + 1) * item, n_blocks):
                row_base += n_waves
                pos += rot
                if pos >= n_waves:
                    pos -= n_waves
                block = (row_base + pos) * item
        taken.append(mine)
    return taken


@pytest.mark.parametrize("n_waves", [1, 2, 3, 5, 8])
def test_dealing_the_blocks(lib, n_waves):
    for chunk in (1, 2, 3, 4, 5, 6, 7, 8, 12, 32):
        for min_waves in {1, n_waves}:
            cap_blocks = 2 * n_waves * chunk + 2
            segment = lib.cgpth_shade_segment_blocks(cap_blocks, min_waves, chunk)
            for n_blocks in range(cap_blocks + 1):
                item = lib.cgpth_shade_item_blocks(n_blocks, n_waves, chunk)
                for rot in {0, 1 % n_waves, n_waves - 1}:
                    taken = _deal(n_blocks, n_waves, item, rot)
                    assert sorted(b for t in taken for b in t) == list(range(n_blocks))
                    for t in taken:
                        assert t == sorted(t) and len(t) <= segment, (n_blocks, n_waves, chunk, item, rot)
                if n_blocks < n_waves * chunk and n_blocks > 0:          # a short list reaches as many waves as it has items
                    assert sum(1 for t in taken if t) == min(n_waves, -(-n_blocks // item))
