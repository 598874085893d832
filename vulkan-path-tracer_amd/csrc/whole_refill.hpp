// whole_refill.hpp — how a wave of the whole-path kernel (kernels_whole.hip k_whole) comes by its fresh samples: the tile cursor and the
// wave's buffer of generated camera rays.  Plain integer arithmetic on wave-uniform values, compiled for the device and — by
// tests/tools/whole_refill_driver.cpp — for the host, where tests/test_whole_refill_cpu.py plays whole grids of waves against it.
//
// The batch's launch indices [0, n) are dealt in tiles of kTile.  Wave w of W takes tiles w, w + W, ... for its first `static_rounds` rounds
// without an atomic, and the tiles behind them (from dyn_first on) a chunk at a time through one shared counter: the caller does the
// atomicAdd of dyn_take() and hands the counter's old value to take_dynamic().
// A wave never generates a camera ray on part of its lanes: when its free lanes want more rays than its buffer holds they first take
// what is left (pop), and then ALL lanes generate the next kTile launch indices of the wave's range — lane j takes w_next + j, live
// where j < gen_count() — into the buffer, from whose front the free lanes go on popping.  The buffer is only ever filled when it is
// empty, so `head` runs from 0 and it needs no wrap.  Every launch index is a path: a launch with a screen rectangle (camera_cull.hpp) has
// no index for a sample outside it (whole_deal.hpp).
// A wave is out of fresh samples when its cursor is done AND its buffer is empty;
// the cursor is only asked for more with an empty buffer, so a wave cannot stop with entries left.
#pragma once
#include <stdint.h>

#include "../../include/vpt_fp32.h"   // VPT_HD

namespace vpt {
namespace refill {

constexpr uint32_t kTile = 64u;   // launch indices per tile = entries of a wave's buffer = lanes of a wave

struct Shape {          // the same for every wave of a launch (little state on purpose: the kernel keeps it in scalar registers)
    uint32_t n;         // launch indices of the batch
    uint32_t n_waves;
    uint32_t static_rounds;
    uint32_t chunk_tiles;   // tiles per atomic (bits 0-7); bit 8: guided
};
VPT_HD uint32_t n_tiles(const Shape& s) { return (s.n + kTile - 1u) / kTile; }
VPT_HD uint32_t dyn_first(const Shape& s) { return s.static_rounds * s.n_waves; }   // tiles from here on are taken through the counter

struct Cursor {
    uint32_t next_static;    // the wave's next tile of the static rounds: wave, wave + n_waves, ... while below dyn_first
    uint32_t w_next, w_end;  // the wave's current range of launch indices
    uint32_t last_seen;      // how far the tile counter had got when this wave last took from it
    bool done;               // the wave asked for a tile and there was none
};
VPT_HD Cursor make_cursor(const Shape& s, uint32_t wave_index) {
    Cursor c;
    c.next_static = wave_index; c.w_next = 0u; c.w_end = 0u; c.last_seen = dyn_first(s); c.done = false;
    return c;
}
VPT_HD bool range_empty(const Cursor& c) { return c.w_next >= c.w_end; }
VPT_HD void set_range(const Shape& s, Cursor& c, uint32_t tile, uint32_t span) {
    if (tile >= n_tiles(s)) { c.done = true; return; }
    c.w_next = tile * kTile;
    c.w_end = (tile + span) * kTile < s.n ? (tile + span) * kTile : s.n;
}
// The next range without the counter; false: the static rounds are used up, go through dyn_take / take_dynamic.
VPT_HD bool take_static(const Shape& s, Cursor& c) {
    if (c.next_static >= dyn_first(s)) return false;
    const uint32_t tile = c.next_static;
    c.next_static += s.n_waves;
    set_range(s, c, tile, 1u);
    return true;
}
// Tiles to add to the counter.  Guided: the chunk shrinks with what is left — by this wave's last look at the counter — so that the
// waves run dry within a tile of each other.
VPT_HD uint32_t dyn_take(const Shape& s, const Cursor& c) {
    uint32_t take = s.chunk_tiles & 0xffu;
    if (s.chunk_tiles & 0x100u) {
        const uint32_t left_tiles = n_tiles(s) > c.last_seen ? n_tiles(s) - c.last_seen : 0u, fair = left_tiles / (2u * s.n_waves);
        take = fair < 1u ? 1u : (fair < take ? fair : take);
    }
    return take;
}
VPT_HD void take_dynamic(const Shape& s, Cursor& c, uint32_t counter_before, uint32_t take) {
    const uint32_t tile = dyn_first(s) + counter_before;
    c.last_seen = tile + take;
    set_range(s, c, tile, take);
}

struct Fresh { uint32_t head, count; };   // generated rays not handed out yet: entries [head, head + count) of the wave's buffer
VPT_HD Fresh make_fresh() { Fresh f; f.head = 0u; f.count = 0u; return f; }
// Lanes that generate in a pass over a non-empty range: lane j < gen_count takes launch index w_next + j and writes entry j.
VPT_HD uint32_t gen_count(const Cursor& c) { const uint32_t left = c.w_end - c.w_next; return left < kTile ? left : kTile; }
VPT_HD void generated(Cursor& c, Fresh& f, uint32_t g) { c.w_next += g; f.head = 0u; f.count = g; }
// `want` free lanes pop: the lane with r free lanes below it takes entry head_before + r when r < the returned count.
VPT_HD uint32_t pop(Fresh& f, uint32_t want) {
    const uint32_t k = want < f.count ? want : f.count;
    f.head += k; f.count -= k;
    return k;
}
VPT_HD bool exhausted(const Cursor& c, const Fresh& f) { return c.done && f.count == 0u; }

}  // namespace refill
}  // namespace vpt
