// whole_deal.hpp — how a launch of the whole-path kernel (kernels_whole.hip k_whole) that has a screen rectangle (camera_cull.hpp) deals its launch
// indices: over the samples INSIDE the rectangle only.  A sample outside starts no path and takes no lane; its frame sum, exactly zero, is written
// in runs of whole waves' stores (run_after), and the launch counts its one ray as a constant (culled()).
// Plain integer arithmetic, compiled for the device and — by tests/tools/whole_deal_driver.cpp — for the host (tests/test_whole_deal_cpu.py).
//
// The index space.  Of a shard (rows y = shard_rank + shard_count * ys of the image) the rectangle [x0, x1] x [y0, y1] holds the columns x0 .. x0 + rw - 1
// of the shard rows ys0 .. ys0 + rh - 1: rect_px = rw * rh samples per frame, and launch index li of a launch of F frames, li < F * rect_px, is
//   f = li / rect_px,  r = li - f * rect_px,  ry = r / rw,  x = x0 + r - ry * rw,  ys = ys0 + ry,  y = shard_rank + shard_count * ys,
//   slot = f * shard_pixels + ys * width + x
// — the slot, seed and camera ray the sample has in a launch without a rectangle (shade_core.hpp pixel_of_slot), so ACC is addressed as ever.
// The two divisions are the compiler's, as pixel_of_slot's are: a multiply-high and a shift by constants the host passes measured +0.13 % on top
// of this, under the bar (profiles/REJECTED.md r21).
// Under split-screen dispatch (RenderParams::split > 1) a dispatch covers one chunk's pixels and the rectangle's share of them differs from chunk
// to chunk: RenderParams::launch_off then holds the prefix sums of split_rect_px() and decode_split() takes a launch index apart (those batches
// are not what anything is timed on).
#pragma once
#include <stdint.h>

#include "camera_cull.hpp"

namespace vpt {
namespace deal {

// What a launch with a rectangle hands its lanes (argument words behind WholeArgs: whole_args.hpp WholeLaunch): the rectangle in the shard, and for
// the runs of samples outside it (run_after) the gap between two of its rows, the last inside sample of a frame, the first one, and the launch's slots.
struct Deal { uint32_t x0, rw, ys0, rect_px, gap, last_in_frame, head, slots; };
// Shard rows ys with first <= shard_rank + shard_count * ys <= last: the first of them and how many.
VPT_HD void shard_rows(uint32_t first, uint32_t last, uint32_t shard_rank, uint32_t shard_count, uint32_t& ys0, uint32_t& rh) {
    ys0 = first > shard_rank ? (first - shard_rank + shard_count - 1u) / shard_count : 0u;
    rh = 0u;
    if (first > last || last < shard_rank) return;
    const uint32_t ys1 = (last - shard_rank) / shard_count;
    if (ys1 >= ys0) rh = ys1 - ys0 + 1u;
}
// r: a rectangle that is not "everything" (r.x0 > r.x1: nothing inside, rect_px == 0: a launch with no index to deal, which only counts).
// slots: frames * shard_pixels of the launch.
VPT_HD Deal make(const cull::Rect& r, uint32_t shard_rank, uint32_t shard_count, uint32_t width, uint32_t slots) {
    Deal d; d.x0 = r.x0; d.rw = 0u; d.ys0 = 0u; d.rect_px = 0u; d.gap = 0u; d.last_in_frame = 0u; d.head = 0u; d.slots = slots;
    uint32_t rh = 0u;
    if (r.x0 <= r.x1 && r.y0 <= r.y1) { d.rw = r.x1 - r.x0 + 1u; shard_rows(r.y0, r.y1, shard_rank, shard_count, d.ys0, rh); }
    d.rect_px = d.rw * rh;
    if (d.rect_px != 0u) { d.gap = width - d.rw; d.head = d.ys0 * width + d.x0; d.last_in_frame = (d.ys0 + rh - 1u) * width + d.x0 + d.rw - 1u; }
    return d;
}
VPT_HD void decode(const Deal& d, uint32_t shard_pixels, uint32_t width, uint32_t shard_rank, uint32_t shard_count, uint32_t li,
                   uint32_t& slot, uint32_t& x, uint32_t& y, uint32_t& f) {
    f = li / d.rect_px;
    const uint32_t r = li - f * d.rect_px, ry = r / d.rw, ys = d.ys0 + ry;
    x = d.x0 + r - ry * d.rw;
    y = shard_rank + shard_count * ys;
    slot = f * shard_pixels + ys * width + x;
}
// The samples OUTSIDE the rectangle still get their frame sum, zero, from the launch (the resolve reads every slot): in slot order they lie in runs
// between the rectangle's rows, and the wave that deals the last sample of a row writes the run behind it — 64 slots per store, no index taken
// apart.  run_after: that run, [first, end), for the row's last sample `slot`: up to the next row's first sample, or, behind a frame's last row
// (frame_end(): the sample is the frame's last inside one), through the rows below, across the frame's end and the next frame's rows above to its
// first inside sample — or to the launch's last slot.  The slots before the launch's first inside sample, [0, d.head), are the wave's that deals
// launch index 0.  The kernel calls these two on wave-uniform values (kernels_whole.hip's refill step): what the host test checks is what runs.
VPT_HD bool frame_end(const Deal& d, uint32_t shard_pixels, uint32_t f, uint32_t slot) { return slot - f * shard_pixels == d.last_in_frame; }
VPT_HD void run_after(const Deal& d, uint32_t shard_pixels, uint32_t slot, bool at_frame_end, uint32_t& first, uint32_t& end) {
    first = slot + 1u;
    if (!at_frame_end) { end = first + d.gap; return; }
    const uint32_t next = slot - d.last_in_frame + shard_pixels + d.head;   // (slot - last_in_frame: the frame's first slot)
    end = next < d.slots ? next : d.slots;
}
// The rays a launch of `frames` frames counts without tracing them: one closest-hit ray per sample outside the rectangle.
VPT_HD uint64_t culled(uint32_t frames, uint32_t shard_pixels, uint32_t rect_px) { return (uint64_t)frames * (shard_pixels - rect_px); }

// ---- split-screen dispatch: chunk c = (cx, cy) of S x S holds the pixels (lx * S + cx, ly * S + cy) (shade_core.hpp launch_pixel)
// The chunk coordinates l with first <= l * S + c <= last: the first of them and how many.
VPT_HD void split_axis(uint32_t first, uint32_t last, uint32_t c, uint32_t S, uint32_t& l0, uint32_t& n) { shard_rows(first, last, c, S, l0, n); }
VPT_HD uint32_t split_rect_px(const cull::Rect& r, uint32_t chunk, uint32_t S) {
    uint32_t lx0, lw, ly0, lh;
    split_axis(r.x0, r.x1, chunk % S, S, lx0, lw); split_axis(r.y0, r.y1, chunk / S, S, ly0, lh);
    return lw * lh;
}
// Launch index li of a batch whose dispatch k starts at off[k] (prefix sums of split_rect_px) over the rectangle [x0, x1] x [y0, y1] — or over the
// whole image, (0, 0) - (width - 1, height - 1), where this is launch_pixel's split-screen branch (shade_core.hpp) and off[] the chunks' sizes.
template <class Off>
VPT_HD void decode_split(uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1, uint32_t S, uint32_t width, uint32_t shard_pixels, const Off& off, uint32_t dispatch_base,
                         uint32_t li, uint32_t& slot, uint32_t& x, uint32_t& y, uint32_t& f) {
    uint32_t k = 0u;
    while (off[k + 1u] <= li) k++;
    const uint32_t r = li - off[k], c = (dispatch_base + k) % (S * S), cx = c % S, cy = c / S;
    uint32_t lx0, lw, ly0, lh;
    split_axis(x0, x1, cx, S, lx0, lw); split_axis(y0, y1, cy, S, ly0, lh);
    const uint32_t ly = r / lw, lx = r - ly * lw;
    x = (lx0 + lx) * S + cx; y = (ly0 + ly) * S + cy; f = k;
    slot = k * shard_pixels + y * width + x;
}

}  // namespace deal
}  // namespace vpt
