// Host driver of vulkan-path-tracer_amd/csrc/whole_refill.hpp for tests/test_whole_refill_cpu.py: a grid of modelled waves of the whole-path
// kernel (kernels_whole.hip k_whole) that share one tile counter.  The cursor and buffer arithmetic is the header's; wave_refill restates only
// the order in which k_whole's refill step calls it, with the launch index standing in for the camera ray an entry holds.  Between refills a
// seeded coin decides which lanes' paths survive (the shade and trace steps), and a seeded scheduler decides which wave runs next, so the
// waves meet the counter in every order.  Built as a shared library and driven through ctypes.
#include <cstdint>
#include <vector>

#include "whole_refill.hpp"

using namespace vpt::refill;

namespace {
struct Rand {   // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    bool below(uint32_t per_mille) { return next() % 1000u < per_mille; }
};
struct Wave {
    Cursor cur;
    Fresh fresh;
    uint32_t buf[kTile];
    bool has_ray[kTile];
};
struct Tally { uint32_t* handed; uint32_t n; uint64_t out_of_range, gen_passes, gen_lanes, partial_gens, counter_adds; };

// k_whole's refill step for one wave
void wave_refill(const Shape& shape, Wave& w, uint32_t& counter, Tally& t) {
    if (exhausted(w.cur, w.fresh)) return;
    for (int pass = 0; pass < 2; pass++) {
        uint32_t want = 0;
        for (uint32_t l = 0; l < kTile; l++) want += w.has_ray[l] ? 0u : 1u;
        if (want == 0u) break;
        if (w.fresh.count == 0u) {
            if (range_empty(w.cur) && !take_static(shape, w.cur)) {
                const uint32_t take = dyn_take(shape, w.cur);
                const uint32_t k = counter; counter += take; t.counter_adds++;   // the atomicAdd
                take_dynamic(shape, w.cur, k, take);
            }
            if (exhausted(w.cur, w.fresh)) break;
            const uint32_t g = gen_count(w.cur);
            for (uint32_t j = 0; j < g; j++) w.buf[j] = w.cur.w_next + j;   // lane j generates launch index w_next + j into entry j
            t.gen_passes++; t.gen_lanes += g; if (g < kTile) t.partial_gens++;
            generated(w.cur, w.fresh, g);
        }
        const uint32_t head = w.fresh.head;
        pop(w.fresh, want);
        uint32_t r = 0;   // free lanes below this one
        for (uint32_t l = 0; l < kTile; l++) {
            if (w.has_ray[l]) continue;
            const uint32_t q = head + r++;
            if (q < w.fresh.head) {
                const uint32_t li = w.buf[q];
                if (li < t.n) t.handed[li]++; else t.out_of_range++;
                w.has_ray[l] = true;
            }
        }
    }
}
}  // namespace

extern "C" {
// Runs n_waves waves to their end.  handed[n]: how often each launch index was handed to a lane.  survive_per_mille: the share of running paths
// that keep their lane from one refill to the next.  out[0] indices >= n handed out, [1] entries left in the buffers of stopped waves,
// [2] generating passes, [3] generating lanes, [4] passes on fewer than kTile lanes, [5] counter additions.
void wr_run(uint32_t n, uint32_t n_waves, uint32_t static_rounds, uint32_t chunk_tiles, uint32_t survive_per_mille, uint64_t seed, uint32_t* handed, uint64_t* out) {
    const Shape shape{n, n_waves, static_rounds, chunk_tiles};
    Rand rng{seed};
    std::vector<Wave> waves(n_waves);
    for (uint32_t i = 0; i < n_waves; i++) {
        Wave& w = waves[i];
        w.cur = make_cursor(shape, i); w.fresh = make_fresh();
        for (uint32_t l = 0; l < kTile; l++) w.has_ray[l] = false;
    }
    Tally t{handed, n, 0, 0, 0, 0, 0};
    uint32_t counter = 0, running = n_waves;
    uint64_t leftover = 0;
    std::vector<uint32_t> live(n_waves);
    for (uint32_t i = 0; i < n_waves; i++) live[i] = i;
    while (running) {
        const uint32_t pick = (uint32_t)(rng.next() % running);
        Wave& w = waves[live[pick]];
        for (uint32_t l = 0; l < kTile; l++) if (w.has_ray[l] && !rng.below(survive_per_mille)) w.has_ray[l] = false;   // paths that ended in the shade / trace steps
        wave_refill(shape, w, counter, t);
        bool any = false;
        for (uint32_t l = 0; l < kTile; l++) any = any || w.has_ray[l];
        if (!any && w.cur.done) {   // no path and no tile to come: the wave stops here whatever its buffer holds (k_whole's loop exit; its ring of parked hits holds no fresh samples)
            leftover += w.fresh.count;
            live[pick] = live[--running];
        }
    }
    out[0] = t.out_of_range; out[1] = leftover; out[2] = t.gen_passes; out[3] = t.gen_lanes; out[4] = t.partial_gens; out[5] = t.counter_adds;
}
}
