// Host driver of vulkan-path-tracer_amd/csrc/wave_cursor.hpp for tests/test_wave_cursor_cpu.py: a stand-alone program (its own main), built once with
// the host compiler and once more with -fsanitize=address,undefined.  A grid of G waves is walked through the cursors' wave-uniform arithmetic
// (namespace cursor, fetch_chunk) with the statements of DealCursor / StrideCursor re-typed around it — the structs are device code, so what is
// checked here is the arithmetic and a MODEL of their control flow, not the structs (nor the kernels that carry the statements written out): those
// run under tests/test_gpu_trace_stream.py and the other GPU stream tests.  The head word is an ordinary counter, and the waves'
// steps are interleaved in the order asked for: 0 round-robin, 1 reversed, 2 wave 0 races ahead until it is exhausted, then the others.
//   wave_cursor_driver deal <G> <per_wave> <chunk, 0: fetch_chunk(n)> <n> <order>
//       a step of a wave: refill, then an idle mask whose popcount walks through 0, 1, 63, 64 and a pseudo-random sequence
//   wave_cursor_driver stride <G> <n> <order>
//       a step of a wave: StrideCursor::next (the waves below active = min(G, ceil(n / 64)) take part, as the kernels' early return has it)
// Output: "key value" pairs.  handed: entries given out; dup: entries given out more than once; beyond: indices taken at or beyond n;
// missing: entries of [0, n) never given out; past: how far the furthest index a lane computed lies behind its run's end; unexhausted: waves that
// did not reach the end within the step budget; chunk_max: fetch_chunk's largest chunk.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "wave_cursor.hpp"

using namespace vpt;

namespace {

struct Tally {
    std::vector<unsigned> seen;
    uint32_t n;
    unsigned long long handed = 0, dup = 0, beyond = 0, past = 0;
    explicit Tally(uint32_t n_) : seen(n_, 0u), n(n_) {}
    void take(uint32_t i) {
        handed++;
        if (i >= n) { beyond++; return; }
        if (seen[i]++) dup++;
    }
    void computed(uint32_t i, uint32_t run_end) { if (i >= run_end && i - run_end + 1u > past) past = i - run_end + 1u; }
    void print(unsigned long long unexhausted) const {
        unsigned long long missing = 0;
        for (unsigned c : seen) if (c == 0u) missing++;
        printf("handed %llu dup %llu beyond %llu missing %llu past %llu unexhausted %llu chunk_max %u\n", handed, dup, beyond, missing, past, unexhausted, kFetchChunkMax);
    }
};

struct DealWave { uint32_t next, end; bool exhausted; unsigned step; };
struct StrideWave { uint32_t pos, end; bool done, exhausted; };

// the order the waves step in: calls step(w) until every wave is exhausted or the budget is spent
template <class Waves, class Step>
unsigned long long interleave(Waves& waves, int order, Step step) {
    const size_t G = waves.size();
    unsigned long long budget = 64ull * 1000ull * 1000ull;
    if (order == 2) while (!waves[0].exhausted && budget--) step(0);
    bool any = true;
    while (any && budget) {
        any = false;
        for (size_t k = 0; k < G && budget; k++) {
            const size_t w = order == 1 ? G - 1 - k : k;
            if (waves[w].exhausted) continue;
            step(w); budget--; any = true;
        }
    }
    unsigned long long unexhausted = 0;
    for (const auto& w : waves) unexhausted += w.exhausted ? 0u : 1u;
    return unexhausted;
}

int run_deal(uint32_t G, uint32_t per_wave, uint32_t chunk_arg, uint32_t n, int order) {
    const uint32_t chunk = chunk_arg ? chunk_arg : fetch_chunk(n);
    const uint32_t n_static = cursor::static_part(G, per_wave);
    uint32_t head = 0u;
    Tally t(n);
    std::vector<DealWave> waves(G);
    for (uint32_t w = 0; w < G; w++) {   // DealCursor::DealCursor
        DealWave& c = waves[w];
        c.next = w * per_wave; c.end = cursor::run_end(c.next, per_wave, n);
        if (c.next >= n) { c.next = 0u; c.end = 0u; }
        c.exhausted = false; c.step = w * 7u;
    }
    static const uint32_t kWant[] = {0u, 1u, 63u, 64u, 17u, 0u, 64u, 5u, 33u, 2u, 64u, 48u};
    uint32_t rnd = 12345u;
    const unsigned long long unexhausted = interleave(waves, order, [&](size_t w) {
        DealWave& c = waves[w];
        if (c.next >= c.end) {   // DealCursor::refill
            if (n_static >= n) c.exhausted = true;
            else {
                const uint32_t reserved = head; head += chunk;   // atomicAdd(head, chunk)
                const uint32_t base = cursor::chunk_first(n_static, reserved);
                if (base >= n) c.exhausted = true;
                else { c.next = base; c.end = cursor::run_end(base, chunk, n); }
            }
        }
        if (c.exhausted) return;
        uint32_t want = kWant[c.step % 12u];
        if (c.step++ % 24u >= 12u) { rnd = rnd * 1664525u + 1013904223u; want = (rnd >> 16) % 65u; }
        for (uint32_t below = 0; below < want; below++) {   // DealCursor::index of the idle lanes: lanes_below() = 0 .. want - 1
            const uint32_t i = c.next + below;
            t.computed(i, c.end);
            if (i < c.end) t.take(i);
        }
        c.next = cursor::deal_advance(c.next, c.end, want);   // DealCursor::advance
    });
    t.print(unexhausted);
    return 0;
}

int run_stride(uint32_t G, uint32_t n, int order) {
    const uint32_t chunk = fetch_chunk(n);
    const uint32_t need = (n + 63u) / 64u, active = need < G ? need : G;
    uint32_t head = 0u;
    Tally t(n);
    std::vector<StrideWave> waves(G);
    for (uint32_t w = 0; w < G; w++) {   // StrideCursor::init; a wave at or beyond `active` returns at once
        waves[w].pos = w * 64u; waves[w].end = waves[w].pos + 64u; waves[w].done = false; waves[w].exhausted = w >= active;
    }
    const unsigned long long unexhausted = interleave(waves, order, [&](size_t w) {
        StrideWave& c = waves[w];
        while (c.pos >= c.end || c.pos >= n) {   // StrideCursor::next
            if (c.done || cursor::stride_static_only(active, n)) c.done = true;
            else {
                const uint32_t reserved = head; head += chunk;
                c.pos = cursor::chunk_first(active * 64u, reserved);
                c.end = c.pos + chunk;
                if (c.pos >= n) c.done = true;
            }
            if (c.done) { c.exhausted = true; return; }
        }
        for (uint32_t lane = 0; lane < 64u; lane++) {   // the kernels use an index only where it is < n
            const uint32_t i = c.pos + lane;
            t.computed(i, n);
            if (i < n) t.take(i);
        }
        c.pos += 64u;
    });
    t.print(unexhausted);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    auto u = [&](int k) { return (uint32_t)strtoul(argv[k], nullptr, 10); };
    if (mode == "deal" && argc == 7) return run_deal(u(2), u(3), u(4), u(5), atoi(argv[6]));
    if (mode == "stride" && argc == 5) return run_stride(u(2), u(3), atoi(argv[4]));
    if (mode == "chunk" && argc == 3) { printf("chunk %u\n", fetch_chunk(u(2))); return 0; }
    fprintf(stderr, "usage: wave_cursor_driver deal <G> <per_wave> <chunk|0> <n> <order> | stride <G> <n> <order> | chunk <n>\n");
    return 2;
}
