// exposure_driver.cpp — auto-exposure on the host: csrc/exposure.hpp's bin_of, meter and adapt driven over a SEQUENCE of meterings exactly as api_post.hip's
// enqueue_post drives k_luminance_histogram and k_exposure_adapt (the plan formed per metering from the options, the state carried from one metering to
// the next, `reset` as the context would pass it).  The library's kernels call the same functions and sum integers, so on the same inputs the device gives
// these bits (tests/test_gpu_exposure.py); against a float64 restatement and for the exact properties: tests/test_exposure_cpu.py.
//   exposure_driver IN OUT
//   IN : vpt_exposure_options (48 bytes), uint32 steps; then per step uint32 kind, reset, w, h and
//        kind 0  float32 rgba [h][w][4]: the image is binned, metered, and the state adapts
//        kind 1  uint32 hist[256] (w, h ignored): a hand-made histogram is metered, and the state adapts
//        kind 2  float32 rgba [h][w][4]: bin_of per pixel only; the state is untouched
//   OUT: per step of kind 0 or 1: the state (32 bytes, vpt_exposure_state), uint32 hist[256], uint64 lo, hi, S, W, uint32 has_target, 0;
//        per step of kind 2: uint32 bin [h][w]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "exposure.hpp"

namespace ex = vpt::exposure;

static bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: exposure_driver IN OUT\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    ex::Options opt;
    uint32_t steps = 0;
    if (!read_exact(f, &opt, sizeof opt) || !read_exact(f, &steps, 4)) { fprintf(stderr, "short header\n"); return 2; }
    if (const char* why = ex::check_options(opt)) { fprintf(stderr, "bad options: %s\n", why); return 3; }
    if (steps > 4096u) { fprintf(stderr, "bad header\n"); return 2; }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    const ex::Plan plan = ex::plan_of(opt);
    ex::State state;
    memset(&state, 0, sizeof state);
    std::vector<float> px;
    std::vector<uint32_t> bins;
    for (uint32_t k = 0; k < steps; k++) {
        uint32_t head[4];
        if (!read_exact(f, head, sizeof head)) { fprintf(stderr, "short input in step %u\n", k); return 2; }
        const uint32_t kind = head[0], reset = head[1], w = head[2], h = head[3];
        if (kind > 2u || reset > ex::kResetAll) { fprintf(stderr, "bad step %u\n", k); return 2; }
        uint32_t hist[ex::kBins] = {};
        if (kind == 1u) {
            if (!read_exact(f, hist, sizeof hist)) { fprintf(stderr, "short input in step %u\n", k); return 2; }
        } else {
            if (w == 0 || h == 0 || (uint64_t)w * h > (1u << 24)) { fprintf(stderr, "bad size in step %u\n", k); return 2; }
            const size_t n = (size_t)w * h;
            px.resize(n * 4); bins.resize(n);
            if (!read_exact(f, px.data(), n * 16)) { fprintf(stderr, "short input in step %u\n", k); return 2; }
            for (size_t i = 0; i < n; i++) {
                bins[i] = ex::bin_of(px[4 * i], px[4 * i + 1], px[4 * i + 2], plan.min_log2, plan.rcp_bin);
                hist[bins[i]] += 1u;
            }
            if (kind == 2u) {
                if (fwrite(bins.data(), 4, n, o) != n) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
                continue;
            }
        }
        // the integers of the metering, for the tests that work them out by hand (meter() forms the same ones)
        uint64_t N = 0;
        for (int b = 1; b < ex::kBins; b++) N += hist[b];
        const ex::Window win = ex::window_of(N, plan.lo_q16, plan.hi_q16);
        uint64_t c = 0, S = 0, W = 0;
        for (int b = 1; b < ex::kBins; b++) { const uint64_t t = ex::take(c, hist[b], win); W += t; S += t * (uint64_t)b; c += hist[b]; }
        const ex::Metered m = ex::meter(hist, plan);
        ex::adapt(state, m, plan, reset);
        const uint64_t ints[4] = {win.lo, win.hi, S, W};
        const uint32_t tail[2] = {m.has_target, 0u};
        if (fwrite(&state, sizeof state, 1, o) != 1 || fwrite(hist, sizeof hist, 1, o) != 1 || fwrite(ints, sizeof ints, 1, o) != 1 || fwrite(tail, sizeof tail, 1, o) != 1) {
            fprintf(stderr, "cannot write %s\n", argv[2]); return 2;
        }
    }
    fclose(f);
    fclose(o);
    return 0;
}
