// svgf_driver.cpp — the viewport loop's two filters on the host, with SVGF's variance: csrc/temporal.hpp's temporal_pixel_variance driven over a SEQUENCE of
// frames exactly as api_post.hip's enqueue_temporal drives k_temporal (two records and two moment records swapped per call), and after every frame
// csrc/denoise.hpp's prepare_pixel_variance / atrous_pixel_variance over that frame's temporal image and variance exactly as enqueue_denoise drives the
// kernels with the temporal source.  With variance == 0 in the header the same loop calls temporal_pixel / prepare_pixel / atrous_pixel: what the library
// does with the option off.  The kernels call the same functions, so on the same inputs the device gives these bits (tests/test_gpu_svgf.py); against a
// float64 restatement and for the exact properties: tests/test_svgf_cpu.py.
//   svgf_driver IN OUT
//   IN : uint32 width, height, frames, flags, max_history, variance, min_history, runs; float32 depth_tolerance, normal_threshold, focus_distance,
//        dof_strength, sigma_luminance; then per denoise run uint32 iterations, flags (1: demodulate; 256: no pass is the last one — the result's .w is
//        the filtered variance instead of alpha), float32 sigma_color, sigma_normal, sigma_depth; then per frame what temporal_driver reads:
//        float32 view_inv[16], proj_inv[16], float32 m, uint32 drop, float32 radiance [h][w][4], normal [h][w][4], albedo [h][w][4], depth [h][w],
//        uint32 instance [h][w]; with variance == 2 (the option on, and) float32 variance [h][w] follows: the denoise runs of this frame take it in
//        place of the temporal one (for the filter's constructed properties)
//   OUT: per frame float32 image [h][w][4], record [h][w][4], moments [h][w][2], variance [h][w] (zeros with variance == 0), then per run float32 [h][w][4]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "temporal.hpp"

namespace tp = vpt::temporal;
namespace dn = vpt::denoise;
using dn::F4;

struct HostPrev {
    const F4* h; const F4* g; const uint32_t* i; int w; const tp::M2* m;
    F4 hist(int x, int y) const { return h[(size_t)y * w + x]; }
    F4 guide(int x, int y) const { return g[(size_t)y * w + x]; }
    uint32_t inst(int x, int y) const { return i[(size_t)y * w + x]; }
    tp::M2 moments(int x, int y) const { return m[(size_t)y * w + x]; }
};
struct HostSrc {
    const F4* e; const F4* g; int w;
    F4 color(int x, int y) const { return e[(size_t)y * w + x]; }
    F4 guide(int x, int y) const { return g[(size_t)y * w + x]; }
};
struct Run { uint32_t iterations, flags; float sigma[3]; };

static bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: svgf_driver IN OUT\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t head[8]; float par[5];
    if (!read_exact(f, head, sizeof head) || !read_exact(f, par, sizeof par)) { fprintf(stderr, "short header\n"); return 2; }
    const uint32_t w = head[0], h = head[1], frames = head[2], flags = head[3], max_history = head[4], variance = head[5] != 0u, given = head[5] == 2u, min_history = head[6], runs = head[7];
    if (w == 0 || h == 0 || (uint64_t)w * h > (1u << 24) || frames > 64u || max_history == 0u || head[5] > 2u || min_history == 0u || runs > 16u) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<Run> run(runs);
    for (Run& r : run)
        if (!read_exact(f, &r, sizeof(Run)) || r.iterations > 6u) { fprintf(stderr, "bad run\n"); return 2; }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    const size_t n = (size_t)w * h;
    std::vector<F4> radiance(n), normal(n), albedo(n), image(n), hist[2], guide[2], dn_guide(n), dn_albedo(n), ping(n), pong(n), out(n);
    std::vector<tp::M2> moments[2];
    std::vector<float> depth(n), var(n, 0.0f), var_given(n, 0.0f);
    std::vector<uint32_t> ids(n), inst[2];
    for (int k = 0; k < 2; k++) { hist[k].resize(n); guide[k].resize(n); inst[k].resize(n); moments[k].assign(n, tp::M2{0.0f, 0.0f}); }
    uint32_t latest = 0;
    bool history = false;
    tp::PrevCamera camera{};
    for (uint32_t fr = 0; fr < frames; fr++) {
        tp::Frame F{};
        uint32_t drop = 0;
        if (!read_exact(f, F.view_inv, 64) || !read_exact(f, F.proj_inv, 64) || !read_exact(f, &F.m, 4) || !read_exact(f, &drop, 4) || !read_exact(f, radiance.data(), n * 16) ||
            !read_exact(f, normal.data(), n * 16) || !read_exact(f, albedo.data(), n * 16) || !read_exact(f, depth.data(), n * 4) || !read_exact(f, ids.data(), n * 4) || (given && !read_exact(f, var_given.data(), n * 4))) {
            fprintf(stderr, "short input in frame %u\n", fr); return 2;
        }
        if (drop) history = false;
        const uint32_t prev = latest, next = prev ^ 1u;
        F.width = w; F.height = h; F.focus_distance = par[2]; F.dof_strength = par[3];
        F.prev = camera;
        F.have_prev = (history && camera.ok) ? 1u : 0u;
        F.max_history = (float)max_history; F.depth_tolerance = par[0]; F.normal_threshold = par[1]; F.flags = flags;
        const float min_len = (float)min_history * F.m;
        const HostPrev src{hist[prev].data(), guide[prev].data(), inst[prev].data(), (int)w, moments[prev].data()};
        for (int y = 0; y < (int)h; y++)
            for (int x = 0; x < (int)w; x++) {
                const size_t p = (size_t)y * w + x;
                const F4 g = dn::pack_guide(normal[p], depth[p]);
                tp::Result r;
                if (variance) {
                    const tp::ResultV rv = tp::temporal_pixel_variance(src, F, min_len, x, y, radiance[p], g, albedo[p], ids[p]);
                    r = rv.r;
                    moments[next][p] = rv.moments;
                    var[p] = rv.variance;
                } else {
                    r = tp::temporal_pixel(src, F, x, y, radiance[p], g, albedo[p], ids[p]);
                }
                image[p] = r.image;
                hist[next][p] = r.record;
                guide[next][p] = g;
                inst[next][p] = ids[p];
            }
        camera = tp::prev_camera_of(F.view_inv, F.proj_inv);
        latest = next; history = true;
        if (fwrite(image.data(), 16, n, o) != n || fwrite(hist[next].data(), 16, n, o) != n || fwrite(moments[next].data(), 8, n, o) != n || fwrite(var.data(), 4, n, o) != n) {
            fprintf(stderr, "cannot write %s\n", argv[2]); return 2;
        }
        // vpt_denoise from the temporal source, once per run
        const float* v_in = given ? var_given.data() : var.data();
        for (const Run& r : run) {
            if (r.iterations == 0) {
                memcpy(out.data(), image.data(), n * 16);
            } else {
                const bool demodulate = (r.flags & 1u) != 0, keep_variance = (r.flags & 256u) != 0;
                for (size_t i = 0; i < n; i++) {
                    dn_albedo[i] = albedo[i];
                    ping[i] = variance ? dn::prepare_pixel_variance(image[i], dn_albedo[i], depth[i], demodulate, v_in[i]) : dn::prepare_pixel(image[i], albedo[i], depth[i], demodulate);
                    dn_guide[i] = dn::pack_guide(normal[i], depth[i]);
                }
                const F4* in = ping.data();
                for (uint32_t it = 0; it < r.iterations; it++) {
                    const bool last = it + 1 == r.iterations;
                    F4* dst = last ? out.data() : (in == ping.data() ? pong.data() : ping.data());
                    const dn::Pass ps = dn::pass_of(it, r.sigma[0], r.sigma[1], r.sigma[2]);
                    const HostSrc s{in, dn_guide.data(), (int)w};
                    for (int y = 0; y < (int)h; y++)
                        for (int x = 0; x < (int)w; x++) {
                            const size_t p = (size_t)y * w + x;
                            dst[p] = variance ? dn::atrous_pixel_variance(s, x, y, (int)w, (int)h, ps, par[4], in[p], dn_guide[p], last && !keep_variance, last && demodulate, dn_albedo[p])
                                              : dn::atrous_pixel(s, x, y, (int)w, (int)h, ps, in[p], dn_guide[p], last && demodulate, dn_albedo[p]);
                        }
                    in = dst;
                }
            }
            if (fwrite(out.data(), 16, n, o) != n) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
        }
    }
    fclose(f);
    fclose(o);
    return 0;
}
