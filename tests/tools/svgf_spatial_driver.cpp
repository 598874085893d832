// svgf_spatial_driver.cpp — the viewport loop's two filters on the host with SVGF's variance AND its spatial estimate for young pixels: svgf_driver.cpp's
// loop with the option on (csrc/temporal.hpp's temporal_pixel_variance over a SEQUENCE of frames, then csrc/denoise.hpp's variance-guided passes over each
// frame's temporal image), and between the two csrc/svgf_spatial.hpp's spatial_variance_pixel over the record the temporal step has just written, exactly as
// api_post.hip's enqueue_temporal launches k_variance_spatial behind k_temporal: the variance image is rewritten in place, nothing else is.  With mode == 0
// the pass is left out and the output is svgf_driver's.  The kernel calls the same function, so on the same inputs the device gives these bits
// (tests/test_gpu_svgf_spatial.py); against a float64 restatement and for the exact properties: tests/test_svgf_spatial_cpu.py.
//   svgf_spatial_driver IN OUT
//   IN : uint32 width, height, frames, flags, max_history, min_history, runs, mode, radius; float32 depth_tolerance, normal_threshold, focus_distance,
//        dof_strength, sigma_luminance, sigma_normal, sigma_depth, min_weight (the last three: the spatial window's); then per denoise run what svgf_driver
//        reads: uint32 iterations, flags (1: demodulate; 256: no pass is the last one), float32 sigma_color, sigma_normal, sigma_depth; then per frame
//        float32 view_inv[16], proj_inv[16], float32 m, uint32 drop, float32 radiance [h][w][4], normal [h][w][4], albedo [h][w][4], depth [h][w],
//        uint32 instance [h][w]
//   OUT: per frame float32 image [h][w][4], record [h][w][4], moments [h][w][2], variance [h][w], then per run float32 [h][w][4]: svgf_driver's layout
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "svgf_spatial.hpp"

namespace tp = vpt::temporal;
namespace dn = vpt::denoise;
namespace sp = vpt::svgf_spatial;
using dn::F4;

struct HostPrev {
    const F4* h; const F4* g; const uint32_t* i; int w; const tp::M2* m;
    F4 hist(int x, int y) const { return h[(size_t)y * w + x]; }
    F4 guide(int x, int y) const { return g[(size_t)y * w + x]; }
    uint32_t inst(int x, int y) const { return i[(size_t)y * w + x]; }
    tp::M2 moments(int x, int y) const { return m[(size_t)y * w + x]; }
};
struct HostRecord {
    const F4* g; const tp::M2* m; int w;
    F4 guide(int x, int y) const { return g[(size_t)y * w + x]; }
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
    if (argc != 3) { fprintf(stderr, "usage: svgf_spatial_driver IN OUT\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t head[9]; float par[8];
    if (!read_exact(f, head, sizeof head) || !read_exact(f, par, sizeof par)) { fprintf(stderr, "short header\n"); return 2; }
    const uint32_t w = head[0], h = head[1], frames = head[2], flags = head[3], max_history = head[4], min_history = head[5], runs = head[6], mode = head[7], radius = head[8];
    if (w == 0 || h == 0 || (uint64_t)w * h > (1u << 24) || frames > 64u || max_history == 0u || min_history == 0u || runs > 16u || mode > 1u || radius < 1u || radius > (uint32_t)sp::kMaxRadius) {
        fprintf(stderr, "bad header\n"); return 2;
    }
    std::vector<Run> run(runs);
    for (Run& r : run)
        if (!read_exact(f, &r, sizeof(Run)) || r.iterations > 6u) { fprintf(stderr, "bad run\n"); return 2; }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    const sp::Plan plan = sp::plan_of(radius, par[5], par[6], par[7]);
    const size_t n = (size_t)w * h;
    std::vector<F4> radiance(n), normal(n), albedo(n), image(n), hist[2], guide[2], dn_guide(n), dn_albedo(n), ping(n), pong(n), out(n);
    std::vector<tp::M2> moments[2];
    std::vector<float> depth(n), var(n, 0.0f);
    std::vector<uint32_t> ids(n), inst[2];
    for (int k = 0; k < 2; k++) { hist[k].resize(n); guide[k].resize(n); inst[k].resize(n); moments[k].assign(n, tp::M2{0.0f, 0.0f}); }
    uint32_t latest = 0;
    bool history = false;
    tp::PrevCamera camera{};
    for (uint32_t fr = 0; fr < frames; fr++) {
        tp::Frame F{};
        uint32_t drop = 0;
        if (!read_exact(f, F.view_inv, 64) || !read_exact(f, F.proj_inv, 64) || !read_exact(f, &F.m, 4) || !read_exact(f, &drop, 4) || !read_exact(f, radiance.data(), n * 16) ||
            !read_exact(f, normal.data(), n * 16) || !read_exact(f, albedo.data(), n * 16) || !read_exact(f, depth.data(), n * 4) || !read_exact(f, ids.data(), n * 4)) {
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
                const tp::ResultV rv = tp::temporal_pixel_variance(src, F, min_len, x, y, radiance[p], g, albedo[p], ids[p]);
                moments[next][p] = rv.moments;
                var[p] = rv.variance;
                image[p] = rv.r.image;
                hist[next][p] = rv.r.record;
                guide[next][p] = g;
                inst[next][p] = ids[p];
            }
        camera = tp::prev_camera_of(F.view_inv, F.proj_inv);
        latest = next; history = true;
        // k_variance_spatial: the variance image in place (a pixel reads its own variance only, and the guides and moments of its neighbours)
        if (mode) {
            const HostRecord rec{guide[next].data(), moments[next].data(), (int)w};
            for (int y = 0; y < (int)h; y++)
                for (int x = 0; x < (int)w; x++) {
                    const size_t p = (size_t)y * w + x;
                    var[p] = sp::spatial_variance_pixel(rec, x, y, (int)w, (int)h, plan, hist[next][p].w, min_len, guide[next][p], var[p]);
                }
        }
        if (fwrite(image.data(), 16, n, o) != n || fwrite(hist[next].data(), 16, n, o) != n || fwrite(moments[next].data(), 8, n, o) != n || fwrite(var.data(), 4, n, o) != n) {
            fprintf(stderr, "cannot write %s\n", argv[2]); return 2;
        }
        // vpt_denoise from the temporal source, once per run
        for (const Run& r : run) {
            if (r.iterations == 0) {
                memcpy(out.data(), image.data(), n * 16);
            } else {
                const bool demodulate = (r.flags & 1u) != 0, keep_variance = (r.flags & 256u) != 0;
                for (size_t i = 0; i < n; i++) {
                    dn_albedo[i] = albedo[i];
                    ping[i] = dn::prepare_pixel_variance(image[i], dn_albedo[i], depth[i], demodulate, var[i]);
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
                            dst[p] = dn::atrous_pixel_variance(s, x, y, (int)w, (int)h, ps, par[4], in[p], dn_guide[p], last && !keep_variance, last && demodulate, dn_albedo[p]);
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
