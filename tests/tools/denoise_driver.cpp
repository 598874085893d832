// denoise_driver.cpp — vpt_denoise on the host: csrc/denoise.hpp's per-pixel functions driven over whole images exactly as api_post.hip's enqueue_denoise
// drives the kernels (prepare, guide packed in place, `iterations` passes between two images, the last one into the result, iterations == 0 a copy).
// The library's kernels call the same functions, so on the same inputs the device gives these bits (tests/test_gpu_denoise.py); against a float64
// restatement and for the filter's exact properties: tests/test_denoise_cpu.py.
//   denoise_driver IN OUT
//   IN : uint32 width, height, iterations, flags; float32 sigma_color, sigma_normal, sigma_depth; then float32 colour [h][w][4], normal [h][w][4],
//        albedo [h][w][4], depth [h][w]
//   OUT: float32 [h][w][4]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "denoise.hpp"

namespace dn = vpt::denoise;

struct HostSrc {
    const dn::F4* e; const dn::F4* g; int w;
    dn::F4 color(int x, int y) const { return e[(size_t)y * w + x]; }
    dn::F4 guide(int x, int y) const { return g[(size_t)y * w + x]; }
};

static bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: denoise_driver IN OUT\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t head[4]; float sigma[3];
    if (!read_exact(f, head, sizeof head) || !read_exact(f, sigma, sizeof sigma)) { fprintf(stderr, "short header\n"); return 2; }
    const uint32_t w = head[0], h = head[1], iterations = head[2], flags = head[3];
    if (w == 0 || h == 0 || (uint64_t)w * h > (1u << 24) || iterations > 6u) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t n = (size_t)w * h;
    std::vector<dn::F4> colour(n), guide(n), albedo(n), ping(n), pong(n), out(n);
    std::vector<float> depth(n);
    if (!read_exact(f, colour.data(), n * 16) || !read_exact(f, guide.data(), n * 16) || !read_exact(f, albedo.data(), n * 16) || !read_exact(f, depth.data(), n * 4)) {
        fprintf(stderr, "short input\n"); return 2;
    }
    fclose(f);
    if (iterations == 0) {
        memcpy(out.data(), colour.data(), n * 16);
    } else {
        const bool demodulate = (flags & 1u) != 0;
        for (size_t i = 0; i < n; i++) {
            ping[i] = dn::prepare_pixel(colour[i], albedo[i], depth[i], demodulate);
            guide[i] = dn::pack_guide(guide[i], depth[i]);
        }
        const dn::F4* in = ping.data();
        for (uint32_t it = 0; it < iterations; it++) {
            const bool last = it + 1 == iterations;
            dn::F4* dst = last ? out.data() : (in == ping.data() ? pong.data() : ping.data());
            const dn::Pass ps = dn::pass_of(it, sigma[0], sigma[1], sigma[2]);
            const HostSrc src{in, guide.data(), (int)w};
            for (int y = 0; y < (int)h; y++)
                for (int x = 0; x < (int)w; x++) {
                    const size_t p = (size_t)y * w + x;
                    dst[p] = dn::atrous_pixel(src, x, y, (int)w, (int)h, ps, in[p], guide[p], last && demodulate, albedo[p]);
                }
            in = dst;
        }
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(out.data(), 16, n, o) != n) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fclose(o);
    return 0;
}
