// firefly_driver.cpp — the firefly filter on the host: csrc/firefly.hpp's staged_luminance over the whole image, then firefly_pixel per pixel, exactly as
// kernels_post.hip's k_firefly stages a tile's luminances and runs the window from them.  The kernel calls the same functions, so on the same inputs the
// device gives these bits (tests/test_gpu_firefly.py); against a float64 restatement and for the exact properties: tests/test_firefly_cpu.py.
//   firefly_driver IN OUT
//   IN : uint32 width, height, radius, rank, demodulate; float32 threshold, floor; then float32 radiance [h][w][4], albedo [h][w][4], depth [h][w]
//        (depth < 0: a miss; the albedo is not looked at unless demodulate is 1)
//   OUT: float32 image [h][w][4]; uint8 clamped [h][w]; uint8 considered [h][w]; uint64 clamped pixels, considered pixels
//   firefly_driver --check IN
//   IN : vpt_firefly_options records of 32 bytes; prints one line per record: "ok", or what check_options — vpt_set_firefly_options' own test — says of it;
//        then the defaults as one line "default mode radius rank threshold floor"
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "firefly.hpp"

namespace ff = vpt::firefly;
using vpt::denoise::F4;

struct HostLum {
    const float* l; int w;
    float lum(int x, int y) const { return l[(size_t)y * w + x]; }
};

static bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

static int check(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    ff::Options o;
    static_assert(sizeof(ff::Options) == 32, "vpt_firefly_options is 32 bytes");
    while (fread(&o, 1, sizeof o, f) == sizeof o) {
        const char* why = ff::check_options(o);
        printf("%s\n", why ? why : "ok");
    }
    fclose(f);
    const ff::Options d = ff::default_options();
    printf("default %u %u %u %g %g\n", d.mode, d.radius, d.rank, d.threshold, d.floor);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "--check") return check(argv[2]);
    if (argc != 3) { fprintf(stderr, "usage: firefly_driver IN OUT\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t head[5]; float par[2];
    if (!read_exact(f, head, sizeof head) || !read_exact(f, par, sizeof par)) { fprintf(stderr, "short header\n"); return 2; }
    const uint32_t w = head[0], h = head[1], radius = head[2], rank = head[3], demodulate = head[4];
    if (w == 0 || h == 0 || (uint64_t)w * h > (1u << 24) || radius < 1u || radius > (uint32_t)ff::kMaxRadius || rank < 1u || rank > (uint32_t)ff::kMaxRank || demodulate > 1u) {
        fprintf(stderr, "bad header\n"); return 2;
    }
    const size_t n = (size_t)w * h;
    std::vector<F4> radiance(n), albedo(n), image(n);
    std::vector<float> depth(n), lum(n);
    std::vector<uint8_t> clamped(n), considered(n);
    if (!read_exact(f, radiance.data(), n * 16) || !read_exact(f, albedo.data(), n * 16) || !read_exact(f, depth.data(), n * 4)) { fprintf(stderr, "short input\n"); return 2; }
    fclose(f);
    const ff::Plan plan = ff::plan_of(radius, rank, par[0], par[1], demodulate != 0u);
    for (size_t i = 0; i < n; i++) lum[i] = ff::staged_luminance(radiance[i], albedo[i], depth[i], demodulate != 0u);
    const HostLum src{lum.data(), (int)w};
    uint64_t count[2] = {0u, 0u};
    for (int y = 0; y < (int)h; y++)
        for (int x = 0; x < (int)w; x++) {
            const size_t p = (size_t)y * w + x;
            const ff::Result r = ff::firefly_pixel(src, x, y, (int)w, (int)h, plan, radiance[p], albedo[p], depth[p]);
            image[p] = r.pixel;
            clamped[p] = r.clamped ? 1 : 0; considered[p] = r.considered ? 1 : 0;
            count[0] += clamped[p]; count[1] += considered[p];
        }
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(image.data(), 16, n, o) != n || fwrite(clamped.data(), 1, n, o) != n || fwrite(considered.data(), 1, n, o) != n || fwrite(count, 8, 2, o) != 2) {
        fprintf(stderr, "cannot write %s\n", argv[2]); return 2;
    }
    fclose(o);
    return 0;
}
