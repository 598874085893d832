// temporal_driver.cpp — vpt_temporal_accumulate on the host: csrc/temporal.hpp's temporal_pixel driven over a SEQUENCE of frames exactly as api_post.hip's
// enqueue_temporal drives k_temporal (two records swapped per call, the previous camera from prev_camera_of, the guide packed as (n.xyz, t), have_prev only
// after a frame and while the previous camera is regular).  The library's kernel calls the same function, so on the same inputs the device gives these bits
// (tests/test_gpu_temporal.py); against a float64 restatement and for the exact properties: tests/test_temporal_cpu.py.
//   temporal_driver IN OUT
//   IN : uint32 width, height, frames, flags, max_history; float32 depth_tolerance, normal_threshold, focus_distance, dof_strength; then per frame
//        float32 view_inv[16], proj_inv[16] (column-major, as vpt_set_camera takes them), float32 m, uint32 drop (1: the history is dropped before this
//        frame), float32 radiance [h][w][4], normal [h][w][4], albedo [h][w][4], depth [h][w], uint32 instance [h][w]
//   OUT: per frame float32 image [h][w][4], then the record float32 [h][w][4] = (e.r, e.g, e.b, length): what the next frame finds as its history
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "temporal.hpp"

namespace tp = vpt::temporal;
using vpt::denoise::F4;

struct HostPrev {
    const F4* h; const F4* g; const uint32_t* i; int w;
    F4 hist(int x, int y) const { return h[(size_t)y * w + x]; }
    F4 guide(int x, int y) const { return g[(size_t)y * w + x]; }
    uint32_t inst(int x, int y) const { return i[(size_t)y * w + x]; }
};

static bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: temporal_driver IN OUT\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t head[5]; float par[4];
    if (!read_exact(f, head, sizeof head) || !read_exact(f, par, sizeof par)) { fprintf(stderr, "short header\n"); return 2; }
    const uint32_t w = head[0], h = head[1], frames = head[2], flags = head[3], max_history = head[4];
    if (w == 0 || h == 0 || (uint64_t)w * h > (1u << 24) || frames > 64u || max_history == 0u) { fprintf(stderr, "bad header\n"); return 2; }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    const size_t n = (size_t)w * h;
    std::vector<F4> radiance(n), normal(n), albedo(n), image(n), hist[2], guide[2];
    std::vector<float> depth(n);
    std::vector<uint32_t> ids(n), inst[2];
    for (int k = 0; k < 2; k++) { hist[k].resize(n); guide[k].resize(n); inst[k].resize(n); }
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
        const HostPrev src{hist[prev].data(), guide[prev].data(), inst[prev].data(), (int)w};
        for (int y = 0; y < (int)h; y++)
            for (int x = 0; x < (int)w; x++) {
                const size_t p = (size_t)y * w + x;
                const F4 g = vpt::denoise::pack_guide(normal[p], depth[p]);
                const tp::Result r = tp::temporal_pixel(src, F, x, y, radiance[p], g, albedo[p], ids[p]);
                image[p] = r.image;
                hist[next][p] = r.record;
                guide[next][p] = g;
                inst[next][p] = ids[p];
            }
        camera = tp::prev_camera_of(F.view_inv, F.proj_inv);
        latest = next; history = true;
        if (fwrite(image.data(), 16, n, o) != n || fwrite(hist[next].data(), 16, n, o) != n) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    }
    fclose(f);
    fclose(o);
    return 0;
}
