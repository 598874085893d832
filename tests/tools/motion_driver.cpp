// motion_driver.cpp — vpt_temporal_accumulate with vpt_temporal_options.instance_motion == 1 on the host: csrc/temporal.hpp's temporal_pixel_motion driven over a
// SEQUENCE of frames exactly as api_post.hip's enqueue_temporal drives k_temporal (temporal_driver.cpp's loop), with the instances' matrices kept as the context
// keeps them: moves are applied through MotionSnapshot::note_move the way vpt_set_instance_transforms applies them, the table of a call comes from
// MotionSnapshot::table, and the snapshot is cleared once a record is made or the history is dropped.  The library's kernel calls the same function, so on the
// same inputs the device gives these bits (tests/test_gpu_motion.py); against a float64 restatement and for the exact properties: tests/test_motion_cpu.py.
//   motion_driver IN OUT
//   IN : uint32 width, height, frames, flags, max_history, variance (0 / 1), min_history, instances, withhold (1: the table is built but not handed to the
//        pixels — what a library without the feature computes); float32 depth_tolerance, normal_threshold, focus_distance, dof_strength; float32 [instances][16]
//        (column-major: the matrices at the start); then per frame float32 view_inv[16], proj_inv[16], float32 m, uint32 drop, uint32 moves, per move uint32
//        first, count and float32 [count][16]; then float32 radiance [h][w][4], normal [h][w][4], albedo [h][w][4], depth [h][w], uint32 instance [h][w]
//   OUT: per frame float32 image [h][w][4], record [h][w][4], moments [h][w][2], variance [h][w] (all zero with variance 0), motion [h][w][2], then uint32
//        table (1: a table was built), uint32 state [instances] (all 0 without a table)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "temporal.hpp"

namespace tp = vpt::temporal;
using vpt::denoise::F4;

struct HostPrev {
    const F4* h; const F4* g; const uint32_t* i; int w; const tp::M2* m;
    F4 hist(int x, int y) const { return h[(size_t)y * w + x]; }
    F4 guide(int x, int y) const { return g[(size_t)y * w + x]; }
    uint32_t inst(int x, int y) const { return i[(size_t)y * w + x]; }
    tp::M2 moments(int x, int y) const { return m ? m[(size_t)y * w + x] : tp::M2{0.0f, 0.0f}; }
};

static bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: motion_driver IN OUT\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t head[9]; float par[4];
    if (!read_exact(f, head, sizeof head) || !read_exact(f, par, sizeof par)) { fprintf(stderr, "short header\n"); return 2; }
    const uint32_t w = head[0], h = head[1], frames = head[2], flags = head[3], max_history = head[4], variance = head[5], min_history = head[6], n_inst = head[7], withhold = head[8];
    if (w == 0 || h == 0 || (uint64_t)w * h > (1u << 24) || frames > 64u || max_history == 0u || variance > 1u || n_inst == 0u || n_inst > 4096u) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<float> xforms((size_t)n_inst * 16);
    if (!read_exact(f, xforms.data(), xforms.size() * 4)) { fprintf(stderr, "short matrices\n"); return 2; }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    const size_t n = (size_t)w * h;
    std::vector<F4> radiance(n), normal(n), albedo(n), image(n), hist[2], guide[2];
    std::vector<tp::M2> moments[2];
    std::vector<float> depth(n), var(n), motion(n * 2);
    std::vector<uint32_t> ids(n), inst[2], state(n_inst);
    for (int k = 0; k < 2; k++) { hist[k].resize(n); guide[k].resize(n); inst[k].resize(n); moments[k].resize(n); }
    uint32_t latest = 0;
    bool history = false;
    tp::PrevCamera camera{};
    tp::MotionSnapshot snapshot;
    std::vector<tp::InstanceMotion> table;
    for (uint32_t fr = 0; fr < frames; fr++) {
        tp::Frame F{};
        uint32_t drop = 0, moves = 0;
        if (!read_exact(f, F.view_inv, 64) || !read_exact(f, F.proj_inv, 64) || !read_exact(f, &F.m, 4) || !read_exact(f, &drop, 4) || !read_exact(f, &moves, 4)) {
            fprintf(stderr, "short input in frame %u\n", fr); return 2;
        }
        if (drop) { history = false; snapshot.clear(); }
        for (uint32_t k = 0; k < moves; k++) {   // vpt_set_instance_transforms: the snapshot first, then the matrices
            uint32_t range[2];
            if (!read_exact(f, range, 8) || range[0] > n_inst || range[1] > n_inst - range[0]) { fprintf(stderr, "bad move in frame %u\n", fr); return 2; }
            if (history) snapshot.note_move(range[0], range[1], n_inst, xforms.data(), 64);
            if (!read_exact(f, xforms.data() + (size_t)range[0] * 16, (size_t)range[1] * 64)) { fprintf(stderr, "short move in frame %u\n", fr); return 2; }
        }
        if (!read_exact(f, radiance.data(), n * 16) || !read_exact(f, normal.data(), n * 16) || !read_exact(f, albedo.data(), n * 16) || !read_exact(f, depth.data(), n * 4) ||
            !read_exact(f, ids.data(), n * 4)) {
            fprintf(stderr, "short input in frame %u\n", fr); return 2;
        }
        const uint32_t prev = latest, next = prev ^ 1u;
        F.width = w; F.height = h; F.focus_distance = par[2]; F.dof_strength = par[3];
        F.prev = camera;
        F.have_prev = (history && camera.ok) ? 1u : 0u;
        F.max_history = (float)max_history; F.depth_tolerance = par[0]; F.normal_threshold = par[1]; F.flags = flags;
        const bool have_table = F.have_prev && snapshot.table(n_inst, xforms.data(), 64, table);
        const tp::InstanceMotion* mt = (have_table && !withhold) ? table.data() : nullptr;
        for (uint32_t i = 0; i < n_inst; i++) state[i] = have_table ? table[i].state : 0u;
        const HostPrev src{hist[prev].data(), guide[prev].data(), inst[prev].data(), (int)w, variance ? moments[prev].data() : nullptr};
        const float min_len = (float)min_history * F.m;
        for (int y = 0; y < (int)h; y++)
            for (int x = 0; x < (int)w; x++) {
                const size_t p = (size_t)y * w + x;
                const F4 g = vpt::denoise::pack_guide(normal[p], depth[p]);
                const tp::ResultM r = tp::temporal_pixel_motion(src, mt, n_inst, F, min_len, x, y, radiance[p], g, albedo[p], ids[p]);
                image[p] = r.v.r.image;
                hist[next][p] = r.v.r.record;
                guide[next][p] = g;
                inst[next][p] = ids[p];
                moments[next][p] = variance ? r.v.moments : tp::M2{0.0f, 0.0f};
                var[p] = variance ? r.v.variance : 0.0f;
                motion[2 * p] = r.mv.x; motion[2 * p + 1] = r.mv.y;
            }
        camera = tp::prev_camera_of(F.view_inv, F.proj_inv);
        snapshot.clear();
        latest = next; history = true;
        const uint32_t used = have_table ? 1u : 0u;
        if (fwrite(image.data(), 16, n, o) != n || fwrite(hist[next].data(), 16, n, o) != n || fwrite(moments[next].data(), 8, n, o) != n || fwrite(var.data(), 4, n, o) != n ||
            fwrite(motion.data(), 8, n, o) != n || fwrite(&used, 4, 1, o) != 1 || fwrite(state.data(), 4, n_inst, o) != n_inst) {
            fprintf(stderr, "cannot write %s\n", argv[2]); return 2;
        }
    }
    fclose(f);
    fclose(o);
    return 0;
}
