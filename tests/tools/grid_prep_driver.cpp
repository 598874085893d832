// Host driver of the density-grid preparation behind vpt_add_density_grid / vpt_add_density_bricks for tests/test_grid_prep_cpu.py: a stand-alone
// program (g++, no HIP runtime linked or called; it may be built with -fsanitize=address,undefined) that runs grid_prep.hpp as api_scene.hip runs it
// — check_bricks, brick_table, brick_maxima; dense_maxima — and reads every voxel of the index box back through grid_value, the function the kernels call.
//
//   grid_prep_driver prep IN OUT     IN:  u32 dx, dy, dz, dense (0 | 1), bricks; dense ? float[dx * dy * dz] : nothing; u32[3 * bricks] coordinates;
//                                         float[512 * bricks] values
//                                    OUT: for the dense grid (if given and accepted), then for the bricked one (if accepted): float max, float[32768]
//                                         block maxima, float[dx * dy * dz] grid_value of every voxel (x fastest); the bricked one's table (u32 per cell) last
//                                    prints "<code>|<message>" of the dense grid ("-|" if none was given) and of the bricked one, one per line
//   grid_prep_driver check DX DY DZ BRICKS NULL GRIDS     prints "<code>|<message>" of grid::check_bricks (NULL = 1: no arrays; GRIDS: grids in use)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "grid_prep.hpp"

using namespace vpt;

namespace {

bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
void put(FILE* f, const void* p, size_t bytes) { if (bytes && fwrite(p, 1, bytes, f) != bytes) { fprintf(stderr, "short write\n"); exit(1); } }

// max, block maxima and every voxel through grid_value
void dump(FILE* out, const DensityGrid& g, const grid::Maxima& m) {
    put(out, &m.max_density, 4);
    put(out, m.block_max.data(), m.block_max.size() * 4);
    std::vector<float> v((size_t)g.dim[0] * g.dim[1] * g.dim[2]);
    size_t i = 0;
    for (uint32_t z = 0; z < g.dim[2]; z++)
        for (uint32_t y = 0; y < g.dim[1]; y++)
            for (uint32_t x = 0; x < g.dim[0]; x++) v[i++] = grid::grid_value(g, x, y, z);
    put(out, v.data(), v.size() * 4);
}

int prep(const char* in_path, const char* out_path) {
    FILE* in = fopen(in_path, "rb");
    if (!in) { fprintf(stderr, "cannot open %s\n", in_path); return 1; }
    uint32_t h[5];
    if (!read_exact(in, h, sizeof(h))) { fprintf(stderr, "short header\n"); return 1; }
    const uint32_t dx = h[0], dy = h[1], dz = h[2], n = h[4];
    std::vector<float> dense(h[3] ? (size_t)dx * dy * dz : 0), values((size_t)n * grid::kBrickVoxels);
    std::vector<uint32_t> coords((size_t)n * 3);
    if (!read_exact(in, dense.data(), dense.size() * 4) || !read_exact(in, coords.data(), coords.size() * 4) || !read_exact(in, values.data(), values.size() * 4)) { fprintf(stderr, "short input\n"); return 1; }
    fclose(in);
    FILE* out = fopen(out_path, "wb");
    if (!out) { fprintf(stderr, "cannot write %s\n", out_path); return 1; }
    if (h[3]) {
        grid::Maxima m;
        const grid::Verdict v = grid::dense_maxima(dx, dy, dz, dense.data(), m);
        printf("%d|%s\n", v.code, v.msg);
        if (!v.code) {
            DensityGrid g{};
            g.values = dense.data(); g.dim[0] = dx; g.dim[1] = dy; g.dim[2] = dz; g.max_density = m.max_density;
            dump(out, g, m);
        }
    } else printf("-|\n");
    grid::Maxima m;
    std::vector<uint32_t> table;
    grid::Verdict v = grid::check_bricks(dx, dy, dz, n, coords.data(), values.data(), 0);
    if (!v.code) v = grid::brick_table(dx, dy, dz, n, coords.data(), table);
    if (!v.code) v = grid::brick_maxima(dx, dy, dz, n, coords.data(), values.data(), m);
    printf("%d|%s\n", v.code, v.msg);
    if (!v.code) {
        DensityGrid g{};
        g.values = values.data(); g.bricks = table.data(); g.dim[0] = dx; g.dim[1] = dy; g.dim[2] = dz; g.max_density = m.max_density; g.brick_count = n;
        g.cells[0] = grid::cells_along(dx); g.cells[1] = grid::cells_along(dy); g.cells[2] = grid::cells_along(dz);
        dump(out, g, m);
        put(out, table.data(), table.size() * 4);
    }
    fclose(out);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "prep")) return prep(argv[2], argv[3]);
    if (argc == 8 && !strcmp(argv[1], "check")) {
        uint32_t a[6];
        for (int i = 0; i < 6; i++) a[i] = (uint32_t)strtoul(argv[2 + i], nullptr, 10);
        const uint32_t c = 0; const float f = 0.0f;   // (check_bricks looks at the pointers, never through them)
        const grid::Verdict v = grid::check_bricks(a[0], a[1], a[2], a[3], a[4] ? nullptr : &c, a[4] ? nullptr : &f, a[5]);
        printf("%d|%s\n", v.code, v.msg);
        return 0;
    }
    fprintf(stderr, "usage: grid_prep_driver prep IN OUT | check DX DY DZ BRICKS NULL GRIDS\n");
    return 2;
}
