// grid_prep.hpp — everything vpt_add_density_grid / vpt_add_density_bricks decide and compute on the host before a byte reaches the device, and the
// one lookup both kinds of grid are read through.  A density grid is either DENSE (every voxel of the index box [0, dim), x fastest) or BRICKED:
// 8 x 8 x 8 bricks — a NanoVDB tree's leaf nodes as they are — plus a table with one word per brick cell of the box (x fastest; kEmptyCell, or the
// brick's ordinal in the value array).  A bricked grid IS the dense grid with 0 in every voxel no brick covers: its maximum, its 32^3 block maxima
// and every value grid_value returns equal the dense grid's bit for bit, and the dense box is never formed — the work here is brick_count * 512.
// Plain C++ on plain values, no context and no HIP call: api_scene.hip uploads what this prepares, tests/tools/grid_prep_driver.cpp runs it on the
// host (tests/test_grid_prep_cpu.py), and grid_value is the function the kernels call (volume.hpp sample_density_grid, kernels_aux.hip).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "device_types.hpp"   // (+ vpt.h, vpt_fp32.h)

// The per-brick host loops run once per call and stay rolled (the library's size is bounded, tests/test_abi.py).
#if defined(__clang__)
#define VPT_GRID_ROLLED _Pragma("unroll 1")
#else
#define VPT_GRID_ROLLED
#endif

namespace vpt {
namespace grid {

constexpr uint32_t kEmptyCell = 0xffffffffu;
constexpr uint32_t kBrickVoxels = VPT_BRICK_DIM * VPT_BRICK_DIM * VPT_BRICK_DIM;   // 512 floats = 2 KB = 16 cache lines
constexpr uint32_t kBlockTable = 32u * 32u * 32u;
constexpr uint64_t kMaxDenseVoxels = 1ull << 31, kMaxCells = 1ull << 26;
constexpr uint32_t kMaxBricks = 1u << 22;

// The raw value of voxel (cx, cy, cz), which the caller has clamped to the index box (unsigned: a size_t made of it costs no sign extension; every
// product below is 64-bit).  Dense: the voxel's place in the box.  Bricked: the cell's table word, then — unless the cell is empty, which costs no
// second load — the voxel's place inside its brick.  One load of values[] for both; the dense place is formed before the branch, not in an else
// (it is the shorter code at every inlined call site, and the fused media kernels' code object has no page to spare: profiles/r10_density_bricks_static.md).
VPT_HD float grid_value(const DensityGrid& g, uint32_t cx, uint32_t cy, uint32_t cz) {
    size_t at = (size_t)cx + (size_t)cy * g.dim[0] + (size_t)cz * g.dim[0] * g.dim[1];
    if (g.bricks) {
        const uint32_t ordinal = g.bricks[(size_t)(cx >> 3) + ((size_t)(cy >> 3) + (size_t)(cz >> 3) * g.cells[1]) * g.cells[0]];
        if (ordinal == kEmptyCell) return 0.0f;
        at = (size_t)ordinal * kBrickVoxels + (size_t)((cx & 7u) + (cy & 7u) * 8u + (cz & 7u) * 64u);
    }
    return g.values[at];
}

struct Verdict {
    int code;          // VPT_OK or the VPT_ERR_* the call returns
    const char* msg;   // static; what vpt_last_error then says
};
constexpr Verdict kAccepted{VPT_OK, ""};
constexpr const char* kNoPositiveValue = "density grid has no positive value";

inline uint32_t cells_along(uint32_t dim) { return dim / VPT_BRICK_DIM + (dim % VPT_BRICK_DIM ? 1u : 0u); }   // ceil(dim / 8); dim + 7 may wrap

// ---- the arithmetic both kinds share (AddDensityDataToVolume, PathTracer.cpp:1390-1442): one voxel into the maximum, one voxel into the block maxima.
// Both are order-free: a maximum, and `<` against what is there; a voxel holding 0 (every voxel no brick covers) changes neither.
inline void max_in(float& mx, float raw) { mx = std::max(mx, raw); }
// (sx, sy, sz): where the voxel is stored.  The table is indexed with y flipped ("Y has to be flipped for vulkan", :1435).
inline void block_max_in(float* block_max, const uint32_t* dim, uint32_t sx, uint32_t sy, uint32_t sz, float raw, float mx) {
    const uint32_t x = sx, y = dim[1] - 1u - sy, z = sz;
    const float dens = vptfp::clamp_(raw / mx, 0.0f, 1.0f);
    const uint32_t bi = ((x * 32u) / dim[0]) + ((y * 32u) / dim[1]) * 32u + ((z * 32u) / dim[2]) * 1024u;
    if (block_max[bi] < dens) block_max[bi] = dens;
}

struct Maxima {
    float max_density = 0.0f;
    std::vector<float> block_max;   // 32^3, value / max_density clamped to [0, 1]
};

// ---- dense
// (the maximum and block maxima of an accepted dense grid; vpt_add_density_grid's argument checks stay where they were)
inline Verdict dense_maxima(uint32_t dx, uint32_t dy, uint32_t dz, const float* d, Maxima& out) {
    const uint32_t dim[3] = {dx, dy, dz};
    const size_t n = (size_t)dx * dy * dz;
    float mx = 0.0f;
    for (size_t i = 0; i < n; i++) max_in(mx, d[i]);
    if (!(mx > 0.0f)) return {VPT_ERR_INVALID_ARGUMENT, kNoPositiveValue};
    out.max_density = mx;
    out.block_max.assign(kBlockTable, 0.0f);
    for (uint32_t z = 0; z < dz; z++)
        for (uint32_t y = 0; y < dy; y++)
            for (uint32_t x = 0; x < dx; x++) {
                const uint32_t sy = dy - 1u - y;
                block_max_in(out.block_max.data(), dim, x, sy, z, d[(size_t)x + (size_t)sy * dx + (size_t)z * dx * dy], mx);
            }
    return kAccepted;
}

// ---- bricked
// Every reason vpt_add_density_bricks rejects its arguments for that needs no look at the data, in the order it reports them.
inline Verdict check_bricks(uint32_t dx, uint32_t dy, uint32_t dz, uint32_t brick_count, const uint32_t* coords, const float* values, size_t grids_in_use) {
    if (dx == 0 || dy == 0 || dz == 0) return {VPT_ERR_INVALID_ARGUMENT, "density grid dimension is zero"};
    const uint64_t xy = (uint64_t)cells_along(dx) * cells_along(dy);   // (< 2^58; times the third only once it is known to be small)
    if (xy > kMaxCells || xy * cells_along(dz) > kMaxCells) return {VPT_ERR_LIMIT, "more than 2^26 brick cells"};
    if (grids_in_use >= VPT_MAX_DENSITY_GRIDS) return {VPT_ERR_LIMIT, "more than VPT_MAX_DENSITY_GRIDS density grids"};
    if (brick_count == 0) return {VPT_ERR_INVALID_ARGUMENT, kNoPositiveValue};
    if (brick_count > kMaxBricks) return {VPT_ERR_LIMIT, "more than 2^22 bricks"};
    if (!coords || !values) return {VPT_ERR_INVALID_ARGUMENT, "no brick coordinates or values"};
    return kAccepted;
}
// The brick table of accepted arguments; rejects a coordinate outside the cell box and one given twice.
inline Verdict brick_table(uint32_t dx, uint32_t dy, uint32_t dz, uint32_t brick_count, const uint32_t* coords, std::vector<uint32_t>& table) {
    const uint32_t cx = cells_along(dx), cy = cells_along(dy), cz = cells_along(dz);
    table.assign((size_t)cx * cy * cz, kEmptyCell);
    for (uint32_t b = 0; b < brick_count; b++) {
        const uint32_t* c = coords + (size_t)b * 3;
        if (c[0] >= cx || c[1] >= cy || c[2] >= cz) return {VPT_ERR_INVALID_ARGUMENT, "brick coordinate outside the grid"};
        uint32_t& cell = table[(size_t)c[0] + (size_t)c[1] * cx + (size_t)c[2] * cx * cy];
        if (cell != kEmptyCell) return {VPT_ERR_INVALID_ARGUMENT, "brick coordinate given twice"};
        cell = b;
    }
    return kAccepted;
}
// f(sx, sy, sz, raw) for every voxel of every brick that lies inside the index box (a partial brick's other voxels are never looked at).
template <class F>
inline void for_each_voxel(const uint32_t* dim, uint32_t brick_count, const uint32_t* coords, const float* values, F f) {
    for (uint32_t b = 0; b < brick_count; b++) {
        const uint32_t x0 = coords[(size_t)b * 3] * VPT_BRICK_DIM, y0 = coords[(size_t)b * 3 + 1] * VPT_BRICK_DIM, z0 = coords[(size_t)b * 3 + 2] * VPT_BRICK_DIM;
        const float* v = values + (size_t)b * kBrickVoxels;
        VPT_GRID_ROLLED
        for (uint32_t i = 0; i < kBrickVoxels; i++) {
            const uint32_t sx = x0 + (i & 7u), sy = y0 + ((i >> 3) & 7u), sz = z0 + (i >> 6);
            if (sx < dim[0] && sy < dim[1] && sz < dim[2]) f(sx, sy, sz, v[i]);
        }
    }
}
inline Verdict brick_maxima(uint32_t dx, uint32_t dy, uint32_t dz, uint32_t brick_count, const uint32_t* coords, const float* values, Maxima& out) {
    const uint32_t dim[3] = {dx, dy, dz};
    float mx = 0.0f;
    for_each_voxel(dim, brick_count, coords, values, [&](uint32_t, uint32_t, uint32_t, float raw) { max_in(mx, raw); });
    if (!(mx > 0.0f)) return {VPT_ERR_INVALID_ARGUMENT, kNoPositiveValue};
    out.max_density = mx;
    out.block_max.assign(kBlockTable, 0.0f);
    float* bm = out.block_max.data();
    for_each_voxel(dim, brick_count, coords, values, [&](uint32_t sx, uint32_t sy, uint32_t sz, float raw) { block_max_in(bm, dim, sx, sy, sz, raw, mx); });
    return kAccepted;
}

// What a grid holds on the device: values + brick table + block maxima (vpt_density_grid_info.device_bytes).
inline uint64_t device_bytes(const DensityGrid& g) {
    if (!g.bricks) return (uint64_t)g.dim[0] * g.dim[1] * g.dim[2] * 4u + kBlockTable * 4u;
    return (uint64_t)g.brick_count * kBrickVoxels * 4u + (uint64_t)g.cells[0] * g.cells[1] * g.cells[2] * 4u + kBlockTable * 4u;
}

}  // namespace grid
}  // namespace vpt
