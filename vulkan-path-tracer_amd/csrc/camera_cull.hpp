// camera_cull.hpp — which pixels' camera rays can reach the scene at all: a rectangle of the image outside which no camera ray, whatever its
// jitter, enters the scene's box.  The whole-path kernel (kernels_whole.hip k_whole) starts no path for a sample outside it: its launch
// indices run over the samples inside alone (whole_deal.hpp), and the others' frame sum, which is exactly zero, is written in runs.  screen_bound is host code in double (api_render.hip batch_begin calls it
// once per batch); Packed / outside are what the kernel sees.  Plain arithmetic, compiled for the device and — by
// tests/tools/camera_cull_driver.cpp — for the host (tests/test_camera_cull_cpu.py).  k_bounce<FIRST> and k_raygen_stream do not use it yet;
// nothing here knows of k_whole.
//
// The geometry.  camera_ray (camera.hpp) sends the sample (x, y) with jitter (j0, j1) in [0, 1) through the image point
//   dx = (x + j0) / width * 2 - 1,  dy = (y + j1) / height * 2 - 1
// along  view3 * normalize(proj3 * (dx, dy, 1, 1)),  view3 / proj3 the rows 0-2 of view_inv / proj_inv — a positive multiple of
// M * (dx, dy, 1) with
//   M = V * [proj3 col 0 | proj3 col 1 | proj3 col 2 + proj3 col 3],  V = view3[:, 0:3];
// with the lens off (camera.hpp lens_off) every ray starts at the camera's position o and `focus - origin` is that direction again.  The ray
// reaches the point c iff c - o = t * M * (dx, dy, 1) with t > 0, i.e. iff q = M^-1 (c - o) has q.z > 0 and (dx, dy) = (q.x, q.y) / q.z.  A
// box all of whose corners have q.z > 0 therefore projects into the convex hull of its corners' image points, and a pixel whose square
// [x, x + 1) x [y, y + 1) of (x + j0, y + j1) lies outside the corners' bounding rectangle sends no ray into the box.
// The box is the union of the root node's used child boxes as the device tree holds them (the padded fp32 boxes of nodes_wide): a ray that
// misses it misses every child of the root, which is all the kernel's search would have found out.
//
// The roundings.  That is the exact ray; the device's is computed in fp32, and the rectangle is grown by kMarginPixels for the difference.
// screen_bound bounds the difference and culls only where it is at most HALF the margin (kRoundingPixels); else it returns "everything".
//   * The step that can be large: focus = o + direction * fd, fd = max(focus_distance, 0.001), is rounded to the ulp of its own size,
//     |o_a| + |direction| * fd at most per component a, and `focus - o` is then only |direction| * fd long.  focus_distance is any float — with
//     the lens off it has no other meaning, and 0 is a natural value — so the final direction is off by up to
//       2^-24 * |(|o_a| + smax * fd)_a| / (smin * fd)   radians,
//     smin / smax bounds of V's singular values (1 for a rigid camera): degrees for a camera 1000 units from the origin with fd = 0.
//   * Everything else (dx and dy, the two matrix products, the two normalisations, the product with fd, the subtraction) is a few relative
//     roundings of quantities of the direction's own size, times the condition of the matrices they pass through: kOtherRoundings * 2^-24 *
//     cond(M) * cond(V), conditions in the Frobenius norm over 3 (1 at best).
//   * A unit direction d off by the vector e has q = M^-1 d off by M^-1 e, and q.z = 1 / |M * (dx, dy, 1)| >= 1 / L, L the largest of
//     that norm over the image's four corners (the norm is convex).  To first order the image point moves by at most
//       (|row 0 of M^-1| + |row 2|) * |e| * L  in dx  and  (|row 1| + |row 2|) * |e| * L  in dy   (|dx|, |dy| <= 1),
//     times width / 2 and height / 2 in pixels.  The terms of higher order are that small again, relatively: the other half of the margin
//     holds them with room to spare.
//
// Why the skipped sample's frame sum is exactly (0, 0, 0, 0) wherever screen_bound culls.  Its path is one camera ray that misses: k_whole runs
// shade_core<kShadeMiss> at depth 0 and whole_finish with thr = 1, pathLight = 0.
//   * shade_core's miss branch: at depth 0 the environment is read only under VPT_FLAG_SHOW_ENV_DIRECTLY, and then only when it is not black; in
//     every other case cp.xyz = 0 and emitted = 0 * sky_intensity: +0, -0, or NaN for an infinite or NaN sky_intensity.  VPT_FLAG_FURNACE sets
//     emitted = 1 (no cull then); the sky MIS weight applies at depth > 0 only.
//   * path_contribution: E * 1 is E; under the luminance clamp lum is +-0 or NaN and the scale max_luminance / max(lum, max_luminance) is 1, or NaN
//     for max_luminance 0 or NaN: contrib is +-0 or NaN.
//   * whole_finish: light = +0 + contrib is +0 (+0 + -0 = +0) or NaN; finite3 passes +0, and 0 + +0 = +0 is stored with w = 0; NaN stores the
//     four zeros of the guard.  Either way ACC[slot] = (0, 0, 0, 0), bit for bit.
// So no cull with the furnace flag, none with an environment that is shown directly and is not black, none with the lens on (origins differ per
// sample), none when a corner is not strictly in front (the camera inside or beside the box), none when M cannot be inverted, and none when
// the roundings' bound is more than half the margin or focus_distance is not a finite number.
#pragma once
#include <stdint.h>

#include "camera.hpp"   // lens_off; + vpt_fp32.h
#include "../../include/vpt.h"   // VPT_FLAG_*

namespace vpt {
namespace cull {

constexpr int kMarginPixels = 2;
constexpr double kRoundingPixels = 1.0;    // what the device's roundings may move a ray by, at most, where there is a rectangle: half the margin
constexpr double kOtherRoundings = 24.0;   // camera_ray's roundings besides focus's, in units of 2^-24 of the direction's length (see above)
constexpr uint32_t kMaxSize = 32768u;   // images wider or higher than this are not culled (Packed keeps 15-bit bounds)

// The scene's box; valid: there is one (the tree rides in LDS and its root has a used child).
struct WorldBox { float lo[3], hi[3]; bool valid; };

// Inclusive pixel rectangle [x0, x1] x [y0, y1] outside which every sample may be skipped.  all: everything is inside (no cull) and the bounds
// are the image's; x0 > x1: nothing is inside.
struct Rect { uint32_t x0, y0, x1, y1; bool all; };

// The rectangle as the kernel's two argument words, one per axis: first | span << 16 with span = last - first, and span 0xffff for "no bound on
// this axis" (it decodes to 0xffffffff).  An empty range is first 0xffff, span 0: no coordinate of an image of at most kMaxSize is inside.
struct Packed { uint32_t x, y; };
constexpr uint32_t kAxisAll = 0xffff0000u;
VPT_HD uint32_t pack_axis(uint32_t first, uint32_t last) { return first > last ? 0xffffu : (first | (last - first) << 16); }
VPT_HD Packed pack(const Rect& r) {
    Packed p;
    if (r.all) { p.x = kAxisAll; p.y = kAxisAll; } else { p.x = pack_axis(r.x0, r.x1); p.y = pack_axis(r.y0, r.y1); }
    return p;
}
VPT_HD uint32_t axis_first(uint32_t w) { return w & 0xffffu; }
VPT_HD uint32_t axis_span(uint32_t w) { return (uint32_t)((int32_t)w >> 16); }   // (a bound's span is below 0x8000; 0xffff becomes 0xffffffff)
VPT_HD bool outside(Packed p, uint32_t x, uint32_t y) { return x - axis_first(p.x) > axis_span(p.x) || y - axis_first(p.y) > axis_span(p.y); }
// Pixels of a width x height image outside the rectangle (host: tests, the laboratory's count).
VPT_HD bool outside(const Rect& r, uint32_t x, uint32_t y) { return !r.all && (x < r.x0 || x > r.x1 || y < r.y0 || y > r.y1); }

inline Rect everything(uint32_t width, uint32_t height) { Rect r; r.x0 = 0u; r.y0 = 0u; r.x1 = width - 1u; r.y1 = height - 1u; r.all = true; return r; }

// One axis: the pixels whose [p, p + 1) can meet [lo, hi] (in pixel units), grown by the margin and clipped to [0, n - 1]; first > last: none.
inline void axis_range(double lo, double hi, uint32_t n, uint32_t& first, uint32_t& last) {
    const double a = __builtin_floor(lo) - kMarginPixels, b = __builtin_floor(hi) + kMarginPixels;
    if (!(b >= 0.0) || !(a <= (double)(n - 1u))) { first = 1u; last = 0u; return; }
    first = a > 0.0 ? (uint32_t)a : 0u;
    last = b < (double)(n - 1u) ? (uint32_t)b : n - 1u;
}

// The rows of a 3x3 matrix's inverse times its determinant — the cross products of its columns (m[col][row]) — and the determinant.
inline double adjugate_rows(const double m[3][3], double adj[3][3]) {
    for (int i = 0; i < 3; i++) {
        const double *u = m[(i + 1) % 3], *v = m[(i + 2) % 3];
        for (int a = 0; a < 3; a++) adj[i][a] = u[(a + 1) % 3] * v[(a + 2) % 3] - u[(a + 2) % 3] * v[(a + 1) % 3];
    }
    return m[0][0] * adj[0][0] + m[0][1] * adj[0][1] + m[0][2] * adj[0][2];
}
inline double row2(const double* r) { return r[0] * r[0] + r[1] * r[1] + r[2] * r[2]; }
inline double frob2(const double m[3][3]) { return row2(m[0]) + row2(m[1]) + row2(m[2]); }

// The rectangle for one camera, image size, set of render parameters and box.
inline Rect screen_bound(const float* view_inv, const float* proj_inv, uint32_t width, uint32_t height, float focus_distance, float dof_strength, uint32_t flags, bool env_black, const WorldBox& box) {
    const Rect all = everything(width, height);
    if (!box.valid || width == 0u || height == 0u || width > kMaxSize || height > kMaxSize) return all;
    if ((flags & VPT_FLAG_FURNACE) || ((flags & VPT_FLAG_SHOW_ENV_DIRECTLY) && !env_black)) return all;
    const V4 o4 = mat_v4(view_inv, v4(0.0f, 0.0f, 0.0f, 1.0f));   // camera_ray's origin
    if (!lens_off(view_inv, v3(o4.x, o4.y, o4.z), dof_strength)) return all;
    if (!(focus_distance < 1.0e30f) || !(focus_distance > -1.0e30f)) return all;   // NaN or beyond any scene: camera_ray's focus is no point
    // V and M by columns, m[col][row] (the two matrices are column-major, m[col * 4 + row])
    double vc[3][3], mc[3][3], vinv[3][3], inv[3][3];
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) {
            double acc = 0.0;
            for (int k = 0; k < 3; k++) acc += (double)view_inv[k * 4 + r] * ((double)proj_inv[c * 4 + k] + (c == 2 ? (double)proj_inv[12 + k] : 0.0));
            mc[c][r] = acc; vc[c][r] = (double)view_inv[c * 4 + r];
        }
    const double det = adjugate_rows(mc, inv), vdet = adjugate_rows(vc, vinv), norm2 = frob2(mc);
    if (!(norm2 < 1.0e300) || !(__builtin_fabs(det) > 1.0e-9 * norm2 * __builtin_sqrt(norm2)) || !(__builtin_fabs(vdet) > 0.0)) return all;   // singular, or not finite
    const float org[3] = {o4.x, o4.y, o4.z};
    {   // the device's roundings (the header's argument): no rectangle where they can move a ray by more than kRoundingPixels
        const double fd = focus_distance > 0.001f ? (double)focus_distance : (double)0.001f, v2 = frob2(vc), vi2 = frob2(vinv) / (vdet * vdet);
        const double smax = __builtin_sqrt(v2), smin = 1.0 / __builtin_sqrt(vi2), cond = __builtin_sqrt(norm2 * frob2(inv) / (det * det) * v2 * vi2) / 9.0;
        double e2 = 0.0, big = 0.0;
        for (int a = 0; a < 3; a++) { const double m = __builtin_fabs((double)org[a]) + smax * fd; e2 += m * m; }
        for (int k = 0; k < 4; k++) {
            double l2 = 0.0;
            for (int r = 0; r < 3; r++) { const double t = (k & 1 ? mc[0][r] : -mc[0][r]) + (k & 2 ? mc[1][r] : -mc[1][r]) + mc[2][r]; l2 += t * t; }
            big = l2 > big ? l2 : big;
        }
        const double e = 5.9604644775390625e-08 * (__builtin_sqrt(e2) / (smin * fd) + kOtherRoundings * cond) * __builtin_sqrt(big) / __builtin_fabs(det);
        const double rx = __builtin_sqrt(row2(inv[0])), ry = __builtin_sqrt(row2(inv[1])), rz = __builtin_sqrt(row2(inv[2]));
        if (!((rx + rz) * e * 0.5 * (double)width <= kRoundingPixels) || !((ry + rz) * e * 0.5 * (double)height <= kRoundingPixels)) return all;
    }
    double lo_x = 1.0e300, hi_x = -1.0e300, lo_y = 1.0e300, hi_y = -1.0e300;
    for (int k = 0; k < 8; k++) {
        double c[3], q[3];
        for (int a = 0; a < 3; a++) c[a] = (double)((k >> a) & 1 ? box.hi[a] : box.lo[a]) - (double)org[a];
        for (int r = 0; r < 3; r++) q[r] = (inv[r][0] * c[0] + inv[r][1] * c[1] + inv[r][2] * c[2]) / det;
        // strictly in front, by a margin: a corner level with the camera has its image point at infinity
        if (!(q[2] > 1.0e-6 * (__builtin_fabs(q[0]) + __builtin_fabs(q[1]) + __builtin_fabs(q[2]))) || !(q[2] < 1.0e300)) return all;
        const double px = (q[0] / q[2] + 1.0) * 0.5 * (double)width, py = (q[1] / q[2] + 1.0) * 0.5 * (double)height;
        lo_x = px < lo_x ? px : lo_x; hi_x = px > hi_x ? px : hi_x;
        lo_y = py < lo_y ? py : lo_y; hi_y = py > hi_y ? py : hi_y;
    }
    Rect r; r.all = false;
    axis_range(lo_x, hi_x, width, r.x0, r.x1);
    axis_range(lo_y, hi_y, height, r.y0, r.y1);
    if (r.x0 > r.x1 || r.y0 > r.y1) { r.x0 = 1u; r.y0 = 1u; r.x1 = 0u; r.y1 = 0u; }   // nothing inside: one way to say it
    return r;
}

}  // namespace cull
}  // namespace vpt
