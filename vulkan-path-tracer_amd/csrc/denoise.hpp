// denoise.hpp — the arithmetic of vpt_denoise, once: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010, as SVGF uses it) over the accumulation
// image, steered by the first-hit guide images (normal, depth, albedo of the VPT_FEATURES_CENTER rays), with optional albedo demodulation.  Plain
// functions on plain values built from vptfp:: leaves only (exp_, max_, fabs_, + - * /), no context and no HIP call: kernels_post.hip calls them per
// pixel, tests/tools/denoise_driver.cpp runs them on the host (tests/test_denoise_cpu.py), and because the library is built without contraction and with
// correctly rounded division the two give the same bits.  The order of every sum is fixed HERE: taps row-major (dy outer, dx inner), then channels r, g, b.
//
//   prepare     e = c.rgb / max_(albedo, 1e-3) per channel (DEMODULATE) or c.rgb; alpha kept.  The guide is packed as (n.x, n.y, n.z, t): a tap costs two
//               16-byte reads.  A miss pixel (t < 0) keeps c as it is, through every pass: its output is its input bit for bit.
//   pass i      step s = 1 << i, 5 x 5 taps q = p + s (dx, dy), kernel k = outer product of [1/16, 1/4, 3/8, 1/4, 1/16]:
//                   e'(p) = sum k(q) w(p, q) e(q) / sum k(q) w(p, q)        over the taps inside the image that are hits
//                   w = exp_(-(dn + dz + dc)), w = 1 at the centre tap (the denominator is >= 9/64)
//                   dn = max_(0, 1 - dot(n_p, n_q)) / sigma_normal
//                   dz = |t_p - t_q| / (sigma_depth s max_(t_p, 1e-6))
//                   dc = |e_p - e_q|^2 / (sigma_color 2^-i)^2                  e of the previous pass
//               The three divisors do not depend on the tap: their reciprocals are formed once (per pass: pass_of; per pixel: the depth's) and a tap
//               multiplies.  exp_ returns exactly 0 below -103.9: a tap across a hard edge has no influence at all.
//   last pass   multiplies by the same max_(albedo, 1e-3) again.
// Non-finite input propagates: a NaN or an infinite colour reaches every pixel whose weight for it is not exactly 0.  There is no guard.
#pragma once
#include <stdint.h>

#include "../../include/vpt_fp32.h"

// The tap loops stay rolled on the device: unrolling the inner one doubles both kernels' code (3.5 KB against 1.7 KB each) and the product library's size
// bound (tests/test_abi.py) has no page to spare for it.
#if defined(__clang__)
#define VPT_DN_ROLLED _Pragma("unroll 1")
#else
#define VPT_DN_ROLLED
#endif

namespace vpt {
namespace denoise {

struct alignas(16) F4 { float x, y, z, w; };

constexpr float kAlbedoFloor = 1.0e-3f, kDepthFloor = 1.0e-6f;

// What a pass needs of vpt_denoise_params, formed once on the host.
struct Pass {
    int step;            // 1 << i
    float rcp_normal;    // 1 / sigma_normal
    float depth_scale;   // sigma_depth * step
    float rcp_color;     // 1 / (sigma_color * 2^-i)^2
};
inline Pass pass_of(uint32_t i, float sigma_color, float sigma_normal, float sigma_depth) {
    Pass p;
    p.step = 1 << i;
    p.rcp_normal = 1.0f / sigma_normal;
    p.depth_scale = sigma_depth * (float)p.step;
    const float sc = sigma_color * vptfp::pow2i_(-(int)i);
    p.rcp_color = 1.0f / (sc * sc);
    return p;
}

VPT_HD F4 f4(float x, float y, float z, float w) { F4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
VPT_HD bool is_hit(const F4& guide) { return !(guide.w < 0.0f); }
VPT_HD F4 pack_guide(const F4& normal, float depth) { return f4(normal.x, normal.y, normal.z, depth); }
VPT_HD F4 albedo_scale(const F4& albedo) {
    return f4(vptfp::max_(albedo.x, kAlbedoFloor), vptfp::max_(albedo.y, kAlbedoFloor), vptfp::max_(albedo.z, kAlbedoFloor), 1.0f);
}
// The prepare pass of one pixel.
VPT_HD F4 prepare_pixel(const F4& c, const F4& albedo, float depth, bool demodulate) {
    if (depth < 0.0f || !demodulate) return c;
    const F4 a = albedo_scale(albedo);
    return f4(c.x / a.x, c.y / a.y, c.z / a.z, c.w);
}
VPT_HD float tap_kernel(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

// One pass of one pixel.  src.color(x, y) / src.guide(x, y): e of the previous pass and the packed guide at a pixel INSIDE the image — where they are read
// from (memory, an LDS tile, a host array) is the caller's business and changes no bit.  ep, gp: the pixel's own.  last + demodulate: re-modulate by albedo.
template <class Src>
VPT_HD F4 atrous_pixel(const Src& src, int x, int y, int w, int h, const Pass& ps, const F4& ep, const F4& gp, bool remodulate, const F4& albedo) {
    if (!is_hit(gp)) return ep;
    const float rcp_depth = 1.0f / (ps.depth_scale * vptfp::max_(gp.w, kDepthFloor));
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
    VPT_DN_ROLLED
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * ps.step;
        if (qy < 0 || qy >= h) continue;
        const float ky = tap_kernel(dy);
        VPT_DN_ROLLED
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * ps.step;
            if (qx < 0 || qx >= w) continue;
            const F4 gq = src.guide(qx, qy);
            const F4 eq = src.color(qx, qy);   // (asked for before gq is looked at: the two reads of a tap are in flight together)
            if (!is_hit(gq)) continue;
            float wt = 1.0f;
            if (dx != 0 || dy != 0) {
                const float nd = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
                const float dn = vptfp::max_(0.0f, 1.0f - nd) * ps.rcp_normal;
                const float dz = vptfp::fabs_(gp.w - gq.w) * rcp_depth;
                const float cx = ep.x - eq.x, cy = ep.y - eq.y, cz = ep.z - eq.z;
                const float dc = ((cx * cx + cy * cy) + cz * cz) * ps.rcp_color;
                wt = vptfp::exp_(-((dn + dz) + dc));
            }
            const float kw = (ky * tap_kernel(dx)) * wt;
            sr = sr + kw * eq.x;
            sg = sg + kw * eq.y;
            sb = sb + kw * eq.z;
            sw = sw + kw;
        }
    }
    F4 r = f4(sr / sw, sg / sw, sb / sw, ep.w);
    if (remodulate) {
        const F4 a = albedo_scale(albedo);
        r.x = r.x * a.x; r.y = r.y * a.y; r.z = r.z * a.z;
    }
    return r;
}

}  // namespace denoise
}  // namespace vpt
