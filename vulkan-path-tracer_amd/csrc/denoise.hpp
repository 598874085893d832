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

// ---- the variance-guided passes (vpt_svgf_options.variance == 1, denoise source TEMPORAL): SVGF's a-trous, Schied et al. 2017
// The variance v of the temporal luminance moments rides in e.w through the passes (>= 0 known, -1 unknown); the source's alpha waits in the .w of the
// denoiser's albedo copy, which no pass reads before the last one puts it back.  A miss keeps its input — alpha included — through every pass, as above.
//   prepare     e.rgb as above; hit: e.w = v, albedo.w = alpha.
//   pass, v_p < 0    the rule above for this pixel, tap for tap (fixed sigma_color, every hit tap: the same sums in the same order); v' = -1.
//   pass, else  g = the 3 x 3 Gaussian (centre 1/4, edges 1/8, corners 1/16; row-major) of v over the pixels at distance 1 — whatever the step — that
//               are inside the image, hits and have v >= 0, divided by the kernel weights that counted (>= 1/4: the centre counts unless v_p is NaN).
//               Taps with v_q < 0 are skipped; for the others w = exp_(-((dn + dz) + dl)), dn and dz as above,
//                   dl = |lum(e_p) - lum(e_q)| / (sigma_luminance sqrt_(g) + 1e-6)      lum = temporal's (0.2126 r + 0.7152 g) + 0.0722 b
//               (the divisor's reciprocal formed once per pixel), w = 1 at the centre.
//                   e' = sum k w e_q / sum k w          v' = sum (k w)^2 v_q / (sum k w)^2
//               With g = 0 (a converged neighbourhood) the reciprocal is 1e6: a tap whose luminance differs by more than 1.04e-4 has weight exactly 0.
//   last pass   multiplies by max_(albedo, 1e-3) again (DEMODULATE) and returns alpha to .w.
constexpr float kLumFloor = 1.0e-6f;
VPT_HD float luminance(const F4& e) { return (0.2126f * e.x + 0.7152f * e.y) + 0.0722f * e.z; }
VPT_HD float prefilter_kernel(int d) { return d == 0 ? 0.5f : 0.25f; }   // outer product: centre 1/4, edges 1/8, corners 1/16
// The prepare pass of one pixel: e (v in .w of a hit) and the albedo copy (alpha in .w of a hit).
VPT_HD F4 prepare_pixel_variance(const F4& c, F4& albedo, float depth, bool demodulate, float v) {
    F4 e = prepare_pixel(c, albedo, depth, demodulate);
    if (depth < 0.0f) return e;
    albedo.w = c.w;
    e.w = v;
    return e;
}
template <class Src>
VPT_HD F4 atrous_pixel_variance(const Src& src, int x, int y, int w, int h, const Pass& ps, float sigma_luminance, const F4& ep, const F4& gp, bool last, bool remodulate, const F4& albedo) {
    if (!is_hit(gp)) return ep;
    const bool fixed = ep.w < 0.0f;   // unknown variance: today's rule
    float rcp_lum = 0.0f;
    const float lp = luminance(ep);
    if (!fixed) {
        float gs = 0.0f, gw = 0.0f;
        VPT_DN_ROLLED
        for (int dy = -1; dy <= 1; dy++) {
            const int qy = y + dy;
            if (qy < 0 || qy >= h) continue;
            VPT_DN_ROLLED
            for (int dx = -1; dx <= 1; dx++) {
                const int qx = x + dx;
                if (qx < 0 || qx >= w) continue;
                const F4 gq = src.guide(qx, qy);
                const F4 eq = src.color(qx, qy);
                if (!is_hit(gq) || !(eq.w >= 0.0f)) continue;
                const float k = prefilter_kernel(dy) * prefilter_kernel(dx);
                gs = gs + k * eq.w;
                gw = gw + k;
            }
        }
        rcp_lum = 1.0f / (sigma_luminance * vptfp::sqrt_(gs / gw) + kLumFloor);
    }
    const float rcp_depth = 1.0f / (ps.depth_scale * vptfp::max_(gp.w, kDepthFloor));
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f, sv = 0.0f;
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
            const F4 eq = src.color(qx, qy);
            if (!is_hit(gq)) continue;
            if (!fixed && eq.w < 0.0f) continue;
            float wt = 1.0f;
            if (dx != 0 || dy != 0) {
                const float nd = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
                const float dn = vptfp::max_(0.0f, 1.0f - nd) * ps.rcp_normal;
                const float dz = vptfp::fabs_(gp.w - gq.w) * rcp_depth;
                float dc;
                if (fixed) {
                    const float cx = ep.x - eq.x, cy = ep.y - eq.y, cz = ep.z - eq.z;
                    dc = ((cx * cx + cy * cy) + cz * cz) * ps.rcp_color;
                } else {
                    dc = vptfp::fabs_(lp - luminance(eq)) * rcp_lum;
                }
                wt = vptfp::exp_(-((dn + dz) + dc));
            }
            const float kw = (ky * tap_kernel(dx)) * wt;
            sr = sr + kw * eq.x;
            sg = sg + kw * eq.y;
            sb = sb + kw * eq.z;
            sw = sw + kw;
            sv = sv + (kw * kw) * eq.w;
        }
    }
    F4 r = f4(sr / sw, sg / sw, sb / sw, fixed ? -1.0f : sv / (sw * sw));
    if (remodulate) {
        const F4 a = albedo_scale(albedo);
        r.x = r.x * a.x; r.y = r.y * a.y; r.z = r.z * a.z;
    }
    if (last) r.w = albedo.w;
    return r;
}

}  // namespace denoise
}  // namespace vpt
