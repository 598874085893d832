// svgf_spatial.hpp — the arithmetic of vpt_svgf_spatial_options, once: SVGF's spatial variance estimate for pixels whose history is too short for the
// temporal one (Schied et al. 2017, §4.2).  temporal.hpp's temporal_pixel_variance writes -1 ("unknown") where a hit pixel's new history length is below
// min_len = min_history * m; such a pixel is YOUNG.  Here a young pixel takes the luminance moments of its neighbourhood — the new moment record, the one
// the temporal step has just written — through a bilateral window, and its variance becomes >= 0: the variance-guided a-trous passes of denoise.hpp then
// filter it like any other pixel.  Plain functions on plain values built from vptfp:: leaves only (exp_, max_, fabs_, + - * /), no context and no HIP
// call: kernels_post.hip k_variance_spatial calls spatial_variance_pixel per young pixel, tests/tools/svgf_spatial_driver.cpp runs it on the host
// (tests/test_svgf_spatial_cpu.py), and because the library is built without contraction and with correctly rounded division the two give the same bits.
// The order of every sum is fixed HERE: taps row-major (dy outer, dx inner), and per tap sw, then s1, then s2.
//
// Per pixel p with guide (n_p, t_p), history length len_p and the temporal step's variance v_in:
//   not young   a miss (t_p < 0), or len_p >= min_len — temporal_pixel_variance's own comparison: v_in bit for bit.
//   young       window of radius R (1..3: 3 x 3 .. 7 x 7) around p.  A tap q outside the image or whose guide is a miss is skipped.  The centre has weight 1.
//               Any other tap, at ring r = max(|dx|, |dy|):
//                   dn = max_(0, 1 - dot(n_p, n_q)) / sigma_normal                 (the dot summed (x + y) + z)
//                   dz = |t_p - t_q| / (sigma_depth r max_(t_p, 1e-6))
//                   wt = exp_(-(dn + dz))
//               The divisors do not depend on the tap: 1 / sigma_normal is formed once on the host (plan_of), the depth's reciprocal once per pixel and
//               ring.  exp_ returns exactly 0 below -103.9: a tap across a hard edge has no influence at all.
//                   sw += wt; s1 += wt mu1_q; s2 += wt mu2_q
//               !(sw >= min_weight): -1 — too little of the window belongs to this surface to say anything, the pixel keeps the fixed-sigma rule (a NaN
//               lands here too).  Otherwise M1 = s1 / sw, M2 = s2 / sw and the variance is max_(0, M2 - M1 M1).
// No history-length boost (SVGF multiplies a young pixel's estimate by 4 / len): a neighbour with a long history contributes its temporal moments, whose
// mu2 - mu1^2 already is the variance of ONE call's luminance, and a neighbourhood of history-less pixels contributes (l, l l), whose spread over the window
// is that same quantity.  Both ends estimate what the temporal variance estimates — the per-call variance the a-trous rule divides luminance differences
// by — so nothing is scaled.
// The instance id is not tested: a young pixel's neighbours on the same surface are what is wanted, whatever the instance.
// Non-finite input propagates: a NaN moment reaches every young pixel that has it as a tap — s1 and s2 are NaN there (a weight that underflowed to exactly 0
// does not stop a NaN either: 0 NaN is NaN, as in denoise.hpp's sums), and max_(0, NaN) is 0, temporal_pixel_variance's answer to NaN moments too.  A
// non-finite guide makes the weights NaN and lands on -1.  There is no guard.
// Only the variance image changes — image, record, moments, history length and motion keep their bits — and the variance image is not history: nothing
// feeds back into the next call.
#pragma once
#include <stdint.h>

#include "temporal.hpp"

namespace vpt {
namespace svgf_spatial {

using denoise::F4;
using temporal::M2;

constexpr int kMaxRadius = 3;

// What the window needs of vpt_svgf_spatial_options, formed once on the host.
struct Plan {
    int radius;          // 1 .. kMaxRadius
    float rcp_normal;    // 1 / sigma_normal
    float sigma_depth;
    float min_weight;
};
inline Plan plan_of(uint32_t radius, float sigma_normal, float sigma_depth, float min_weight) {
    Plan p;
    p.radius = (int)radius;
    p.rcp_normal = 1.0f / sigma_normal;
    p.sigma_depth = sigma_depth;
    p.min_weight = min_weight;
    return p;
}

// One pixel.  src.guide(x, y) / src.moments(x, y): the packed guide (n.xyz, t) and the moments {mu1, mu2} of the NEW record at a pixel INSIDE the image —
// where they are read from (memory, an LDS tile, a host array) is the caller's business and changes no bit.  len_p, gp, v_in: the pixel's own.
template <class Src>
VPT_HD float spatial_variance_pixel(const Src& src, int x, int y, int w, int h, const Plan& plan, float len_p, float min_len, const F4& gp, float v_in) {
    if (!denoise::is_hit(gp) || len_p >= min_len) return v_in;
    const float tp = vptfp::max_(gp.w, denoise::kDepthFloor);
    // rcp_depth[r - 1], as three values: an array indexed by the ring would live in scratch on the device
    const float rd1 = 1.0f / ((plan.sigma_depth * 1.0f) * tp), rd2 = 1.0f / ((plan.sigma_depth * 2.0f) * tp), rd3 = 1.0f / ((plan.sigma_depth * 3.0f) * tp);
    float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
    VPT_DN_ROLLED
    for (int dy = -plan.radius; dy <= plan.radius; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= h) continue;
        const int ay = dy < 0 ? -dy : dy;
        VPT_DN_ROLLED
        for (int dx = -plan.radius; dx <= plan.radius; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= w) continue;
            const F4 gq = src.guide(qx, qy);
            const M2 mq = src.moments(qx, qy);   // (asked for before gq is looked at: the two reads of a tap are in flight together)
            if (!denoise::is_hit(gq)) continue;
            float wt = 1.0f;
            if (dx != 0 || dy != 0) {
                const int ax = dx < 0 ? -dx : dx;
                const int r = ax > ay ? ax : ay;
                const float nd = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
                const float dn = vptfp::max_(0.0f, 1.0f - nd) * plan.rcp_normal;
                const float dz = vptfp::fabs_(gp.w - gq.w) * (r == 1 ? rd1 : (r == 2 ? rd2 : rd3));
                wt = vptfp::exp_(-(dn + dz));
            }
            sw = sw + wt;
            s1 = s1 + wt * mq.mu1;
            s2 = s2 + wt * mq.mu2;
        }
    }
    if (!(sw >= plan.min_weight)) return temporal::kUnknownVariance;
    const float m1 = s1 / sw, m2 = s2 / sw;
    return vptfp::max_(0.0f, m2 - m1 * m1);
}

}  // namespace svgf_spatial
}  // namespace vpt
