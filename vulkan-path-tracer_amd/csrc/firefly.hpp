// firefly.hpp — the arithmetic of vpt_firefly_options, once: outlier ("firefly") rejection ahead of the viewport chain's two filters.  One 1-spp spike on a
// dark wall enters the temporal history and stays for max_history images, inflates its own second moment so that the variance-guided rule widens around it,
// is spread into a 5 x 5 blot by every a-trous pass and drags the exposure histogram's top bin; the integrator's max_luminance clamp is global and knows
// nothing of the wall.  Here a hit pixel whose luminance stands above threshold x the rank-th largest luminance of its neighbours is scaled down to that
// limit before k_temporal or k_denoise_prepare reads it.  Plain functions on plain values built from vptfp:: leaves only (max_, + - * /), no context and no
// HIP call: kernels_post.hip k_firefly calls firefly_pixel per pixel, tests/tools/firefly_driver.cpp runs it on the host (tests/test_firefly_cpu.py), and
// because the library is built without contraction and with correctly rounded division the two give the same bits.
//
// Luminance of a pixel q inside the image, from the accumulation image c and the first-hit guides of the consuming call:
//       l(q) = denoise::luminance(denoise::prepare_pixel(c_q, albedo_q, depth_q, demodulate))
//   demodulate is what the consuming call demodulates with (VPT_TEMPORAL_DEMODULATE for vpt_temporal_accumulate, VPT_DENOISE_DEMODULATE for vpt_denoise): the
//   clamp works in the space the filter works in.  A miss (depth < 0) has no luminance: staged_luminance gives -1 for it, and a position outside the image is
//   never asked for.
// Per pixel p:
//   miss        the output is the input bit for bit; a miss is never a tap.
//   hit         the (2R + 1)^2 window without its centre, R = 1..2, rows then columns.  A tap q counts when it is inside the image, a hit, and l_q >= 0: a NaN
//               or a negative luminance is no tap, +inf is one.  n = the number of counted taps; L = the rank-th largest counted luminance, rank 1..3, kept
//               as the three largest in registers by comparisons alone — an order statistic: nothing is rounded and the scan order cannot change it.
//                   n < rank           the output is the input bit for bit (too few neighbours to call anything an outlier)
//                   limit = max_(threshold L, floor)
//                   l_p > limit        s = limit / l_p, rgb' = (r s, g s, b s), alpha kept; the pixel counts as CLAMPED
//                   otherwise          the output is the input bit for bit — a NaN centre lands here.
//               A hit with n >= rank counts as CONSIDERED, clamped or not.
// No guard beyond that, as in the rest of the chain.  A +inf centre over a finite limit gives s = 0: its finite channels become 0 and its infinite ones
// 0 inf = NaN; over an infinite limit (a +inf neighbour at the rank) it is untouched.  Repairing non-finite pixels is not this filter's business.
// What the clamp costs — two documented limits:
//   bias        the clamp REMOVES energy: a pixel that was a legitimate rare bright sample is dimmed like a wrong one, so the mean of the filtered images lies
//               below the mean of the unfiltered ones.  tests/test_gpu_firefly.py reports the loss in mean luminance beside the gain in L2.
//   thin lights an emitter ONE pixel wide has no neighbour as bright as itself and is dimmed to threshold x its surroundings (or to floor, whichever is
//               larger).  floor is the lever: everything at or below it is never touched, whatever surrounds it.
// Only the image handed to the filter changes: the accumulation image keeps its bits (the kernel never writes in place), and no record is touched.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "denoise.hpp"

namespace vpt {
namespace firefly {

using denoise::F4;

constexpr int kMaxRadius = 2, kMaxRank = 3;
constexpr float kNoLuminance = -1.0f;   // what a miss stages
// The two counts of a launch — clamped and considered pixels — are summed by one integer atomic per wave and count.  A 4K image is 130,000 waves, nearly all of
// which have something to add to `considered`: on ONE word those adds would queue behind each other for longer than the pass itself takes (the reason
// k_luminance_histogram bounds its adds per word).  So a launch adds into kCounterSlots pairs, each on a 128-byte line of its own, a block choosing its pair by
// its index; the host sums the pairs when the state is read.  Integer sums: the totals do not depend on the arrival order or on the slot.
constexpr uint32_t kCounterSlots = 64u, kCounterStride = 32u;   // words from one pair to the next
constexpr size_t kCounterBytes = (size_t)kCounterSlots * kCounterStride * 4u;

// include/vpt.h's vpt_firefly_options, field for field (api_post.hip asserts the size), with its defaults and vpt_set_firefly_options' test of a record:
// nullptr, or what is wrong with it — here so that the host tests can ask without a device (tests/test_firefly_abi_cpu.py).
struct Options {
    uint32_t mode, radius, rank;
    float threshold, floor;
    uint32_t reserved[3];
};
inline Options default_options() { return Options{0u, 1u, 2u, 2.0f, 1.0f, {0u, 0u, 0u}}; }
inline const char* check_options(const Options& o) {
    const float big = 3.402823466e+38f;   // (FLT_MAX.  x <= big: finite; a NaN fails every comparison)
    if (o.mode > 1u) return "firefly options: mode must be 0 or 1";
    if (o.radius - 1u >= (uint32_t)kMaxRadius) return "firefly options: radius must be 1..2";
    if (o.rank - 1u >= (uint32_t)kMaxRank || o.rank > (2u * o.radius + 1u) * (2u * o.radius + 1u) - 1u) return "firefly options: rank must be 1..3 and no more than the window's taps";
    if (!(o.threshold >= 1.0f && o.threshold <= big)) return "firefly options: threshold must be finite and >= 1";
    if (!(o.floor >= 0.0f && o.floor <= big)) return "firefly options: floor must be finite and >= 0";
    if (o.reserved[0] | o.reserved[1] | o.reserved[2]) return "firefly options: reserved words must be 0";
    return nullptr;
}

// What the window needs of vpt_firefly_options and of the consuming call, formed once on the host.
struct Plan {
    int radius;        // 1 .. kMaxRadius
    int rank;          // 1 .. kMaxRank
    float threshold;   // >= 1
    float floor;       // >= 0
    int demodulate;    // the consuming call's
};
inline Plan plan_of(uint32_t radius, uint32_t rank, float threshold, float floor, bool demodulate) {
    Plan p;
    p.radius = (int)radius; p.rank = (int)rank; p.threshold = threshold; p.floor = floor; p.demodulate = demodulate ? 1 : 0;
    return p;
}

struct Result {
    F4 pixel;
    bool clamped;      // l_p > limit: rgb was scaled
    bool considered;   // a hit with n >= rank
};

// l(q), or -1 for a miss.  albedo is read by prepare_pixel only when demodulating a hit: a caller without an albedo image passes anything.
VPT_HD float staged_luminance(const F4& c, const F4& albedo, float depth, bool demodulate) {
    if (depth < 0.0f) return kNoLuminance;
    return denoise::luminance(denoise::prepare_pixel(c, albedo, depth, demodulate));
}

// One pixel.  src.lum(x, y): staged_luminance of a pixel INSIDE the image — where it is read from (an LDS tile, a host array) is the caller's business and
// changes no bit.  c_p, albedo_p, depth_p: the pixel's own.
template <class Src>
VPT_HD Result firefly_pixel(const Src& src, int x, int y, int w, int h, const Plan& plan, const F4& c_p, const F4& albedo_p, float depth_p) {
    Result r;
    r.pixel = c_p; r.clamped = false; r.considered = false;
    if (depth_p < 0.0f) return r;
    float t1 = kNoLuminance, t2 = kNoLuminance, t3 = kNoLuminance;   // the three largest counted luminances, t1 >= t2 >= t3
    int n = 0;
    VPT_DN_ROLLED
    for (int dy = -plan.radius; dy <= plan.radius; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= h) continue;
        VPT_DN_ROLLED
        for (int dx = -plan.radius; dx <= plan.radius; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= w || (dx == 0 && dy == 0)) continue;
            const float l = src.lum(qx, qy);
            if (!(l >= 0.0f)) continue;
            n++;
            if (l > t1) { t3 = t2; t2 = t1; t1 = l; }
            else if (l > t2) { t3 = t2; t2 = l; }
            else if (l > t3) t3 = l;
        }
    }
    if (n < plan.rank) return r;
    r.considered = true;
    const float L = plan.rank == 1 ? t1 : (plan.rank == 2 ? t2 : t3);
    const float limit = vptfp::max_(plan.threshold * L, plan.floor);
    const float l_p = staged_luminance(c_p, albedo_p, depth_p, plan.demodulate != 0);
    if (l_p > limit) {
        const float s = limit / l_p;
        r.pixel = denoise::f4(c_p.x * s, c_p.y * s, c_p.z * s, c_p.w);
        r.clamped = true;
    }
    return r;
}

}  // namespace firefly
}  // namespace vpt
