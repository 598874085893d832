// exposure.hpp — the arithmetic of auto-exposure (vpt_set_exposure_options), once: a 256-bin histogram of the post source's log2 luminance, a trimmed mean
// of it, and an exposure that follows the mean from call to call.  Plain functions on plain values built from vptfp:: leaves only (log_, exp_, floor_,
// rint_, min_, max_, clamp_, isinf_), no context and no HIP call: kernels_post.hip's k_luminance_histogram calls bin_of per pixel and k_exposure_adapt calls
// take / finish / adapt, tests/tools/exposure_driver.cpp runs the same functions on the host (tests/test_exposure_cpu.py).  The histogram and every sum over
// it are INTEGERS, so the order pixels and bins are visited in cannot matter, and because the library is built without contraction and with correctly
// rounded division the device gives the host compile's bits (tests/test_gpu_exposure.py).
//
//   plan        formed once per call on the host from the options (plan_of): rcp_bin = 254 / (max_log2 - min_log2), lo_q16 = rint_(low_percentile 65536),
//               hi_q16 = rint_(high_percentile 65536), key_log2 = log_(key) (1 / ln 2).
//   bin_of      l = temporal::luminance(r, g, b) = (0.2126 r + 0.7152 g) + 0.0722 b; alpha is ignored.
//               !(l > 0) — zero, negative, NaN — is bin 0, the BLACK bin, which never takes part in the average: a black environment or miss pixels do
//               not drag the exposure.  isinf_(l) is bin 255.  Otherwise t = (log_(l) (1 / ln 2) - min_log2) rcp_bin: !(t >= 0) is bin 1, t >= 254 is
//               bin 255, else 1 + (int)floor_(t).  Bins 1 and 255 so hold everything below and above the range.
//   meter       N = sum hist[1..255] (64-bit).  N == 0: no target.  lo = (N lo_q16) >> 16, hi = min(max((N hi_q16) >> 16, lo + 1), N).  With c_b the count
//               in bins 1 .. b - 1, bin b contributes take_b = max(0, min(c_b + hist[b], hi) - max(c_b, lo)) of its pixels: W = sum take_b = hi - lo,
//               S = sum take_b b.  mean_bin = (float)((double)S / (double)W) — both exact in double —, avg_log2 = min_log2 + (mean_bin - 0.5) / rcp_bin,
//               target_log2 = clamp_(key_log2 - avg_log2 + compensation_log2, min_exposure_log2, max_exposure_log2).
//   adapt       reset (the first metering after enabling, or after vpt_exposure_reset) clears `valid`.  With a target: not valid -> cur = target, valid;
//               else a = target > cur ? rate_up : rate_down and cur = cur + (target - cur) a — where a is 1, cur is target itself, not the rounding of
//               the expression.  Without a target (N == 0) cur, target_log2 and avg_log2 stay as they are, and a state that is not valid has cur = 0 and
//               stays not valid: the next metering with a target jumps.  scale = exp_(cur ln 2).  Every metering counts in `meterings`.
#pragma once
#include <stdint.h>

#include "temporal.hpp"

namespace vpt {
namespace exposure {

constexpr int kBins = 256;
constexpr float kInvLn2 = 1.44269504088896341f, kLn2 = 0.693147180559945309f;

// vpt_exposure_options, field for field (api_post.hip asserts the sizes agree).
struct Options {
    uint32_t mode;
    float min_log2, max_log2, low_percentile, high_percentile, key, compensation_log2, min_exposure_log2, max_exposure_log2, rate_up, rate_down;
    uint32_t reserved;
};
// vpt_exposure_state, field for field: what k_exposure_adapt keeps on the device (followed there by the latest metering's histogram).
struct State {
    float scale, cur_log2, target_log2, avg_log2;
    uint32_t valid, meterings;
    uint64_t counted;
};
struct Plan {
    float min_log2, rcp_bin;
    uint32_t lo_q16, hi_q16;
    float key_log2, compensation_log2, min_exposure_log2, max_exposure_log2, rate_up, rate_down;
};
constexpr uint32_t kResetNone = 0u, kResetJump = 1u, kResetAll = 2u;   // adapt's `reset`: keep / clear `valid` (vpt_exposure_reset) / a state of zeros (mode has changed)

inline Options default_options() { return Options{0u, -10.0f, 6.0f, 0.5f, 0.95f, 0.18f, 0.0f, -8.0f, 8.0f, 0.1f, 0.25f, 0u}; }
inline bool finite_(float x) { return !vptfp::isnan_(x) && !vptfp::isinf_(x); }
// Every constraint of vpt_exposure_options (include/vpt.h); nullptr: the options are good.
inline const char* check_options(const Options& o) {
    const float f[10] = {o.min_log2, o.max_log2, o.low_percentile, o.high_percentile, o.key, o.compensation_log2, o.min_exposure_log2, o.max_exposure_log2, o.rate_up, o.rate_down};
    for (float v : f) if (!finite_(v)) return "every field must be finite";
    if (o.mode > 1u) return "mode must be 0 or 1";
    if (!(o.min_log2 < o.max_log2)) return "min_log2 must be < max_log2";
    if (!(o.low_percentile >= 0.0f && o.low_percentile < o.high_percentile && o.high_percentile <= 1.0f)) return "0 <= low_percentile < high_percentile <= 1 must hold";
    if (!(o.key > 0.0f)) return "key must be > 0";
    if (!(o.min_exposure_log2 <= o.max_exposure_log2)) return "min_exposure_log2 must be <= max_exposure_log2";
    if (!(o.rate_up > 0.0f && o.rate_up <= 1.0f && o.rate_down > 0.0f && o.rate_down <= 1.0f)) return "rate_up and rate_down must be in (0, 1]";
    if (o.reserved) return "reserved words must be 0";
    return nullptr;
}
inline Plan plan_of(const Options& o) {
    Plan p;
    p.min_log2 = o.min_log2;
    p.rcp_bin = 254.0f / (o.max_log2 - o.min_log2);
    p.lo_q16 = (uint32_t)vptfp::rint_(o.low_percentile * 65536.0f);
    p.hi_q16 = (uint32_t)vptfp::rint_(o.high_percentile * 65536.0f);
    p.key_log2 = vptfp::log_(o.key) * kInvLn2;
    p.compensation_log2 = o.compensation_log2;
    p.min_exposure_log2 = o.min_exposure_log2; p.max_exposure_log2 = o.max_exposure_log2;
    p.rate_up = o.rate_up; p.rate_down = o.rate_down;
    return p;
}

VPT_HD uint32_t bin_of(float r, float g, float b, float min_log2, float rcp_bin) {
    const float l = temporal::luminance(r, g, b);
    if (!(l > 0.0f)) return 0u;
    if (vptfp::isinf_(l)) return 255u;
    const float t = (vptfp::log_(l) * kInvLn2 - min_log2) * rcp_bin;
    if (!(t >= 0.0f)) return 1u;
    if (t >= 254.0f) return 255u;
    return 1u + (uint32_t)(int)vptfp::floor_(t);   // t in [0, 254): the conversion is exact and in range
}

VPT_HD uint64_t umin64(uint64_t a, uint64_t b) { return b < a ? b : a; }
VPT_HD uint64_t umax64(uint64_t a, uint64_t b) { return a < b ? b : a; }
struct Window { uint64_t lo, hi; };   // the pixels [lo, hi) of the N counted ones, in order of luminance, are averaged
VPT_HD Window window_of(uint64_t N, uint32_t lo_q16, uint32_t hi_q16) {
    Window w;
    w.lo = (N * lo_q16) >> 16;
    w.hi = umin64(umax64((N * hi_q16) >> 16, w.lo + 1u), N);
    return w;
}
// What a bin holding h pixels, with c pixels in the bins below it, contributes to the window.
VPT_HD uint64_t take(uint64_t c, uint32_t h, Window w) {
    const uint64_t a = umin64(c + h, w.hi), b = umax64(c, w.lo);
    return a > b ? a - b : 0u;
}
struct Metered { uint64_t N; uint32_t has_target; float avg_log2, target_log2; };
// From the sums to the target.  W = hi - lo > 0 wherever N > 0, but for a low_percentile so close to 1 that lo_q16 rounds to 65536 (lo = N): no target then.
VPT_HD Metered finish(uint64_t N, uint64_t S, uint64_t W, const Plan& p) {
    Metered m;
    m.N = N; m.has_target = (N != 0u && W != 0u) ? 1u : 0u; m.avg_log2 = 0.0f; m.target_log2 = 0.0f;
    if (!m.has_target) return m;
    const float mean_bin = (float)((double)S / (double)W);
    m.avg_log2 = p.min_log2 + (mean_bin - 0.5f) / p.rcp_bin;
    m.target_log2 = vptfp::clamp_(p.key_log2 - m.avg_log2 + p.compensation_log2, p.min_exposure_log2, p.max_exposure_log2);
    return m;
}
// meter, bin after bin (the host's form; k_exposure_adapt gives every lane four bins and scans — the sums are integers).
VPT_HD Metered meter(const uint32_t* hist, const Plan& p) {
    uint64_t N = 0;
    for (int b = 1; b < kBins; b++) N += hist[b];
    const Window w = window_of(N, p.lo_q16, p.hi_q16);
    uint64_t c = 0, S = 0, W = 0;
    for (int b = 1; b < kBins; b++) {
        const uint64_t t = take(c, hist[b], w);
        W += t; S += t * (uint64_t)b;
        c += hist[b];
    }
    return finish(N, S, W, p);
}
VPT_HD void adapt(State& s, const Metered& m, const Plan& p, uint32_t reset) {
    if (reset == kResetAll) { s.cur_log2 = 0.0f; s.target_log2 = 0.0f; s.avg_log2 = 0.0f; s.valid = 0u; s.meterings = 0u; }
    if (reset != kResetNone) s.valid = 0u;
    if (m.has_target) {
        const float target = m.target_log2;
        if (!s.valid) { s.cur_log2 = target; s.valid = 1u; }
        else {
            const float a = target > s.cur_log2 ? p.rate_up : p.rate_down;
            s.cur_log2 = a == 1.0f ? target : s.cur_log2 + (target - s.cur_log2) * a;
        }
        s.target_log2 = target; s.avg_log2 = m.avg_log2;
    } else if (!s.valid) {
        s.cur_log2 = 0.0f;
    }
    s.scale = vptfp::exp_(s.cur_log2 * kLn2);
    s.meterings += 1u;
    s.counted = m.N;
}

}  // namespace exposure
}  // namespace vpt
