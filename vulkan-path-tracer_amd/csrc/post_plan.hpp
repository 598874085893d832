// post_plan.hpp — which launches a vpt_postprocess makes: the sizes of the bloom mips a context allocates (mips_of) and, for a mip_count, the ordered
// steps of the two schedules (fused_plan, reference_plan).  The one place that decides it: api_post.hip's enqueue_post walks a plan and issues one launch per
// step, kernels_post.hip's wrappers fill their kernel arguments from a step's level range.  Plain arithmetic on plain values and no HIP, so that the host
// test (tests/test_post_plan_cpu.py through tests/tools/post_plan_driver.cpp) holds every step of it to tests/post_plan.py, the restatement in Python.
#pragma once
#include <algorithm>
#include <cstdint>

namespace vpt {
namespace post {

// ---- the constants of the plan (tests/post_plan.py parses them out of this file: each a plain `constexpr int|uint32_t NAME = <integer>;`)
constexpr uint32_t kMaxMips = 10;                     // PostProcessor.cpp:136-157 (MAX_BLOOM_LEVELS)
constexpr uint32_t kBloomTailMaxTexels = 2048;        // largest mip the one-launch tail (k_bloom_tail) keeps in LDS ...
constexpr uint32_t kBloomTailMaxLevels = 8;           // ... and the levels it can hold
constexpr int kTailMaxBase = 8448;                    // the tail's base mip is staged in LDS up to this many texels (k_bloom_tail<true>)
constexpr uint32_t kBloomDownChainTexels = 160000;    // 480 x 270 and below: smaller than what fills the chip for the length of a launch
constexpr uint32_t kBloomDownChainMax = 3;            // down-samples one k_bloom_down_chain launch makes (2 or 3)
constexpr uint32_t kBloomChainMax = 4;                // up-samples one k_bloom_up_chain launch makes

// The mips a context allocates for a w x h image: mip 0 is the image's size, each next one half the even part of the one before, down to 2 texels a side.
struct Mips {
    uint32_t count = 0;
    uint32_t w[kMaxMips] = {}, h[kMaxMips] = {};
    uint64_t texels(uint32_t i) const { return (uint64_t)w[i] * h[i]; }
};
inline Mips mips_of(uint32_t w, uint32_t h) {
    Mips m;
    while (m.count < kMaxMips) {
        m.w[m.count] = w; m.h[m.count] = h; m.count++;
        w = (w - w % 2u) / 2u; h = (h - h % 2u) / 2u;
        if (w < 2u || h < 2u) break;
    }
    return m;
}

// One launch.  Levels are mip indices, [first, first + count):
//   Threshold   mip 0 = the thresholded image                                      DownFirst   mip 1 from the image, the threshold inside
//   Down        mip `first` from mip first - 1                                     DownChain   `count` (2 or 3) successive down-samples of mip first - 1, all written
//   Tail        the levels go down and up in LDS.  staged: the base (mip first - 1) is read only and mip `first`, finished, is written; otherwise
//               (a base too large for LDS) the base itself is updated and mip `first` is not written
//   Up          mip first + 1 up-sampled into mip `first`                          UpChain     mips first .. first + count - 1 receive their up-samples, only
//                                                                                              mip `first` is written; mip first + count is read as it stands
//   Final       last up-sample + tonemap: count == 1, mip 1 is up-sampled into the image-sized mip 0 inside the launch; count == 0, there is no mip 1
//   Tonemap     the image and mip 0
enum Kind : uint8_t { kThreshold, kDownFirst, kDown, kDownChain, kTail, kUp, kUpChain, kFinal, kTonemap };
struct Step { uint8_t kind, first, count, staged; };

// The longest plan is the reference's: threshold, a down- and an up-sample per mip above 0, tonemap.  The fused one has a first down-sample, a tail and a
// final, and at most one launch per level 2 .. kMaxMips - 1 on either side of the tail.
constexpr uint32_t kMaxSteps = 2 * kMaxMips;
static_assert(1u + 2u * (kMaxMips - 1u) + 1u <= kMaxSteps && 3u + 2u * (kMaxMips - 2u) <= kMaxSteps, "Plan::steps holds the longest plan");
static_assert(kMaxMips <= 255u, "Step keeps a level in a byte");
struct Plan {
    uint32_t n = 0;
    Step steps[kMaxSteps] = {};
    void add(Kind kind, uint32_t first, uint32_t count, bool staged = false) { steps[n++] = Step{kind, (uint8_t)first, (uint8_t)count, (uint8_t)staged}; }
};

inline uint32_t clamp_mip_count(const Mips& m, uint32_t mip_count) { return std::max(1u, std::min(mip_count, m.count)); }

// PostProcessor.cpp:193-246 pass by pass: threshold, down x (n - 1), up x (n - 1), tonemap.
inline Plan reference_plan(const Mips& m, uint32_t mip_count) {
    const uint32_t mc = clamp_mip_count(m, mip_count);
    Plan p;
    p.add(kThreshold, 0, 1);
    for (uint32_t i = 1; i < mc; i++) p.add(kDown, i, 1);
    for (uint32_t i = mc - 1; i > 0; i--) p.add(kUp, i - 1, 1);
    p.add(kTonemap, 0, 1);
    return p;
}

// The tail starts at level 2 or above and the mips end at kMaxMips: it never has more levels than it can hold.
static_assert(kMaxMips - 2u <= kBloomTailMaxLevels, "the tail holds every level from 2 up");
static_assert(kBloomDownChainMax >= 2u && kBloomChainMax >= 2u, "a chain is at least two levels");

// The fused schedule, same values (kernels_post.hip): mip 0 is never materialised unless the caller asks the final launch for it.
inline Plan fused_plan(const Mips& m, uint32_t mip_count) {
    const uint32_t mc = clamp_mip_count(m, mip_count);
    Plan p;
    // T = first mip the one-launch tail keeps in LDS (<= kBloomTailMaxTexels texels, and >= 2: its base mip must exist in memory); mc: no tail
    uint32_t T = mc;
    for (uint32_t i = 2; i < mc; i++) if (m.texels(i) <= kBloomTailMaxTexels) { T = i; break; }
    if (mc >= 2u) p.add(kDownFirst, 1, 1);
    // down-samples between mip 1 and the tail's base: one launch each while the levels are large, the last (up to three, at most kBloomDownChainTexels
    // texels in the first of them) in one launch
    for (uint32_t i = 2; i < T;) {
        const uint32_t left = T - i;
        if (left >= 2u && left <= kBloomDownChainMax && m.texels(i) <= kBloomDownChainTexels) { p.add(kDownChain, i, left); i += left; }
        else { p.add(kDown, i, 1); i++; }
    }
    uint32_t up_from = T - 1u;   // the highest level that is final once the tail has run
    if (T < mc) {
        const bool staged = m.texels(T - 1u) <= (uint64_t)kTailMaxBase;
        p.add(kTail, T, mc - T, staged);
        if (staged) up_from = T;   // the staged tail leaves mip T finished in memory and mip T - 1 as the down-samples left it
    }
    // up-samples of the levels between the tail and mip 1: up to kBloomChainMax of them per launch
    for (uint32_t top = up_from; top > 1u;) {
        const uint32_t n = std::min(top - 1u, kBloomChainMax), base = top - n;
        p.add(n == 1u ? kUp : kUpChain, base, n);
        top = base;
    }
    p.add(kFinal, 0, mc >= 2u ? 1u : 0u);
    return p;
}

}  // namespace post
}  // namespace vpt
