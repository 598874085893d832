// Host driver of the parts of a whole-path batch (vulkan-path-tracer_amd/csrc/path_plan.hpp: Parts, split_parts, Schedule::parts as decide() fills
// it) for tests/test_whole_parts_cpu.py.  Two uses of one file:
//  * a shared library driven through ctypes: wp_run walks a table of cases, one row of uint32 per case, and writes one row of results per case;
//  * a stand-alone program (main): walks the same axes itself and checks the shape of every answer — what the test builds with
//    -fsanitize=address,undefined, so that the arithmetic runs under the sanitizers without a Python process around it.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "path_plan.hpp"

using namespace vpt::plan;

namespace {
// A context whose scene rides in LDS, with buffers that hold the batch.
Schedule decide_case(uint32_t pipeline, uint32_t split, bool capturing, bool on_lane, uint32_t forced, uint32_t frames, uint32_t shard_pixels, uint32_t n_slots, bool plain) {
    Facts f;
    f.pipeline = pipeline; f.has_scene = true; f.lds_scene = true; f.whole_grid = true; f.split = split; f.max_depth = 8;
    f.whole_parts = forced; f.whole_plain = plain; f.shard_pixels = shard_pixels;
    return decide(f, frames, frames, frames, n_slots, on_lane, capturing);
}
// first[0] == 0 < first[1] < ... < first[n] == frames, 1 <= n <= kMaxParts, nothing behind first[n]
bool well_formed(const Parts& p, uint32_t frames) {
    if (p.n < 1u || p.n > kMaxParts || p.first[0] != 0u || p.first[p.n] != frames) return false;
    for (uint32_t i = 0; i < p.n; i++) if (p.first[i + 1] <= p.first[i]) return false;
    return true;
}
}  // namespace

extern "C" {
enum { kIn = 9, kOut = 3 + kMaxParts + 1 };
uint32_t wp_in_columns() { return kIn; }
uint32_t wp_out_columns() { return kOut; }
// 0: kMaxParts, 1: kPartsCount, 2: kPartsRatio, 3 / 4: low / high word of kPartsMinSamples
uint32_t wp_constant(uint32_t which) {
    return which == 0 ? kMaxParts : which == 1 ? kPartsCount : which == 2 ? kPartsRatio : which == 3 ? (uint32_t)kPartsMinSamples : (uint32_t)(kPartsMinSamples >> 32);
}
// in:  pipeline, split, capturing, on_lane, forced parts, frames, shard_pixels, n_slots, whole_plain
// out: err, kind, parts.n, parts.first[0 .. kMaxParts]
void wp_run(uint64_t cases, const uint32_t* in, uint32_t* out) {
    for (uint64_t i = 0; i < cases; i++, in += kIn, out += kOut) {
        const Schedule s = decide_case(in[0], in[1], in[2] != 0, in[3] != 0, in[4], in[5], in[6], in[7], in[8] != 0);
        out[0] = (uint32_t)s.err; out[1] = (uint32_t)s.kind; out[2] = s.parts.n;
        memcpy(out + 3, s.parts.first, sizeof(s.parts.first));
    }
}
}

int main() {
    const uint32_t pixels[] = {1u, 63u, 64u, 65u, 1850u, 2073600u, 259200u};
    const uint32_t pipelines[] = {VPT_PIPELINE_AUTO, VPT_PIPELINE_FUSED, VPT_PIPELINE_STAGED, VPT_PIPELINE_WHOLE};
    uint64_t cases = 0, split_cases = 0;
    for (uint32_t k = 0; k < 43u; k++) {
        const uint32_t frames = k < 40u ? k + 1u : k == 40u ? 904u : k == 41u ? 6912u : 8192u;
        for (uint32_t px : pixels) {
            if ((uint64_t)frames * px >= (1ull << 31)) continue;   // (batch_cap: a batch's slots fit 31 bits)
            for (uint32_t pipeline : pipelines)
                for (uint32_t split = 1; split <= 2u; split++)
                    for (uint32_t flags = 0; flags < 8u; flags++)
                        for (uint32_t forced = 0; forced <= kMaxParts; forced++) {
                            const uint32_t n_slots = split == 1u ? frames * px : frames * px / 4u;
                            const Schedule s = decide_case(pipeline, split, (flags & 1u) != 0, (flags & 2u) != 0, forced, frames, px, n_slots, (flags & 4u) != 0);
                            cases++;
                            if (s.err != VPT_OK) continue;
                            const bool may = s.kind == Kind::Whole && split == 1u && (flags & 3u) == 0u && (forced != 0u || (flags & 4u) != 0u);   // (the rule splits PLAIN scenes only)
                            bool ok = well_formed(s.parts, frames) && (may || s.parts.n == 1u);
                            if (may && forced != 0u) {
                                ok = ok && s.parts.n == (forced < frames ? forced : frames);
                                for (uint32_t i = 0; i < s.parts.n; i++) {
                                    const uint32_t len = s.parts.first[i + 1] - s.parts.first[i];
                                    ok = ok && (len == frames / s.parts.n || len == frames / s.parts.n + 1u);
                                }
                            }
                            if (!ok) { printf("bad parts: pipeline %u split %u flags %u forced %u frames %u pixels %u\n", pipeline, split, flags, forced, frames, px); return 1; }
                            split_cases += s.parts.n > 1u;
                        }
        }
    }
    // every ratio and count the -D overrides allow, on every batch length
    for (uint32_t frames = 1; frames <= 8192u; frames = frames < 64u ? frames + 1u : frames * 2u + 1u)
        for (uint32_t n = 1; n <= kMaxParts + 1u; n++)
            for (uint32_t ratio = 1; ratio <= 16u; ratio++) {
                cases++;
                if (!well_formed(split_parts(frames, n, ratio), frames)) { printf("bad parts: frames %u n %u ratio %u\n", frames, n, ratio); return 1; }
            }
    printf("%llu cases, %llu split\n", (unsigned long long)cases, (unsigned long long)split_cases);
    return split_cases != 0 ? 0 : 1;
}
