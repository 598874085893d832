// path_plan.hpp — how many frames of SAMPLES and of resident PATHS a context's path buffers hold: the batch cap chosen for an image size
// (api_context.hip check_render_size), the longest batch of a schedule (batch_cap), the residency of a batch (resident_frames_for) and the
// plan by which the buffers grow (ensure_path_buffers).  Plain arithmetic on plain values and no HIP, so that the host test
// (tests/test_path_plan_cpu.py) walks the same code through sequences of batches against a modelled device memory.
// And HOW a batch runs (Facts -> Policy, decide, async_shape, media_supported): the one place that decides it; api_render.hip turns the
// decision into buffers and launches, tests/test_batch_schedule_cpu.py walks it over every reachable combination of its inputs.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/vpt.h"   // VPT_PIPELINE_* / VPT_BUILD_* / VPT_ERR_* / VPT_ASYNC_MAX_BOUNCES (plain C)

namespace vpt {
namespace plan {

constexpr uint64_t kBytesPerPath = 380;          // core slot records 68 + stream records ~290 (slack included) + queues 8 + image share
constexpr uint32_t kMaxFramesInFlight = 8192;   // frames of one batch.  A 1/8 shard of 1080p holds ~448M paths at 1728 frames and its default batch is four times that
                                                // (6912 frames = 1.79 G samples, what a whole 1080p image renders per batch at 904 frames): with round 5's bound of 2048 a rank of an 8-GPU
                                                // job rendered 3.5 x shorter batches than a 1-GPU job, i.e. bench.py's "weak" scaling did not keep the per-rank work fixed
constexpr uint64_t kResidentPaths = 448ull << 20;   // samples of a batch by default (see frames_for_size)
// What alloc_path_buffers allocates: per SAMPLE of a batch two float4 records and the anisotropy word (+4 B for the sample index with
// samples_per_frame > 1, +8 B with media), per RESIDENT path two queue words and the stream records (17 float4 + 6 B).
constexpr uint64_t kSampleBytes = 36, kResidentBytes = 8 + 17 * 16 + 6;

// The rest of a streams batch goes to k_finish (kernels_finish.hip) — one launch instead of seven per bounce —
//  * after kFinishAfterBounces (3) bounces when the batch is small from the start (a frame or two per call: its launches never fill the chip for long), and
//  * as soon as the host sees fewer than kFinishBelowPaths paths alive in a large one (the last of depth-32 paths: 20 bounce-sets on nearly empty queues).
#ifndef VPT_FINISH_AFTER   // (-D overrides: the A/B builds of tests/tools/ab_variants.sh)
#define VPT_FINISH_AFTER 3
#endif
#ifndef VPT_FINISH_BELOW
#define VPT_FINISH_BELOW (1u << 18)
#endif
constexpr uint32_t kFinishSmallBatchPaths = 6u << 20, kFinishAfterBounces = VPT_FINISH_AFTER, kFinishBelowPaths = VPT_FINISH_BELOW;

// A large whole-path batch runs as a few PARTS of consecutive frames, one launch of k_whole each, and the resolve of part i runs on the lane's
// second stream beside the launch of part i + 1: k_whole is bound by VALU issue and leaves the memory idle, the resolve is a pass over the
// part's frame sums at the memory roof and leaves the VALU idle, so only the last part's resolve stays exposed.  One more launch costs about
// 0.3 ms (ramp, drain of the rings, launch gap), the resolve about 2.7 ms per G samples:
//  * batches of at least kPartsMinSamples samples are split (the smallest size measured to gain: 226 frames of 1080p; 56 frames lose 2.4 %),
//  * on scenes that run k_whole's PLAIN instantiation only: three waves of the general one (168 registers) leave no room for a resolve wave (24) among a
//    SIMD's 512 registers, and the compact material scene ran 0.3-0.6 % slower split,
//  * into kPartsCount parts, each 1 / kPartsRatio as long as the one before (1: equal parts), so the exposed last resolve is short.
// Measured: profiles/r17_whole_resolve_overlap_ab.md.
#ifndef VPT_PARTS_MIN_SAMPLES   // (-D overrides, as above)
#define VPT_PARTS_MIN_SAMPLES (27ull << 24)
#endif
#ifndef VPT_PARTS_COUNT
#define VPT_PARTS_COUNT 3
#endif
#ifndef VPT_PARTS_RATIO
#define VPT_PARTS_RATIO 4
#endif
constexpr uint32_t kMaxParts = 8;
constexpr uint64_t kPartsMinSamples = VPT_PARTS_MIN_SAMPLES;
constexpr uint32_t kPartsCount = VPT_PARTS_COUNT, kPartsRatio = VPT_PARTS_RATIO;
static_assert(kPartsCount >= 1 && kPartsCount <= kMaxParts && kPartsRatio >= 1 && kPartsRatio <= 16, "parts of a whole-path batch");

// The parts of a batch: part i is frames [first[i], first[i + 1]) of it; ascending, none empty, first[0] == 0 and first[n] == frames.
struct Parts {
    uint32_t n = 1;
    uint32_t first[kMaxParts + 1] = {};
};
inline Parts one_part(uint32_t frames) { Parts p; p.first[1] = frames; return p; }
// `n` parts of `frames` frames, each 1 / ratio as long as the one before as far as whole frames allow (ratio 1: equal parts, the remainder goes
// to the first ones); min(n, frames) parts when the batch has fewer frames than that.
inline Parts split_parts(uint32_t frames, uint32_t n, uint32_t ratio) {
    n = std::max(1u, std::min(std::min(n, kMaxParts), frames));
    Parts p; p.n = n;
    uint64_t total = 0, w = 1, cum = 0;
    for (uint32_t i = 0; i < n; i++) { total += w; w *= ratio; }   // weights ratio^(n-1), ..., ratio, 1
    for (uint32_t i = 0; i < n; i++) {
        w /= ratio; cum += w;
        p.first[i + 1] = ratio == 1u ? (i + 1u) * (frames / n) + std::min(i + 1u, frames % n) : (uint32_t)((uint64_t)frames * cum / total);
    }
    for (uint32_t i = n - 1; i >= 1; i--) p.first[i] = std::min(p.first[i], frames - (n - i));   // none empty: room for the parts behind ...
    for (uint32_t i = 1; i < n; i++) p.first[i] = std::max(p.first[i], p.first[i - 1] + 1u);      // ... and a frame for each
    p.first[n] = frames;
    return p;
}

// What scene, parameters and configuration say, as plain values (api_context.hip facts_of).
struct Facts {
    uint32_t pipeline = VPT_PIPELINE_AUTO, build_flags = 0;   // vpt_config
    bool lab_build = false;          // the laboratory build (-DVPT_LAB=1): round 1's stage kernels exist
    bool has_scene = false;
    bool lds_scene = false;          // the scene's BVH rides in LDS (otherwise it lives in memory)
    bool whole_grid = false;         // ... and the whole-path kernel has a grid for it
    bool media = false;              // volumes or an atmosphere
    uint32_t samples_per_frame = 1, split = 1, max_depth = 0;
    bool depth_bounded = true;       // every path ends within max_depth * samples_per_frame bounces (api_scene.hip update_depth_bounded)
    uint32_t whole_frames_bound = 0xffffffffu;   // VPT_PIPELINE_AUTO runs batches of at most this many frames as ONE whole-path launch (VPT_LAB_WHOLE_FRAMES)
    bool whole_plain = false;        // ... which runs its PLAIN instantiation on this scene (counting aside): 158 registers, so that a resolve wave fits beside three of its waves per SIMD
    uint32_t whole_parts = 0;        // != 0: a whole-path batch runs as this many equal parts wherever it may be split at all (VPT_LAB_WHOLE_PARTS); 0: the rule of decide()
    bool profile = false, count_traversal = false;   // vpt_config: kernels are timed / visits counted, one kernel at a time
    uint32_t shard_pixels = 1;
    uint32_t cfg_frames = 0, cfg_resident = 0;   // vpt_config.frames_in_flight / .resident_frames
};

// What the scene, the parameters and the configuration allow: the part of the facts that sizes the path buffers.
struct Policy {
    bool has_scene = false;
    bool regen = false;          // paths are regenerated by refill (streams pipeline, no media, whole-frame dispatches)
    uint32_t whole_frames = 0;   // batches of up to this many frames run as whole-path launches (0: none)
    uint32_t cfg_frames = 0;     // vpt_config.frames_in_flight (0: the library chooses)
    uint32_t cfg_resident = 0;   // vpt_config.resident_frames
};

// What the context carries between calls.
struct State {
    uint64_t px = 1;                 // pixels of the shard
    uint32_t frames_in_flight = 1;   // F: the largest batch with every sample resident (or what the caller asked for)
    uint32_t frames_cap = 0;         // upper bound of F after an out-of-memory failure of a size the library chose itself
    uint32_t long_factor = 4;        // batch_cap(): contexts that keep only part (or none) of a batch's paths resident take batches this many times F
    uint32_t frames_alloc = 0;       // frames of samples the buffers hold now
    uint32_t resident_alloc = 0;     // frames of paths the queues and stream records hold (<= frames_alloc)
};

// Device bytes of buffers holding `frames` frames of samples of which `resident` frames of paths are resident (plain batches).
inline uint64_t plan_bytes(uint64_t px, uint64_t frames, uint64_t resident) { return px * (frames * kSampleBytes + resident * kResidentBytes); }

// F for an image shard of `px` pixels: vpt_config.frames_in_flight, or ~448M resident paths whatever the shard size (226 frames at 1080p;
// kBytesPerPath x 448M = ~170 GB of the 288 GB, and never more than 60 % of the memory that is free right now): the last bounces of a batch
// are short launches that cannot fill 256 CUs, and a larger batch makes them longer for the same fixed cost.  Msamples/s from 32M to 128M
// paths: Cornell +8 %, atrium +16 %, glass bust (depth 32) +78 %; 128M to 256M: +0 / +2 / +18 %; 256M to 512M: +0 / +2.4 / +9.1 %
// (profiles/r03_frames_sweep.json).  This is the CAP of a batch; the buffers hold what has actually been asked for (grow).
inline uint64_t frames_for_size(uint32_t cfg_frames, uint64_t px, bool free_known, uint64_t free_bytes) {
    uint64_t F = cfg_frames;
    if (F == 0) {
        uint64_t paths = kResidentPaths;
        if (free_known) paths = std::min<uint64_t>(paths, (uint64_t)(free_bytes * 0.6) / kBytesPerPath);
        F = paths / px;
    }
    return std::max<uint64_t>(1, std::min<uint64_t>(F, kMaxFramesInFlight));
}

inline bool whole_policy(const Policy& p, uint32_t frames) { return frames <= p.whole_frames; }

// Frames of paths a batch of `frames` frames keeps resident.  Whole-path launches keep their paths in registers (one frame of records
// stays: what a per-bounce batch of one frame would need).  Without regeneration every sample is resident.  Default schedule of a context that
// regenerates (profiles/r05_frames_sweep.json, 1080p): batches of 4 x F frames with F / 2 frames of paths resident — 904 / 113 frames:
// 126 GB instead of 142 GB for 226 / 226.  vpt_config.resident_frames != 0: as asked (a value >= the batch keeps every sample resident);
// an explicit batch size without an explicit residency keeps every sample resident.
inline uint32_t resident_frames_for(const Policy& p, uint32_t F, uint32_t frames) {
    if (whole_policy(p, frames)) return 1u;
    if (!p.regen) return frames;
    uint64_t k = p.cfg_resident;
    if (k == 0) k = p.cfg_frames != 0 ? frames : std::max(1u, F / 2u);
    return (uint32_t)std::min<uint64_t>(frames, k);
}

// Do the buffers hold a batch of `frames` frames as they are?
inline bool holds(const Policy& p, const State& s, uint32_t frames) {
    return frames <= s.frames_alloc && resident_frames_for(p, s.frames_in_flight, frames) <= s.resident_alloc;
}

// The largest batch the context renders at once.  F is what fits with EVERY sample resident (or what the caller asked for).  A context
// whose batches keep only part of their paths resident (regeneration: 36 B per sample + ~290 B per resident path) or none (whole-path
// launches) takes batches long_factor (4) times as long, as far as they need no more memory than F frames with every sample resident
// (which binds only at F == 1).
inline uint32_t batch_cap(const Policy& p, const State& s) {
    const uint32_t F = s.frames_in_flight;
    if (p.cfg_frames != 0 || p.cfg_resident != 0 || !p.has_scene) return F;
    const uint64_t by_slots = ((1ull << 31) - 1ull) / std::max<uint64_t>(1, s.px);
    uint32_t cap = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>((uint64_t)F * s.long_factor, kMaxFramesInFlight), by_slots));
    if (!p.regen && !whole_policy(p, cap)) return F;
    const uint64_t budget = (uint64_t)F * (kSampleBytes + kResidentBytes), res = resident_frames_for(p, F, cap);
    if ((uint64_t)cap * kSampleBytes + res * kResidentBytes > budget) cap = (uint32_t)std::max<uint64_t>(F, (budget - std::min(budget, res * kResidentBytes)) / kSampleBytes);
    return cap;
}

// What a batch of up to `left` frames takes once the buffers have been grown for min(left, batch_cap): no more than they hold, and without
// regeneration or whole-path launches no more than their resident frames.
inline uint32_t fit_batch(const Policy& p, const State& s, uint32_t n) {
    n = std::min(n, s.frames_alloc);   // (a size the library chose itself may have been halved)
    if (!p.regen && !whole_policy(p, n)) n = std::min(n, s.resident_alloc);
    return n;
}

enum AllocResult { kAllocOk = 0, kAllocOutOfMemory = 1, kAllocFailed = 2 };
struct Grown {
    int result;                 // kAllocOk: (frames, resident) are allocated; otherwise the last allocation's result, and the caller restores (frames, resident)
    uint32_t frames, resident;
};

// Grows the buffers so that a batch of `want` frames (<= batch_cap) fits; alloc(frames, resident) replaces them and returns an AllocResult.
// A size the library chose itself (vpt_config.frames_in_flight == 0) is halved and tried again when the device runs out of memory after all
// (another process, fragmentation) — F then drops to what was obtained and the caller renders in smaller batches; an explicit size
// fails as it is and the context keeps the buffers it had.
//  * A long batch (beyond F) is sized for its own residency: keeping a larger old residency there would exceed the budget F was chosen for.
//  * A batch that keeps every sample resident does not carry the frames of an earlier long batch (whole-path launches or regeneration,
//    36 B per sample): at ~326 B per sample those would need up to 4 x the memory F was chosen for.  It gets the frames it asks for.
template <class Alloc>
Grown grow(const Policy& p, State& s, uint32_t want, Alloc&& alloc) {
    const uint32_t old = std::max(s.frames_alloc, 1u), old_res = std::max(s.resident_alloc, 1u);
    uint32_t tryf = std::max(want, old);
    if (tryf > s.frames_in_flight && resident_frames_for(p, s.frames_in_flight, tryf) == tryf) tryf = want;
    while (true) {
        const uint32_t F = s.frames_in_flight;
        const uint32_t keep_res = tryf > F ? resident_frames_for(p, F, tryf) : std::max(resident_frames_for(p, F, tryf), std::min(old_res, tryf));
        const int r = alloc(tryf, keep_res);
        if (r == kAllocOk) {
            s.frames_alloc = tryf; s.resident_alloc = keep_res;
            return Grown{kAllocOk, tryf, keep_res};
        }
        s.frames_alloc = 0; s.resident_alloc = 0;
        if (r != kAllocOutOfMemory || p.cfg_frames != 0 || tryf <= 1u) return Grown{r, old, old_res};
        if (tryf > F && s.long_factor > 1u) s.long_factor /= 2u;   // a long batch did not fit: shorter long batches from now on
        tryf = std::max(tryf / 2u, 1u);
        s.frames_cap = tryf;
        s.frames_in_flight = std::min(s.frames_in_flight, tryf);
    }
}

// ---- how a batch runs ---------------------------------------------------------------------------------------------------------

// Media (volumes / atmosphere) run in the fused per-bounce kernel, or on the streams when the BVH lives in memory: VPT_PIPELINE_AUTO and
// _FUSED, and _STAGED unless the scene rides in LDS.  (vpt_set_volumes / vpt_set_atmosphere may come before the scene: _STAGED passes then,
// and the batch is refused instead.)
inline bool media_supported(const Facts& f) {
    return f.pipeline <= VPT_PIPELINE_STAGED && !(f.pipeline == VPT_PIPELINE_STAGED && f.has_scene && f.lds_scene);
}

// ... on the streams (kernels_media.hip: the traversal then runs on the vote-scheduled kernels) when the BVH lives in memory, in the fused
// per-bounce kernel when it rides in LDS or when the fused pipeline is asked for.
inline bool media_on_streams(const Facts& f) {
    return f.media && !f.lds_scene && (f.pipeline == VPT_PIPELINE_AUTO || f.pipeline == VPT_PIPELINE_STAGED);
}

inline Policy policy_of(const Facts& f) {
    Policy p;
    p.has_scene = f.has_scene;
    // Paths are regenerated — the next ray queue refilled with fresh camera rays behind every shade stage, kernels_stream.hip k_refill_plan — on
    // the STREAMS pipeline (scenes whose BVH lives in memory, or the stream kernels asked for; no media, whole-frame dispatches).  Everything
    // else keeps every sample of a batch resident: the fused per-bounce kernels (scenes that ride in LDS run whole-path launches, which hold
    // no records at all; what is left for k_bounce — media, several samples per frame — is not worth a second mechanism), round 1's stage
    // kernels (records by slot), media batches (per-entry media streams), split-screen dispatches (launch indices map to pixels per dispatch).
    p.regen = f.has_scene && !f.media && f.split == 1u &&
              (f.pipeline == VPT_PIPELINE_STAGED || f.pipeline == VPT_PIPELINE_STAGED_SORTED || (f.pipeline == VPT_PIPELINE_AUTO && !f.lds_scene));
    // One launch per batch (kernels_whole.hip k_whole): the scene rides in LDS, no media, one sample per pixel and frame.
    // VPT_PIPELINE_WHOLE asks for it; AUTO takes it wherever it applies (whole_frames_bound bounds the batch size, for the A/B).
    const bool whole_possible = f.has_scene && f.lds_scene && f.whole_grid && !f.media && f.samples_per_frame == 1u;
    p.whole_frames = !whole_possible ? 0u : f.pipeline == VPT_PIPELINE_WHOLE ? 0xffffffffu : f.pipeline == VPT_PIPELINE_AUTO ? f.whole_frames_bound : 0u;
    p.cfg_frames = f.cfg_frames; p.cfg_resident = f.cfg_resident;
    return p;
}

enum class Kind : uint32_t {
    Whole,           // a launch of k_whole runs every path from its camera ray to its end (one per part of the batch: Schedule::parts)
    Fused,           // one kernel per bounce, bounce 0 included (k_bounce); media ride in it too
    Streams,         // extend -> shade (streams out) -> sky rays, light rays -> join on the vote-scheduled traversal kernels
    StreamsSorted,   // ... with the shade queue sorted by material class
    MediaStreams,    // the media variant of the streams (kernels_media.hip)
    StagedR1         // round 1's stage kernels (laboratory build)
};
inline bool runs_fused(Kind k) { return k == Kind::Whole || k == Kind::Fused; }   // (they share the counters: queue-size words rotated by the bounce kernels)
inline bool runs_streams(Kind k) { return k == Kind::Streams || k == Kind::StreamsSorted || k == Kind::MediaStreams; }

struct Schedule {
    Kind kind = Kind::Fused;
    bool regen = false;       // only `resident` frames of the batch's samples are in flight at a time; refills start the rest
    uint32_t resident = 0;    // frames of paths the batch keeps resident
    bool finisher = false;    // ONE launch of k_finish may run what is left of the batch to its end ...
    uint32_t finish_at = 0;   // ... and does once this many bounces have run (0: when the host sees few paths alive, if at all)
    bool overlap = false;     // the shadow-ray kernels and the join of bounce k run on the second stream, beside the extend of bounce k + 1
    Parts parts;              // Kind::Whole: one launch and one resolve per part, the resolve of part i on the second stream beside the launch of part i + 1
    int err = VPT_OK;         // != VPT_OK: the batch is refused with `msg`, and nothing else of the schedule means anything
    const char* msg = nullptr;
};

// How a batch of `frames` frames runs on buffers that hold `frames_alloc` frames of samples and `resident_alloc` frames of paths.  n_slots:
// the samples of the batch (frames * shard_pixels, less under split-screen dispatch).  on_lane: the batch runs on a lane of its context
// (api_ctx.hpp struct Lane: one of vpt_ctx::extra), capturing: it is being captured into a graph — one stream only either way.
inline Schedule decide(const Facts& f, uint32_t frames, uint32_t frames_alloc, uint32_t resident_alloc, uint32_t n_slots, bool on_lane, bool capturing) {
    const Policy p = policy_of(f);
    Schedule s;
    auto refuse = [&s](int err, const char* msg) { s.err = err; s.msg = msg; return s; };
    // path regeneration: only `resident` frames of the batch's samples are in flight; the room ended paths leave in the next ray queue is
    // refilled with the batch's next unstarted samples behind every shade stage, until they are used up
    const bool whole = whole_policy(p, frames) && frames <= frames_alloc;   // (keeps its paths in registers: no records, nothing to regenerate)
    s.resident = whole ? frames : std::min(frames, resident_alloc);
    s.parts = one_part(frames);
    s.regen = s.resident < frames;
    if (s.regen && !p.regen) return refuse(VPT_ERR_DEVICE, "internal: this batch needs all of its samples resident");
    // AUTO: fused for LDS-resident scenes, the stream pipeline otherwise (atrium 1150 vs 575, glass bust 2410 vs 1290, Cornell box with
    // the 960-triangle glass sphere 2880 vs 2600 Msamples/s: no scene measured prefers the fused kernel once its BVH lives in memory)
    const bool media_stream = media_on_streams(f);
    const bool fused = (f.media && !media_stream) || f.pipeline == VPT_PIPELINE_FUSED || (f.pipeline == VPT_PIPELINE_AUTO && f.lds_scene) || f.pipeline == VPT_PIPELINE_WHOLE;
    if (f.pipeline == VPT_PIPELINE_WHOLE && !whole)
        return refuse(VPT_ERR_UNSUPPORTED, "VPT_PIPELINE_WHOLE needs a scene whose BVH rides in LDS, no media, samples_per_frame == 1 and every sample of a batch resident");
    // (a scene that rides in LDS and is forced into the staged pipeline runs the stream kernels on its tree in memory; round 1's stage kernels: VPT_PIPELINE_STAGED_R1 only)
    const bool stream = !fused && f.pipeline != VPT_PIPELINE_STAGED_R1;
    if (f.media && !media_supported(f))   // (the setters let only _STAGED on a scene that rides in LDS come this far)
        return refuse(VPT_ERR_UNSUPPORTED, "media with VPT_PIPELINE_STAGED need a scene whose BVH lives in memory (this one rides in LDS: use VPT_PIPELINE_AUTO or _FUSED)");
    if (!fused && !stream && !f.lab_build) return refuse(VPT_ERR_UNSUPPORTED, "VPT_PIPELINE_STAGED_R1 needs the laboratory build");
    s.kind = whole ? Kind::Whole : fused ? Kind::Fused : !stream ? Kind::StagedR1 : media_stream ? Kind::MediaStreams :
             f.pipeline == VPT_PIPELINE_STAGED_SORTED ? Kind::StreamsSorted : Kind::Streams;
    // Two streams: the tail of one persistent traversal kernel is filled by the next one's first blocks.  Off while kernels are timed or
    // visits counted (one kernel at a time then), in the sorted and the media pipeline, and where the batch has one stream only.
    s.overlap = s.kind == Kind::Streams && !f.profile && !f.count_traversal && !capturing && !on_lane;   // (a lane's batch stays on its one stream: the lanes overlap each other)
    s.finisher = !(f.build_flags & VPT_BUILD_STREAMS_ONLY) && (s.kind == Kind::Streams || s.kind == Kind::StreamsSorted);
    if (s.finisher && !s.regen && n_slots <= kFinishSmallBatchPaths) s.finish_at = kFinishAfterBounces;
    // Parts need the second stream and launch indices that are frames of shard_pixels samples: not a captured batch, not a lane's, no split-screen
    // dispatch.  Timed and counted batches split like the others: bench.py divides the counters of an unprofiled run by the times of a profiled one.
    if (s.kind == Kind::Whole && f.split == 1u && !capturing && !on_lane) {
        if (f.whole_parts != 0u) s.parts = split_parts(frames, f.whole_parts, 1u);
        else if (f.whole_plain && n_slots >= kPartsMinSamples) s.parts = split_parts(frames, kPartsCount, kPartsRatio);   // (the general instantiation's 168 registers leave the resolve no room: nothing to gain, two launches to pay)
    }
    return s;
}

// What vpt_render_async makes of a decided batch of `nf` frames.
struct AsyncShape {
    bool fixed = false;                // a fixed schedule: every path has ended behind the launches enqueued, whatever the random numbers say
    uint32_t bounces_to_enqueue = 0;   // bounce 0 included
    bool lanes_ok = false;             // the batch may go to a lane
    bool graph_ok = false;             // ... may be replayed from a captured graph
    bool partial_grids = false;        // ... and its kernels take part of the persistent grid, beside the other lanes' frames
};
inline AsyncShape async_shape(const Facts& f, const Schedule& s, uint32_t nf, uint32_t resident_alloc, uint32_t graph_streak) {
    AsyncShape a;
    const uint64_t bounds = (uint64_t)f.max_depth * f.samples_per_frame;
    const bool whole = s.kind == Kind::Whole;   // ONE launch that runs every path to its end, whatever max_depth is
    const bool fused_auto = runs_fused(s.kind) && !f.media;
    const bool streams_pipe = s.kind == Kind::Streams || s.kind == Kind::StreamsSorted;
    // a small batch of the streams pipeline ends in ONE launch that runs every path to its end (k_finish): a fixed schedule whatever max_depth
    // is.  This is decide()'s finish_at rule with nf * shard_pixels where that one has n_slots: the two differ under split-screen dispatch (fewer
    // slots than pixels), where this one is the stricter — kept so: it sets how many launches such a batch enqueues.
    const bool stream_finish = streams_pipe && !(f.build_flags & VPT_BUILD_STREAMS_ONLY) && nf <= resident_alloc && (uint64_t)nf * f.shard_pixels <= kFinishSmallBatchPaths;
    a.fixed = whole || stream_finish || (f.depth_bounded && !f.media && bounds <= VPT_ASYNC_MAX_BOUNCES && nf <= resident_alloc);   // (a regenerating batch has no fixed length)
    a.bounces_to_enqueue = stream_finish ? kFinishAfterBounces + 1u : (uint32_t)std::min<uint64_t>(bounds, VPT_ASYNC_MAX_BOUNCES);
    const bool plain_launches = f.profile || f.count_traversal || f.split != 1u;
    // the streams pipeline's fixed batch (a frame per call on a scene whose BVH lives in memory: seven launches per bounce, every one of them
    // short) goes over the lanes and is replayed from a captured graph too — each lane's batch on ONE stream
    const bool stream_fixed = a.fixed && streams_pipe && s.kind != Kind::StreamsSorted;
    const bool replayable = a.fixed && (fused_auto || stream_fixed) && !plain_launches;
    a.lanes_ok = replayable && nf == 1u;
    a.graph_ok = replayable && graph_streak >= 2u;   // asked for again with nothing changed since the last two calls
    a.partial_grids = a.fixed && fused_auto && !plain_launches && nf == 1u && graph_streak >= 2u;
    return a;
}

}  // namespace plan
}  // namespace vpt
