// kernels.hpp — host-callable launch wrappers of the HIP stages (definitions in kernels_*.hip).  The limits of the post chain's schedule (how many levels a
// tail or a chain takes, which base a tail stages) are not here: post_plan.hpp holds them once, with the plan that uses them.
#pragma once
#include "device_types.hpp"
#include "denoise.hpp"
#include "temporal.hpp"
#include "svgf_spatial.hpp"
#include "firefly.hpp"
#include "exposure.hpp"
#include "post_plan.hpp"
#include "whole_deal.hpp"   // + camera_cull.hpp
#include "../../include/vpt_lab.h"   // VPT_TRACE_* / VPT_LAB_* constants (the functions exist in the laboratory build only)
#ifndef VPT_LAB
#define VPT_LAB 0
#endif

namespace vpt {

void launch_bounce(hipStream_t s, uint32_t blocks, bool lds_scene, bool count, bool first, const DeviceScene& sc, const RenderParams& P,
                   const PathState& ps, const StreamState& ss, const uint32_t* queue, uint32_t* queue_next, Counters* ctr, uint32_t parity, uint32_t n_slots,
                   uint32_t dispatch_base, uint32_t k3, bool plain = false);
int bounce_blocks_per_cu(bool lds_scene, const DeviceScene& sc, bool plain = false);
void launch_whole(hipStream_t s, uint32_t blocks, bool count, const DeviceScene& sc, const RenderParams& P, const PathState& ps, Counters* ctr, uint32_t n_slots,
                  uint32_t dispatch_base, bool plain, uint32_t static_rounds, uint32_t chunk_tiles, cull::Packed rect, const deal::Deal& deal, uint64_t culled);   // rect "everything": n_slots slots; else n_slots launch indices over the rectangle, zeros for the other slots of deal.slots (whole_deal.hpp)
constexpr uint32_t kWholeNarrowOff = 1u << 9;   // in launch_whole's chunk_tiles, laboratory build only (VPT_LAB_NARROW_OFF): the launch flags no child word of its LDS tree, every node step is four-wide
int whole_blocks_per_cu(const DeviceScene& sc, bool plain);
// the rest of a streams batch in one launch (kernels_finish.hip k_finish): every path of queue[parity] run to its end
void launch_finish(hipStream_t s, uint32_t blocks, bool count, const DeviceScene& sc, const RenderParams& P, const PathState& ps, const StreamState& ss, const uint32_t* queue,
                   StreamCounters* sctr, Counters* ctr, uint32_t parity);
int finish_blocks_per_cu(const DeviceScene& sc);
void launch_resolve(hipStream_t s, const RenderParams& P, const PathState& ps, float* image, uint32_t frames, uint32_t frame_base, const uint32_t* guard);
// The first hit of a set of rays and what lies there (kernels_aux.hip k_first_hit), behind vpt_trace_rays, vpt_render_features and vpt_pick.  The rays are
// the caller's (rays != nullptr: n of them, hits[i] is all that is written) or the camera's: every pixel of the image in 8 x 8 tiles, or, with
// pick != nullptr, the one pixel `pixel` (y * width + x), whose outputs land at index 0.  All pointers are device memory; a null output is not written.
struct FirstHitArgs {
    const vpt_ray* rays; vpt_hit* hits; uint32_t n;
    uint32_t mode, frame;   // VPT_FEATURES_*; the dispatch whose sample 0 a VPT_FEATURES_SAMPLE ray is
    float* depth; uint4* ids; float4* normal; float4* albedo;   // vpt_feature_buffers
    float4* pick; uint32_t pixel;   // pick[0] = u, v, 0, 0; pick[1] = origin + t * direction, 0
};
void launch_first_hit(hipStream_t s, uint32_t blocks, const DeviceScene& sc, const RenderParams& P, const FirstHitArgs& a);
void launch_trace_rays(hipStream_t s, uint32_t blocks, const DeviceScene& sc, const vpt_ray* rays, uint32_t n, vpt_hit* hits);
// vpt_read_density_grid: out[i] = the value the samplers' lookup returns at voxel ijk[3i .. 3i + 2] of g (device pointers inside g, ijk and out on the device)
void launch_read_density_grid(hipStream_t s, const DensityGrid& g, const int32_t* ijk, uint32_t n, float* out);
void launch_scatter_rows(hipStream_t s, const float* gathered, float* full, uint32_t w, uint32_t h, uint32_t shard_count, uint32_t stride_px);
void launch_precompute_materials(hipStream_t s, const DeviceScene& sc, uint32_t flags, MatResolved* out, uint32_t n);
void launch_precompute_tri_ng(hipStream_t s, const DeviceScene& sc, float4* out);
void launch_precompute_tri_shade(hipStream_t s, const DeviceScene& sc, float4* out);
void launch_precompute_emissive(hipStream_t s, const DeviceScene& sc, EmissiveTri* out, uint32_t total);
// vpt_set_instance_transforms (kernels_aux.hip): the leaf-ordered triangles under new matrices for instances [first, first + count) into `out`, with
// words[0] raised if the sliver set would change and words[1] = bits of the scene extent; then one launch per height of the tree, lowest first
void launch_retransform_tris(hipStream_t s, const DeviceScene& sc, uint32_t total_tris, uint32_t n_inst, uint32_t first, uint32_t count, const float* xf, BvhTri* out, uint32_t* words);
void launch_refit_level(hipStream_t s, const DeviceScene& sc, const uint32_t* order, uint32_t begin, uint32_t end, const BvhTri* tris, float pad, float* boxes, BvhNode* nodes_out, BvhNodeWide* wide_out);
size_t traverse_lds_bytes(const DeviceScene& sc, bool lds_scene, int stack_rows);   // stack_rows: LDS entries per lane (traverse.hpp kStackDepth; k_whole: kWholeStackRows)
size_t stack_overflow_bytes(uint32_t blocks);  // per-thread spill region of the traversal stacks for a grid of `blocks`
// ... preset to a word no stack entry can be (a node index of 2.1e9; leaf codes are negative), so that what was spilled can be counted:
// *out += the words of region[0 .. words) that no longer hold it
constexpr int kSpillPatternByte = 0x7f;
constexpr uint32_t kSpillPattern = 0x7f7f7f7f;
void launch_count_spilled(hipStream_t s, const uint32_t* region, uint32_t words, unsigned long long* out);
#if VPT_LAB   // round 1's stage kernels (kernels_lab_r1.hip): laboratory build only
void launch_raygen(hipStream_t s, const RenderParams& P, const PathState& ps, uint32_t* queue, Counters* ctr, uint32_t n_slots, uint32_t dispatch_base);
void launch_prepare(hipStream_t s, Counters* ctr, uint32_t parity);
void launch_fold(hipStream_t s, Counters* ctr);
void launch_extend(hipStream_t s, uint32_t blocks, bool lds_scene, bool count, const DeviceScene& sc, const PathState& ps,
                   const uint32_t* queue, Counters* ctr, uint32_t parity);
void launch_shade(hipStream_t s, uint32_t blocks, const DeviceScene& sc, const RenderParams& P, const PathState& ps,
                  const uint32_t* queue, uint32_t* queue_next, uint32_t* cqueue, Counters* ctr, uint32_t parity);
void launch_connect(hipStream_t s, uint32_t blocks, bool lds_scene, bool count, const DeviceScene& sc, const RenderParams& P,
                    const PathState& ps, const uint32_t* cqueue, Counters* ctr, uint32_t parity);
int traverse_blocks_per_cu(bool lds_scene, const DeviceScene& sc);
int shade_blocks_per_cu();
#endif

// ray-stream traversal kernels (kernels_trace.hip)
struct TraceArgs {
    const float4* ro;       // origin.xyz | -
    const float4* rd;       // direction.xyz | -
    const uint32_t* order;  // optional: entry i of the stream is ray order[i]
    const uint32_t* valid;  // optional (with order == nullptr): entry i is a hole when valid[i] == 0xffffffff
    float4* hit;            // closest: t (< 0 miss), u, v | primitive; any-hit: x = 1 occluded / -1 clear
    uint32_t* hinst;        // closest: instance
    uint32_t n;
    const uint32_t* n_dev;  // optional: the stream length lives in device memory (a queue size word); overrides n
    uint32_t* head;         // work cursor for entries beyond the waves' static first 64 (zeroed before the launch)
    float tmin, tmax;
    uint32_t normalize_dir; // RayGen.slang:70 normalises the payload direction before tracing
    uint32_t store_gid;     // 1: the hit record's fourth word is the GLOBAL triangle id (what the shade stage wants), 0: PrimitiveIndex (lab, vpt_hit)
    uint32_t param;         // variant parameter (vote: idle lanes that trigger a fetch step; 0 = default)
    unsigned char* cls;     // closest-hit only, optional: per queue entry, the shade class of what the ray hit (kShade*; 0xff for a hole)
    uint32_t cull;          // closest-hit only: 1 = drop stale stack entries at the pop (vote.hpp pop_or_done_cull); hits are unchanged
    uint32_t one_tri;       // trace lab: 1 = ONE triangle per triangle step (round 3's step) instead of the product's up to two (vote.hpp vote_tri2_step_*); hits are unchanged
    uint32_t packed;        // trace lab: 1 = the node step's plane arithmetic in packed fp32 instructions (traverse.hpp node_entries_pk); hits are unchanged
};
void launch_trace(hipStream_t s, uint32_t blocks, uint32_t variant, bool any, bool count, const DeviceScene& sc, const TraceArgs& a, Counters* ctr);
int trace_blocks_per_cu(uint32_t variant, bool any);

// staged pipeline on compact streams (kernels_stream.hip)
void launch_stream_begin(hipStream_t s, StreamCounters* sc, uint32_t n_first, uint32_t n_total);
// path regeneration by refill: the room the ended paths left in the next ray queue is filled with the batch's next unstarted samples
void launch_refill(hipStream_t s, uint32_t blocks, const RenderParams& P, const PathState& ps, const StreamState& ss, uint32_t* queue_next, StreamCounters* sc, uint32_t parity_next,
                   uint32_t cap, uint32_t dispatch_base);
void launch_raygen_stream(hipStream_t s, const RenderParams& P, const PathState& ps, const StreamState& ss, uint32_t* queue, uint32_t n_slots, uint32_t dispatch_base, bool media);
void launch_prepare_stream(hipStream_t s, StreamCounters* sc, uint32_t parity);
void launch_classify(hipStream_t s, const uint32_t* queue, const unsigned char* cls, uint32_t* const* class_queue, StreamCounters* sc, uint32_t parity, uint32_t max_entries, uint32_t shade_waves);
void launch_layout_single(hipStream_t s, StreamCounters* sc, uint32_t parity, uint32_t shade_waves);
void launch_shade_stream(hipStream_t s, uint32_t blocks, uint32_t cls, bool sorted, const DeviceScene& sc, const RenderParams& P, const PathState& ps, const StreamState& ss,
                         const uint32_t* queue, const uint32_t* order, uint32_t* queue_next, Counters* ctr, StreamCounters* sctr, uint32_t parity);
void launch_classify_instances(hipStream_t s, const DeviceScene& sc, unsigned char* out, uint32_t n);
void launch_trace_shadow(hipStream_t s, uint32_t blocks, bool light, bool count, const DeviceScene& sc, const StreamState& ss, Counters* ctr,
                         StreamCounters* sctr, uint32_t param, uint32_t ray_queries = 1u);   // ray_queries: USE_RAY_QUERIES (RTCommon.slang:52 / :64)
void launch_join(hipStream_t s, uint32_t blocks, const RenderParams& P, const PathState& ps, const StreamState& ss, const StreamCounters* sctr, const uint32_t* queue,
                 const uint32_t* queue_next, uint32_t parity);
int shade_stream_blocks_per_cu();
int join_blocks_per_cu();
// participating media on the streams (kernels_media.hip)
void launch_media_scatter(hipStream_t s, uint32_t blocks, const DeviceScene& sc, const PathState& ps, const StreamState& ss, const MediaState& ms, const uint32_t* queue,
                          const StreamCounters* sctr, uint32_t parity);
void launch_layout_media(hipStream_t s, StreamCounters* sctr, uint32_t parity, uint32_t shade_waves, uint32_t tail_waves);
void launch_shade_media(hipStream_t s, uint32_t blocks, const DeviceScene& sc, const RenderParams& P, const PathState& ps, const StreamState& ss, const MediaState& ms,
                        const uint32_t* queue, Counters* ctr, StreamCounters* sctr, uint32_t parity);
void launch_media_tail(hipStream_t s, uint32_t blocks, const DeviceScene& sc, const RenderParams& P, const PathState& ps, const StreamState& ss, const MediaState& ms,
                       const uint32_t* queue, uint32_t* queue_next, Counters* ctr, StreamCounters* sctr, uint32_t parity);
int shade_media_blocks_per_cu();
int media_tail_blocks_per_cu();
int trace_shadow_blocks_per_cu();

// lookup-table generator (kernels_lut.hip)
void launch_lut(hipStream_t s, int kind, float* table, uint32_t sx, uint32_t sy, uint32_t sz, uint32_t sample_count, uint32_t time_hash,
                uint32_t first_dispatch, uint32_t n_dispatches);

// post-process chain (kernels_post.hip).  Which of these a vpt_postprocess launches, on which levels, is post_plan.hpp's decision; the wrappers that take
// (mips, m, first, n) serve one of its steps: mips = the context's mip pointers, m = their sizes, [first, first + n) = the step's levels
void launch_bloom_threshold(hipStream_t s, const float* in, float* out, uint32_t w, uint32_t h, float threshold, float falloff);
void launch_bloom_down(hipStream_t s, const float* in, uint32_t iw, uint32_t ih, float* out, uint32_t ow, uint32_t oh, float strength);
void launch_bloom_up(hipStream_t s, const float* in, uint32_t iw, uint32_t ih, float* out, uint32_t ow, uint32_t oh, float strength);
// mips[first .. first + n - 1] = successive down-samples of mips[first - 1], all written, one launch; n = 2 or 3
void launch_bloom_down_chain(hipStream_t s, float* const* mips, const post::Mips& m, uint32_t first, uint32_t n, float strength);
// mips[first .. first + n - 1] receive their up-samples in one launch (only mips[first] is written); mips[first + n] is read as it stands; n = 2 .. 4
void launch_bloom_up_chain(hipStream_t s, float* const* mips, const post::Mips& m, uint32_t first, uint32_t n, float strength);
// fused schedule: threshold inside the first down-sample, the small mips down and up in one launch, last up-sample + tonemap in one
void launch_bloom_down_first(hipStream_t s, const float* hdr, uint32_t iw, uint32_t ih, float* out, uint32_t ow, uint32_t oh, float strength, float threshold, float falloff);
// staged (the plan's choice, for a base mip small enough to be kept in LDS): mips[first .. first + n - 1] go down and up in LDS and mips[first], finished, is written —
// the up-sample into the base, mips[first - 1], is the caller's (the up chain's); otherwise (huge base) the base itself is updated and mips[first] is not written
void launch_bloom_tail(hipStream_t s, float* const* mips, const post::Mips& m, uint32_t first, uint32_t n, bool staged, float strength);
void launch_post_final(hipStream_t s, const float* hdr, const float* mip1, uint32_t mw, uint32_t mh, float* bloom0_out, uint8_t* out, uint32_t w, uint32_t h,
                       float threshold, float falloff, float strength, float exposure, float gamma, bool linear_tap, const float* scale = nullptr);
void launch_tonemap(hipStream_t s, const float* hdr, const float* bloom0, uint8_t* out, uint32_t w, uint32_t h, float exposure,
                    float gamma, bool linear_tap, const float* scale = nullptr);
// Auto-exposure (exposure.hpp holds the arithmetic).  scale (launch_tonemap, launch_post_final; device memory): nullptr — the multiply is c * exposure, the
// bits of a build without the option; otherwise c * (exposure * *scale), the product formed once.  What the two kernels below keep on the device:
struct ExposureDevice {
    exposure::State state;
    uint32_t hist[exposure::kBins];   // the latest metering's histogram (vpt_get_exposure_histogram)
    uint32_t acc[exposure::kBins];    // what k_luminance_histogram adds into: all zeros between two meterings (k_exposure_adapt leaves it so)
};
// acc[bin_of(pixel)] += 1 for the n RGBA32F pixels of img: a grid-stride pass of at most kHistMaxBlocks blocks of kHistThreads threads, two pixels per
// thread and trip — an image of more than 2 * kHistMaxBlocks * kHistThreads pixels takes a second trip
constexpr uint32_t kHistThreads = 1024, kHistMaxBlocks = 256;
void launch_luminance_histogram(hipStream_t s, const float* img, uint32_t n, const exposure::Plan& p, ExposureDevice* d);
// one wave: meter and adapt on acc, the state and a copy of acc written, acc zeroed (reset: exposure::kReset*)
void launch_exposure_adapt(hipStream_t s, const exposure::Plan& p, uint32_t reset, ExposureDevice* d);
// vpt_denoise (denoise.hpp holds the arithmetic).  prepare: e = the (demodulated) colour of c; `guide` holds the first-hit normal image on entry and the
// packed (n.xyz, t) on exit.  atrous: one pass in -> out at ps.step (steps 1 and 2 through an LDS tile, larger ones from memory); remodulate: the last pass
// of a demodulated run, which reads `albedo`.  All images RGBA32F of w x h but depth (one float per pixel).
// variance (the variance-guided passes; nullptr / false: off): prepare puts a hit's variance into e.w and its alpha into albedo.w; a pass then runs
// atrous_pixel_variance on taps from memory with sigma_luminance, and the `last` one returns the alpha.
void launch_denoise_prepare(hipStream_t s, const float* c, const float* depth, float* albedo, float* guide, float* e, uint32_t w, uint32_t h, bool demodulate, const float* variance);
void launch_denoise_atrous(hipStream_t s, const float* in, const float* guide, const float* albedo, float* out, uint32_t w, uint32_t h, const denoise::Pass& ps, bool remodulate,
                           bool variance, float sigma_luminance, bool last);
// vpt_temporal_accumulate (temporal.hpp holds the arithmetic): one launch over f.width x f.height.  cur, albedo, out: RGBA32F; depth: one float, ids: k_first_hit's
// uint4, per pixel.  The previous record (prev_*: never read when f.have_prev is 0) and the new one are (hist F4, guide F4, inst uint32) per pixel; `guide`
// holds the first-hit normal image on entry and the packed (n.xyz, t) on exit.  variance != nullptr: the luminance moments (two floats per pixel, previous
// and new) are carried too and the variance image (one float per pixel) is written; min_len = min_history * m.  motion_table != nullptr: motion_count
// records, one per instance — a hit pixel is reprojected through its instance's; motion != nullptr: the motion image (two floats per pixel) is written.
void launch_temporal(hipStream_t s, const float* cur, const float* depth, const float* albedo, const uint32_t* ids, const float* prev_hist, const float* prev_guide, const uint32_t* prev_inst,
                     float* hist, float* guide, uint32_t* inst, float* out, const temporal::Frame& f, const float* prev_moments, float* moments, float* variance, float min_len,
                     const temporal::InstanceMotion* motion_table, uint32_t motion_count, float* motion);
// vpt_svgf_spatial_options (svgf_spatial.hpp holds the arithmetic): one launch over w x h behind launch_temporal, on the record it has just written — guide
// (packed F4), moments (two floats) and hist (F4, whose .w is the length) per pixel.  `variance` is rewritten in place at the young hit pixels (length below
// min_len) and nowhere else; a block whose 64 x 4 tile holds none returns before it reads a neighbour.
void launch_variance_spatial(hipStream_t s, const float* guide, const float* moments, const float* hist, float* variance, uint32_t w, uint32_t h, const svgf_spatial::Plan& plan, float min_len);
// vpt_firefly_options (firefly.hpp holds the arithmetic): one launch over w x h AHEAD of launch_temporal / launch_denoise_prepare, which are then handed `out`
// for their image.  cur, albedo, out: RGBA32F; depth: one float per pixel — the consuming call's first-hit guides.  albedo == nullptr: the consuming call does
// not demodulate and nothing is read through it (plan.demodulate follows the pointer).  cur is never written.  counters: firefly::kCounterBytes of device memory, kCounterSlots pairs
// (clamped, considered) kCounterStride words apart, each block adding into one of them: the caller zeroes them ahead of the launch, on the same stream, and sums them.
void launch_firefly(hipStream_t s, const float* cur, const float* albedo, const float* depth, float* out, uint32_t* counters, uint32_t w, uint32_t h, const firefly::Plan& plan);

}  // namespace vpt
