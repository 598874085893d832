// api_ctx.hpp — what the host layer of the C-ABI (include/vpt.h) shares between its files: the context, its lanes and batches, and the helpers more
// than one api_*.hip calls.  Internal: no other file includes it.
//   api_context.hip  the context's life: create, size, configure, tear down; lanes, path buffers, the timing pool
//   api_scene.hip    what a batch only reads: scene installation and its partial updates
//   api_render.hip   a batch from decision to resolve; asynchronous batches, tickets, statistics
//   api_post.hip     the image passes behind a render: post-process (bloom, tonemap, RGBA8: one launch per step of post_plan.hpp's plan), denoise, temporal
//                    accumulation with SVGF's variance and instance motion
//   api_comm.hip     shards and gathers (the only file that sees RCCL)
//   api_lab.hip      the vpt_lab_* entry points (laboratory library only)
// None of them defines a __global__ function or launches one directly: the host layer calls the launch_* wrappers of kernels.hpp only.  That is
// what keeps these files free of a fat binary of their own (_build.link), which the product library's size bound has no room for.
// What these files decide is decided in headers that compile without HIP and are tested on the CPU — path_plan.hpp, scene_prep.hpp, camera_cull.hpp,
// post_plan.hpp, exposure.hpp, denoise.hpp, temporal.hpp (the last four through kernels.hpp) — the files here turn the decisions into buffers and launches.
// There is no CPU fallback in the host layer: without a HIP device vpt_create() fails.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "camera_cull.hpp"
#include "kernels.hpp"
#include "path_plan.hpp"
#include "scene_prep.hpp"   // scene::EmissiveList, a member of the context (the functions: api_scene.hip only)

using namespace vpt;

struct ncclComm;   // RCCL's communicator (ncclComm_t is a pointer to it): api_comm.hip alone includes rccl.h

// One wavefront batch in progress: what render_batch's stages hand to each other (and what an asynchronous batch leaves behind for
// the call that finishes it).
struct BatchState {
    uint32_t frames = 0, dispatch_base = 0, n_slots = 0;
    uint32_t n_first = 0;   // slots the camera-ray launch starts (n_slots, or the resident part of it when paths are regenerated)
    plan::Schedule sd;      // how it runs (path_plan.hpp decide); sd.finish_at is set late when the host sees few paths alive (batch_finish)
    int primary_grid = 0;   // grid of the fused / whole-path kernels: the context's, or the part of it a pipelined frame takes (vpt_render_async)
    int tail_grid = 0;      // > 0: grid of the fused bounces >= 2 (pipelined 1-frame batches)
    bool count = false;
    bool finished = false;  // k_finish has been enqueued: no bounce follows
    uint32_t parity = 0, k3 = 0;
    bool join_pending = false;
    uint64_t iter = 0, iter_cap = 0, min_bounces = 0;
};
// The fused / whole-path kernels' grids of one batch: the context's (`primary`, every bounce: tail == 0), or the part of it a pipelined frame takes.
struct Grids { int primary, tail; };
// Counter words a finished batch copies to pinned host memory (asynchronously, behind its resolve).
struct HostCounters {
    Counters ctr;
    uint32_t alive[2], queue_len[2];
    uint32_t refill_next;   // regenerating batches: samples started so far (StreamCounters::refill_next)
};
constexpr int kTickets = 16;
constexpr int kLanes = 3;

// What ONE batch in flight owns: streams, counters, path buffers, spill regions, its captured graph.  Everything a batch only reads — scene
// tables, parameters, grids, the accumulation image — is the context's and exists once.  The context renders on its main lane; pipelined
// 1-frame batches (vpt_ctx::extra) go over up to two more.
struct Lane {
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;             // staged pipeline: the shadow-ray kernels and the join of bounce k run here, beside the extend of bounce k + 1
    hipEvent_t ev_shade = nullptr, ev_join = nullptr;
    hipEvent_t ev_resolved = nullptr;          // recorded behind this lane's latest resolve
    Counters* ctr = nullptr;
    StreamCounters* sctr = nullptr;            // stream pipeline: lengths, exact live counts and work cursors, one cache line each
    HostCounters* h_ctr = nullptr;             // pinned
    uint32_t* d_dispatch_base = nullptr;       // graph replays read the batch's first dispatch index from here (RenderParams::dispatch_base_dev)
    uint32_t* spill = nullptr;                 // spill region of the traversal kernels (DeviceScene::stack_overflow of this lane's launches: lane_scene)
    uint32_t* spill2 = nullptr;                // ... of those launched on stream2; == spill in a lane whose batches stay on one stream
    uint32_t stack_overflow_words = 0;         // words per spill region

    uint32_t frames_alloc = 0;   // frames of SAMPLES the slot-addressed buffers hold now: they grow to the largest batch actually requested (ensure_path_buffers)
    uint32_t resident_alloc = 0; // frames of PATHS the queues and stream records hold (<= frames_alloc; less when paths are regenerated)
    bool ps_has_sidx = false, ps_has_media = false;   // the per-sample words only some batches touch are allocated only for them: sample index (samples_per_frame > 1), VolumeDepth / ColorChannel (media)
    uint32_t stream_slack = 0;   // entries a stream may hold beyond its true count: unwritten chunk tails (vote.hpp WaveAppender)
    void* ps_block = nullptr;    // slot-addressed records every pipeline uses (L, ACC, M + the dword arrays)
    PathState ps{};
    uint32_t* queue[2] = {nullptr, nullptr};
    void* ss_block = nullptr;    // stream records of the staged pipeline (kernels_stream.hip)
    StreamState ss{};
    // (only the main lane ever fills these)
    void* ps_legacy = nullptr;   // round 1's stage kernels only (A, B, T, H, C*, hinst): allocated on their first use
    uint32_t* cqueue = nullptr;  // connect queue (two-ended)
    uint32_t* class_queue[kShadeClasses] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // the shade queue sorted by class
    unsigned char* cls_q = nullptr;          // shade class per ray-queue entry, written by the extend stage
    void* media_block = nullptr; // streams of the media variant of the staged pipeline (kernels_media.hip): allocated on first use
    MediaState ms{};
    uint32_t media_frames = 0;   // frames a media batch on the streams can hold (ensure_media_buffers)

    hipGraphExec_t graph = nullptr;  // the fixed batch captured on this lane; current while graph_gen == vpt_ctx::state_gen
    uint64_t graph_gen = 0;
    uint32_t graph_frames = 0, graph_bounces = 0;
    uint64_t graph_kernel_launches[VPT_KERNEL_COUNT] = {};
    bool graph_broken = false;       // a capture failed once on this lane: stay on plain launches
    BatchState graph_batch;          // the captured batch as it stands before its resolve
    BatchState last_fixed;           // the latest fixed-schedule batch enqueued on this lane (drain checks that nothing outlived it)
    bool last_fixed_valid = false;
};

struct vpt_ctx {
    vpt_config cfg{};
    std::string err;
    int cu_count = 256;

    // host copies (SetMaterial / emissive list maintenance / stats)
    bool has_scene = false;
    bool buffers_ok = false;     // render buffers allocated for the current size (false after a failed vpt_resize)
    uint32_t texture_count = 0;  // of the current scene: vpt_set_material validates texture indices against it
    ncclComm* comm = nullptr;    // vpt_comm_init: one rank per process (an ncclComm_t)
    int comm_rank = -1, comm_world = 0;
    float* gather_buf = nullptr; // root: shard_count padded shards back to back
    // trace lab (vpt_lab_*): a resident ray set
    float4 *lab_ro = nullptr, *lab_rd = nullptr, *lab_hit = nullptr;
    uint32_t *lab_hinst = nullptr, *lab_order = nullptr;
    uint32_t lab_n = 0; float lab_tmin = 0.0f, lab_tmax = 0.0f;
#if VPT_LAB
    std::vector<unsigned char> lab_holes;   // vpt_lab_set_holes: empty, or lab_n bytes; the device's copy (TraceArgs::valid) is the second half of lab_order
#endif
    std::vector<vpt_material> materials;
    std::vector<MeshDesc> meshes;
    std::vector<InstanceDesc> instances;
    scene::EmissiveList emissive;
    uint64_t total_vertices = 0, total_indices = 0;
    uint32_t bvh_depth = 0;
    uint32_t total_tris = 0;                // global triangle ids of the scene, slivers included
    std::vector<uint32_t> refit_level_off;  // heights of the tree: nodes refit_order[off[h] .. off[h + 1]) have height h (bvh_refit.hpp levels)
    const uint32_t* refit_order = nullptr;  // on the device, freed with the scene
    bool lab_trees_stale = false;           // instances have moved since vpt_set_scene: bvh_input is gone and the trace lab's lazily built trees cannot be made

    DeviceScene dsc{};
    std::vector<void*> scene_allocs;
    // The scene tables the host patches or the precompute kernels fill after the upload: the writable pointer to each (DeviceScene's are
    // const), set together with DeviceScene's by alloc_table and nowhere else.
    struct Writable {
        vpt_material* materials = nullptr;
        EmissiveDesc* emissive = nullptr;
        MatResolved* mat_resolved = nullptr;
        EmissiveTri* emissive_tri = nullptr;
        uint32_t* emissive_tri_offset = nullptr;
        float4* tri_ng = nullptr;
        float4* tri_shade = nullptr;
        unsigned char* inst_class = nullptr;   // shade class per instance (kernels_aux.hip k_classify_instances)
    } dw;
    std::vector<BvhTri> bvh_input;          // the triangles the BVH was built from (trace lab: the eight-wide tree is built from them on first use)
    bool lds_scene = false;
    bool scene_plain = false;    // every material's five textures are 1x1 and the environment is black: the fused kernel's PLAIN instantiation serves it
    std::vector<unsigned char> tex_1x1;   // per texture of the scene
    bool sbvh = false;
    int trav_blocks = 1024;

    vpt_params params{};
    RenderParams P{};
    uint32_t frames_in_flight = 1;   // largest batch the context will render at once (the cap; vpt_config.frames_in_flight)
    uint32_t frames_cap = 0;     // upper bound of frames_in_flight after an out-of-memory failure of a size the library chose itself
    uint32_t long_factor = 4;    // batch_cap(): contexts that keep only part (or none) of a batch's paths resident take batches this many times frames_in_flight
    int whole_blocks = 0;        // persistent grid of the whole-path kernel (kernels_whole.hip k_whole), 0: the scene does not ride in LDS
    uint32_t lab_whole_sched = 4u;   // how k_whole's waves get their tiles (VPT_LAB_WHOLE_SCHED): tiles per atomic | static-rounds mode << 4
    uint32_t lab_whole_frames = 0xffffffffu;   // VPT_PIPELINE_AUTO runs batches of at most this many frames as ONE whole-path launch (VPT_LAB_WHOLE_FRAMES); default: every batch
                                               // (Cornell box 1080p, Msamples/s whole vs per-bounce at 1 / 4 / 16 / 64 / 226 frames per batch: 3821 / 6413 / 7737 / 8183 / 8315 vs
                                               // 2401 / 4753 / 6493 / 7244 / 7359; general instantiation 8840 vs 7713: profiles/r04_whole_ab.json)
    uint32_t lab_whole_parts = 0;    // != 0: whole-path batches run as this many equal parts (VPT_LAB_WHOLE_PARTS); 0: path_plan.hpp's rule
    // The scene's box as the device tree holds it — the union of the root's used child boxes in nodes_wide — from vpt_set_scene, and from the refitted
    // root after vpt_set_instance_transforms: what camera_cull.hpp bounds on the screen for every whole-path batch (whole_cull_rect).
    cull::WorldBox whole_box{};
    bool lab_whole_cull = true;      // false: whole-path batches skip no sample (VPT_LAB_WHOLE_CULL 0)
    bool lab_narrow_off = false;     // true: whole-path launches flag no child word, every node step is four-wide (VPT_LAB_NARROW_OFF 1)
    bool depth_bounded = true;   // every path ends within max_depth * samples_per_frame bounces (no material scatters inside a medium): see vpt_render_async
    // asynchronous batches (vpt_render_async / vpt_postprocess_device / vpt_wait)
    hipEvent_t tick_ev[kTickets] = {};
    uint64_t tick_issued = 0;
    bool async_dirty = false;        // work has been enqueued without a host synchronisation behind it
    bool out_active = false;         // an enqueued batch whose paths may outlive the bounces enqueued so far: the next call finishes it
    BatchState out_batch;
    uint64_t out_ticket = 0;
    uint64_t state_gen = 1;          // bumped by everything a captured batch bakes in (scene tables' addresses, params, camera, grids)
    uint32_t graph_streak = 0;       // asynchronous batches asked for since state_gen last changed
    uint64_t graph_streak_gen = 0;
    // Pipelined 1-frame batches (vpt_render_async): a frame of the fused fixed schedule is a chain of ~9 dependent launches, each bounded
    // below by the latency of one bounce (~60-90 us on nearly empty queues), so one frame at a time leaves most of the chip idle
    // (profiles/r04_latency_probe.json: 0.95 ms of kernels per 1080p frame against 0.33 ms per frame in 16-frame batches).  Consecutive
    // frames are independent until their resolve, so they go round-robin over kLanes lanes — the main one and kLanes - 1 more, created on
    // first use with a stream, counters, 1-frame path buffers and a spill region of their own (struct Lane) — and only the resolves are
    // ordered (frame k's waits for frame k - 1's: the running mean is applied in frame order).
    Lane main;
    Lane* extra[kLanes - 1] = {};
    Lane* lane(int k) { return k == 0 ? &main : extra[k - 1]; }   // lane k, nullptr: not created yet
    Lane* order_lane = nullptr;      // the lane the latest resolve was enqueued on (nullptr: nothing pipelined since the last drain)
    hipEvent_t ev_post = nullptr;    // recorded behind the latest vpt_postprocess_device — the next frame's resolve must not touch the image before
    bool post_pending = false;
    uint32_t lane_rr = 0;
    // vpt_lab_set; defaults = what tests/tools/latency_probe.py measured best (profiles/r04_latency_probe.json): a frame goes to the first
    // lane whose previous frame has been resolved (so a host with two frames in flight alternates between two lanes, one with three
    // uses all three), every lane launches the full persistent grid, and the bounces >= 2 of a 1-frame batch — queues of a quarter of
    // the frame's paths and less — a third of it, which leaves room for the other lanes' blocks
    uint32_t lab_lanes = 3, lab_lane_grid = 1, lab_tail_grid = 3;
    unsigned long long* d_spill_count = nullptr;
    bool spill_dirty = true;         // traversal kernels have run since the spill regions were last counted (vpt_get_stats counts lazily)
    uint64_t spill_cached[2] = {0, 0};
    double set_scene_ms = 0.0, bvh_build_ms = 0.0, set_environment_ms = 0.0, set_transforms_ms = 0.0;

    int shade_media_blocks = 768, media_tail_blocks = 768;
    uint32_t class_present = 0x1fu;   // shade classes some instance of the scene belongs to (bit kShadeMiss always set): the others get no launch
    int shade_stream_blocks = 768, shadow_blocks = 2048, finish_blocks = 768;
    std::vector<vpt_volume> volumes;       // homogeneous box volumes (vpt_set_volumes)
    vpt_volume* d_volumes = nullptr;
    std::vector<DensityGrid> grids;        // device pointers inside (vpt_add_density_grid)
    DensityGrid* d_grids = nullptr;
    uint32_t phase = VPT_PHASE_HENYEY_GREENSTEIN;
    uint32_t* d_launch_off = nullptr;  // split-screen: launch-grid prefix sums of the dispatches of a batch
    int shade_blocks = 1024, primary_blocks = 768, max_blocks = 1536, join_blocks = 2048;
    int primary_blocks_general = 768, primary_blocks_plain = 768;   // grids of the fused kernel's two instantiations (primary_blocks = the one scene_plain picks)
    int vote_blocks = 2048;   // persistent grid of the vote-scheduled traversal kernels
    uint32_t vote_param = 256u + 16u;  // weighted vote, fetch step at 16 idle lanes (profiles/r02_trace_lab_*.json)
    float* image = nullptr;       // this shard's rows, RGBA32F
    float* full_image = nullptr;  // whole image when shard_count > 1 (after vpt_assemble_shards)
    bool full_valid = false;

    uint64_t dispatch_count = 0;
    uint32_t frame_count = 0, samples_accum = 0;
    vpt_stats stats{};

    // post: the bloom mips of post_w x post_h — their sizes as post_plan.hpp's mips_of gives them, one allocation each
    std::vector<float*> mips;
    post::Mips mip_dims;
    uint8_t* post_out = nullptr;
    uint32_t post_w = 0, post_h = 0;
    // denoise (api_post.hip): allocated on the first vpt_denoise*, freed with the render buffers (vpt_resize, vpt_destroy)
    float* dn_block = nullptr;       // one allocation: guide (normal, then packed) | albedo | ping | pong | out | depth
    float *dn_guide = nullptr, *dn_albedo = nullptr, *dn_depth = nullptr, *dn_ping = nullptr, *dn_pong = nullptr, *dn_out = nullptr;
    uint32_t dn_w = 0, dn_h = 0;     // size the block was made for
    bool dn_valid = false;           // dn_out holds a denoised image of dn_w x dn_h
    uint32_t post_source = VPT_POST_SOURCE_RADIANCE;
    // temporal accumulation (api_post.hip): allocated on the first vpt_temporal_accumulate*, freed with the render buffers (vpt_resize, vpt_destroy)
    float* tp_block = nullptr;       // one allocation: out | hist[0] | hist[1] | guide[0] | guide[1] | albedo | ids | depth | inst[0] | inst[1]
    float *tp_out = nullptr, *tp_hist[2] = {nullptr, nullptr}, *tp_guide[2] = {nullptr, nullptr}, *tp_albedo = nullptr, *tp_depth = nullptr;
    uint32_t *tp_ids = nullptr, *tp_inst[2] = {nullptr, nullptr};
    uint32_t tp_w = 0, tp_h = 0;     // size the block was made for
    uint32_t tp_latest = 0;          // which of the two records the latest call wrote
    bool tp_valid = false;           // tp_out and record tp_latest hold a result of tp_w x tp_h
    bool tp_history = false;         // ... and the next call may reproject it (dropped by everything that changes what a pixel means: reset_accum)
    temporal::PrevCamera tp_camera{};   // the camera record tp_latest was made with
    uint32_t denoise_source = VPT_DENOISE_SOURCE_RADIANCE;
    // SVGF's variance (vpt_set_svgf_options): allocated on the first temporal call with the option on, for the size of tp_block, and freed wherever tp_block is
    vpt_svgf_options svgf{0u, 4.0f, 4u, 0u};
    float* sv_block = nullptr;       // one allocation: moments[0] | moments[1] (mu1, mu2 per pixel, swapped with the records) | variance
    float *sv_moments[2] = {nullptr, nullptr}, *sv_variance = nullptr;
    bool sv_valid = false;           // the latest temporal result was made with the option on: moments tp_latest and the variance image go with it
    // ... and its spatial estimate for young pixels (vpt_set_svgf_spatial_options): state only, no memory; ignored while svgf.variance is 0
    vpt_svgf_spatial_options sv_spatial{0u, 3u, 0.1f, 0.05f, 4.0f, {0u, 0u, 0u}};
    // outlier rejection ahead of the two filters (vpt_set_firefly_options): nothing of this is allocated or launched while mode is 0
    vpt_firefly_options ff_options{0u, 1u, 2u, 2.0f, 1.0f, {0u, 0u, 0u}};
    float* ff_block = nullptr;       // one allocation: the filtered image (RGBA32F of ff_w x ff_h) | firefly::kCounterBytes of counter pairs (clamped, considered); made by the first filtered
                                     // call, re-made for another size, freed with the render buffers (vpt_resize, vpt_destroy)
    uint32_t ff_w = 0, ff_h = 0;     // size the block was made for
    bool ff_valid = false;           // the block holds the latest filtered call's image and counts
    uint32_t ff_calls = 0;           // filtered calls since mode went to 1
    // moved instances (vpt_set_temporal_options): nothing of this is allocated, kept or uploaded while instance_motion is 0
    vpt_temporal_options tp_options{0u, {0u, 0u, 0u}};
    temporal::MotionSnapshot tp_snapshot;   // the matrices, at the latest record, of the instances moved since: only while a history is there to carry
    float* tp_motion = nullptr;      // the motion image, 8 B per pixel of tp_w x tp_h: allocated on the first temporal call with the option on, freed wherever tp_block is
    temporal::InstanceMotion* tp_motion_table[2] = {nullptr, nullptr};   // the per-instance records, swapped like the records of the image: the table a queued k_temporal reads is never written
    std::vector<temporal::InstanceMotion> tp_motion_host[2];             // ... and what each was uploaded from
    size_t tp_motion_cap = 0;        // records each table holds
    uint32_t tp_motion_latest = 0;
    bool tp_motion_valid = false;    // the latest temporal result was made with the option on: tp_motion goes with it
    // auto-exposure (vpt_set_exposure_options): nothing of this is allocated or launched while mode is 0.  The adapted state is a scalar about the scene's
    // brightness: it lives on the device, outside the render buffers, and survives vpt_resize and every reset
    exposure::Options ex_options = exposure::default_options();
    ExposureDevice* ex_dev = nullptr;        // state | latest histogram | accumulating histogram: allocated (zeroed) by the first metering, freed by vpt_destroy
    uint32_t ex_reset = exposure::kResetAll; // what the next metering is told (k_exposure_adapt's `reset`): mode has changed / vpt_exposure_reset / nothing
    bool ex_metered = false;                 // a metering has been enqueued since mode went to 1: state and histogram can be read back

    // profiling events
    std::vector<hipEvent_t> ev_pool;
    struct Pending { int kernel; hipEvent_t a, b; };
    std::vector<Pending> pending;
    size_t ev_next = 0;
};
// ---- the helpers more than one file calls (a helper of a single file is in that file's anonymous namespace)
namespace vpt {
namespace api {

// A failed HIP call: its text, HIP's message, the file and the line go to vpt_last_error (api_context.hip).
int hip_failed(vpt_ctx* c, hipError_t e, const char* call, const char* file, int line);
#define HIPCHK(ctx, call)                                                                            \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) return ::vpt::api::hip_failed((ctx), e_, #call, __FILE__, __LINE__);   \
    } while (0)
int fail(vpt_ctx* c, int code, const char* msg);

inline uint32_t shard_rows_of(uint32_t height, uint32_t rank, uint32_t count) { return rank < height ? (height - rank + count - 1) / count : 0; }
inline const float* whole_image(vpt_ctx* c) { return c->P.shard_count > 1 ? c->full_image : c->image; }

// api_context.hip
plan::Facts facts_of(const vpt_ctx* c);
hipError_t memset_now(hipStream_t s, void* p, int v, size_t n);
void free_spill(Lane& L);
void free_lab(vpt_ctx* c);
void destroy_graph(Lane& L);
int check_stream_slack(vpt_ctx* c);
plan::Policy policy_of(const vpt_ctx* c);
plan::State plan_state(const vpt_ctx* c);
uint32_t batch_cap(const vpt_ctx* c);
bool path_buffers_hold(const vpt_ctx* c, uint32_t frames);
int ensure_path_buffers(vpt_ctx* c, uint32_t want);
int ensure_media_buffers(vpt_ctx* c, Lane& L);
int ensure_sorted_buffers(vpt_ctx* c, Lane& L);
int ensure_legacy_buffers(vpt_ctx* c, Lane& L);
// The accumulation starts afresh (PathTracer.h:183).  keep_history: the caller changed nothing a pixel's history depends on but the camera, which
// vpt_temporal_accumulate reprojects through (vpt_set_camera, vpt_reset); every other caller drops the temporal history with the accumulation.
void reset_accum(vpt_ctx* c, bool keep_history = false);
void free_denoise_buffers(vpt_ctx* c);    // dn_block and the result in it
void free_temporal_buffers(vpt_ctx* c);   // tp_block with its result and history, and what goes wherever it goes: sv_block, the motion image and tables
int alloc_spill(vpt_ctx* c, Lane& L, int regions);
Lane* get_lane(vpt_ctx* c, int k);
int ensure_lane_buffers(vpt_ctx* c, Lane& L);
void destroy_lanes(vpt_ctx* c);
// the timing pool: every launch of the host layer goes through TIMED
void begin_timing(vpt_ctx* c, hipStream_t s, int kernel, hipEvent_t* a, hipEvent_t* b);
void end_timing(hipStream_t s, hipEvent_t b);
void collect_timing(vpt_ctx* c);   // call after a stream sync
#define TIMED(ctx, s, kid, launch_expr)                     \
    do {                                                    \
        hipEvent_t ea_, eb_;                                \
        ::vpt::api::begin_timing(ctx, s, kid, &ea_, &eb_);  \
        launch_expr;                                        \
        ::vpt::api::end_timing(s, eb_);                     \
    } while (0)

// api_scene.hip
void free_scene(vpt_ctx* c);
int refresh_material_tables(vpt_ctx* c);
// One launch of k_first_hit on the main lane's stream, nothing waited for (vpt_render_features, vpt_pick, vpt_denoise): every pointer of `a` is device memory.
void enqueue_first_hit(vpt_ctx* c, const FirstHitArgs& a);
// A scene table holding the n elements at src, zeros behind them up to min_elems (at least one element), freed with the scene: DeviceScene's
// pointer to it and, for a table that is written after the upload, the writable one (vpt_ctx::Writable) are set here, from one allocation sized by
// their own element type.  (the work is done once, on bytes; the templates only size and type it)
int upload_bytes(vpt_ctx* c, const void* src, size_t bytes, size_t total_bytes, void** out);
template <class T>
int upload(vpt_ctx* c, const T* src, size_t n, const T** out, size_t min_elems = 1, T** writable = nullptr) {
    void* d = nullptr;
    int rc = upload_bytes(c, src, n * sizeof(T), std::max(n, min_elems) * sizeof(T), &d);
    if (d) { *out = (T*)d; if (writable) *writable = (T*)d; }
    return rc;
}
template <class T>
int upload(vpt_ctx* c, const std::vector<T>& v, const T** out, size_t min_elems = 1, T** writable = nullptr) {
    return upload(c, v.data(), v.size(), out, min_elems, writable);
}

// api_render.hip
DeviceScene lane_scene(const vpt_ctx* c, const Lane& L);
cull::Rect whole_cull_rect(const vpt_ctx* c);   // the pixels outside which the next whole-path batch starts no path (camera_cull.hpp)
uint64_t issue_ticket(vpt_ctx* c, hipStream_t on);
int finish_outstanding(vpt_ctx* c);
int drain(vpt_ctx* c);
int quiesce(vpt_ctx* c);

}  // namespace api
}  // namespace vpt
