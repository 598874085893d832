// api_context.hip — the context of the C-ABI (include/vpt.h): everything that creates, sizes, configures or tears it down.  Render and path
// buffers (sized by path_plan.hpp), the lanes of asynchronous batches, the timing pool, parameters and camera, and the LUT driver.
#include <cmath>

#include "api_ctx.hpp"

using namespace vpt::api;

// ---- helpers of this file alone
namespace {

// Media: homogeneous box volumes or the atmosphere.
bool media_on(const vpt_ctx* c) { return !c->volumes.empty() || c->dsc.atm_on; }
// Everything sized by (frames held) x (shard pixels): path records, queues, streams.
void free_path_buffers(Lane& L) {
    destroy_graph(L);   // the captured batch holds these addresses
    if (L.ps_block) (void)hipFree(L.ps_block);
    L.ps_block = nullptr;
    if (L.ps_legacy) (void)hipFree(L.ps_legacy);
    L.ps_legacy = nullptr;
    for (int i = 0; i < 2; i++) { if (L.queue[i]) (void)hipFree(L.queue[i]); L.queue[i] = nullptr; }
    if (L.cqueue) (void)hipFree(L.cqueue);
    L.cqueue = nullptr;
    if (L.ss_block) (void)hipFree(L.ss_block);
    L.ss_block = nullptr;
    if (L.media_block) (void)hipFree(L.media_block);
    L.media_block = nullptr; L.ms = MediaState{}; L.media_frames = 0;
    for (uint32_t k = 0; k < kShadeClasses; k++) { if (L.class_queue[k]) (void)hipFree(L.class_queue[k]); L.class_queue[k] = nullptr; }
    if (L.cls_q) (void)hipFree(L.cls_q);
    L.cls_q = nullptr;
    L.ps = PathState{}; L.ss = StreamState{};
    L.frames_alloc = 0; L.resident_alloc = 0;
}
void free_render_buffers(vpt_ctx* c) {
    free_path_buffers(c->main);
    if (c->image) (void)hipFree(c->image);
    c->image = nullptr;
    if (c->full_image) (void)hipFree(c->full_image);
    c->full_image = nullptr;
    if (c->gather_buf) (void)hipFree(c->gather_buf);
    c->gather_buf = nullptr;
    for (float* m : c->mips) (void)hipFree(m);
    c->mips.clear(); c->mip_dims = post::Mips{};
    if (c->post_out) (void)hipFree(c->post_out);
    c->post_out = nullptr; c->post_w = c->post_h = 0;
    free_denoise_buffers(c);
    free_temporal_buffers(c);
    if (c->ff_block) (void)hipFree(c->ff_block);   // the firefly filter's image and counters: re-made by the next filtered call
    c->ff_block = nullptr; c->ff_w = c->ff_h = 0; c->ff_valid = false;
}

// Size checks of a (width, height) before anything is freed or changed; *frames_out = the largest batch this context will render.
int check_render_size(vpt_ctx* c, uint32_t width, uint32_t height, uint32_t* frames_out) {
    const uint64_t rows = shard_rows_of(height, c->cfg.shard_rank, c->cfg.shard_count);
    const uint64_t px = rows * width;
    if (px == 0) return fail(c, VPT_ERR_INVALID_ARGUMENT, "empty shard");
    if (px >= (1ull << 31) || (uint64_t)width * height >= (1ull << 31)) return fail(c, VPT_ERR_INVALID_ARGUMENT, "image too large");
    size_t free_b = 0, total_b = 0;
    const bool free_known = c->cfg.frames_in_flight == 0 && hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    const uint64_t F = plan::frames_for_size(c->cfg.frames_in_flight, px, free_known, free_b);   // the CAP of a batch (path_plan.hpp)
    if (px * F >= (1ull << 31)) return fail(c, VPT_ERR_INVALID_ARGUMENT, "too many paths in flight");
    *frames_out = (uint32_t)F;
    return VPT_OK;
}

// Buffers for batches of up to `frames` frames of this shard of which `resident` frames of paths are in flight at a time (the caller
// has drained the streams): slot-addressed records (frame sum, medium, per-sample words: 36 B per SAMPLE of the batch) and the queues
// and stream records (~290 B per RESIDENT path).
int alloc_path_buffers(vpt_ctx* c, Lane& L, uint32_t frames, uint32_t resident) {
    free_path_buffers(L);
    const RenderParams& P = c->P;
    resident = std::min(resident, frames);
    if ((uint64_t)P.shard_pixels * frames >= (1ull << 31)) return fail(c, VPT_ERR_INVALID_ARGUMENT, "too many paths in flight");
    const uint32_t samples = P.shard_pixels * frames;
    uint32_t cap = P.shard_pixels * resident;
    // slot-addressed records every pipeline uses: 2 float4 records + up to 4 dword arrays per slot (device_types.hpp PathState): the medium
    // anisotropy always; the sample index only for samples_per_frame > 1, VolumeDepth / ColorChannel only with media — 36 B per sample of
    // a plain batch (the kernels touch those words under exactly these conditions; path_words_ok() replaces the buffers when a batch needs more).
    // The records of round 1's stage kernels come with ensure_legacy_buffers()
    const bool want_sidx = P.samples_per_frame > 1u, want_media = media_on(c);
    const size_t kRecords = 2, kWords = 1u + (want_sidx ? 1u : 0u) + (want_media ? 2u : 0u);
    size_t stride = ((size_t)samples + 63) & ~(size_t)63;
    HIPCHK(c, hipMalloc(&L.ps_block, stride * (16 * kRecords + 4 * kWords)));
    float4* rb = (float4*)L.ps_block;
    PathState& s = L.ps;
    s = PathState{};
    s.capacity = cap;
    s.ACC = rb; s.M = rb + stride;
    uint32_t* wb = (uint32_t*)(rb + stride * kRecords);
    s.maniso = (float*)wb; wb += stride;
    if (want_sidx) { s.sidx = wb; wb += stride; }
    if (want_media) { s.vdepth = wb; s.cchan = (int32_t*)(wb + stride); }
    L.ps_has_sidx = want_sidx; L.ps_has_media = want_media;
    // streams written by chunked appends hold up to one unwritten chunk tail per wave that appended to them: at most
    // 256 entries per 64 items processed, and never more than one per resident wave of the largest persistent grid.  A launch
    // appends in chunks only when its queue holds >= kFusedExactBelow (fused kernel) / kAppendExactBelow (streams) entries, holes
    // included; below that every append is exact and no stream ever holds a hole, so buffers that cannot reach that length need no slack.
    // (the appending kernels' persistent grids: blocks per CU from the occupancy query, the fused kernel's at most 3 by its LDS; checked
    // against the real grids by check_stream_slack once the scene is known.  Round 3 reserved for 8192 blocks: 2 GB of a large batch's streams)
    const int fused_per_cu = (std::max(c->primary_blocks_general, c->primary_blocks_plain) + std::max(c->cu_count, 1) - 1) / std::max(c->cu_count, 1);   // (the scene's, once one is set)
    const int per_cu = std::max(std::max(4, fused_per_cu), std::max(shade_stream_blocks_per_cu(), std::max(shade_media_blocks_per_cu(), media_tail_blocks_per_cu())));
    const uint64_t max_tails = (uint64_t)c->cu_count * (uint64_t)per_cu * 4u * kAppendChunk;
    L.stream_slack = cap < kFusedExactBelow ? 256u : (uint32_t)std::min<uint64_t>((uint64_t)cap * 4 + 256, max_tails);
    const size_t scap = (size_t)cap + L.stream_slack;
    for (int i = 0; i < 2; i++) HIPCHK(c, hipMalloc((void**)&L.queue[i], scap * 4));
    {
        const size_t sst = (scap + 63) & ~(size_t)63;
        HIPCHK(c, hipMalloc(&L.ss_block, sst * (16 * 17 + 4 + 2)));
        float4* q = (float4*)L.ss_block;
        StreamState& t = L.ss;
        t.PE = q; t.PS = q + sst; t.PL = q + 2 * sst; t.PT = q + 3 * sst; t.SKO = q + 4 * sst; t.SKD = q + 5 * sst; t.LTO = q + 6 * sst; t.LTD = q + 7 * sst;
        t.RA[0] = q + 8 * sst; t.RA[1] = q + 9 * sst; t.RB[0] = q + 10 * sst; t.RB[1] = q + 11 * sst; t.RT[0] = q + 12 * sst; t.RT[1] = q + 13 * sst;
        t.RL[0] = q + 14 * sst; t.RL[1] = q + 15 * sst;
        t.SH = q + 16 * sst; t.SHI = (uint32_t*)(q + 17 * sst);
        t.vis_sky = (unsigned char*)(t.SHI + sst); t.vis_light = t.vis_sky + sst;
        t.cap = (uint32_t)scap;
    }
    L.frames_alloc = frames; L.resident_alloc = resident;
    return VPT_OK;
}

// (Re)allocates everything that depends on the image size: the accumulation image(s) and the path buffers of ONE frame.  On failure
// the context keeps NO render buffers and says so (buffers_ok == false): vpt_render / vpt_get_* / vpt_postprocess then return an error
// instead of touching freed memory.
int alloc_render_buffers(vpt_ctx* c) {
    c->buffers_ok = false;
    c->frames_cap = 0;
    uint32_t F = 1;
    int rc = check_render_size(c, c->cfg.width, c->cfg.height, &F);
    if (rc != VPT_OK) return rc;
    free_render_buffers(c);
    RenderParams& P = c->P;
    P.width = c->cfg.width; P.height = c->cfg.height;
    P.shard_rank = c->cfg.shard_rank; P.shard_count = c->cfg.shard_count;
    P.shard_rows = shard_rows_of(P.height, P.shard_rank, P.shard_count);
    P.shard_pixels = P.shard_rows * P.width;
    c->frames_in_flight = F;
    auto images = [&]() -> int {
        // padded to the largest shard's row count (vpt_shard_floats): the buffer is handed to ncclGather as it is
        const size_t image_bytes = (size_t)shard_rows_of(P.height, 0, P.shard_count) * P.width * 16;
        HIPCHK(c, hipMalloc((void**)&c->image, image_bytes));
        HIPCHK(c, memset_now(c->main.stream, c->image, 0, image_bytes));
        if (P.shard_count > 1) {
            HIPCHK(c, hipMalloc((void**)&c->full_image, (size_t)P.width * P.height * 16));
            HIPCHK(c, memset_now(c->main.stream, c->full_image, 0, (size_t)P.width * P.height * 16));
        }
        return VPT_OK;
    };
    rc = images();
    if (rc == VPT_OK) rc = alloc_path_buffers(c, c->main, 1, 1);
    if (rc != VPT_OK) {
        std::string keep = c->err;
        free_render_buffers(c);
        (void)hipGetLastError();
        c->err = keep;
        return rc;
    }
    c->full_valid = false;
    c->buffers_ok = true;
    return check_stream_slack(c);
}

// Do the per-sample word arrays allocated cover what the next batch touches (samples_per_frame / media may have changed since)?
bool path_words_ok(const vpt_ctx* c, const Lane& L) {
    const bool want_sidx = c->P.samples_per_frame > 1u, want_media = media_on(c);
    return (!want_sidx || L.ps_has_sidx) && (!want_media || L.ps_has_media);
}

void sync_params(vpt_ctx* c) {
    RenderParams& P = c->P;
    const vpt_params& p = c->params;
    P.samples_per_frame = p.samples_per_frame; P.max_depth = p.max_depth;
    P.max_luminance = p.max_luminance; P.focus_distance = p.focus_distance; P.dof_strength = p.dof_strength;
    P.sky_azimuth = p.sky_azimuth; P.sky_altitude = p.sky_altitude; P.sky_intensity = p.sky_intensity;
    P.emissive_pdf_bias = p.emissive_pdf_bias; P.flags = p.flags; P.base_seed = p.base_seed;
    P.split = p.screen_chunk_count; P.launch_off = c->d_launch_off;
    // the angles exactly as the shaders form them (Sampler.slang:333-334, Miss.slang:28-29); same header, same bits as on the device
    // (VPT_PI: camera.hpp's, the shaders' M_PI as fp32)
    vptfp::sincos_(P.sky_azimuth / 180.0f * VPT_PI, &P.sky_rot[0], &P.sky_rot[1]);
    vptfp::sincos_(P.sky_altitude / 180.0f * VPT_PI, &P.sky_rot[2], &P.sky_rot[3]);
    vptfp::sincos_(-(P.sky_altitude / 180.0f * VPT_PI), &P.sky_rot[4], &P.sky_rot[5]);
    vptfp::sincos_(-(P.sky_azimuth / 180.0f * VPT_PI), &P.sky_rot[6], &P.sky_rot[7]);
}

// ---- lanes (struct Lane)
// Streams, events and counters of a lane.  A failure leaves what it got for lane_destroy.
int lane_init(vpt_ctx* c, Lane& L) {
    HIPCHK(c, hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
    HIPCHK(c, hipStreamCreateWithFlags(&L.stream2, hipStreamNonBlocking));
    for (hipEvent_t* e : {&L.ev_shade, &L.ev_join, &L.ev_resolved}) HIPCHK(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    HIPCHK(c, hipMalloc((void**)&L.ctr, sizeof(Counters)));
    HIPCHK(c, memset_now(L.stream, L.ctr, 0, sizeof(Counters)));
    HIPCHK(c, hipMalloc((void**)&L.sctr, sizeof(StreamCounters)));
    HIPCHK(c, memset_now(L.stream, L.sctr, 0, sizeof(StreamCounters)));
    if (hipHostMalloc((void**)&L.h_ctr, sizeof(HostCounters), hipHostMallocDefault) != hipSuccess) { L.h_ctr = nullptr; return fail(c, VPT_ERR_DEVICE, "hipHostMalloc of a lane's counters failed"); }
    memset(L.h_ctr, 0, sizeof(HostCounters));
    HIPCHK(c, hipMalloc((void**)&L.d_dispatch_base, 256));
    return VPT_OK;
}
// The one teardown of a lane: nothing of it is in flight, then its graph, its buffers, its events and streams.
void lane_destroy(Lane& L) {
    if (L.stream) (void)hipStreamSynchronize(L.stream);
    if (L.stream2) (void)hipStreamSynchronize(L.stream2);
    free_path_buffers(L);   // (the captured graph first)
    free_spill(L);
    if (L.h_ctr) (void)hipHostFree(L.h_ctr);
    if (L.d_dispatch_base) (void)hipFree(L.d_dispatch_base);
    if (L.ctr) (void)hipFree(L.ctr);
    if (L.sctr) (void)hipFree(L.sctr);
    for (hipEvent_t e : {L.ev_shade, L.ev_join, L.ev_resolved}) if (e) (void)hipEventDestroy(e);
    if (L.stream2) (void)hipStreamDestroy(L.stream2);
    if (L.stream) (void)hipStreamDestroy(L.stream);
    L = Lane{};
}

}  // namespace

// ---- helpers the other api_*.hip files call too (declared in api_ctx.hpp)
namespace vpt {
namespace api {

// A failed HIP call: its text, HIP's message, the file and the line go to vpt_last_error (one copy of the formatting, not one per call site: the
// product library's size is bounded, tests/test_abi.py).
__attribute__((noinline, cold)) int hip_failed(vpt_ctx* c, hipError_t e, const char* call, const char* file, int line) {
    char buf[512];
    snprintf(buf, sizeof(buf), "%s failed: %s (%s:%d)", call, hipGetErrorString(e), file, line);
    c->err = buf;
    return (e == hipErrorOutOfMemory) ? VPT_ERR_OUT_OF_MEMORY : VPT_ERR_DEVICE;
}

int fail(vpt_ctx* c, int code, const char* msg) { c->err = msg; return code; }

// What path_plan.hpp decides from: how a batch runs and how the path buffers are sized.  A handful of loads — every batch asks.
plan::Facts facts_of(const vpt_ctx* c) {
    plan::Facts f;
    f.pipeline = c->cfg.pipeline; f.build_flags = c->cfg.build_flags; f.lab_build = VPT_LAB != 0;
    f.has_scene = c->has_scene; f.lds_scene = c->lds_scene; f.whole_grid = c->whole_blocks > 0; f.media = media_on(c);
    f.samples_per_frame = c->P.samples_per_frame; f.split = c->P.split; f.max_depth = c->P.max_depth; f.depth_bounded = c->depth_bounded;
    f.whole_frames_bound = c->lab_whole_frames; f.whole_parts = c->lab_whole_parts;
    f.whole_plain = c->scene_plain && !c->dsc.strict_hits && c->dsc.env_black;   // (launch_whole's choice, counting aside)
    f.profile = c->cfg.profile != 0; f.count_traversal = c->cfg.count_traversal != 0;
    f.shard_pixels = c->P.shard_pixels;
    f.cfg_frames = c->cfg.frames_in_flight; f.cfg_resident = c->cfg.resident_frames;
    return f;
}

// hipMemset is asynchronous to the host and runs on the null stream, which the context's non-blocking streams do not wait for: a kernel
// enqueued after it may run before the clear has landed (a batch behind vpt_set_scene's image clear lost pixels that way).  Every clear of
// memory the kernels touch goes through here instead: on the stream that uses the memory, waited for.
hipError_t memset_now(hipStream_t s, void* p, int v, size_t n) {
    hipError_t e = hipMemsetAsync(p, v, n, s);
    return e == hipSuccess ? hipStreamSynchronize(s) : e;
}

void free_spill(Lane& L) {
    if (L.spill) (void)hipFree(L.spill);
    L.spill = L.spill2 = nullptr; L.stack_overflow_words = 0;
}
void free_lab(vpt_ctx* c) {
    for (void* p : {(void*)c->lab_ro, (void*)c->lab_rd, (void*)c->lab_hit, (void*)c->lab_hinst, (void*)c->lab_order}) if (p) (void)hipFree(p);
    c->lab_ro = c->lab_rd = c->lab_hit = nullptr; c->lab_hinst = c->lab_order = nullptr; c->lab_n = 0;
}
void destroy_graph(Lane& L) {
    if (L.graph) (void)hipGraphExecDestroy(L.graph);
    L.graph = nullptr; L.graph_gen = 0;
}

// Every wave of a launch that appends to a stream may leave one unwritten chunk tail in it (vote.hpp WaveAppender): the streams are
// allocated with room for stream_slack such entries.  Refuse — not after a kernel has written past a stream — if a device with more
// CUs / other occupancy than the allocation assumed ever needs more.  Called wherever the grids (vpt_set_scene) or the buffers change.
int check_stream_slack(vpt_ctx* c) {
    if (!c->has_scene || c->main.frames_alloc == 0 || c->main.ps.capacity < kFusedExactBelow) return VPT_OK;   // short streams are appended to exactly: no tails
    const uint64_t appending_waves = 4ull * (uint64_t)std::max(std::max(c->shade_stream_blocks, c->primary_blocks), std::max(c->shade_media_blocks, c->media_tail_blocks));
    if (appending_waves * kAppendChunk > (uint64_t)c->main.stream_slack && (uint64_t)c->main.ps.capacity * 4 + 256 > (uint64_t)c->main.stream_slack)
        return fail(c, VPT_ERR_DEVICE, "internal: the stream slack allocated for chunk tails is smaller than one chunk per appending wave of this device");
    return VPT_OK;
}

// The sizing of the path buffers is path_plan.hpp's: what it needs to know of this context.
plan::Policy policy_of(const vpt_ctx* c) { return plan::policy_of(facts_of(c)); }
plan::State plan_state(const vpt_ctx* c) {
    plan::State s;
    s.px = c->P.shard_pixels; s.frames_in_flight = c->frames_in_flight; s.frames_cap = c->frames_cap; s.long_factor = c->long_factor;
    s.frames_alloc = c->main.frames_alloc; s.resident_alloc = c->main.resident_alloc;
    return s;
}
uint32_t batch_cap(const vpt_ctx* c) { return plan::batch_cap(policy_of(c), plan_state(c)); }

bool path_buffers_hold(const vpt_ctx* c, uint32_t frames) { return plan::holds(policy_of(c), plan_state(c), frames) && path_words_ok(c, c->main); }
// Grows the main lane's buffers so that a batch of `want` frames (<= batch_cap) fits, by plan::grow; the caller has drained the streams.  On
// failure the context keeps the buffers it had (or none: buffers_ok == false) and the error of the allocation that failed.
int ensure_path_buffers(vpt_ctx* c, uint32_t want) {
    if (path_buffers_hold(c, want)) return VPT_OK;
    c->state_gen++;   // (batches of another shape from here on: the count of unchanged calls behind a graph replay starts again)
    int rc = VPT_OK;
    std::string keep;
    plan::State s = plan_state(c);
    const plan::Grown g = plan::grow(policy_of(c), s, want, [&](uint32_t frames, uint32_t resident) {
        rc = alloc_path_buffers(c, c->main, frames, resident);
        if (rc == VPT_OK) return (int)plan::kAllocOk;
        keep = c->err;
        free_path_buffers(c->main);
        (void)hipGetLastError();
        return (int)(rc == VPT_ERR_OUT_OF_MEMORY || rc == VPT_ERR_DEVICE ? plan::kAllocOutOfMemory : plan::kAllocFailed);
    });
    c->frames_in_flight = s.frames_in_flight; c->frames_cap = s.frames_cap; c->long_factor = s.long_factor;
    if (g.result != plan::kAllocOk) {
        if (alloc_path_buffers(c, c->main, g.frames, g.resident) != VPT_OK) { free_path_buffers(c->main); (void)hipGetLastError(); c->buffers_ok = false; }
        c->err = keep;
        return rc;
    }
    return check_stream_slack(c);
}

// Round 1's stage kernels (VPT_PIPELINE_STAGED_R1 only: laboratory build)
// keep a path's records by slot: 13 more float4 records (pathLight among them), the hit instance and the two-ended connect queue, 216 bytes per path,
// allocated when such a batch is first rendered and kept until the next resize.
// The class queues of VPT_PIPELINE_STAGED_SORTED (21 bytes per path), likewise on first use.
// Media on the streams pipeline: 11 more float4 streams per queue entry (176 bytes per path), allocated when such a batch is first
// rendered and kept until the next resize.  They are sized to what is free then (at most 85 % of it): a media batch holds
// media_frames frames, which may be fewer than frames_in_flight (vpt_render then renders in more, smaller batches; the image is
// the same for any batch size).
int ensure_media_buffers(vpt_ctx* c, Lane& L) {
    if (L.media_block) return VPT_OK;
    const uint64_t px = c->P.shard_pixels;
    uint64_t frames = L.resident_alloc;   // what the queues and streams hold now (free_path_buffers drops this block with them)
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const uint64_t fit = (uint64_t)(free_b * 0.85) / (16ull * 11ull);
        const uint64_t fit_frames = fit > L.stream_slack ? (fit - L.stream_slack) / px : 0;
        frames = std::min<uint64_t>(frames, fit_frames);
    }
    if (frames == 0) return fail(c, VPT_ERR_DEVICE, "out of device memory for the media streams (176 bytes per resident path)");
    const size_t sst = (((size_t)frames * px + L.stream_slack) + 63) & ~(size_t)63;
    if (hipMalloc(&L.media_block, sst * 16 * 11) != hipSuccess) {
        (void)hipGetLastError();
        L.media_block = nullptr;
        return fail(c, VPT_ERR_DEVICE, "out of device memory for the media streams (176 bytes per resident path): lower vpt_config.frames_in_flight");
    }
    L.media_frames = (uint32_t)frames;
    float4* q = (float4*)L.media_block;
    L.ms.MS = q;
    for (int k = 0; k < 10; k++) L.ms.MP[k] = q + (size_t)(k + 1) * sst;
    return VPT_OK;
}

int ensure_sorted_buffers(vpt_ctx* c, Lane& L) {
    if (L.cls_q) return VPT_OK;
    const size_t scap = L.ss.cap;
    for (uint32_t k = 0; k < kShadeClasses; k++) if (!L.class_queue[k]) HIPCHK(c, hipMalloc((void**)&L.class_queue[k], scap * 4));
    HIPCHK(c, hipMalloc((void**)&L.cls_q, scap));
    return VPT_OK;
}

int ensure_legacy_buffers(vpt_ctx* c, Lane& L) {
    const size_t cap = L.ps.capacity, stride = (cap + 63) & ~(size_t)63;
    if (!L.ps_legacy) {
        HIPCHK(c, hipMalloc(&L.ps_legacy, stride * (16 * 13 + 4)));
        float4* q = (float4*)L.ps_legacy;
        PathState& s = L.ps;
        s.L = q + stride * 12;
        s.A = q; s.B = q + stride; s.T[0] = q + stride * 2; s.T[1] = q + stride * 3; s.H = q + stride * 4;
        s.CE = q + stride * 5; s.CS = q + stride * 6; s.CSO = q + stride * 7; s.CSD = q + stride * 8; s.CL = q + stride * 9; s.CLO = q + stride * 10; s.CLD = q + stride * 11;
        s.hinst = (uint32_t*)(q + stride * 13);
    }
    if (!L.cqueue) HIPCHK(c, hipMalloc((void**)&L.cqueue, cap * 4));   // (a failed call leaves what it got; the next one completes it)
    return VPT_OK;
}

void reset_accum(vpt_ctx* c, bool keep_history) { c->frame_count = 0; c->dispatch_count = 0; c->samples_accum = 0; if (!keep_history) { c->tp_history = false; c->tp_snapshot.clear(); } }  // PathTracer.h:183
// The denoiser's images: re-made by the next vpt_denoise*, whose result is gone with them.
void free_denoise_buffers(vpt_ctx* c) {
    if (c->dn_block) (void)hipFree(c->dn_block);
    c->dn_block = nullptr; c->dn_w = c->dn_h = 0; c->dn_valid = false;
}
// The temporal records and result, gone with the size they were made for, and what was allocated beside them for that size: the luminance moments
// (vpt_svgf_options.variance), the motion image and the per-instance tables (vpt_temporal_options.instance_motion).
void free_temporal_buffers(vpt_ctx* c) {
    if (c->tp_block) (void)hipFree(c->tp_block);
    c->tp_block = nullptr; c->tp_w = c->tp_h = 0; c->tp_valid = c->tp_history = false;
    if (c->sv_block) (void)hipFree(c->sv_block);
    c->sv_block = nullptr; c->sv_valid = false;
    if (c->tp_motion) (void)hipFree(c->tp_motion);
    for (int k = 0; k < 2; k++) { if (c->tp_motion_table[k]) (void)hipFree(c->tp_motion_table[k]); c->tp_motion_table[k] = nullptr; }
    c->tp_motion = nullptr; c->tp_motion_cap = 0; c->tp_motion_valid = false;
}

void begin_timing(vpt_ctx* c, hipStream_t s, int kernel, hipEvent_t* a, hipEvent_t* b) {
    *a = *b = nullptr;
    c->stats.kernel_launches[kernel]++;
    if (!c->cfg.profile) return;
    if (c->ev_next + 2 > c->ev_pool.size()) {
        for (int i = 0; i < 64; i++) { hipEvent_t e; (void)hipEventCreate(&e); c->ev_pool.push_back(e); }
    }
    *a = c->ev_pool[c->ev_next++]; *b = c->ev_pool[c->ev_next++];
    (void)hipEventRecord(*a, s);
    c->pending.push_back({kernel, *a, *b});
}
void end_timing(hipStream_t s, hipEvent_t b) { if (b) (void)hipEventRecord(b, s); }
void collect_timing(vpt_ctx* c) {
    for (auto& p : c->pending) { float ms = 0.0f; if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) c->stats.kernel_ms[p.kernel] += ms; }
    c->pending.clear(); c->ev_next = 0;
}

// ---- lanes (struct Lane; lane_init and lane_destroy above)
// `regions` per-thread overflow regions of the traversal stacks, each for the largest persistent grid the scene launches, preset to a
// word no stack entry can be (a node index of 2.1e9; leaf codes are negative): vpt_get_stats counts what was spilled.
int alloc_spill(vpt_ctx* c, Lane& L, int regions) {
    const size_t region = stack_overflow_bytes((uint32_t)c->max_blocks);
    HIPCHK(c, hipMalloc((void**)&L.spill, regions * region));
    L.spill2 = regions > 1 ? (uint32_t*)((char*)L.spill + region) : L.spill;
    HIPCHK(c, memset_now(L.stream, L.spill, kSpillPatternByte, regions * region));
    L.stack_overflow_words = (uint32_t)(region / 4);
    return VPT_OK;
}
// Lane k >= 1: created on first use with one frame of path buffers for the context's image size and one spill region (its batches stay on
// one stream).  nullptr: out of memory — pipelining is an optimisation, the frame then goes to a lane there is.
Lane* get_lane(vpt_ctx* c, int k) {
    Lane*& slot = c->extra[k - 1];
    if (slot) return slot;
    Lane* L = new Lane();
    if (lane_init(c, *L) != VPT_OK || alloc_path_buffers(c, *L, 1, 1) != VPT_OK || alloc_spill(c, *L, 1) != VPT_OK) {
        (void)hipGetLastError();
        lane_destroy(*L);
        delete L;
        c->err.clear();
        return nullptr;
    }
    return slot = L;
}
// The lane's per-sample words must cover the next batch (samples_per_frame may have changed since; vpt_set_params drained every lane
// before it did, so nothing of this lane is in flight when they are replaced).
int ensure_lane_buffers(vpt_ctx* c, Lane& L) {
    return path_words_ok(c, L) ? VPT_OK : alloc_path_buffers(c, L, 1, 1);
}
void destroy_lanes(vpt_ctx* c) {
    for (Lane*& L : c->extra)
        if (L) { lane_destroy(*L); delete L; L = nullptr; }
    c->order_lane = nullptr;
}

}  // namespace api
}  // namespace vpt

extern "C" {

void vpt_default_params(vpt_params* p) {  // PathTracer.h:197-233
    p->samples_per_frame = 1; p->max_samples = 5000; p->max_depth = 200; p->max_luminance = 500.0f;
    p->focus_distance = 1.0f; p->dof_strength = 0.0f; p->sky_azimuth = 0.0f; p->sky_altitude = 0.0f; p->sky_intensity = 1.0f;
    p->screen_chunk_count = 1; p->emissive_pdf_bias = 0.0f; p->flags = VPT_FLAGS_DEFAULT; p->base_seed = 1;
}
void vpt_default_post_params(vpt_post_params* p) {  // PostProcessor.h:8-21
    p->schedule = VPT_POST_FUSED;
    p->exposure = 1.0f; p->gamma = 2.2f; p->bloom_threshold = 2.0f; p->bloom_strength = 1.0f; p->mip_count = 10; p->falloff_range = 5.0f;
}

vpt_ctx* vpt_create(const vpt_config* cfg, int* err) {
    auto set = [&](int e) { if (err) *err = e; };
    if (!cfg || cfg->width == 0 || cfg->height == 0 || cfg->shard_count == 0 || cfg->shard_rank >= cfg->shard_count || cfg->pipeline > VPT_PIPELINE_WHOLE) { set(VPT_ERR_INVALID_ARGUMENT); return nullptr; }
#if !VPT_LAB
    if (cfg->pipeline == VPT_PIPELINE_STAGED_R1) { set(VPT_ERR_UNSUPPORTED); return nullptr; }   // round 1's stage kernels live in the laboratory build (libvpt_hip_lab.so)
#endif
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) { set(VPT_ERR_NO_DEVICE); return nullptr; }
    if (hipSetDevice(cfg->device) != hipSuccess) { set(VPT_ERR_NO_DEVICE); return nullptr; }
    vpt_ctx* c = new vpt_ctx();
    c->cfg = *cfg;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess) c->cu_count = prop.multiProcessorCount;
    bool ok = lane_init(c, c->main) == VPT_OK && hipEventCreateWithFlags(&c->ev_post, hipEventDisableTiming) == hipSuccess &&
              hipMalloc((void**)&c->d_launch_off, (plan::kMaxFramesInFlight + 1) * 4) == hipSuccess && hipMalloc((void**)&c->d_spill_count, 256) == hipSuccess;
    for (int k = 0; ok && k < kTickets; k++)
        if (hipEventCreateWithFlags(&c->tick_ev[k], hipEventDisableTiming) != hipSuccess) { c->tick_ev[k] = nullptr; ok = false; }
    if (!ok) { (void)hipGetLastError(); set(VPT_ERR_DEVICE); vpt_destroy(c); return nullptr; }
    vpt_default_params(&c->params);
    const float id[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    memcpy(c->P.view_inv, id, 64); memcpy(c->P.proj_inv, id, 64);
    sync_params(c);
    int rc = alloc_render_buffers(c);
    if (rc != VPT_OK) { set(rc); vpt_destroy(c); return nullptr; }
    set(VPT_OK);
    return c;
}

void vpt_destroy(vpt_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    if (c->main.stream) (void)hipStreamSynchronize(c->main.stream);
    if (c->main.stream2) (void)hipStreamSynchronize(c->main.stream2);
    destroy_lanes(c);
    (void)vpt_comm_destroy(c);
    if (c->ev_post) (void)hipEventDestroy(c->ev_post);
    for (int k = 0; k < kTickets; k++) if (c->tick_ev[k]) (void)hipEventDestroy(c->tick_ev[k]);
    if (c->d_spill_count) (void)hipFree(c->d_spill_count);
    free_lab(c);
    free_scene(c);
    free_render_buffers(c);
    if (c->d_launch_off) (void)hipFree(c->d_launch_off);
    if (c->ex_dev) (void)hipFree(c->ex_dev);
    if (c->d_volumes) (void)hipFree(c->d_volumes);
    for (DensityGrid& g : c->grids) { (void)hipFree((void*)g.values); (void)hipFree((void*)g.block_max); (void)hipFree((void*)g.bricks); }
    if (c->d_grids) (void)hipFree(c->d_grids);
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    lane_destroy(c->main);
    delete c;
}

const char* vpt_last_error(const vpt_ctx* c) { return c ? c->err.c_str() : "null context"; }

int vpt_set_camera(vpt_ctx* c, const float* vi, const float* pi) {
    if (!c || !vi || !pi) return VPT_ERR_INVALID_ARGUMENT;
    memcpy(c->P.view_inv, vi, 64); memcpy(c->P.proj_inv, pi, 64);   // host state only: batches already enqueued carry their own copy
    c->state_gen++;
    reset_accum(c, true);   // (the temporal history is reprojected through the new camera)
    return VPT_OK;
}

int vpt_set_params(vpt_ctx* c, const vpt_params* p) {
    if (!c || !p) return VPT_ERR_INVALID_ARGUMENT;
    if (p->samples_per_frame == 0 || p->samples_per_frame > 0xffffffu) return fail(c, VPT_ERR_INVALID_ARGUMENT, "samples_per_frame must be >= 1");
    // MAX_DEPTH (Defines.slang:16) marks a finished path; a larger MaxDepth would make the reference loop forever on a miss
    if (p->max_depth == 0 || p->max_depth > kMaxDepthLimit) return fail(c, VPT_ERR_INVALID_ARGUMENT, "max_depth must be in [1, 1000000]");
    if (p->screen_chunk_count == 0 || p->screen_chunk_count > 64) return fail(c, VPT_ERR_INVALID_ARGUMENT, "screen_chunk_count must be in [1, 64]");
    if (p->screen_chunk_count != 1 && c->P.shard_count != 1) return fail(c, VPT_ERR_UNSUPPORTED, "split-screen dispatch needs the whole image in one context (shard_count == 1): its first dispatch copies pixels across rows");
    {   // SetMaxSamplesAccumulated alone keeps the accumulated image (PathTracer.cpp:1003-1006 does not reset)
        vpt_params same = *p; same.max_samples = c->params.max_samples;
        if (p->max_samples != c->params.max_samples && memcmp(&same, &c->params, sizeof(vpt_params)) == 0) { c->params.max_samples = p->max_samples; return VPT_OK; }
    }
    { int rd = drain(c); if (rd) return rd; }
    c->state_gen++;
    const bool flags_changed = c->params.flags != p->flags;
    c->dsc.strict_hits = (p->flags & VPT_FLAG_LOCAL_HITS) ? 1u : 0u;
    c->params = *p;
    sync_params(c);
    reset_accum(c);
    if (flags_changed && c->has_scene) {  // FURNACE_TEST_MODE is baked into the resolved-material table
        HIPCHK(c, hipSetDevice(c->cfg.device));
        int rc2 = refresh_material_tables(c); if (rc2) return rc2;
    }
    return VPT_OK;
}

// The seed alone, for a viewport that wants other random numbers every frame: what vpt_set_params does for it (nothing in flight, no captured batch
// replayed with the old seed), but the accumulation restarts the way vpt_set_camera restarts it — the temporal history stays.
int vpt_set_base_seed(vpt_ctx* c, uint32_t base_seed) {
    if (!c) return VPT_ERR_INVALID_ARGUMENT;
    { int rd = drain(c); if (rd) return rd; }
    c->state_gen++;
    c->params.base_seed = base_seed;
    sync_params(c);
    reset_accum(c, true);
    return VPT_OK;
}

int vpt_resize(vpt_ctx* c, uint32_t w, uint32_t h) {
    if (!c || w == 0 || h == 0) return VPT_ERR_INVALID_ARGUMENT;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    uint32_t F = 1;
    int rc = check_render_size(c, w, h, &F);   // nothing is freed or changed for a size this context cannot hold
    if (rc != VPT_OK) return rc;
    if ((rc = drain(c))) return rc;
    destroy_lanes(c);   // (they hold path buffers of the old size)
    c->state_gen++;
    c->cfg.width = w; c->cfg.height = h;
    reset_accum(c);
    return alloc_render_buffers(c);
}

int vpt_reset(vpt_ctx* c) { if (!c) return VPT_ERR_INVALID_ARGUMENT; reset_accum(c, true); return VPT_OK; }

int vpt_device_identity(vpt_ctx* c, char* out, uint32_t out_bytes) {
    if (!c || !out || out_bytes < 32) return VPT_ERR_INVALID_ARGUMENT;
    HIPCHK(c, hipDeviceGetPCIBusId(out, (int)out_bytes, c->cfg.device));
    return VPT_OK;
}

int vpt_lut_calculate(int device, uint32_t kind, uint32_t sx, uint32_t sy, uint32_t sz, uint32_t sample_count, uint32_t time_ms, float* out) {
    // sampleCount / 20 passes (LookupTableCalculator.cpp:97); fewer than one pass would divide the table by zero
    if (!out || kind > VPT_LUT_REFRACT_BELOW || sx == 0 || sy == 0 || sz == 0 || (uint64_t)sx * sy * sz > (1u << 28) || sample_count < 20u)
        return VPT_ERR_INVALID_ARGUMENT;
    if (hipSetDevice(device) != hipSuccess) return VPT_ERR_DEVICE;
    const size_t cells = (size_t)sx * sy * sz;
    float* d = nullptr;
    if (hipMalloc((void**)&d, cells * 4) != hipSuccess) return VPT_ERR_OUT_OF_MEMORY;
    hipStream_t s = nullptr;
    int rc = VPT_OK;
    if (hipStreamCreate(&s) != hipSuccess || hipMemsetAsync(d, 0, cells * 4, s) != hipSuccess) rc = VPT_ERR_DEVICE;
    const uint32_t passes = sample_count / 20u, time_hash = vptfp::pcg_hash(time_ms);
    const uint32_t per_launch = 4096;  // bounds one launch to ~80k samples per cell
    for (uint32_t first = 0; !rc && first < passes; first += per_launch) {
        launch_lut(s, (int)kind, d, sx, sy, sz, sample_count, time_hash, first, std::min(per_launch, passes - first));
        if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = VPT_ERR_DEVICE;
    }
    if (!rc && hipMemcpy(out, d, cells * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = VPT_ERR_DEVICE;
    if (!rc) for (size_t i = 0; i < cells; i++) out[i] /= (float)passes;  // LookupTableCalculator.cpp:152-155
    if (s) (void)hipStreamDestroy(s);
    (void)hipFree(d);
    return rc;
}

}  // extern "C"
