// api_render.hip — a batch from decision to resolve: the wavefront stages as path_plan.hpp schedules them, asynchronous batches (fixed schedules,
// captured graphs, lanes, tickets), the radiance image and the statistics.
#include "api_ctx.hpp"

using namespace vpt::api;
using plan::Kind;

// ---- helpers of this file alone
namespace {

// ---- One batch of `frames` consecutive dispatches starting at dispatch index `dispatch_base`, in stages: batch_begin (camera rays /
// bounce 0), batch_bounces (k more bounces), batch_resolve (the guarded resolve + the counters on their way to pinned host memory),
// batch_check (host synchronisation: how many paths are still alive).  The bounce loop runs without host round-trips: every stage
// reads its queue size from device memory, so the host only looks at the counters every few bounces (render_batch) or not at all
// until somebody waits (vpt_render_async).

// Split-screen dispatch (split S > 1): RayTrace(ceil(W/S), ceil(H/S)) per dispatch, in-bounds part only (PathTracer.cpp:145-150, RayGen.slang:24).
uint32_t split_dispatch_slots(const RenderParams& P, uint32_t dispatch) {
    const uint32_t S = P.split, ch = dispatch % (S * S), cx = ch % S, cy = ch / S;
    const uint32_t lw = cx < P.width ? (P.width - cx + S - 1) / S : 0, lh = cy < P.height ? (P.height - cy + S - 1) / S : 0;
    return lw * lh;
}
// Samples of a batch.
uint32_t batch_slots(const RenderParams& P, uint32_t frames, uint32_t dispatch_base) {
    if (P.split <= 1) return frames * P.shard_pixels;
    uint32_t n = 0;
    for (uint32_t k = 0; k < frames; k++) n += split_dispatch_slots(P, dispatch_base + k);
    return n;
}
// How a batch of `frames` frames runs on lane L, by path_plan.hpp: the context's facts `f`, the lane's buffers.
int decide_batch(vpt_ctx* c, const Lane& L, const plan::Facts& f, uint32_t frames, uint32_t dispatch_base, bool capturing, plan::Schedule& sd) {
    if (frames == 0 || frames > L.frames_alloc) return fail(c, VPT_ERR_DEVICE, "internal: batch larger than the path buffers");
    sd = plan::decide(f, frames, L.frames_alloc, L.resident_alloc, batch_slots(c->P, frames, dispatch_base), &L != &c->main, capturing);
    return sd.err != VPT_OK ? fail(c, sd.err, sd.msg) : VPT_OK;
}
// The path buffers as part of a whole-path batch sees them: its first sample is the part's slot 0 (seeds come from pixel and dispatch index, results
// go to ACC[slot]: a sample computes the same in whichever part it runs).
PathState part_state(const vpt_ctx* c, const Lane& L, uint32_t first_frame) {
    PathState ps = L.ps;
    const size_t at = (size_t)first_frame * c->P.shard_pixels;
    ps.ACC += at; ps.M += at; ps.maniso += at;
    return ps;
}
// The guarded resolve of part `i` of batch b (a batch that is not split is its own part 0) on stream `on`.  Frames resolve in order.
void resolve_part(vpt_ctx* c, Lane& L, const BatchState& b, uint32_t i, hipStream_t on) {
    const uint32_t first = b.sd.parts.first[i];
    const uint32_t* guard = plan::runs_fused(b.sd.kind) ? &L.ctr->alive3[b.k3] : plan::runs_streams(b.sd.kind) ? &L.sctr->alive[b.parity].v : &L.ctr->ray_count[b.parity];
    TIMED(c, on, VPT_K_RESOLVE, launch_resolve(on, c->P, part_state(c, L, first), c->image, b.sd.parts.first[i + 1] - first, b.dispatch_base + first, guard));
}
// Turns the decided schedule into buffers and launches.
int batch_begin(vpt_ctx* c, Lane& L, const plan::Schedule& sd, uint32_t frames, uint32_t dispatch_base, Grids grids, BatchState& b) {
    hipStream_t s = L.stream;
    b = BatchState{};
    b.frames = frames; b.dispatch_base = dispatch_base; b.sd = sd;
    b.primary_grid = grids.primary; b.tail_grid = grids.tail;
    c->spill_dirty = true;
    const uint32_t n_slots = batch_slots(c->P, frames, dispatch_base);
    // A whole-path batch whose camera sees the scene's box inside a rectangle of the image (camera_cull.hpp) deals its launch indices over the
    // samples inside it alone (whole_deal.hpp); the same rectangle for every part.
    const cull::Rect wrect = sd.kind == Kind::Whole ? whole_cull_rect(c) : cull::everything(c->P.width, c->P.height);
    uint32_t n_split_dealt = 0;   // split-screen dispatch with a rectangle: the batch's launch indices
    if (c->P.split > 1) {   // launch-grid prefix sums of the batch's dispatches
        std::vector<uint32_t> off(frames + 1, 0u);
        for (uint32_t k = 0; k < frames; k++)
            off[k + 1] = off[k] + (wrect.all ? split_dispatch_slots(c->P, dispatch_base + k) : deal::split_rect_px(wrect, (dispatch_base + k) % (c->P.split * c->P.split), c->P.split));
        n_split_dealt = off[frames];
        HIPCHK(c, hipMemcpyAsync(c->d_launch_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipStreamSynchronize(s));  // `off` is a stack-lifetime staging buffer
    }
    b.n_slots = n_slots;
    b.n_first = sd.regen ? sd.resident * c->P.shard_pixels : n_slots;   // launch-grid size of the camera-ray kernel = the most paths ever resident
    b.count = c->cfg.count_traversal != 0;
    if (sd.kind == Kind::MediaStreams) {
        int rl = ensure_media_buffers(c, L); if (rl != VPT_OK) return rl;
        if (frames > L.media_frames) return fail(c, VPT_ERR_DEVICE, "internal: media batch larger than the media streams");
    }
    if (sd.kind == Kind::StagedR1) { int rl = ensure_legacy_buffers(c, L); if (rl != VPT_OK) return rl; }
    if (sd.kind == Kind::StreamsSorted) { int rl = ensure_sorted_buffers(c, L); if (rl != VPT_OK) return rl; }
    b.min_bounces = (uint64_t)c->P.max_depth * c->P.samples_per_frame;
    b.iter_cap = (b.min_bounces * 4ull + 1024ull) * ((frames + sd.resident - 1) / sd.resident);
    if (n_slots == 0) return VPT_OK;
    HIPCHK(c, hipMemsetAsync(L.ctr, 0, offsetof(Counters, stat_closest), s));  // queue words only, stat_* keep running
    const DeviceScene dsc = lane_scene(c, L);
    if (sd.kind == Kind::Whole) {  // the batch's paths from camera ray to their end, one launch per part; no queue is written, alive3[] stays 0 for the resolve's guard
        b.parity = 1; b.k3 = 1; b.iter = 1;
        const bool dealt = !wrect.all, split = c->P.split > 1;
        const cull::Packed rect = cull::pack(wrect);
        for (uint32_t i = 0; i < sd.parts.n; i++) {
            // a part's launch indices: its frames' samples — those inside the rectangle, where there is one; the others are the constant the launch adds
            // to its closest-hit rays (parts are counted in frames, and a split-screen batch is never split into parts: path_plan.hpp decide)
            const uint32_t first = sd.parts.first[i], part_frames = sd.parts.n > 1u ? sd.parts.first[i + 1] - first : frames;
            const uint32_t part_slots = sd.parts.n > 1u ? part_frames * c->P.shard_pixels : n_slots;
            const deal::Deal dl = dealt ? deal::make(wrect, c->P.shard_rank, c->P.shard_count, c->P.width, part_slots) : deal::Deal{};
            const uint32_t n_part = !dealt ? part_slots : split ? n_split_dealt : part_frames * dl.rect_px;
            const uint64_t culled = part_slots - n_part;
            // The zero frame sums of the samples outside: the launch's waves write them, in runs, as they deal the rows of the rectangle (whole_deal.hpp
            // run_after).  Where no wave does — the rectangle holds none of this context's samples (n_part == 0), or split-screen dispatch, whose chunks have
            // no such runs — a fill of the part's sums does.  A part without a sample inside is still launched, one block with no index to deal: its one
            // lane adds the part's culled rays on the device, so a replayed graph (enqueue_graph) counts them in every replay as it counts every other ray.
            if (dealt && (n_part == 0u || split)) HIPCHK(c, hipMemsetAsync(part_state(c, L, first).ACC, 0, (size_t)(split ? frames * c->P.shard_pixels : part_slots) * 16, s));
            const uint32_t grid = std::max(1u, std::min<uint32_t>((uint32_t)std::min(c->whole_blocks, b.primary_grid), (n_part + 255u) / 256u));   // (blocks of 256 lanes)
            // tiles of 64 samples: `rounds` per wave; mode 0: the first round static, mode 1: all but the last, mode 2: half of them; the rest through the counter
            const uint32_t n_waves = grid * 4u, rounds = ((n_part + 63u) / 64u) / n_waves, mode = c->lab_whole_sched >> 4;
            const uint32_t static_rounds = (mode == 0u || mode == 3u) ? std::min(rounds, 1u) : mode == 1u ? (rounds >= 2u ? rounds - 1u : 0u) : rounds / 2u;
            // (mode 3: mode 0 with guided chunks — at most the given tiles per atomic, fewer towards the end of the batch)
            if (i) HIPCHK(c, hipMemsetAsync(&L.ctr->extend_head, 0, 4, s));   // the tile cursor starts at 0 in every part
            TIMED(c, s, VPT_K_PRIMARY, launch_whole(s, grid, b.count, dsc, c->P, part_state(c, L, first), L.ctr, n_part, dispatch_base + first, c->scene_plain, static_rounds, std::max(1u, c->lab_whole_sched & 15u) | (mode == 3u ? 0x100u : 0u) | (c->lab_narrow_off ? kWholeNarrowOff : 0u), rect, dl, culled));
            if (i + 1u < sd.parts.n) {   // this part's resolve on the second stream, beside the next part's launch (the last part's: batch_resolve)
                HIPCHK(c, hipEventRecord(L.ev_shade, s));
                HIPCHK(c, hipStreamWaitEvent(L.stream2, L.ev_shade, 0));
                resolve_part(c, L, b, i, L.stream2);
            }
        }
    } else if (sd.kind == Kind::Fused) {  // bounce 0 of every slot needs no input records; survivors land in queue[1]
        TIMED(c, s, VPT_K_PRIMARY, launch_bounce(s, (uint32_t)b.primary_grid, c->lds_scene, b.count, true, dsc, c->P, L.ps, L.ss, nullptr, L.queue[1], L.ctr, 0u, b.n_first, dispatch_base, 0u, c->scene_plain));
        b.parity = 1; b.k3 = 1; b.iter = 1;
    } else if (plan::runs_streams(sd.kind)) {
        TIMED(c, s, VPT_K_PRIMARY, launch_raygen_stream(s, c->P, L.ps, L.ss, L.queue[0], b.n_first, dispatch_base, sd.kind == Kind::MediaStreams));
        launch_stream_begin(s, L.sctr, b.n_first, n_slots);
        b.parity = 0;
    } else {
#if VPT_LAB
        TIMED(c, s, VPT_K_PRIMARY, launch_raygen(s, c->P, L.ps, L.queue[0], L.ctr, n_slots, dispatch_base));
#endif
        b.parity = 0;
    }
    return VPT_OK;
}

int batch_bounces(vpt_ctx* c, Lane& L, BatchState& b, uint32_t bounces) {
    hipStream_t s = L.stream;
    const Kind kind = b.sd.kind;
    const bool count = b.count, sorted = kind == Kind::StreamsSorted, overlap = b.sd.overlap, stream = plan::runs_streams(kind);
    uint32_t& parity = b.parity;
    const uint32_t n_slots = b.n_first;   // (upper bound of a queue's live entries)
    if (n_slots == 0 || kind == Kind::Whole) return VPT_OK;   // (a whole-path batch has no bounces left to launch)
    const DeviceScene dsc = lane_scene(c, L);
    for (uint32_t j = 0; j < bounces; j++) {
        b.iter++;
        if (kind == Kind::Fused) {  // no reset kernel in between: the bounce kernels rotate three queue-size words
            const int grid = (b.tail_grid > 0 && b.iter >= 3) ? b.tail_grid : b.primary_grid;   // (b.iter counts bounce 0)
            TIMED(c, s, VPT_K_BOUNCE, launch_bounce(s, (uint32_t)grid, c->lds_scene, count, false, dsc, c->P, L.ps, L.ss, L.queue[parity], L.queue[parity ^ 1u], L.ctr, parity, 0u, 0u, b.k3, c->scene_plain));
            parity ^= 1u; b.k3 = (b.k3 + 1u) % 3u;
            continue;
        }
        // a memory-resident BVH runs the staged pipeline on the vote-scheduled traversal kernels and compact streams
        // (kernels_trace.hip, kernels_stream.hip) — a scene that rides in LDS and is forced into the staged pipeline too; round 1's
        // stage kernels serve VPT_PIPELINE_STAGED_R1 only
        if (kind == Kind::MediaStreams) {   // distance -> scatter -> extend -> shade -> sky rays, light rays -> tail (kernels_media.hip), one stream
            launch_prepare_stream(s, L.sctr, parity);
            TraceArgs a{};
            a.ro = L.ss.RA[parity]; a.rd = L.ss.RB[parity]; a.order = nullptr; a.valid = L.queue[parity]; a.hit = L.ss.SH; a.hinst = L.ss.SHI; a.cls = nullptr;
            a.n = 0; a.n_dev = &L.sctr->queue_len[parity].v; a.store_gid = 1u; a.param = c->vote_param;
            // GetDistanceToGeometry (RTCommon.slang:86-101): the payload direction as it is, TMin 1e-5, TMax 1e6
            a.head = &L.sctr->shade_head.v; a.tmin = 0.00001f; a.tmax = 1000000.0f; a.normalize_dir = 0u;
            if (!(c->P.flags & VPT_FLAG_RAY_QUERIES)) { a.tmax = 1000.0f; a.normalize_dir = 1u; }   // RTCommon.slang:103-117
            TIMED(c, s, VPT_K_EXTEND, launch_trace(s, (uint32_t)c->vote_blocks, VPT_TRACE_VOTE, false, count, dsc, a, L.ctr));
            TIMED(c, s, VPT_K_SHADE, launch_media_scatter(s, (uint32_t)c->shade_blocks, dsc, L.ps, L.ss, L.ms, L.queue[parity], L.sctr, parity));
            a.head = &L.sctr->extend_head.v; a.tmin = 0.01f; a.tmax = 100000.0f; a.normalize_dir = 1u;
            TIMED(c, s, VPT_K_EXTEND, launch_trace(s, (uint32_t)c->vote_blocks, VPT_TRACE_VOTE, false, count, dsc, a, L.ctr));
            launch_layout_media(s, L.sctr, parity, (uint32_t)c->shade_media_blocks * 4u, (uint32_t)c->media_tail_blocks * 4u);
            TIMED(c, s, VPT_K_SHADE, launch_shade_media(s, (uint32_t)c->shade_media_blocks, dsc, c->P, L.ps, L.ss, L.ms, L.queue[parity], L.ctr, L.sctr, parity));
            TIMED(c, s, VPT_K_SHADOW, launch_trace_shadow(s, (uint32_t)c->shadow_blocks, false, count, dsc, L.ss, L.ctr, L.sctr, c->vote_param, (c->P.flags & VPT_FLAG_RAY_QUERIES) ? 1u : 0u));
            TIMED(c, s, VPT_K_SHADOW, launch_trace_shadow(s, (uint32_t)c->shadow_blocks, true, count, dsc, L.ss, L.ctr, L.sctr, c->vote_param, (c->P.flags & VPT_FLAG_RAY_QUERIES) ? 1u : 0u));
            TIMED(c, s, VPT_K_JOIN, launch_media_tail(s, (uint32_t)c->media_tail_blocks, dsc, c->P, L.ps, L.ss, L.ms, L.queue[parity], L.queue[parity ^ 1u], L.ctr, L.sctr, parity));
            parity ^= 1u;
            continue;
        }
        if (stream && b.finished) continue;   // k_finish has been enqueued: nothing is alive behind it
        if (stream && b.sd.finish_at != 0u && b.iter > b.sd.finish_at) {   // (b.iter counts this bounce): the rest of the batch in one launch
            if (b.join_pending) { HIPCHK(c, hipStreamWaitEvent(s, L.ev_join, 0)); b.join_pending = false; }   // pathLight of the queue's entries is final behind the previous join
            TIMED(c, s, VPT_K_BOUNCE, launch_finish(s, (uint32_t)c->finish_blocks, count, dsc, c->P, L.ps, L.ss, L.queue[parity], L.sctr, L.ctr, parity));
            b.finished = true;
            continue;
        }
        if (stream) {   // stream pipeline: extend -> classify -> shade per class (streams out) -> sky rays, light rays -> join
            launch_prepare_stream(s, L.sctr, parity);
            TraceArgs a{};
            a.ro = L.ss.RA[parity]; a.rd = L.ss.RB[parity]; a.order = nullptr; a.valid = L.queue[parity]; a.hit = L.ss.SH; a.hinst = L.ss.SHI; a.cls = L.cls_q;
            a.n = 0; a.n_dev = &L.sctr->queue_len[parity].v; a.head = &L.sctr->extend_head.v;
            a.tmin = 0.01f; a.tmax = 100000.0f; a.normalize_dir = 1u; a.store_gid = 1u; a.param = c->vote_param;
            if (!sorted) a.cls = nullptr;
            TIMED(c, s, VPT_K_EXTEND, launch_trace(s, (uint32_t)c->vote_blocks, VPT_TRACE_VOTE, false, count, dsc, a, L.ctr));
            // the shade stage of this bounce overwrites the pending records and shadow-ray streams the join of the previous
            // bounce reads (overlapped mode: that join runs on the second stream, beside the extend launched above)
            if (overlap && b.join_pending) { HIPCHK(c, hipStreamWaitEvent(s, L.ev_join, 0)); b.join_pending = false; }
            if (sorted) {   // the shade queue sorted by material class: one dense queue and one launch per class present in the scene
                TIMED(c, s, VPT_K_SHADE, launch_classify(s, L.queue[parity], L.cls_q, L.class_queue, L.sctr, parity, n_slots + L.stream_slack, (uint32_t)c->shade_stream_blocks * 4u));
                for (uint32_t k = 0; k < kShadeClasses; k++)
                    if (c->class_present & (1u << k))
                        TIMED(c, s, VPT_K_SHADE, launch_shade_stream(s, (uint32_t)c->shade_stream_blocks, k, true, dsc, c->P, L.ps, L.ss, L.queue[parity], L.class_queue[k], L.queue[parity ^ 1u], L.ctr, L.sctr, parity));
            } else {
                launch_layout_single(s, L.sctr, parity, (uint32_t)c->shade_stream_blocks * 4u);
                TIMED(c, s, VPT_K_SHADE, launch_shade_stream(s, (uint32_t)c->shade_stream_blocks, 0u, false, dsc, c->P, L.ps, L.ss, L.queue[parity], nullptr, L.queue[parity ^ 1u], L.ctr, L.sctr, parity));
            }
            hipStream_t sb = s;
            DeviceScene dsc_shadow = dsc;
            if (overlap) {   // shadow rays and join of this bounce on the second stream: the next bounce's extend does not depend on them
                HIPCHK(c, hipEventRecord(L.ev_shade, s));
                HIPCHK(c, hipStreamWaitEvent(L.stream2, L.ev_shade, 0));
                sb = L.stream2;
                dsc_shadow.stack_overflow = L.spill2;   // its own stack spill region: it runs beside the next extend
            }
            // regeneration: fresh camera rays into the room the ended paths left in the next queue (entries behind the ones the join of this
            // bounce addresses, so it may run beside the shadow kernels and the join)
            if (b.sd.regen) TIMED(c, s, VPT_K_PRIMARY, launch_refill(s, 2048u, c->P, L.ps, L.ss, L.queue[parity ^ 1u], L.sctr, parity ^ 1u, b.n_first, b.dispatch_base));
            TIMED(c, s, VPT_K_SHADOW, launch_trace_shadow(sb, (uint32_t)c->shadow_blocks, false, count, dsc_shadow, L.ss, L.ctr, L.sctr, c->vote_param, (c->P.flags & VPT_FLAG_RAY_QUERIES) ? 1u : 0u));
            TIMED(c, s, VPT_K_SHADOW, launch_trace_shadow(sb, (uint32_t)c->shadow_blocks, true, count, dsc_shadow, L.ss, L.ctr, L.sctr, c->vote_param, (c->P.flags & VPT_FLAG_RAY_QUERIES) ? 1u : 0u));
            TIMED(c, s, VPT_K_JOIN, launch_join(sb, (uint32_t)c->join_blocks, c->P, L.ps, L.ss, L.sctr, L.queue[parity], L.queue[parity ^ 1u], parity));
            if (overlap) { HIPCHK(c, hipEventRecord(L.ev_join, L.stream2)); b.join_pending = true; }
            parity ^= 1u;
            continue;
        }
#if VPT_LAB
        launch_prepare(s, L.ctr, parity);
        TIMED(c, s, VPT_K_EXTEND, launch_extend(s, (uint32_t)c->trav_blocks, c->lds_scene, count, dsc, L.ps, L.queue[parity], L.ctr, parity));
        TIMED(c, s, VPT_K_SHADE, launch_shade(s, (uint32_t)c->shade_blocks, dsc, c->P, L.ps, L.queue[parity], L.queue[parity ^ 1u], L.cqueue, L.ctr, parity));
        TIMED(c, s, VPT_K_CONNECT, launch_connect(s, (uint32_t)c->trav_blocks, c->lds_scene, count, dsc, c->P, L.ps, L.cqueue, L.ctr, parity));
#endif
        parity ^= 1u;
    }
    return VPT_OK;
}

// The resolve rides right behind the bounces that are expected to be the last ones; it does nothing if a path is still alive
// (in-medium walks do not consume depth), in which case more bounces and another resolve follow.  Behind it the counters travel to
// pinned host memory, for whoever synchronises next.
int batch_resolve(vpt_ctx* c, Lane& L, BatchState& b) {
    hipStream_t s = L.stream;
    if (b.n_slots == 0) return VPT_OK;
#if VPT_LAB
    if (b.sd.kind == Kind::StagedR1) launch_fold(s, L.ctr);
#endif
    if (b.sd.overlap && b.join_pending) { HIPCHK(c, hipStreamWaitEvent(s, L.ev_join, 0)); b.join_pending = false; }   // the resolve reads the frame sums the join writes
    const bool stream = plan::runs_streams(b.sd.kind);
    if (b.sd.parts.n > 1u) {   // the last part's resolve follows the others', which went to the second stream (batch_begin)
        HIPCHK(c, hipEventRecord(L.ev_join, L.stream2));
        HIPCHK(c, hipStreamWaitEvent(s, L.ev_join, 0));
    }
    resolve_part(c, L, b, b.sd.parts.n - 1u, s);
    HIPCHK(c, hipMemcpyAsync(&L.h_ctr->ctr, L.ctr, sizeof(Counters), hipMemcpyDeviceToHost, s));
    if (stream) {  // the exact number of live paths, and the queue length (holes included), which must fit the queue allocation
        HIPCHK(c, hipMemcpyAsync(&L.h_ctr->alive[0], &L.sctr->alive[b.parity].v, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(&L.h_ctr->queue_len[0], &L.sctr->queue_len[b.parity].v, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(&L.h_ctr->refill_next, &L.sctr->refill_next, 4, hipMemcpyDeviceToHost, s));
    }
    return VPT_OK;
}

// The device-side ray statistics are running totals per lane (Counters::stat_*), copied to pinned memory behind every resolve.
void update_ray_stats(vpt_ctx* c) {
    unsigned long long v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < kLanes; k++)
        if (const Lane* L = c->lane(k)) {
            const Counters& h = L->h_ctr->ctr;
            v[0] += h.stat_closest; v[1] += h.stat_shadow; v[2] += h.stat_connect; v[3] += h.stat_primary_hits; v[4] += h.stat_primary_alive; v[5] += h.stat_primary_rays;
            v[6] += h.stat_finish_paths; v[7] += h.stat_finish_closest; v[8] += h.stat_finish_shadow;
        }
    c->stats.closest_rays = v[0]; c->stats.shadow_rays = v[1]; c->stats.connect_paths = v[2];
    c->stats.primary_hits = v[3]; c->stats.primary_survivors = v[4]; c->stats.primary_shadow_rays = v[5];
    c->stats.finish_paths = v[6]; c->stats.finish_closest_rays = v[7]; c->stats.finish_shadow_rays = v[8];
}

// Host synchronisation: statistics, overflow checks, *alive = paths of the batch still in flight.
int batch_check(vpt_ctx* c, Lane& L, BatchState& b, uint32_t* alive) {
    *alive = 0;
    if (b.n_slots == 0) return VPT_OK;
    HIPCHK(c, hipStreamSynchronize(L.stream));
    collect_timing(c);
    const Counters& h = L.h_ctr->ctr;
    update_ray_stats(c);
    const bool counted = c->cfg.count_traversal != 0;   // (the finisher and the fused kernel on a tree in memory always count: reported only when asked for, so the figures are never partial)
    c->stats.nodes_visited = counted ? h.stat_nodes : 0;
    c->stats.tris_tested = counted ? h.stat_tris : 0;
    c->stats.shadow_nodes_visited = counted ? h.stat_shadow_nodes : 0;
    c->stats.shadow_tris_tested = counted ? h.stat_shadow_tris : 0;
    uint32_t n = plan::runs_fused(b.sd.kind) ? h.alive3[b.k3] : h.ray_count[b.parity];
    if (plan::runs_streams(b.sd.kind)) {
        n = L.h_ctr->alive[0];
        const uint64_t len = L.h_ctr->queue_len[0];
        const uint64_t room = b.sd.kind == Kind::MediaStreams ? (uint64_t)L.media_frames * c->P.shard_pixels + L.stream_slack : (uint64_t)L.ps.capacity + L.stream_slack;
        if (len > room || len > (uint64_t)L.ps.capacity + L.stream_slack) { (void)hipStreamSynchronize(L.stream2); return fail(c, VPT_ERR_DEVICE, "internal: stream overflow"); }
    }
    if (n > b.n_first) { (void)hipStreamSynchronize(L.stream2); return fail(c, VPT_ERR_DEVICE, "internal: queue overflow"); }
    if (n != 0 && b.iter > b.iter_cap) { (void)hipStreamSynchronize(L.stream2); return fail(c, VPT_ERR_DEVICE, "internal: bounce loop did not terminate"); }
    *alive = n;
    return VPT_OK;
}

// Runs a begun batch to its end: resolve + check, and while paths are alive four more bounces at a time.
int batch_finish(vpt_ctx* c, Lane& L, BatchState& b, bool resolve_enqueued) {
    while (true) {
        if (!resolve_enqueued) { int rc = batch_resolve(c, L, b); if (rc) return rc; }
        resolve_enqueued = false;
        uint32_t n = 0;
        int rc = batch_check(c, L, b, &n);
        if (rc) return rc;
        if (n == 0) break;
        // few paths left — and, in a regenerating batch, no sample left to start: the next launch finishes them
        if (b.sd.finisher && (!b.sd.regen || L.h_ctr->refill_next >= b.n_slots) && !b.finished && b.sd.finish_at == 0u && n < plan::kFinishBelowPaths) b.sd.finish_at = (uint32_t)b.iter;
        rc = batch_bounces(c, L, b, b.sd.regen ? 8u : 4u);   // (a regenerating batch runs many more launches than max_depth: fewer host round trips)
        if (rc) return rc;
    }
    HIPCHK(c, hipGetLastError());
    return VPT_OK;
}

int render_batch(vpt_ctx* c, uint32_t frames, uint32_t dispatch_base) {
    Lane& L = c->main;
    plan::Schedule sd;
    int rc = decide_batch(c, L, facts_of(c), frames, dispatch_base, false, sd);
    if (rc) return rc;
    BatchState b;
    rc = batch_begin(c, L, sd, frames, dispatch_base, Grids{c->primary_blocks, 0}, b);
    if (rc) return rc;
    if (b.n_slots == 0) return VPT_OK;
    // the host looks at the queue after max_depth bounces (when a surface-only batch is done) or after eight, whichever comes first
    const uint32_t first = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(b.min_bounces - (plan::runs_fused(sd.kind) ? 1 : 0), 1), 8);
    rc = batch_bounces(c, L, b, first);
    if (rc) return rc;
    rc = batch_finish(c, L, b, false);
    if (rc) return rc;
    c->stats.samples += (uint64_t)b.n_slots * c->P.samples_per_frame;
    return VPT_OK;
}

// ---- asynchronous batches: a batch enqueued whole, as plain launches or through a captured graph
// A whole batch as a fixed schedule: bounce 0 (or the camera rays) and `bounces_total` bounces in all; the guarded resolve is the caller's.
int enqueue_fixed(vpt_ctx* c, Lane& L, const plan::Schedule& sd, uint32_t frames, uint32_t dispatch_base, uint32_t bounces_total, Grids grids, BatchState& b) {
    int rc = batch_begin(c, L, sd, frames, dispatch_base, grids, b);
    if (rc) return rc;
    if (b.n_slots == 0) return VPT_OK;
    return batch_bounces(c, L, b, plan::runs_fused(sd.kind) ? bounces_total - 1u : bounces_total);
}
// The same through a captured hipGraph: the fused pipeline's batch (memset, bounce 0, bounces) with the first dispatch index read from
// device memory, captured once per (state, frames, bounces) — grids included — and replayed.  b: the batch as it stands before its resolve.
// The captured batch is decided for ONE stream (no shadow / join overlap on stream2).
int enqueue_graph(vpt_ctx* c, Lane& L, const plan::Facts& f, uint32_t frames, uint32_t dispatch_base, uint32_t bounces_total, Grids grids, bool* used, BatchState& b) {
    *used = false;
    if (L.graph_broken) return VPT_OK;
    if (!L.graph || L.graph_gen != c->state_gen || L.graph_frames != frames || L.graph_bounces != bounces_total) {
        destroy_graph(L);
        uint64_t before[VPT_KERNEL_COUNT];
        memcpy(before, c->stats.kernel_launches, sizeof(before));
        c->P.dispatch_base_dev = L.d_dispatch_base;
        hipGraph_t g = nullptr;
        bool ok = hipStreamBeginCapture(L.stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
        plan::Schedule sd;
        int rc = ok ? decide_batch(c, L, f, frames, 0u, true, sd) : VPT_ERR_DEVICE;
        if (rc == VPT_OK) rc = enqueue_fixed(c, L, sd, frames, 0u, bounces_total, grids, L.graph_batch);
        if (ok && hipStreamEndCapture(L.stream, &g) != hipSuccess) { ok = false; g = nullptr; }
        c->P.dispatch_base_dev = nullptr;
        for (int k = 0; k < VPT_KERNEL_COUNT; k++) { L.graph_kernel_launches[k] = c->stats.kernel_launches[k] - before[k]; c->stats.kernel_launches[k] = before[k]; }
        if (ok && rc == VPT_OK && g && hipGraphInstantiate(&L.graph, g, nullptr, nullptr, 0) != hipSuccess) { ok = false; L.graph = nullptr; }
        if (g) (void)hipGraphDestroy(g);
        if (!ok || rc != VPT_OK || !L.graph) {   // capture is an optimisation: without it the batch goes out as plain launches
            (void)hipGetLastError();
            destroy_graph(L);
            L.graph_broken = true;
            c->err.clear();
            return VPT_OK;
        }
        L.graph_gen = c->state_gen; L.graph_frames = frames; L.graph_bounces = bounces_total;
    }
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)L.d_dispatch_base, (int)dispatch_base, 1, L.stream));
    HIPCHK(c, hipGraphLaunch(L.graph, L.stream));
    for (int k = 0; k < VPT_KERNEL_COUNT; k++) c->stats.kernel_launches[k] += L.graph_kernel_launches[k];
    c->stats.graph_launches++;
    b = L.graph_batch;
    b.dispatch_base = dispatch_base;
    *used = true;
    return VPT_OK;
}

// The next batch of a render call: how many dispatches it takes (PathTrace's accounting), with the path buffers grown to hold them.
// *nf == 0: max_samples reached (PathTrace returns true and launches nothing).
int next_batch(vpt_ctx* c, uint32_t left, uint32_t* nf) {
    *nf = 0;
    if (c->samples_accum >= c->params.max_samples) return VPT_OK;   // PathTracer.cpp:124-125
    // dispatches until PathTrace would return true: samples = floor(dispatches / S^2) * spp (PathTracer.cpp:151-153)
    const uint64_t S2 = (uint64_t)c->params.screen_chunk_count * c->params.screen_chunk_count;
    const uint64_t frames_needed = ((uint64_t)c->params.max_samples + c->params.samples_per_frame - 1) / c->params.samples_per_frame;
    const uint64_t disp_left = frames_needed * S2 - c->dispatch_count;
    uint32_t n = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(left, batch_cap(c)), disp_left);
    if (!path_buffers_hold(c, n)) {   // the buffers grow to the largest batch asked for (and to the words it touches); nothing may be in flight while they are replaced
        int rc = drain(c);
        if (rc) return rc;
        if ((rc = ensure_path_buffers(c, n))) return rc;
    }
    n = plan::fit_batch(policy_of(c), plan_state(c), n);
    if (plan::media_on_streams(facts_of(c))) {   // media on the streams: the batch is what the media streams hold
        int rm = ensure_media_buffers(c, c->main);
        if (rm) return rm;
        n = std::min(n, c->main.media_frames);
    }
    *nf = n;
    return VPT_OK;
}
void advance_counts(vpt_ctx* c, uint32_t nf) {
    const uint64_t S2 = (uint64_t)c->params.screen_chunk_count * c->params.screen_chunk_count;
    c->dispatch_count += nf;
    c->frame_count = (uint32_t)(c->dispatch_count / S2);
    c->samples_accum = c->frame_count * c->params.samples_per_frame;
    c->full_valid = false;
}

}  // namespace

// ---- helpers the other api_*.hip files call too (declared in api_ctx.hpp)
namespace vpt {
namespace api {

// The scene as a launch on lane L reads it: the context's tables, the lane's own spill region.
DeviceScene lane_scene(const vpt_ctx* c, const Lane& L) {
    DeviceScene d = c->dsc;
    d.stack_overflow = L.spill;
    return d;
}
cull::Rect whole_cull_rect(const vpt_ctx* c) {
    cull::WorldBox box = c->whole_box;
    box.valid = box.valid && c->has_scene && c->lab_whole_cull && c->cfg.count_traversal == 0;   // (k_whole's counting instantiations have no test: kernels_whole.hip)
    return cull::screen_bound(c->P.view_inv, c->P.proj_inv, c->P.width, c->P.height, c->P.focus_distance, c->P.dof_strength, c->P.flags, c->dsc.env_black != 0u, box);
}

// ---- asynchronous batches: tickets, and what waits for them
// The ticket of everything enqueued up to here; `on`: the stream the latest of it went to (vpt_wait).
uint64_t issue_ticket(vpt_ctx* c, hipStream_t on) {
    c->tick_issued++;
    (void)hipEventRecord(c->tick_ev[c->tick_issued % kTickets], on);
    c->async_dirty = true;
    return c->tick_issued;
}
// An enqueued batch whose paths may outlive the bounces enqueued with it (always on the main lane): finish it exactly as render_batch would have.
int finish_outstanding(vpt_ctx* c) {
    if (!c->out_active) return VPT_OK;
    c->out_active = false;
    return batch_finish(c, c->main, c->out_batch, true);
}
// Everything enqueued so far — on every lane — has finished when this returns (and an unfinished batch has been finished).
int drain(vpt_ctx* c) {
    int rc = finish_outstanding(c);
    if (rc) return rc;
    if (!c->async_dirty) return VPT_OK;
    c->async_dirty = false;
    for (int k = 0; k < kLanes; k++) {
        Lane* L = c->lane(k);
        if (!L) continue;
        HIPCHK(c, hipStreamSynchronize(L->stream));
        if (!L->last_fixed_valid) continue;
        L->last_fixed_valid = false;   // a fixed-schedule batch: nothing may have outlived it (its guarded resolve would have been a no-op)
        const BatchState& f = L->last_fixed;
        if (plan::runs_streams(f.sd.kind)) {
            if (L->h_ctr->alive[0] != 0u) return fail(c, VPT_ERR_DEVICE, "internal: a path outlived a fixed-schedule batch");
            if ((uint64_t)L->h_ctr->queue_len[0] > (uint64_t)L->ps.capacity + L->stream_slack) return fail(c, VPT_ERR_DEVICE, "internal: stream overflow");
        } else if (plan::runs_fused(f.sd.kind) && L->h_ctr->ctr.alive3[f.k3] != 0u) return fail(c, VPT_ERR_DEVICE, "internal: a path outlived a fixed-schedule batch");
    }
    c->order_lane = nullptr; c->post_pending = false;
    HIPCHK(c, hipStreamSynchronize(c->main.stream2));
    collect_timing(c);
    update_ray_stats(c);   // fixed-schedule batches copy their counters to pinned memory too
    HIPCHK(c, hipGetLastError());
    return VPT_OK;
}
// What every entry that replaces something batches in flight read begins with: the context's device current, nothing in flight.
int quiesce(vpt_ctx* c) {
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return drain(c);
}

}  // namespace api
}  // namespace vpt

extern "C" {

int vpt_render(vpt_ctx* c, uint32_t dispatches, int* done) {
    if (!c) return VPT_ERR_INVALID_ARGUMENT;
    if (!c->has_scene) return fail(c, VPT_ERR_NO_SCENE, "vpt_render before vpt_set_scene");
    if (!c->buffers_ok) return fail(c, VPT_ERR_DEVICE, "no render buffers: the last vpt_resize failed");
    { int rd = quiesce(c); if (rd) return rd; }
    if (done) *done = 0;
    uint32_t left = dispatches;
    while (left > 0) {
        uint32_t nf = 0;
        int rc = next_batch(c, left, &nf);
        if (rc) return rc;
        if (nf == 0) { if (done) *done = 1; break; }
        rc = render_batch(c, nf, (uint32_t)c->dispatch_count);  // returns with the stream drained
        if (rc) return rc;
        advance_counts(c, nf);
        left -= nf;
    }
    return VPT_OK;
}

// PathTrace(cmd) as the reference has it: recorded, not waited for (include/vpt.h).
int vpt_render_async(vpt_ctx* c, uint32_t dispatches, int* done, uint64_t* ticket) {
    if (!c) return VPT_ERR_INVALID_ARGUMENT;
    if (!c->has_scene) return fail(c, VPT_ERR_NO_SCENE, "vpt_render_async before vpt_set_scene");
    if (!c->buffers_ok) return fail(c, VPT_ERR_DEVICE, "no render buffers: the last vpt_resize failed");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (done) *done = 0;
    uint32_t left = dispatches;
    while (left > 0) {
        int rc = finish_outstanding(c);   // the path buffers are single: an unfinished batch goes first
        if (rc) return rc;
        uint32_t nf = 0;
        if ((rc = next_batch(c, left, &nf))) return rc;
        if (nf == 0) { if (done) *done = 1; break; }
        const uint32_t base = (uint32_t)c->dispatch_count;
        if (c->graph_streak_gen == c->state_gen) c->graph_streak++; else { c->graph_streak = 0; c->graph_streak_gen = c->state_gen; }
        const plan::Facts f = facts_of(c);
        plan::Schedule sd;
        if ((rc = decide_batch(c, c->main, f, nf, base, false, sd))) return rc;
        const plan::AsyncShape shape = plan::async_shape(f, sd, nf, c->main.resident_alloc, c->graph_streak);
        const bool fixed = shape.fixed;
        const uint32_t enq = shape.bounces_to_enqueue;
        // the fixed 1-frame batch goes to the next lane (vpt_ctx::main / extra); asked for again with nothing changed since the last two calls it
        // is replayed from the lane's captured graph
        Lane* X = &c->main;
        if (shape.lanes_ok) {
            const int max_lanes = (int)std::max(1u, std::min(c->lab_lanes, (uint32_t)kLanes));
            Lane* idle = nullptr;   // the first lane whose previous frame has been resolved
            uint32_t have = 0;
            for (int k = 0; k < max_lanes; k++) {
                Lane* L = c->lane(k);
                if (!L) { if (!idle) idle = get_lane(c, k); break; }   // every existing lane is busy: one more
                have++;
                if (!idle && hipEventQuery(L->ev_resolved) == hipSuccess) idle = L;
            }
            (void)hipGetLastError();   // (hipErrorNotReady is not an error)
            if (!idle) idle = c->lane((int)(c->lane_rr++ % have));   // all lanes busy: round robin
            X = idle;
            if (X != &c->main) {   // the same decision on the lane's own buffers
                if ((rc = ensure_lane_buffers(c, *X))) return rc;
                if ((rc = decide_batch(c, *X, f, nf, base, false, sd))) return rc;
            }
        }
        // a batch on the main lane behind pipelined frames: their resolves come first (frame order), and the records it overwrites are the main lane's own
        if (X == &c->main && c->order_lane && c->order_lane != X) HIPCHK(c, hipStreamWaitEvent(X->stream, c->order_lane->ev_resolved, 0));
        BatchState b;
        bool graphed = false;
        // Frames in steady accumulation share the chip: each lane's kernels take a third of the persistent grid (one block per CU of the
        // three the fused kernel's LDS allows), so that the three lanes' chains are co-resident and the tail of one frame — launches that are
        // bounded by one bounce's latency, not by throughput — runs beside the first bounces of the next two.  (A full-size grid fills every
        // CU's LDS and keeps the other lanes' blocks out until it retires.)
        Grids grids{c->primary_blocks, 0};
        auto part = [&](uint32_t div) { return std::max(c->cu_count, (c->primary_blocks / (int)std::max(1u, div) / std::max(c->cu_count, 1)) * c->cu_count); };
        if (shape.partial_grids) {
            grids.primary = part(std::max(1u, c->lab_lane_grid));
            grids.tail = c->lab_tail_grid > 1u ? std::min(grids.primary, part(c->lab_tail_grid)) : 0;
        }
        if (shape.graph_ok && (rc = enqueue_graph(c, *X, f, nf, base, enq, grids, &graphed, b))) return rc;
        if (!graphed && (rc = enqueue_fixed(c, *X, sd, nf, base, enq, grids, b))) return rc;
        if (fixed && b.n_slots) {   // frames resolve in order: this one's resolve waits for the previous frame's, whichever lane that ran on
            if (c->order_lane && c->order_lane != X) HIPCHK(c, hipStreamWaitEvent(X->stream, c->order_lane->ev_resolved, 0));
            if (c->post_pending && X != &c->main) HIPCHK(c, hipStreamWaitEvent(X->stream, c->ev_post, 0));   // ... and for the post-process that is still reading the image
        }
        if ((rc = batch_resolve(c, *X, b))) return rc;
        if (fixed && b.n_slots) {
            HIPCHK(c, hipEventRecord(X->ev_resolved, X->stream));
            c->order_lane = X;
            X->last_fixed = b; X->last_fixed_valid = true;
        }
        c->stats.samples += (uint64_t)b.n_slots * c->P.samples_per_frame;
        advance_counts(c, nf);
        left -= nf;
        const uint64_t t = issue_ticket(c, X->stream);
        if (!fixed && b.n_slots) { c->out_active = true; c->out_batch = b; c->out_ticket = t; }
    }
    if (ticket) *ticket = c->tick_issued;
    return VPT_OK;
}

int vpt_wait(vpt_ctx* c, uint64_t ticket) {
    if (!c) return VPT_ERR_INVALID_ARGUMENT;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (ticket == 0 || ticket >= c->tick_issued) return drain(c);
    if (c->out_active && c->out_ticket <= ticket) { int rc = finish_outstanding(c); if (rc) return rc; }
    // the events are reused round-robin and recorded in stream order: the latest record of ticket's event belongs to a ticket >= it
    HIPCHK(c, hipEventSynchronize(c->tick_ev[ticket % kTickets]));
    return VPT_OK;
}

int vpt_get_radiance_device(vpt_ctx* c, void* dst) {
    if (!c || !dst) return VPT_ERR_INVALID_ARGUMENT;
    if (!c->buffers_ok) return fail(c, VPT_ERR_DEVICE, "no render buffers: the last vpt_resize failed");
    if (c->P.shard_count > 1 && !c->full_valid) return fail(c, VPT_ERR_INVALID_ARGUMENT, "sharded context: call vpt_assemble_shards first");
    { int rd = quiesce(c); if (rd) return rd; }
    HIPCHK(c, hipMemcpyAsync(dst, whole_image(c), (size_t)c->P.width * c->P.height * 16, hipMemcpyDeviceToDevice, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return VPT_OK;
}
int vpt_get_radiance(vpt_ctx* c, float* dst) {
    if (!c || !dst) return VPT_ERR_INVALID_ARGUMENT;
    if (!c->buffers_ok) return fail(c, VPT_ERR_DEVICE, "no render buffers: the last vpt_resize failed");
    if (c->P.shard_count > 1 && !c->full_valid) return fail(c, VPT_ERR_INVALID_ARGUMENT, "sharded context: call vpt_assemble_shards first");
    { int rd = quiesce(c); if (rd) return rd; }
    HIPCHK(c, hipMemcpy(dst, whole_image(c), (size_t)c->P.width * c->P.height * 16, hipMemcpyDeviceToHost));
    return VPT_OK;
}
int vpt_set_radiance(vpt_ctx* c, const float* src, uint32_t frame_count) {
    if (!c || !src) return VPT_ERR_INVALID_ARGUMENT;
    if (!c->buffers_ok) return fail(c, VPT_ERR_DEVICE, "no render buffers: the last vpt_resize failed");
    { int rd = quiesce(c); if (rd) return rd; }
    const uint32_t W = c->P.width;
    if (c->P.shard_count == 1) {
        HIPCHK(c, hipMemcpy(c->image, src, (size_t)W * c->P.height * 16, hipMemcpyHostToDevice));
    } else {
        HIPCHK(c, hipMemcpy(c->full_image, src, (size_t)W * c->P.height * 16, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy2D(c->image, (size_t)W * 16, src + (size_t)c->P.shard_rank * W * 4, (size_t)W * 16 * c->P.shard_count, (size_t)W * 16,
                              c->P.shard_rows, hipMemcpyHostToDevice));
        c->full_valid = true;
    }
    c->frame_count = frame_count;
    c->dispatch_count = (uint64_t)frame_count * c->params.screen_chunk_count * c->params.screen_chunk_count;
    c->samples_accum = frame_count * c->params.samples_per_frame;
    c->tp_history = false;   // the image is the caller's now: no temporal history describes it
    return VPT_OK;
}

int vpt_get_stats(vpt_ctx* c, vpt_stats* out) {
    if (!c || !out) return VPT_ERR_INVALID_ARGUMENT;
    if (c->async_dirty || c->out_active) {
        HIPCHK(c, hipSetDevice(c->cfg.device));
        int rd = drain(c); if (rd) return rd;
    }
    vpt_stats s = c->stats;
    s.frames = c->frame_count; s.dispatches = c->dispatch_count;
    s.total_vertex_count = c->total_vertices; s.total_index_count = c->total_indices;
    s.bvh_nodes = c->dsc.node_count; s.bvh_triangles = c->dsc.tri_count;
    s.bvh_node_bytes = c->lds_scene ? sizeof(BvhNodeWide) : sizeof(BvhNode); s.bvh_tri_bytes = sizeof(BvhTri);
    s.emissive_mesh_count = (uint32_t)c->emissive.list.size(); s.emissive_triangle_count = c->emissive.tris;
    s.frames_in_flight = batch_cap(c); s.shard_pixels = c->P.shard_pixels;   // (the largest batch the context renders at once with its current scene and parameters)
    s.build_flags = (c->sbvh ? VPT_BUILD_SBVH : 0u) | (c->cfg.build_flags & (VPT_BUILD_GENERAL_KERNELS | VPT_BUILD_STREAMS_ONLY));
    s.frames_allocated = c->main.frames_alloc; s.resident_frames = c->main.resident_alloc;
    s.set_scene_ms = c->set_scene_ms; s.bvh_build_ms = c->bvh_build_ms; s.set_environment_ms = c->set_environment_ms;
    // what the traversal kernels have written into their spill regions: counted when something has run since the last count (the scan reads
    // ~0.4 GB: a host that asks for the statistics after every frame would otherwise pay 0.1-0.2 ms per call for a number that does not change)
    if (c->has_scene && c->main.spill && c->spill_dirty) {
        HIPCHK(c, hipSetDevice(c->cfg.device));
        unsigned long long h[2] = {0ull, 0ull};
        HIPCHK(c, hipMemsetAsync(c->d_spill_count, 0, 16, c->main.stream));
        for (int k = 0; k < kLanes; k++) {   // first figure: every lane's region (the extra lanes': pipelined asynchronous frames), second: the main lane's second-stream region
            const Lane* L = c->lane(k);
            if (!L || !L->spill) continue;
            launch_count_spilled(c->main.stream, L->spill, L->stack_overflow_words, c->d_spill_count);
            if (L->spill2 != L->spill) launch_count_spilled(c->main.stream, L->spill2, L->stack_overflow_words, c->d_spill_count + 1);
        }
        HIPCHK(c, hipMemcpyAsync(h, c->d_spill_count, 16, hipMemcpyDeviceToHost, c->main.stream));
        HIPCHK(c, hipStreamSynchronize(c->main.stream));
        c->spill_cached[0] = h[0]; c->spill_cached[1] = h[1];
        c->spill_dirty = false;
    }
    s.stack_spills[0] = c->has_scene ? c->spill_cached[0] : 0; s.stack_spills[1] = c->has_scene ? c->spill_cached[1] : 0;
    *out = s;
    return VPT_OK;
}
int vpt_get_set_transforms_ms(const vpt_ctx* c, double* out_ms) {
    if (!c || !out_ms) return VPT_ERR_INVALID_ARGUMENT;
    *out_ms = c->set_transforms_ms;
    return VPT_OK;
}
int vpt_reset_stats(vpt_ctx* c) {
    if (!c) return VPT_ERR_INVALID_ARGUMENT;
    { int rd = quiesce(c); if (rd) return rd; }
    c->stats = vpt_stats{};
    for (int k = 0; k < kLanes; k++)
        if (Lane* L = c->lane(k)) { HIPCHK(c, memset_now(L->stream, L->ctr, 0, sizeof(Counters))); memset(L->h_ctr, 0, sizeof(HostCounters)); }
    return VPT_OK;
}

int vpt_get_whole_cull(const vpt_ctx* c, uint32_t* rect) {
    if (!c || !rect) return VPT_ERR_INVALID_ARGUMENT;
    if (!c->has_scene) return VPT_ERR_NO_SCENE;
    const cull::Rect r = whole_cull_rect(c);
    rect[0] = r.x0; rect[1] = r.y0; rect[2] = r.x1; rect[3] = r.y1;
    return VPT_OK;
}

}  // extern "C"
