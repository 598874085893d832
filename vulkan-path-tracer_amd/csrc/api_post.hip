// api_post.hip — the image passes that run behind a render, each as a blocking entry and a _device entry queued behind the frames in flight:
//   vpt_postprocess           the bloom chain + tonemap and the RGBA8 output: the mips' sizes and the schedule are post_plan.hpp's, enqueue_post meters the
//                             exposure and then issues one launch (kernels_post.hip) per step of the plan
//   vpt_denoise               the edge-avoiding a-trous filter over first-hit guides, variance-guided with vpt_svgf_options.variance
//   vpt_temporal_accumulate   the image carried across camera and instance moves: the two records, SVGF's luminance moments and variance, the per-instance
//                             motion tables and the motion image, with their options and read-backs
//   vpt_set_firefly_options   outlier rejection ahead of the two calls above: enqueue_firefly queues k_firefly between their guides and their own first launch
#include "api_ctx.hpp"

using namespace vpt::api;

// ---- helpers of this file alone
namespace {

int ensure_post_buffers(vpt_ctx* c) {
    const uint32_t w = c->P.width, h = c->P.height;
    if (c->post_w == w && c->post_h == h && !c->mips.empty()) return VPT_OK;
    for (float* m : c->mips) (void)hipFree(m);
    c->mips.clear();
    if (c->post_out) (void)hipFree(c->post_out);
    c->post_out = nullptr;
    c->mip_dims = post::mips_of(w, h);
    for (uint32_t i = 0; i < c->mip_dims.count; i++) {
        float* m = nullptr;
        HIPCHK(c, hipMalloc((void**)&m, (size_t)c->mip_dims.texels(i) * 16));
        c->mips.push_back(m);
    }
    HIPCHK(c, hipMalloc((void**)&c->post_out, (size_t)w * h * 4));
    c->post_w = w; c->post_h = h;
    return VPT_OK;
}

// PostProcessor::PostProcess, PostProcessor.cpp:193-246: the launches, on the context's stream, nothing waited for.
int enqueue_post(vpt_ctx* c, const vpt_post_params* pp, bool bloom0) {
    int rc = ensure_post_buffers(c);
    if (rc) return rc;
    hipStream_t s = c->main.stream;
    const float* hdr = c->post_source == VPT_POST_SOURCE_DENOISED ? c->dn_out : whole_image(c);   // (post_source_ready has been asked)
    const uint32_t W = c->P.width, H = c->P.height;
    const bool linear_tap = (c->params.flags & VPT_FLAG_TONEMAP_LINEAR_BLOOM_TAP) != 0;
    // Auto-exposure: the source image is metered before bloom and the tonemap kernels read the adapted scale from the device — nothing is read back or
    // waited for.  The two launches are timed with the tonemap.
    const float* scale = nullptr;
    if (c->ex_options.mode) {
        if (!c->ex_dev) {
            HIPCHK(c, hipMalloc((void**)&c->ex_dev, sizeof(ExposureDevice)));
            HIPCHK(c, hipMemsetAsync(c->ex_dev, 0, sizeof(ExposureDevice), s));
        }
        const exposure::Plan plan = exposure::plan_of(c->ex_options);
        TIMED(c, s, VPT_K_TONEMAP, launch_luminance_histogram(s, hdr, W * H, plan, c->ex_dev));
        TIMED(c, s, VPT_K_TONEMAP, launch_exposure_adapt(s, plan, c->ex_reset, c->ex_dev));
        c->ex_reset = exposure::kResetNone; c->ex_metered = true;
        scale = &c->ex_dev->state.scale;
    }
    // Which launches, on which levels, is post_plan.hpp's decision: one launch per step, in the plan's order.
    const post::Mips& m = c->mip_dims;
    float* const* mips = c->mips.data();
    const post::Plan plan = pp->schedule == VPT_POST_REFERENCE_PASSES ? post::reference_plan(m, pp->mip_count) : post::fused_plan(m, pp->mip_count);
    auto launch = [&](const post::Step& st) {
        const uint32_t f = st.first, n = st.count;
        switch (st.kind) {
        case post::kThreshold: launch_bloom_threshold(s, hdr, mips[0], W, H, pp->bloom_threshold, pp->falloff_range); break;
        case post::kDownFirst: launch_bloom_down_first(s, hdr, W, H, mips[1], m.w[1], m.h[1], pp->bloom_strength, pp->bloom_threshold, pp->falloff_range); break;
        case post::kDown: launch_bloom_down(s, mips[f - 1], m.w[f - 1], m.h[f - 1], mips[f], m.w[f], m.h[f], pp->bloom_strength); break;
        case post::kDownChain: launch_bloom_down_chain(s, mips, m, f, n, pp->bloom_strength); break;
        case post::kTail: launch_bloom_tail(s, mips, m, f, n, st.staged != 0, pp->bloom_strength); break;
        case post::kUp: launch_bloom_up(s, mips[f + 1], m.w[f + 1], m.h[f + 1], mips[f], m.w[f], m.h[f], pp->bloom_strength); break;
        case post::kUpChain: launch_bloom_up_chain(s, mips, m, f, n, pp->bloom_strength); break;
        case post::kFinal:   // n == 1: mip 1 is up-sampled inside the launch; bloom0: the caller wants mip 0, which nothing else materialises
            launch_post_final(s, hdr, n ? mips[1] : nullptr, n ? m.w[1] : 0u, n ? m.h[1] : 0u, bloom0 ? mips[0] : nullptr, c->post_out, W, H, pp->bloom_threshold,
                              pp->falloff_range, pp->bloom_strength, pp->exposure, pp->gamma, linear_tap, scale);
            break;
        case post::kTonemap: launch_tonemap(s, hdr, mips[0], c->post_out, W, H, pp->exposure, pp->gamma, linear_tap, scale); break;
        }
    };
    for (uint32_t i = 0; i < plan.n; i++) TIMED(c, s, plan.steps[i].kind < post::kFinal ? VPT_K_BLOOM : VPT_K_TONEMAP, launch(plan.steps[i]));
    return VPT_OK;
}
// A temporal result / a denoised image of the current size exists: not before the first call, and not after a resize.
bool temporal_ready(const vpt_ctx* c) { return c->tp_valid && c->tp_w == c->P.width && c->tp_h == c->P.height; }
bool denoised_ready(const vpt_ctx* c) { return c->dn_valid && c->dn_w == c->P.width && c->dn_h == c->P.height; }
int post_preconditions(vpt_ctx* c) {
    if (!c->buffers_ok) return fail(c, VPT_ERR_DEVICE, "no render buffers: the last vpt_resize failed");
    if (c->P.shard_count > 1 && !c->full_valid) return fail(c, VPT_ERR_INVALID_ARGUMENT, "sharded context: call vpt_assemble_shards first");
    return VPT_OK;
}
// VPT_POST_SOURCE_DENOISED needs a denoised image of the current size: never denoised, or resized since, is the caller's error.
int post_source_ready(vpt_ctx* c) {
    if (c->post_source == VPT_POST_SOURCE_DENOISED && !denoised_ready(c))
        return fail(c, VPT_ERR_INVALID_ARGUMENT, "post source is the denoised image and there is none of this size: call vpt_denoise first");
    return VPT_OK;
}

// ---- vpt_firefly_options: the pass ahead of a filter.  *image is the filter's source on entry; with the option on, k_firefly is queued on it — reading the
// consuming call's guides, which enqueue_first_hit has just queued — and *image becomes the filtered copy.  The source itself is never written.
bool firefly_ready(const vpt_ctx* c) { return c->ff_valid && c->ff_w == c->P.width && c->ff_h == c->P.height; }
int enqueue_firefly(vpt_ctx* c, const float** image, const float* albedo, const float* depth, bool demodulate) {
    if (!c->ff_options.mode) return VPT_OK;
    const uint32_t w = c->P.width, h = c->P.height;
    const size_t npx = (size_t)w * h;
    if (!(c->ff_block && c->ff_w == w && c->ff_h == h)) {
        if (c->ff_block) (void)hipFree(c->ff_block);
        c->ff_block = nullptr; c->ff_valid = false;
        HIPCHK(c, hipMalloc((void**)&c->ff_block, npx * 16 + firefly::kCounterBytes));   // the image, then the counter pairs
        c->ff_w = w; c->ff_h = h;
    }
    uint32_t* counters = (uint32_t*)(c->ff_block + npx * 4);
    const vpt_firefly_options& o = c->ff_options;
    HIPCHK(c, hipMemsetAsync(counters, 0, firefly::kCounterBytes, c->main.stream));
    launch_firefly(c->main.stream, *image, demodulate ? albedo : nullptr, depth, c->ff_block, counters, w, h, firefly::plan_of(o.radius, o.rank, o.threshold, o.floor, demodulate));
    *image = c->ff_block;
    c->ff_valid = true; c->ff_calls++;
    return VPT_OK;
}

// ---- vpt_denoise
int check_denoise(vpt_ctx* c, const vpt_denoise_params* dp, const void* device_out) {
    if (!c || !dp) return VPT_ERR_INVALID_ARGUMENT;
    if (dp->iterations > VPT_DENOISE_MAX_ITERATIONS) return fail(c, VPT_ERR_INVALID_ARGUMENT, "more than VPT_DENOISE_MAX_ITERATIONS iterations");
    if (!(dp->sigma_color > 0.0f) || !(dp->sigma_normal > 0.0f) || !(dp->sigma_depth > 0.0f)) return fail(c, VPT_ERR_INVALID_ARGUMENT, "every sigma must be > 0");
    if (dp->flags & ~VPT_DENOISE_DEMODULATE) return fail(c, VPT_ERR_INVALID_ARGUMENT, "unknown denoise flag bits");
    if (((uintptr_t)device_out & 15u) != 0u) return fail(c, VPT_ERR_INVALID_ARGUMENT, "the device image must be 16-byte aligned");
    if (!c->has_scene) return fail(c, VPT_ERR_NO_SCENE, "no scene");
    if (c->denoise_source == VPT_DENOISE_SOURCE_TEMPORAL && !temporal_ready(c))
        return fail(c, VPT_ERR_INVALID_ARGUMENT, "denoise source is the temporal image and there is none of this size: call vpt_temporal_accumulate first");
    if (c->denoise_source == VPT_DENOISE_SOURCE_TEMPORAL && c->svgf.variance && !c->sv_valid)
        return fail(c, VPT_ERR_INVALID_ARGUMENT, "the variance-guided filter needs a temporal result made with vpt_svgf_options.variance == 1");
    return post_preconditions(c);
}
int ensure_denoise_buffers(vpt_ctx* c) {
    const uint32_t w = c->P.width, h = c->P.height;
    if (c->dn_block && c->dn_w == w && c->dn_h == h) return VPT_OK;
    free_denoise_buffers(c);
    const size_t npx = (size_t)w * h;
    HIPCHK(c, hipMalloc((void**)&c->dn_block, npx * (5 * 16 + 4)));   // five RGBA32F images, then the depths: every image 16-byte aligned
    float* p = c->dn_block;
    c->dn_guide = p; c->dn_albedo = p + npx * 4; c->dn_ping = p + npx * 8; c->dn_pong = p + npx * 12; c->dn_out = p + npx * 16; c->dn_depth = p + npx * 20;
    c->dn_w = w; c->dn_h = h;
    return VPT_OK;
}
// Guides, prepare, passes: the launches on the main lane's stream, nothing waited for.  The image is whole_image(c) as the stream finds it.
int enqueue_denoise(vpt_ctx* c, const vpt_denoise_params* dp) {
    int rc = ensure_denoise_buffers(c);
    if (rc) return rc;
    hipStream_t s = c->main.stream;
    const uint32_t W = c->P.width, H = c->P.height;
    const float* src = c->denoise_source == VPT_DENOISE_SOURCE_TEMPORAL ? c->tp_out : whole_image(c);   // (check_denoise has asked for it)
    if (dp->iterations == 0) {
        HIPCHK(c, hipMemcpyAsync(c->dn_out, src, (size_t)W * H * 16, hipMemcpyDeviceToDevice, s));
    } else {
        const bool demodulate = (dp->flags & VPT_DENOISE_DEMODULATE) != 0;
        const bool variance = c->denoise_source == VPT_DENOISE_SOURCE_TEMPORAL && c->svgf.variance != 0u;   // (check_denoise: the variance image is there)
        FirstHitArgs a{};
        a.n = ((W + 7u) / 8u) * ((H + 7u) / 8u) * 64u;
        a.mode = VPT_FEATURES_CENTER;
        a.depth = c->dn_depth; a.normal = (float4*)c->dn_guide; a.albedo = (float4*)c->dn_albedo;
        enqueue_first_hit(c, a);
        // (the temporal image was filtered ahead of the history: not again)
        if (c->denoise_source == VPT_DENOISE_SOURCE_RADIANCE && (rc = enqueue_firefly(c, &src, c->dn_albedo, c->dn_depth, demodulate))) return rc;
        launch_denoise_prepare(s, src, c->dn_depth, c->dn_albedo, c->dn_guide, c->dn_ping, W, H, demodulate, variance ? c->sv_variance : nullptr);
        const float* in = c->dn_ping;
        for (uint32_t i = 0; i < dp->iterations; i++) {
            const bool last = i + 1 == dp->iterations;
            float* out = last ? c->dn_out : (in == c->dn_ping ? c->dn_pong : c->dn_ping);
            launch_denoise_atrous(s, in, c->dn_guide, c->dn_albedo, out, W, H, denoise::pass_of(i, dp->sigma_color, dp->sigma_normal, dp->sigma_depth), last && demodulate,
                                  variance, c->svgf.sigma_luminance, last);
            in = out;
        }
    }
    c->dn_valid = true;
    return VPT_OK;
}

// ---- vpt_temporal_accumulate
int check_temporal(vpt_ctx* c, const vpt_temporal_params* tp, const void* device_out) {
    if (!c || !tp) return VPT_ERR_INVALID_ARGUMENT;
    if (tp->max_history == 0u) return fail(c, VPT_ERR_INVALID_ARGUMENT, "max_history must be >= 1");
    if (!(tp->depth_tolerance > 0.0f)) return fail(c, VPT_ERR_INVALID_ARGUMENT, "depth_tolerance must be > 0");
    if (!(tp->normal_threshold >= -1.0f && tp->normal_threshold <= 1.0f)) return fail(c, VPT_ERR_INVALID_ARGUMENT, "normal_threshold must be in [-1, 1]");
    if (tp->flags & ~(VPT_TEMPORAL_DEMODULATE | VPT_TEMPORAL_MATCH_INSTANCE)) return fail(c, VPT_ERR_INVALID_ARGUMENT, "unknown temporal flag bits");
    if (tp->reserved[0] | tp->reserved[1]) return fail(c, VPT_ERR_INVALID_ARGUMENT, "reserved words must be 0");
    if (((uintptr_t)device_out & 15u) != 0u) return fail(c, VPT_ERR_INVALID_ARGUMENT, "the device image must be 16-byte aligned");
    if (!c->has_scene) return fail(c, VPT_ERR_NO_SCENE, "no scene");
    int rc = post_preconditions(c);
    if (rc) return rc;
    if (c->frame_count == 0u) return fail(c, VPT_ERR_INVALID_ARGUMENT, "nothing rendered since the last reset: there are no new samples to blend in");
    return VPT_OK;
}
int ensure_temporal_buffers(vpt_ctx* c) {
    const uint32_t w = c->P.width, h = c->P.height;
    if (c->tp_block && c->tp_w == w && c->tp_h == h) return VPT_OK;
    free_temporal_buffers(c);   // (the moments, the motion image and tables were made for the old size too)
    const size_t npx = (size_t)w * h;
    HIPCHK(c, hipMalloc((void**)&c->tp_block, npx * (7 * 16 + 3 * 4)));   // seven 16-byte images first (every one 16-byte aligned), then the three of one word
    float* p = c->tp_block;
    c->tp_out = p; c->tp_hist[0] = p + npx * 4; c->tp_hist[1] = p + npx * 8; c->tp_guide[0] = p + npx * 12; c->tp_guide[1] = p + npx * 16;
    c->tp_albedo = p + npx * 20; c->tp_ids = (uint32_t*)(p + npx * 24);
    c->tp_depth = p + npx * 28; c->tp_inst[0] = (uint32_t*)(p + npx * 29); c->tp_inst[1] = (uint32_t*)(p + npx * 30);
    c->tp_w = w; c->tp_h = h;
    return VPT_OK;
}
// The luminance moments and the variance image, 20 B per pixel, for the size tp_block was made for: only ever with vpt_svgf_options.variance == 1.
int ensure_variance_buffers(vpt_ctx* c) {
    if (c->sv_block) return VPT_OK;
    const size_t npx = (size_t)c->tp_w * c->tp_h;
    HIPCHK(c, hipMalloc((void**)&c->sv_block, npx * (2 * 8 + 4)));
    c->sv_moments[0] = c->sv_block; c->sv_moments[1] = c->sv_block + npx * 2; c->sv_variance = c->sv_block + npx * 4;
    return VPT_OK;
}
// vpt_temporal_options.instance_motion == 1: the motion image, 8 B per pixel of the size tp_block was made for ...
int ensure_motion_image(vpt_ctx* c) {
    if (c->tp_motion) return VPT_OK;
    HIPCHK(c, hipMalloc((void**)&c->tp_motion, (size_t)c->tp_w * c->tp_h * 8));
    return VPT_OK;
}
// ... and, when an instance's matrix differs from the one it had at the previous record, the per-instance records: built on the host, into the table the
// previous call did not read (that call's k_temporal may still be queued), by a copy in the main stream's order.  *table stays nullptr when nothing moved.
int upload_motion_table(vpt_ctx* c, bool have_prev, const temporal::InstanceMotion** table) {
    *table = nullptr;
    const uint32_t n = (uint32_t)c->instances.size();
    const uint32_t k = c->tp_motion_latest ^ 1u;
    if (!have_prev || n == 0u || !c->tp_snapshot.table(n, c->instances[0].xform, sizeof(InstanceDesc), c->tp_motion_host[k])) return VPT_OK;
    if (c->tp_motion_cap < n) {
        HIPCHK(c, hipStreamSynchronize(c->main.stream));   // (a queued k_temporal may read the tables freed here: they go only behind it)
        for (int j = 0; j < 2; j++) {
            if (c->tp_motion_table[j]) (void)hipFree(c->tp_motion_table[j]);
            c->tp_motion_table[j] = nullptr;
        }
        c->tp_motion_cap = 0;
        HIPCHK(c, hipMalloc((void**)&c->tp_motion_table[0], (size_t)n * sizeof(temporal::InstanceMotion)));
        HIPCHK(c, hipMalloc((void**)&c->tp_motion_table[1], (size_t)n * sizeof(temporal::InstanceMotion)));
        c->tp_motion_cap = n;
    }
    HIPCHK(c, hipMemcpyAsync(c->tp_motion_table[k], c->tp_motion_host[k].data(), (size_t)n * sizeof(temporal::InstanceMotion), hipMemcpyHostToDevice, c->main.stream));
    c->tp_motion_latest = k;
    *table = c->tp_motion_table[k];
    return VPT_OK;
}
// Guides into the new record, k_temporal against the previous one: the launches on the main lane's stream, nothing waited for.  The image is
// whole_image(c) as the stream finds it; m is the frame count as the host has it now.  Nothing of the context changes before the last launch is queued.
int enqueue_temporal(vpt_ctx* c, const vpt_temporal_params* tp) {
    int rc = ensure_temporal_buffers(c);
    if (rc) return rc;
    const bool variance = c->svgf.variance != 0u;
    if (variance && (rc = ensure_variance_buffers(c))) return rc;
    const bool motion = c->tp_options.instance_motion != 0u;
    const bool history = c->tp_valid && c->tp_history;
    const temporal::InstanceMotion* motion_table = nullptr;
    if (motion && (rc = ensure_motion_image(c))) return rc;
    if (motion && (rc = upload_motion_table(c, history && c->tp_camera.ok, &motion_table))) return rc;
    const uint32_t W = c->P.width, H = c->P.height;
    const uint32_t prev = c->tp_latest, next = prev ^ 1u;
    FirstHitArgs a{};
    a.n = ((W + 7u) / 8u) * ((H + 7u) / 8u) * 64u;
    a.mode = VPT_FEATURES_CENTER;
    a.depth = c->tp_depth; a.normal = (float4*)c->tp_guide[next]; a.albedo = (float4*)c->tp_albedo; a.ids = (uint4*)c->tp_ids;
    enqueue_first_hit(c, a);
    temporal::Frame f{};
    memcpy(f.view_inv, c->P.view_inv, 64); memcpy(f.proj_inv, c->P.proj_inv, 64);
    f.width = W; f.height = H; f.focus_distance = c->P.focus_distance; f.dof_strength = c->P.dof_strength;
    f.prev = c->tp_camera;
    f.have_prev = (history && c->tp_camera.ok) ? 1u : 0u;
    f.m = (float)c->frame_count; f.max_history = (float)tp->max_history;
    f.depth_tolerance = tp->depth_tolerance; f.normal_threshold = tp->normal_threshold; f.flags = tp->flags;
    const float* cur = whole_image(c);
    if ((rc = enqueue_firefly(c, &cur, c->tp_albedo, c->tp_depth, (tp->flags & VPT_TEMPORAL_DEMODULATE) != 0))) return rc;
    launch_temporal(c->main.stream, cur, c->tp_depth, c->tp_albedo, c->tp_ids, c->tp_hist[prev], c->tp_guide[prev], c->tp_inst[prev],
                    c->tp_hist[next], c->tp_guide[next], c->tp_inst[next], c->tp_out, f, variance ? c->sv_moments[prev] : nullptr, variance ? c->sv_moments[next] : nullptr,
                    variance ? c->sv_variance : nullptr, (float)c->svgf.min_history * f.m, motion_table, (uint32_t)c->instances.size(), motion ? c->tp_motion : nullptr);
    if (variance && c->sv_spatial.mode)   // the young pixels' variance from their neighbourhood, on the record just written: the variance image alone changes
        launch_variance_spatial(c->main.stream, c->tp_guide[next], c->sv_moments[next], c->tp_hist[next], c->sv_variance, W, H,
                                svgf_spatial::plan_of(c->sv_spatial.radius, c->sv_spatial.sigma_normal, c->sv_spatial.sigma_depth, c->sv_spatial.min_weight), (float)c->svgf.min_history * f.m);
    c->tp_camera = temporal::prev_camera_of(c->P.view_inv, c->P.proj_inv);
    c->tp_snapshot.clear();   // the new record was made with the matrices the instances have now
    c->tp_latest = next; c->tp_valid = true; c->tp_history = true; c->sv_valid = variance; c->tp_motion_valid = motion;
    return VPT_OK;
}

// ---- what the entry points share around their enqueue_* call (`enqueue`: that call, returning its error code)
// A blocking entry: every frame in flight drained first, the pass waited for.  timing: its launches go to the kernel statistics (vpt_postprocess).
template <class Enqueue>
int run_blocking(vpt_ctx* c, Enqueue enqueue, bool timing = false) {
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc = drain(c);
    if (rc || (rc = enqueue())) return rc;
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    if (timing) collect_timing(c);
    HIPCHK(c, hipGetLastError());
    return VPT_OK;
}
// A _device entry: the pass goes behind the frames in flight on the context's stream and nothing is waited for; the next frame's resolve waits for ev_post
// (the pass reads the image).  With dst, `bytes` of the context's image `src` are copied there behind the pass: src is read after the enqueue, which
// allocates it on its first call.
template <class Enqueue, class T>
int run_behind_frames(vpt_ctx* c, Enqueue enqueue, void* dst, T* vpt_ctx::*src, size_t bytes, uint64_t* ticket) {
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc = finish_outstanding(c);   // the image must be complete: an unfinished batch is finished first
    if (rc) return rc;
    if (c->order_lane && c->order_lane != &c->main) HIPCHK(c, hipStreamWaitEvent(c->main.stream, c->order_lane->ev_resolved, 0));   // the latest frame was resolved on another lane
    if ((rc = enqueue())) return rc;
    if (dst) HIPCHK(c, hipMemcpyAsync(dst, c->*src, bytes, hipMemcpyDeviceToDevice, c->main.stream));
    HIPCHK(c, hipEventRecord(c->ev_post, c->main.stream));
    c->post_pending = true;
    const uint64_t t = issue_ticket(c, c->main.stream);
    if (ticket) *ticket = t;
    return VPT_OK;
}
// A read-back: nothing in flight and the main stream idle, so a blocking copy finds what the latest pass left.
int settle_for_readback(vpt_ctx* c, bool set_device = true) {
    if (set_device) HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc = quiesce(c);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return VPT_OK;
}
// The moment record (two floats per pixel) or the variance image (one) of the latest temporal result, which must have been made with the option on.
int read_variance_result(vpt_ctx* c, float* host, bool moments) {
    if (!c || !host) return VPT_ERR_INVALID_ARGUMENT;
    if (!(temporal_ready(c) && c->sv_valid)) return fail(c, VPT_ERR_INVALID_ARGUMENT, "no temporal result of this size made with vpt_svgf_options.variance == 1");
    int rc = settle_for_readback(c);
    if (rc) return rc;
    const size_t npx = (size_t)c->tp_w * c->tp_h;
    HIPCHK(c, hipMemcpy(host, moments ? c->sv_moments[c->tp_latest] : c->sv_variance, npx * (moments ? 8 : 4), hipMemcpyDeviceToHost));
    return VPT_OK;
}

}  // namespace

extern "C" {

void vpt_default_temporal_params(vpt_temporal_params* p) {
    if (p) *p = vpt_temporal_params{32u, 0.02f, 0.9f, VPT_TEMPORAL_DEMODULATE | VPT_TEMPORAL_MATCH_INSTANCE, {0u, 0u}};
}
int vpt_temporal_accumulate(vpt_ctx* c, const vpt_temporal_params* tp, float* rgba_host) {
    int rc = check_temporal(c, tp, nullptr);
    if (rc || (rc = run_blocking(c, [&] { return enqueue_temporal(c, tp); }))) return rc;
    if (rgba_host) HIPCHK(c, hipMemcpy(rgba_host, c->tp_out, (size_t)c->tp_w * c->tp_h * 16, hipMemcpyDeviceToHost));
    return VPT_OK;
}
// Behind the frames in flight on the context's stream, like vpt_denoise_device: the next frame's resolve waits for it (it reads the image).
int vpt_temporal_accumulate_device(vpt_ctx* c, const vpt_temporal_params* tp, void* rgba_device, uint64_t* ticket) {
    int rc = check_temporal(c, tp, rgba_device);
    if (rc) return rc;
    return run_behind_frames(c, [&] { return enqueue_temporal(c, tp); }, rgba_device, &vpt_ctx::tp_out, (size_t)c->P.width * c->P.height * 16, ticket);
}
int vpt_temporal_reset(vpt_ctx* c) {
    if (!c) return VPT_ERR_INVALID_ARGUMENT;
    c->tp_history = false;   // (the latest result stays readable)
    return VPT_OK;
}
int vpt_get_temporal_history(vpt_ctx* c, float* length_host) {
    if (!c || !length_host) return VPT_ERR_INVALID_ARGUMENT;
    if (!temporal_ready(c)) return fail(c, VPT_ERR_INVALID_ARGUMENT, "no temporal result of this size: call vpt_temporal_accumulate first");
    int rc = settle_for_readback(c);
    if (rc) return rc;
    const size_t npx = (size_t)c->tp_w * c->tp_h;
    std::vector<float> rec(npx * 4);   // (r, g, b, length) per pixel
    HIPCHK(c, hipMemcpy(rec.data(), c->tp_hist[c->tp_latest], npx * 16, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < npx; i++) length_host[i] = rec[i * 4 + 3];
    return VPT_OK;
}
// ---- SVGF's variance: options, and the two read-backs of the latest temporal result made with them
void vpt_default_svgf_options(vpt_svgf_options* o) {
    if (o) *o = vpt_svgf_options{0u, 4.0f, 4u, 0u};
}
int vpt_set_svgf_options(vpt_ctx* c, const vpt_svgf_options* o) {
    if (!c || !o) return VPT_ERR_INVALID_ARGUMENT;
    if (o->variance > 1u) return fail(c, VPT_ERR_INVALID_ARGUMENT, "variance must be 0 or 1");
    if (!(o->sigma_luminance > 0.0f)) return fail(c, VPT_ERR_INVALID_ARGUMENT, "sigma_luminance must be > 0");
    if (o->min_history == 0u) return fail(c, VPT_ERR_INVALID_ARGUMENT, "min_history must be >= 1");
    if (o->reserved) return fail(c, VPT_ERR_INVALID_ARGUMENT, "reserved words must be 0");
    if (o->variance != c->svgf.variance) c->tp_history = false;   // a record without moments is never read as one with them
    c->svgf = *o;
    return VPT_OK;
}
int vpt_get_svgf_options(const vpt_ctx* c, vpt_svgf_options* o) {
    if (!c || !o) return VPT_ERR_INVALID_ARGUMENT;
    *o = c->svgf;
    return VPT_OK;
}
// ---- ... and the spatial estimate for young pixels: validated and stored; enqueue_temporal acts on it.  No record is touched, so the history stays.
void vpt_default_svgf_spatial_options(vpt_svgf_spatial_options* o) {
    if (o) *o = vpt_svgf_spatial_options{0u, 3u, 0.1f, 0.05f, 4.0f, {0u, 0u, 0u}};
}
int vpt_set_svgf_spatial_options(vpt_ctx* c, const vpt_svgf_spatial_options* o) {
    if (!c || !o) return VPT_ERR_INVALID_ARGUMENT;
    const float big = 3.402823466e+38f;   // (FLT_MAX.  x <= big: finite; a NaN fails every comparison)
    if (o->mode > 1u || o->radius - 1u >= (uint32_t)svgf_spatial::kMaxRadius || !(o->sigma_normal > 0.0f && o->sigma_normal <= big) || !(o->sigma_depth > 0.0f && o->sigma_depth <= big) ||
        !(o->min_weight >= 1.0f && o->min_weight <= big) || (o->reserved[0] | o->reserved[1] | o->reserved[2]))
        return fail(c, VPT_ERR_INVALID_ARGUMENT, "svgf spatial options: mode 0 or 1, radius 1..3, finite sigmas > 0, finite min_weight >= 1, reserved words 0");
    c->sv_spatial = *o;
    return VPT_OK;
}
int vpt_get_svgf_spatial_options(const vpt_ctx* c, vpt_svgf_spatial_options* o) {
    if (!c || !o) return VPT_ERR_INVALID_ARGUMENT;
    *o = c->sv_spatial;
    return VPT_OK;
}
// ---- outlier rejection ahead of the two filters: validated and stored; enqueue_temporal and enqueue_denoise act on it.  No record is touched, so the history stays.
static_assert(sizeof(vpt_firefly_options) == sizeof(firefly::Options), "firefly.hpp mirrors include/vpt.h");
void vpt_default_firefly_options(vpt_firefly_options* o) {
    const firefly::Options d = firefly::default_options();
    if (o) memcpy(o, &d, sizeof d);
}
int vpt_set_firefly_options(vpt_ctx* c, const vpt_firefly_options* o) {
    if (!c || !o) return VPT_ERR_INVALID_ARGUMENT;
    firefly::Options n;
    memcpy(&n, o, sizeof n);
    if (const char* why = firefly::check_options(n)) return fail(c, VPT_ERR_INVALID_ARGUMENT, why);
    if (o->mode && !c->ff_options.mode) c->ff_calls = 0;
    c->ff_options = *o;
    return VPT_OK;
}
int vpt_get_firefly_options(const vpt_ctx* c, vpt_firefly_options* o) {
    if (!c || !o) return VPT_ERR_INVALID_ARGUMENT;
    *o = c->ff_options;
    return VPT_OK;
}
int vpt_get_firefly_state(vpt_ctx* c, vpt_firefly_state* out) {
    if (!c || !out) return VPT_ERR_INVALID_ARGUMENT;
    *out = vpt_firefly_state{0u, 0u, 0u, 0u};
    if (!firefly_ready(c)) return VPT_OK;
    int rc = settle_for_readback(c);
    if (rc) return rc;
    uint32_t n[firefly::kCounterSlots * firefly::kCounterStride];
    HIPCHK(c, hipMemcpy(n, c->ff_block + (size_t)c->ff_w * c->ff_h * 4, sizeof n, hipMemcpyDeviceToHost));
    out->calls = c->ff_calls;
    for (uint32_t k = 0; k < firefly::kCounterSlots; k++) { out->clamped += n[k * firefly::kCounterStride]; out->considered += n[k * firefly::kCounterStride + 1u]; }
    return VPT_OK;
}
int vpt_get_firefly_image(vpt_ctx* c, float* rgba_host) {
    if (!c || !rgba_host) return VPT_ERR_INVALID_ARGUMENT;
    if (!firefly_ready(c)) return fail(c, VPT_ERR_INVALID_ARGUMENT, "no filtered image of this size: run a filtered call with vpt_firefly_options.mode == 1 first");
    int rc = settle_for_readback(c);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(rgba_host, c->ff_block, (size_t)c->ff_w * c->ff_h * 16, hipMemcpyDeviceToHost));
    return VPT_OK;
}
int vpt_get_temporal_variance(vpt_ctx* c, float* var_host) { return read_variance_result(c, var_host, false); }
int vpt_get_temporal_moments(vpt_ctx* c, float* mu_host) { return read_variance_result(c, mu_host, true); }
// ---- moved instances: the option, and the motion image of the latest temporal result made with it
void vpt_default_temporal_options(vpt_temporal_options* o) {
    if (o) *o = vpt_temporal_options{0u, {0u, 0u, 0u}};
}
int vpt_set_temporal_options(vpt_ctx* c, const vpt_temporal_options* o) {
    if (!c || !o) return VPT_ERR_INVALID_ARGUMENT;
    if (o->instance_motion > 1u) return fail(c, VPT_ERR_INVALID_ARGUMENT, "instance_motion must be 0 or 1");
    if (o->reserved[0] | o->reserved[1] | o->reserved[2]) return fail(c, VPT_ERR_INVALID_ARGUMENT, "reserved words must be 0");
    if (o->instance_motion != c->tp_options.instance_motion) { c->tp_history = false; c->tp_snapshot.clear(); }   // no move was followed while the option was off
    c->tp_options = *o;
    return VPT_OK;
}
int vpt_get_temporal_options(const vpt_ctx* c, vpt_temporal_options* o) {
    if (!c || !o) return VPT_ERR_INVALID_ARGUMENT;
    *o = c->tp_options;
    return VPT_OK;
}
int vpt_get_temporal_motion(vpt_ctx* c, float* motion_host) {
    if (!c || !motion_host) return VPT_ERR_INVALID_ARGUMENT;
    if (!(temporal_ready(c) && c->tp_options.instance_motion && c->tp_motion_valid && c->tp_motion))
        return fail(c, VPT_ERR_INVALID_ARGUMENT, "no temporal result of this size made with vpt_temporal_options.instance_motion == 1");
    int rc = settle_for_readback(c);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(motion_host, c->tp_motion, (size_t)c->tp_w * c->tp_h * 8, hipMemcpyDeviceToHost));
    return VPT_OK;
}

int vpt_set_denoise_source(vpt_ctx* c, uint32_t source) {
    if (!c) return VPT_ERR_INVALID_ARGUMENT;
    if (source > VPT_DENOISE_SOURCE_TEMPORAL) return fail(c, VPT_ERR_INVALID_ARGUMENT, "unknown denoise source");
    c->denoise_source = source;
    return VPT_OK;
}

void vpt_default_denoise_params(vpt_denoise_params* p) {
    if (p) *p = vpt_denoise_params{5u, 1.0f, 0.1f, 0.05f, VPT_DENOISE_DEMODULATE, 0u};
}
int vpt_denoise(vpt_ctx* c, const vpt_denoise_params* dp, float* rgba_host) {
    int rc = check_denoise(c, dp, nullptr);
    if (rc || (rc = run_blocking(c, [&] { return enqueue_denoise(c, dp); }))) return rc;
    if (rgba_host) HIPCHK(c, hipMemcpy(rgba_host, c->dn_out, (size_t)c->dn_w * c->dn_h * 16, hipMemcpyDeviceToHost));
    return VPT_OK;
}
// Behind the frames in flight on the context's stream, like vpt_postprocess_device: the next frame's resolve waits for it (it reads the image).
int vpt_denoise_device(vpt_ctx* c, const vpt_denoise_params* dp, void* rgba_device, uint64_t* ticket) {
    int rc = check_denoise(c, dp, rgba_device);
    if (rc) return rc;
    return run_behind_frames(c, [&] { return enqueue_denoise(c, dp); }, rgba_device, &vpt_ctx::dn_out, (size_t)c->P.width * c->P.height * 16, ticket);
}
int vpt_set_post_source(vpt_ctx* c, uint32_t source) {
    if (!c) return VPT_ERR_INVALID_ARGUMENT;
    if (source > VPT_POST_SOURCE_DENOISED) return fail(c, VPT_ERR_INVALID_ARGUMENT, "unknown post source");
    c->post_source = source;
    return VPT_OK;
}

int vpt_postprocess(vpt_ctx* c, const vpt_post_params* pp, uint8_t* out8, float* bloom0) {
    if (!c || !pp || !out8) return VPT_ERR_INVALID_ARGUMENT;
    int rc = post_preconditions(c);
    if (rc) return rc;
    if ((rc = post_source_ready(c)) || (rc = run_blocking(c, [&] { return enqueue_post(c, pp, bloom0 != nullptr); }, true))) return rc;
    const uint32_t W = c->P.width, H = c->P.height;
    HIPCHK(c, hipMemcpy(out8, c->post_out, (size_t)W * H * 4, hipMemcpyDeviceToHost));
    if (bloom0) HIPCHK(c, hipMemcpy(bloom0, c->mips[0], (size_t)W * H * 16, hipMemcpyDeviceToHost));
    return VPT_OK;
}

// PostProcess(cmd) as the reference has it: recorded behind the render on the same stream, the RGBA8 image stays on the device.
int vpt_postprocess_device(vpt_ctx* c, const vpt_post_params* pp, void* rgba8_device, uint64_t* ticket) {
    if (!c || !pp) return VPT_ERR_INVALID_ARGUMENT;
    int rc = post_preconditions(c);
    if (rc) return rc;
    if ((rc = post_source_ready(c))) return rc;
    return run_behind_frames(c, [&] { return enqueue_post(c, pp, false); }, rgba8_device, &vpt_ctx::post_out, (size_t)c->P.width * c->P.height * 4, ticket);
}
// ---- auto-exposure: the options (context state: stored and validated here, acted on by enqueue_post) and the read-backs of the latest metering
static_assert(sizeof(vpt_exposure_options) == sizeof(exposure::Options) && sizeof(vpt_exposure_state) == sizeof(exposure::State), "exposure.hpp mirrors include/vpt.h");
void vpt_default_exposure_options(vpt_exposure_options* o) {
    const exposure::Options d = exposure::default_options();
    if (o) memcpy(o, &d, sizeof d);
}
int vpt_set_exposure_options(vpt_ctx* c, const vpt_exposure_options* o) {
    if (!c || !o) return VPT_ERR_INVALID_ARGUMENT;
    exposure::Options n;
    memcpy(&n, o, sizeof n);
    if (const char* why = exposure::check_options(n)) return fail(c, VPT_ERR_INVALID_ARGUMENT, why);
    if (n.mode != c->ex_options.mode) { c->ex_reset = exposure::kResetAll; c->ex_metered = false; }   // the adapted state belongs to one stretch of mode == 1
    c->ex_options = n;
    return VPT_OK;
}
int vpt_get_exposure_options(const vpt_ctx* c, vpt_exposure_options* o) {
    if (!c || !o) return VPT_ERR_INVALID_ARGUMENT;
    memcpy(o, &c->ex_options, sizeof *o);
    return VPT_OK;
}
int vpt_exposure_reset(vpt_ctx* c) {
    if (!c) return VPT_ERR_INVALID_ARGUMENT;
    if (c->ex_reset == exposure::kResetNone) c->ex_reset = exposure::kResetJump;
    return VPT_OK;
}
int vpt_get_exposure_state(vpt_ctx* c, vpt_exposure_state* out) {
    if (!c || !out) return VPT_ERR_INVALID_ARGUMENT;
    *out = vpt_exposure_state{1.0f, 0.0f, 0.0f, 0.0f, 0u, 0u, 0u};
    if (!c->ex_options.mode || !c->ex_metered) return VPT_OK;
    int rc = settle_for_readback(c);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(out, &c->ex_dev->state, sizeof *out, hipMemcpyDeviceToHost));
    return VPT_OK;
}
int vpt_get_exposure_histogram(vpt_ctx* c, uint32_t* out) {
    if (!c || !out) return VPT_ERR_INVALID_ARGUMENT;
    if (!c->ex_options.mode || !c->ex_metered) return fail(c, VPT_ERR_INVALID_ARGUMENT, "no metering yet: post-process with vpt_exposure_options.mode == 1 first");
    int rc = settle_for_readback(c);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(out, c->ex_dev->hist, sizeof c->ex_dev->hist, hipMemcpyDeviceToHost));
    return VPT_OK;
}

const void* vpt_output_device(vpt_ctx* c) { return c ? c->post_out : nullptr; }
int vpt_get_output(vpt_ctx* c, uint8_t* out8) {
    if (!c || !out8) return VPT_ERR_INVALID_ARGUMENT;
    if (!c->post_out) return fail(c, VPT_ERR_INVALID_ARGUMENT, "vpt_get_output before the first post-process");
    int rc = settle_for_readback(c, false);   // (the one read-back that leaves the calling thread's device as it is)
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(out8, c->post_out, (size_t)c->post_w * c->post_h * 4, hipMemcpyDeviceToHost));
    return VPT_OK;
}

}  // extern "C"
