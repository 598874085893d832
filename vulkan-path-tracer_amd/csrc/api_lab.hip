// api_lab.hip — the laboratory's entry points (include/vpt_lab.h): knobs of the pipelined lanes and the whole-path schedule, and the trace lab on a
// resident ray set.  Compiled into the laboratory library only (_build.LAB_SOURCES); the product library has none of it.
#include "api_ctx.hpp"
#include "bvh_build.hpp"

using namespace vpt::api;

extern "C" {

int vpt_lab_set(vpt_ctx* c, uint32_t key, uint32_t value) {
    if (!c || (value > 3u && key != VPT_LAB_WHOLE_FRAMES && key != VPT_LAB_WHOLE_SCHED && key != VPT_LAB_WHOLE_PARTS)) return VPT_ERR_INVALID_ARGUMENT;
    { int rd = quiesce(c); if (rd) return rd; }
    if (key == VPT_LAB_LANES && value >= 1u) c->lab_lanes = value;
    else if (key == VPT_LAB_LANE_GRID && value >= 1u) c->lab_lane_grid = value;
    else if (key == VPT_LAB_TAIL_GRID && value >= 1u) c->lab_tail_grid = value;
    else if (key == VPT_LAB_WHOLE_SCHED && (value & 15u) >= 1u && (value >> 4) <= 3u) c->lab_whole_sched = value;
    else if (key == VPT_LAB_WHOLE_FRAMES) c->lab_whole_frames = value == 0xffffu ? 0xffffffffu : value;   // (0xffff: no bound, the default)
    else if (key == VPT_LAB_WHOLE_PARTS && value <= plan::kMaxParts) c->lab_whole_parts = value;
    else if (key == VPT_LAB_WHOLE_CULL && value <= 1u) c->lab_whole_cull = value != 0u;
    else if (key == VPT_LAB_NARROW_OFF && value <= 1u) c->lab_narrow_off = value != 0u;
    else return VPT_ERR_INVALID_ARGUMENT;
    c->state_gen++;   // captured batches hold the old grids
    return VPT_OK;
}
int vpt_lab_whole_culled(const vpt_ctx* c, uint64_t* out) {
    if (!c || !out) return VPT_ERR_INVALID_ARGUMENT;
    *out = c->main.h_ctr ? c->main.h_ctr->ctr.whole_culled : 0u;   // (the counters a batch copies to pinned memory behind its resolve: batch_resolve)
    return VPT_OK;
}
// Every buffer of the resident set is kLabGuard entries longer than the set: wave.hpp fetch_chunk's largest chunk, which is as far as a fetch step that
// forgot the end of the stream could reach.  The guard holds rays a kernel can trace (zeros), entries of `order` and of the hole mask that name
// themselves, and results filled with 0xAA before every launch: a launch that leaves another byte there has worked on entries beyond n, and fails.
static constexpr uint32_t kLabGuard = 1024u;
// (vote.hpp kHole / kRayHole: what a stream entry nobody wrote holds in a ray queue / in RD.z of a shadow-ray stream)
static constexpr uint32_t kLabHole = 0xffffffffu, kLabRayHole = 0xfffffffeu;
static int guard_untouched(vpt_ctx* c, const void* dev, size_t bytes) {
    std::vector<unsigned char> g(bytes);
    HIPCHK(c, hipMemcpy(g.data(), dev, bytes, hipMemcpyDeviceToHost));
    for (unsigned char b : g) if (b != 0xAA) return fail(c, VPT_ERR_DEVICE, "the launch wrote results beyond the last ray of the set");
    return VPT_OK;
}
int vpt_lab_set_rays(vpt_ctx* c, const vpt_ray* rays, uint32_t n) {
    if (!c || !rays || n == 0 || n > 0xffffffffu - kLabGuard) return VPT_ERR_INVALID_ARGUMENT;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    free_lab(c);
    const size_t m = (size_t)n + kLabGuard;
    std::vector<float4> ro(m, make_float4(0.0f, 0.0f, 0.0f, 0.0f)), rd(m, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (uint32_t i = 0; i < n; i++) {
        ro[i] = make_float4(rays[i].origin[0], rays[i].origin[1], rays[i].origin[2], 0.0f);
        rd[i] = make_float4(rays[i].direction[0], rays[i].direction[1], rays[i].direction[2], 0.0f);
    }
    HIPCHK(c, hipMalloc((void**)&c->lab_ro, m * 16)); HIPCHK(c, hipMalloc((void**)&c->lab_rd, m * 16));
    HIPCHK(c, hipMalloc((void**)&c->lab_hit, m * 16)); HIPCHK(c, hipMalloc((void**)&c->lab_hinst, m * 4));
    HIPCHK(c, hipMalloc((void**)&c->lab_order, m * 8));   // the caller's order | the hole mask as TraceArgs::valid wants it (vpt_lab_set_holes)
    c->lab_holes.clear();
    HIPCHK(c, hipMemcpy(c->lab_ro, ro.data(), m * 16, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->lab_rd, rd.data(), m * 16, hipMemcpyHostToDevice));
    c->lab_n = n; c->lab_tmin = rays[0].tmin; c->lab_tmax = rays[0].tmax;
    return VPT_OK;
}
int vpt_lab_set_holes(vpt_ctx* c, const unsigned char* hole) {
    if (!c) return VPT_ERR_INVALID_ARGUMENT;
    if (c->lab_n == 0) return fail(c, VPT_ERR_INVALID_ARGUMENT, "vpt_lab_set_holes before vpt_lab_set_rays");
    { int rd = quiesce(c); if (rd) return rd; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    c->lab_holes.clear();
    if (!hole) return VPT_OK;
    const uint32_t n = c->lab_n;
    const size_t m = (size_t)n + kLabGuard;
    std::vector<uint32_t> valid(m);
    for (size_t i = 0; i < m; i++) valid[i] = (i < n && hole[i]) ? kLabHole : (uint32_t)i;
    HIPCHK(c, hipMemcpy(c->lab_order + m, valid.data(), m * 4, hipMemcpyHostToDevice));
    c->lab_holes.assign(hole, hole + n);
    return VPT_OK;
}
int vpt_lab_trace(vpt_ctx* c, uint32_t variant, uint32_t any_hit, const uint32_t* order, uint32_t param, uint32_t reps, vpt_hit* hits, float* best_ms,
                  uint64_t* visits) {
    if (!c || variant > VPT_TRACE_VOTE4S || reps == 0) return VPT_ERR_INVALID_ARGUMENT;
    if ((variant == VPT_TRACE_POOL || variant == VPT_TRACE_PAIR) && any_hit) return fail(c, VPT_ERR_UNSUPPORTED, "VPT_TRACE_POOL / _PAIR are closest-hit variants");
    if (!c->has_scene) return fail(c, VPT_ERR_NO_SCENE, "no scene");
    if (c->lds_scene) return fail(c, VPT_ERR_UNSUPPORTED, "the trace lab runs on scenes whose BVH lives in memory");
    if (c->lab_n == 0) return fail(c, VPT_ERR_INVALID_ARGUMENT, "vpt_lab_trace before vpt_lab_set_rays");
    { int rd = quiesce(c); if (rd) return rd; }
    if ((variant == VPT_TRACE_VOTE4S || variant == VPT_TRACE_VOTE8) && c->lab_trees_stale) return fail(c, VPT_ERR_UNSUPPORTED, "instances have moved since vpt_set_scene: this variant's tree is gone until the next one");
    if (variant == VPT_TRACE_VOTE4S && !c->dsc.nodes4s) {   // split-order experiment: the same binary tree collapsed pair-wise with order tables, over the same leaf-ordered triangles
        std::vector<BvhNode> n4, n4s; std::vector<BvhNodeWide> w4; std::vector<BvhTri> lt; int d = 0;
        BvhBuildOptions opt; opt.spatial_splits = c->sbvh; opt.nodes4s = &n4s;
        build_bvh_ex(c->bvh_input, n4, w4, lt, &d, opt);
        int rc4 = upload(c, n4s, &c->dsc.nodes4s);
        if (rc4) return rc4;
    }
    if (variant == VPT_TRACE_VOTE8 && !c->dsc.nodes8) {   // BVH8 experiment: the same binary tree collapsed eight-wide, over the same leaf-ordered triangles
        std::vector<BvhNode> n4; std::vector<BvhNodeWide> w4; std::vector<BvhTri> lt; std::vector<BvhNode8> n8; int d = 0;
        build_bvh(c->bvh_input, n4, w4, lt, &d, &n8, c->sbvh);
        if (n8.empty()) return fail(c, VPT_ERR_UNSUPPORTED, "no eight-wide tree for an empty scene");
        int rc8 = upload(c, n8, &c->dsc.nodes8);
        if (rc8) return rc8;
        c->stats.bvh8_nodes = (uint32_t)n8.size();
    }
    const uint32_t n = c->lab_n;
    const bool holes = !c->lab_holes.empty();
    if (holes && variant != VPT_TRACE_VOTE) return fail(c, VPT_ERR_UNSUPPORTED, "only VPT_TRACE_VOTE knows holes: vpt_lab_set_holes(ctx, NULL) first");
    c->spill_dirty = true;   // traversal kernels run: vpt_get_stats recounts the spill regions
    const size_t m = (size_t)n + kLabGuard;
    if (order) {   // (with holes: an entry that names a hole holds the hole word instead, as in a queue of the pipeline)
        std::vector<uint32_t> o(m);
        for (size_t i = 0; i < m; i++) o[i] = i < n ? order[i] : (uint32_t)i;
        if (holes) for (uint32_t i = 0; i < n; i++) {
            if (o[i] >= n) return fail(c, VPT_ERR_INVALID_ARGUMENT, "order_host is no permutation of the resident rays");
            if (c->lab_holes[o[i]]) o[i] = kLabHole;
        }
        HIPCHK(c, hipMemcpy(c->lab_order, o.data(), m * 4, hipMemcpyHostToDevice));
    }
    TraceArgs a{};
    a.ro = c->lab_ro; a.rd = c->lab_rd; a.order = order ? c->lab_order : nullptr; a.hit = c->lab_hit; a.hinst = c->lab_hinst;
    a.valid = holes && !order ? c->lab_order + m : nullptr;
    a.n = n; a.head = &c->main.ctr->extend_head; a.tmin = c->lab_tmin; a.tmax = c->lab_tmax; a.normalize_dir = 0u; a.param = (variant == VPT_TRACE_POOL || variant == VPT_TRACE_PAIR) ? param : param & 0xfff1ffffu;
    a.cull = variant == VPT_TRACE_VOTE ? (param >> 17) & 1u : 0u;     // lab: bit 17 = stale-entry culling (closest-hit, VPT_TRACE_VOTE)
    a.one_tri = variant == VPT_TRACE_VOTE ? (param >> 19) & 1u : 0u;     // lab: bit 19 = one triangle per triangle step, as before round 4 (VPT_TRACE_VOTE, product vote parameters)
    a.packed = variant == VPT_TRACE_VOTE ? (param >> 18) & 1u : 0u;   // lab: bit 18 = packed plane arithmetic in the node step (VPT_TRACE_VOTE, product vote parameters)
    // (the pool variant's spill region is indexed by slot: 512 slots per block against 256 threads)
    const uint32_t blocks = (uint32_t)std::min(trace_blocks_per_cu(variant, any_hit != 0) * c->cu_count, (variant == VPT_TRACE_POOL || variant == VPT_TRACE_PAIR) ? c->max_blocks / 2 : c->max_blocks);
    hipEvent_t e0, e1;
    HIPCHK(c, hipEventCreate(&e0)); HIPCHK(c, hipEventCreate(&e1));
    float best = 1e30f;
    for (uint32_t r = 0; r < reps + (visits ? 1u : 0u); r++) {
        const bool count = visits && r == reps;
        HIPCHK(c, hipMemsetAsync(c->main.ctr, 0, sizeof(Counters), c->main.stream));
        // what a launch leaves untouched shows: the guard always, the whole set when it has holes
        HIPCHK(c, hipMemsetAsync(c->lab_hit + (holes ? 0u : n), 0xAA, (holes ? m : kLabGuard) * 16, c->main.stream));
        HIPCHK(c, hipMemsetAsync(c->lab_hinst + (holes ? 0u : n), 0xAA, (holes ? m : kLabGuard) * 4, c->main.stream));
        HIPCHK(c, hipEventRecord(e0, c->main.stream));
        launch_trace(c->main.stream, blocks, variant, any_hit != 0, count, lane_scene(c, c->main), a, c->main.ctr);
        HIPCHK(c, hipEventRecord(e1, c->main.stream));
        HIPCHK(c, hipStreamSynchronize(c->main.stream));
        HIPCHK(c, hipGetLastError());
        int rg = guard_untouched(c, c->lab_hit + n, kLabGuard * 16);
        if (!rg) rg = guard_untouched(c, c->lab_hinst + n, kLabGuard * 4);
        if (rg) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); return rg; }
        float ms = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
        if (!count) best = std::min(best, ms);
        else {
            Counters h{};
            HIPCHK(c, hipMemcpy(&h, c->main.ctr, sizeof(Counters), hipMemcpyDeviceToHost));
            visits[0] = h.stat_nodes; visits[1] = h.stat_tris;
        }
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    HIPCHK(c, memset_now(c->main.stream, c->main.ctr, 0, sizeof(Counters)));
    if (best_ms) *best_ms = best;
    if (hits) {
        std::vector<float4> h4(n); std::vector<uint32_t> hi(n, 0xffffffffu);
        HIPCHK(c, hipMemcpy(h4.data(), c->lab_hit, (size_t)n * 16, hipMemcpyDeviceToHost));
        if (!any_hit) HIPCHK(c, hipMemcpy(hi.data(), c->lab_hinst, (size_t)n * 4, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; i++) {
            hits[i].t = h4[i].x; hits[i].u = h4[i].y; hits[i].v = h4[i].z;
            uint32_t prim; memcpy(&prim, &h4[i].w, 4);
            hits[i].primitive = any_hit ? 0xffffffffu : prim; hits[i].instance = hi[i];
        }
    }
    return VPT_OK;
}

namespace {
struct ShadowLabBuffers {   // what one vpt_lab_trace_shadow call allocates, freed however it ends
    float4 *ro = nullptr, *rd = nullptr;
    unsigned char* vis = nullptr;
    StreamCounters* sctr = nullptr;
    ~ShadowLabBuffers() { for (void* p : {(void*)ro, (void*)rd, (void*)vis, (void*)sctr}) if (p) (void)hipFree(p); }
};
}  // namespace
int vpt_lab_trace_shadow(vpt_ctx* c, uint32_t light, uint32_t ray_queries, const uint32_t* expect, const unsigned char* media, const unsigned char* hole,
                         unsigned char* vis, uint64_t* visits) {
    if (!c || !vis || (light && !expect)) return VPT_ERR_INVALID_ARGUMENT;
    if (!c->has_scene) return fail(c, VPT_ERR_NO_SCENE, "no scene");
    if (c->lds_scene) return fail(c, VPT_ERR_UNSUPPORTED, "the trace lab runs on scenes whose BVH lives in memory");
    if (c->lab_n == 0) return fail(c, VPT_ERR_INVALID_ARGUMENT, "vpt_lab_trace_shadow before vpt_lab_set_rays");
    if (light && !ray_queries) return fail(c, VPT_ERR_UNSUPPORTED, "without ray queries the pipeline queues no light rays");   // (shade_core.hpp)
    const uint32_t n = c->lab_n;
    if (light) for (uint32_t i = 0; i < n; i++)
        if (expect[i] >= c->total_tris) return fail(c, VPT_ERR_INVALID_ARGUMENT, "expect_host: no such triangle");   // (the kernel looks it up in tri_slot_of_gid)
    { int rd = quiesce(c); if (rd) return rd; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // the stream as shade_core queues it: RO = origin | d.x, RD = d.y, d.z, bits of the sampled triangle's id (sky rays: 0xffffffff; a hole: kRayHole), media flag
    const size_t m = (size_t)n + kLabGuard;   // (the guard: sky rays of zeros, or light rays that expect ray 0's triangle)
    float guard_id; { const uint32_t id = light ? expect[0] : 0xffffffffu; memcpy(&guard_id, &id, 4); }
    std::vector<float4> o(n), d(n), ro(m, make_float4(0.0f, 0.0f, 0.0f, 0.0f)), rd(m, make_float4(0.0f, 0.0f, guard_id, 0.0f));
    HIPCHK(c, hipMemcpy(o.data(), c->lab_ro, (size_t)n * 16, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(d.data(), c->lab_rd, (size_t)n * 16, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t id = (hole && hole[i]) ? kLabRayHole : light ? expect[i] : 0xffffffffu;
        float idf; memcpy(&idf, &id, 4);
        ro[i] = make_float4(o[i].x, o[i].y, o[i].z, d[i].x);
        rd[i] = make_float4(d[i].y, d[i].z, idf, (media && media[i]) ? 1.0f : 0.0f);
    }
    ShadowLabBuffers b;
    HIPCHK(c, hipMalloc((void**)&b.ro, m * 16)); HIPCHK(c, hipMalloc((void**)&b.rd, m * 16));
    HIPCHK(c, hipMalloc((void**)&b.vis, m)); HIPCHK(c, hipMalloc((void**)&b.sctr, sizeof(StreamCounters)));
    HIPCHK(c, hipMemcpy(b.ro, ro.data(), m * 16, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(b.rd, rd.data(), m * 16, hipMemcpyHostToDevice));
    StreamCounters* const sc = b.sctr;
    hipStream_t s = c->main.stream;
    HIPCHK(c, hipMemsetAsync(b.vis, 0xAA, m, s));   // untouched entries show
    HIPCHK(c, hipMemsetAsync(sc, 0, sizeof(StreamCounters), s));   // (the cursor among them)
    HIPCHK(c, hipMemcpyAsync(light ? &sc->light_len.v : &sc->sky_len.v, &n, 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(c->main.ctr, 0, sizeof(Counters), s));
    StreamState ss{};
    ss.SKO = b.ro; ss.SKD = b.rd; ss.LTO = b.ro; ss.LTD = b.rd; ss.vis_sky = b.vis; ss.vis_light = b.vis; ss.cap = n;
    c->spill_dirty = true;
    launch_trace_shadow(s, (uint32_t)c->shadow_blocks, light != 0u, visits != nullptr, lane_scene(c, c->main), ss, c->main.ctr, sc, c->vote_param, ray_queries ? 1u : 0u);
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    if (visits) {
        Counters h{};
        HIPCHK(c, hipMemcpy(&h, c->main.ctr, sizeof(Counters), hipMemcpyDeviceToHost));
        visits[0] = h.stat_shadow_nodes; visits[1] = h.stat_shadow_tris;
    }
    HIPCHK(c, memset_now(s, c->main.ctr, 0, sizeof(Counters)));
    HIPCHK(c, hipMemcpy(vis, b.vis, (size_t)n, hipMemcpyDeviceToHost));
    return guard_untouched(c, b.vis + n, kLabGuard);
}

}  // extern "C"
