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
    else return VPT_ERR_INVALID_ARGUMENT;
    c->state_gen++;   // captured batches hold the old grids
    return VPT_OK;
}
int vpt_lab_whole_culled(const vpt_ctx* c, uint64_t* out) {
    if (!c || !out) return VPT_ERR_INVALID_ARGUMENT;
    *out = c->main.h_ctr ? c->main.h_ctr->ctr.whole_culled : 0u;   // (the counters a batch copies to pinned memory behind its resolve: batch_resolve)
    return VPT_OK;
}
int vpt_lab_set_rays(vpt_ctx* c, const vpt_ray* rays, uint32_t n) {
    if (!c || !rays || n == 0) return VPT_ERR_INVALID_ARGUMENT;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    free_lab(c);
    std::vector<float4> ro(n), rd(n);
    for (uint32_t i = 0; i < n; i++) {
        ro[i] = make_float4(rays[i].origin[0], rays[i].origin[1], rays[i].origin[2], 0.0f);
        rd[i] = make_float4(rays[i].direction[0], rays[i].direction[1], rays[i].direction[2], 0.0f);
    }
    HIPCHK(c, hipMalloc((void**)&c->lab_ro, (size_t)n * 16)); HIPCHK(c, hipMalloc((void**)&c->lab_rd, (size_t)n * 16));
    HIPCHK(c, hipMalloc((void**)&c->lab_hit, (size_t)n * 16)); HIPCHK(c, hipMalloc((void**)&c->lab_hinst, (size_t)n * 4));
    HIPCHK(c, hipMalloc((void**)&c->lab_order, (size_t)n * 4));
    HIPCHK(c, hipMemcpy(c->lab_ro, ro.data(), (size_t)n * 16, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->lab_rd, rd.data(), (size_t)n * 16, hipMemcpyHostToDevice));
    c->lab_n = n; c->lab_tmin = rays[0].tmin; c->lab_tmax = rays[0].tmax;
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
    c->spill_dirty = true;   // traversal kernels run: vpt_get_stats recounts the spill regions
    if (order) HIPCHK(c, hipMemcpy(c->lab_order, order, (size_t)n * 4, hipMemcpyHostToDevice));
    TraceArgs a{};
    a.ro = c->lab_ro; a.rd = c->lab_rd; a.order = order ? c->lab_order : nullptr; a.hit = c->lab_hit; a.hinst = c->lab_hinst;
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
        HIPCHK(c, hipEventRecord(e0, c->main.stream));
        launch_trace(c->main.stream, blocks, variant, any_hit != 0, count, lane_scene(c, c->main), a, c->main.ctr);
        HIPCHK(c, hipEventRecord(e1, c->main.stream));
        HIPCHK(c, hipStreamSynchronize(c->main.stream));
        HIPCHK(c, hipGetLastError());
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

}  // extern "C"
