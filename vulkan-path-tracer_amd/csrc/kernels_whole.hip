// kernels_whole.hip — k_whole: whole paths in one launch, for scenes whose BVH rides in LDS (VPT_PIPELINE_WHOLE; the headline kernel).
// With it: the vote-scheduled searches on the tree in LDS (measured and not taken, built only with -DVPT_WHOLE_VOTE=1), the VPT_DIAG_* measuring
// switches, launch_whole and whole_blocks_per_cu.  A wave is 64 lanes.
#include "kernels.hpp"
#include "traverse.hpp"
#include "wave.hpp"
#include "shade_core.hpp"
#include "vote.hpp"
#include "whole_refill.hpp"
#include "whole_args.hpp"

namespace vpt {

// ------------------------------------------------------------------ vote-scheduled traversal of the tree in LDS (k_whole)
// The per-lane loops of traverse.hpp make a wave run the node branch AND the leaf branch of every iteration as soon as its lanes stand at
// different places of their trees — on the Cornell box a ray needs 1.9 node visits and 1.4 triangle tests, in no particular order.  These are
// the same searches with the wave-level vote of the stream kernels (vote.hpp): every iteration the lanes that are in the call execute ONE kind of
// step — an inner-node step (fp32 node from LDS, four slab tests, nearest-first order / slot order) or a one-triangle step — chosen by ballot, and
// a lane that wants the other kind waits a turn.  A ray's own sequence of visits, tests and interval updates is exactly that of
// trace_closest_pass / trace_occluded_pass (the state machine is per ray; only the interleaving changes), so hits, visibility and the visit
// counters are identical.  Lanes outside the call (no ray, no shadow ray) are simply not part of the ballots.  The validating (STRICT)
// instantiations keep the per-lane loops.
// MEASURED AND NOT TAKEN (round 5, same box, alternating, three rounds: profiles/r05_whole_vote_ab.json): Cornell 1080p 8277-8281 Msamples/s with it
// against 8376-8378 with the per-lane loops (-1.2 %), images and ray statistics identical; 168 VGPRs either way, 16 instead of 36 B of scratch.
// The tree is twelve triangles under three nodes: a lane's two or three steps are over before a vote per step can pay for itself, and what
// idles the lanes of this kernel (47 of 64 per VALU instruction) is the shader's own branching, not the searches.  Built only with
// -DVPT_WHOLE_VOTE=1 (tests/tools/build_variant.py).
#ifndef VPT_WHOLE_VOTE
#define VPT_WHOLE_VOTE 0
#endif
#ifndef VPT_DIAG_NO_LIGHT_SEARCH
#define VPT_DIAG_NO_LIGHT_SEARCH 0
#endif
#ifndef VPT_DIAG_REFILL_LANES
#define VPT_DIAG_REFILL_LANES 0
#endif
// A/B switch (tests/tools/build_variant.py -DVPT_WHOLE_CAM_LDS=0: the kernel before it): the camera lives in LDS between two refills and in no
// register, and one-sample frames are a compile-time fact.  Cornell 1080p, same box, alternating: 8827-8833 Msamples/s against 8641-8658
// (profiles/r11_whole_uniform_ab.md).
#ifndef VPT_WHOLE_CAM_LDS
#define VPT_WHOLE_CAM_LDS 1
#endif
// A/B switch (tests/tools/build_variant.py -DVPT_WHOLE_ARGS_AT_USE=0: the kernel before it): the loop reads the words of the scene, the parameters
// and the path buffers again from the kernel's argument segment where it uses them (whole_args.hpp) and holds none of them in registers across the
// trace loops.  Cornell 1080p, same box, alternating: 9250-9269 Msamples/s against 9100-9109 (profiles/r14_whole_uniforms_ab.md).  Builds on the
// camera block: one-sample frames are a compile-time fact of WholeParams.
#ifndef VPT_WHOLE_ARGS_AT_USE
#define VPT_WHOLE_ARGS_AT_USE 1
#endif
#if VPT_WHOLE_ARGS_AT_USE && !VPT_WHOLE_CAM_LDS
#error "VPT_WHOLE_ARGS_AT_USE needs VPT_WHOLE_CAM_LDS"
#endif
#define VPT_KERNARG __attribute__((address_space(4)))   // the constant address space: where a kernel's arguments lie
template <> struct OneSampleFrames<VPT_KERNARG WholeParams> { static constexpr bool value = true; };
constexpr int kWalkDone = 0x7fffffff;
template <class Stack>
__device__ __forceinline__ int walk_pop(Stack& stack) { return stack.sp ? (int)stack.pop() : kWalkDone; }
template <bool COUNT, class Stack>
__device__ __forceinline__ bool lds_closest_vote(const LdsSceneSrc& src, V3 o, V3 d, float tmin, float tmax, Stack stack, HitRec& best, TravStats& st) {
    best.t = tmax; best.u = 0.0f; best.v = 0.0f; best.prim = 0xffffffffu; best.inst = 0xffffffffu; best.gid = 0xffffffffu; best.slot = 0;
    bool found = false;
    const RaySlabWide slab = make_slab<false>(src, o, d);
    stack.sp = 0;
    int cur = 0;   // root is inner node 0
    while (true) {
        const bool at_node = cur >= 0 && cur != kWalkDone, at_leaf = cur < 0;
        const uint32_t nn = (uint32_t)__popcll(__ballot(at_node)), nl = (uint32_t)__popcll(__ballot(at_leaf));
        if (nn + nl == 0u) break;
        const bool node_wins = 4u * nn > kVoteWeight4 * nl;   // a node step retires about twice the work of a triangle step
        if (node_wins & at_node) {
            NodeDataWide n;
            load_node(src, slab, cur, n);
            if (COUNT) st.nodes++;
            float t0, t1, t2, t3;
            node_entries(n, slab, tmin, best.t, t0, t1, t2, t3);
            int c0 = n.c0, c1 = n.c1, c2 = n.c2, c3 = n.c3;
            cswap(t0, c0, t1, c1); cswap(t2, c2, t3, c3); cswap(t0, c0, t2, c2); cswap(t1, c1, t3, c3); cswap(t1, c1, t2, c2);
            if (t0 < kMissT) {  // nearest child next, the others pushed far -> near
                if (t3 < kMissT) stack.push((uint32_t)c3);
                if (t2 < kMissT) stack.push((uint32_t)c2);
                if (t1 < kMissT) stack.push((uint32_t)c1);
                cur = c0;
            } else cur = walk_pop(stack);
        }
        if (!node_wins & at_leaf) {   // ONE triangle of the lane's leaf
            const uint32_t enc = (uint32_t)(~cur);
            const int first = (int)(enc >> 3);
            const uint32_t more = enc & 7u;
            float4 a, b, c;
            src.tri(first, a, b, c);
            if (COUNT) st.tris++;
            float t, u, v;
            const bool hit = ray_triangle_flat(o, d, vptfp::v3(a.x, a.y, a.z), vptfp::v3(a.w, b.x, b.y), vptfp::v3(b.z, b.w, c.x), tmin, tmax, t, u, v);
            const uint32_t gid = __float_as_uint(c.w);
            if (hit & (!found | (t < best.t) | ((t == best.t) & (gid < best.gid)))) {
                best.t = t; best.u = u; best.v = v; best.prim = __float_as_uint(c.y); best.inst = __float_as_uint(c.z); best.gid = gid;
                found = true;
            }
            if (more) cur = ~(int)((((uint32_t)first + 1u) << 3) | (more - 1u));
            else cur = walk_pop(stack);
        }
    }
    return found;
}
// any-hit: LIGHT = false: occluded <=> some triangle is hit in (tmin, tmax); LIGHT = true: something beats the sampled triangle's hit at t_e (traverse.hpp)
template <bool COUNT, bool LIGHT, class Stack>
__device__ __forceinline__ bool lds_occluded_vote(const LdsSceneSrc& src, V3 o, V3 d, float tmin, float tmax, float t_e, uint32_t expect, Stack stack, TravStats& st) {
    const float tlimit = LIGHT ? t_e : tmax;
    const RaySlabWide slab = make_slab<false>(src, o, d);
    stack.sp = 0;
    int cur = 0;
    bool occluded = false;
    while (true) {
        const bool at_node = cur >= 0 && cur != kWalkDone, at_leaf = cur < 0;
        const uint32_t nn = (uint32_t)__popcll(__ballot(at_node)), nl = (uint32_t)__popcll(__ballot(at_leaf));
        if (nn + nl == 0u) break;
        const bool node_wins = 4u * nn > kVoteWeight4 * nl;
        if (node_wins & at_node) {
            NodeDataWide n;
            load_node(src, slab, cur, n);
            if (COUNT) st.nodes++;
            float t0, t1, t2, t3;
            node_entries(n, slab, tmin, tlimit, t0, t1, t2, t3);
            int next = kWalkDone;   // order is irrelevant for an any-hit search: hit children in slot order
            if (t3 < kMissT) next = n.c3;
            if (t2 < kMissT) { if (next != kWalkDone) stack.push((uint32_t)next); next = n.c2; }
            if (t1 < kMissT) { if (next != kWalkDone) stack.push((uint32_t)next); next = n.c1; }
            if (t0 < kMissT) { if (next != kWalkDone) stack.push((uint32_t)next); next = n.c0; }
            cur = next != kWalkDone ? next : walk_pop(stack);
        }
        if (!node_wins & at_leaf) {
            const uint32_t enc = (uint32_t)(~cur);
            const int first = (int)(enc >> 3);
            const uint32_t more = enc & 7u;
            float4 a, b, c;
            src.tri(first, a, b, c);
            if (COUNT) st.tris++;
            float t, u, v;
            const bool hit = ray_triangle_flat(o, d, vptfp::v3(a.x, a.y, a.z), vptfp::v3(a.w, b.x, b.y), vptfp::v3(b.z, b.w, c.x), tmin, tmax, t, u, v);
            const uint32_t gid = __float_as_uint(c.w);
            if (hit & (!LIGHT | (t < t_e) | ((t == t_e) & (gid < expect)))) { occluded = true; cur = kWalkDone; }
            else if (more) cur = ~(int)((((uint32_t)first + 1u) << 3) | (more - 1u));
            else cur = walk_pop(stack);
        }
    }
    return occluded;
}
// sky_visible / light_visible of k_whole's non-validating instantiations (the interval and direction rules of traverse.hpp sky_visible)
template <bool COUNT, class Sc, class Stack>
__device__ __forceinline__ bool sky_visible_vote(const Sc& sc, const float4* lds_nodes, const float4* lds_tris, V3 o, V3 d, const Stack& stack, TravStats& st, bool rq) {
    const float tmin = rq ? 0.0001f : 0.00001f, tmax = rq ? 1000000.0f : 1000.0f;
    if (!rq) d = normalize(d);
    LdsSceneSrc src{lds_nodes, lds_tris, false, kSlabFmaReach * sc.scene_extent};
    return !lds_occluded_vote<COUNT, false>(src, o, d, tmin, tmax, 0.0f, 0u, stack, st);
}
template <bool COUNT, class Sc, class Stack>
__device__ __forceinline__ bool light_visible_vote(const Sc& sc, const float4* lds_nodes, const float4* lds_tris, V3 o, V3 d, uint32_t gid, const Stack& stack, TravStats& st) {
    const uint32_t slot = sc.tri_slot_of_gid[gid];
    if (slot == 0xffffffffu) return false;  // the sampled light triangle is a sliver: nothing can hit it
    LdsSceneSrc src{lds_nodes, lds_tris, false, kSlabFmaReach * sc.scene_extent};
    float4 a, b, c;
    src.tri((int)slot, a, b, c);   // traverse.hpp closest_is: the sampled triangle by its own record first, then the search for anything that beats it
    if (COUNT) st.tris++;
    float t_e, u, v;
    if (!vptfp::ray_triangle(o, d, vptfp::v3(a.x, a.y, a.z), vptfp::v3(a.w, b.x, b.y), vptfp::v3(b.z, b.w, c.x), 0.0001f, 1000000.0f, &t_e, &u, &v)) return false;
    return !lds_occluded_vote<COUNT, true>(src, o, d, 0.0001f, 1000000.0f, t_e, gid, stack, st);
}

// ------------------------------------------------------------------ whole paths in one launch
// The reference's RayGen invocation IS a whole path: one thread runs the bounce loop of its pixel's sample to the end
// (RayGen.slang:66-114).  k_whole is that loop on persistent waves, for scenes whose BVH rides in LDS and which have no media:
// a lane keeps its path in registers from bounce to bounce, and a lane whose path has ended takes the next unstarted sample of the
// batch, so a launch runs until the batch's samples are used up and no path record, queue or counter crosses HBM in between —
// only the per-sample frame sums (ACC) do.  One launch per batch instead of max_depth: what a 1-frame batch at 1080p needs (its
// later bounces are launches of 10^5 paths that do not fill the chip, vpt_render_async).
// A wave alternates two steps, each on full lanes:
//   trace   every lane holds a ray — a survivor of the shade step or a fresh camera ray — and finds its closest hit; misses run the
//           miss shader and end there, hits are parked in a wave-private ring in LDS (hit record + the path's registers);
//   shade   once the ring holds 64 hits: closest-hit shader, the <= 2 shadow queries, contribution, Russian roulette for those 64;
//           survivors keep their lanes for the next trace step.
// Per path this is k_bounce's arithmetic in k_bounce's order (same shade_core, same connect code), and which lane or wave runs a
// sample cannot matter: seeds come from (pixel, frame), results go to ACC[slot].  pathLight of a parked hit waits in ACC[slot].
template <class Pm, class Ps>
__device__ __forceinline__ V3 whole_finish(const Pm& P, const Ps& ps, uint32_t slot, V3 E, V3 thr_prev, V3 light_prev, const ShadeOut& o) {
    V3 contrib = E * thr_prev;
    if (o.cflags & kCF_Clamp) {
        float lum = dot(contrib, v3(0.212671f, 0.715160f, 0.072169f));
        contrib = contrib * (P.max_luminance / max_(lum, P.max_luminance));
    }
    V3 light = light_prev + contrib;
    if (o.terminated) {  // end of the sample: NaN/Inf guard, frame sum (RayGen.slang:116-128)
        bool ok = !isinf_(light.x) && !isinf_(light.y) && !isinf_(light.z) && !isnan_(light.x) && !isnan_(light.y) && !isnan_(light.z);
        ps.ACC[slot] = ok ? f4(v3s(0.0f) + light, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    return light;
}
// Samples are dealt in tiles of 64 (consecutive pixels of a row).  Wave w of W takes tiles w, w + W, ... for the first `static_rounds` rounds
// without an atomic, and the tiles behind them `chunk_tiles` at a time through ctr->extend_head (the host picks both: api_render.hip batch_begin).
// (Measured and not kept: one-wave blocks, which leave the CU as soon as THEIR paths have ended and so let the next frame's launch in earlier —
// a 1-frame launch at 1080p 542 us against 509 us, and slower with two or three frames in flight too: profiles/r04_whole_lanes.json.)
template <bool COUNT, bool STRICT, bool PLAIN>
#if VPT_WHOLE_ARGS_AT_USE
__global__ __launch_bounds__(kTraverseBlock, 3) void k_whole(WholeArgs a) {   // (ONE parameter: the argument segment is a WholeArgs)
    // what runs once, before the loop, reads the arguments as any kernel does
    DeviceScene sc = a.sc;
    RenderParams P = a.P;
    const PathState ps = a.ps;
    Counters* const ctr = a.ctr;
    const uint32_t n_slots = a.n_slots, static_rounds = a.static_rounds, chunk_tiles = a.chunk_tiles;
#else
__global__ __launch_bounds__(kTraverseBlock, 3) void k_whole(DeviceScene sc, RenderParams P, PathState ps, Counters* ctr, uint32_t n_slots, uint32_t dispatch_base,
                                                            uint32_t static_rounds, uint32_t chunk_tiles) {
#endif
    sc.strict_hits = STRICT ? 1u : 0u;
    if (PLAIN) { sc.all_plain = 1u; sc.env_black = 1u; } else sc.all_plain = 0u;
#if VPT_WHOLE_CAM_LDS
    // the planner gives this kernel one-sample frames only (path_plan.hpp whole_possible): a compile-time fact here, so shade_core's "next sample of the
    // pixel" branch — the other reader of the camera's matrices — drops out and nothing of the camera is live outside the refill step
    P.samples_per_frame = 1u;
#endif
#if !VPT_WHOLE_ARGS_AT_USE
    if (P.dispatch_base_dev) dispatch_base = *P.dispatch_base_dev;   // a replayed graph: the batch's first dispatch index lives in device memory
    const bool rq = (P.flags & VPT_FLAG_RAY_QUERIES) != 0u;
#endif
    extern __shared__ __align__(16) unsigned char smem[];
    const TravStackT<kWholeStackRows> stack = make_stack<kWholeStackRows>(smem, sc.stack_overflow);
    float4* lds_nodes = reinterpret_cast<float4*>(smem + kWholeStackRows * kTraverseBlock * 4);
    float4* lds_tris = lds_nodes + sc.node_count * 8;
#if VPT_WHOLE_CAM_LDS
    // camera_ray's part of P, read once per tile of 64 samples: from LDS there (a uniform address broadcasts) instead of ~40 scalar registers held
    // across the shade and trace steps; staged behind stage_scene's barrier
    __shared__ CameraBlock cam;
    if (threadIdx.x == 0u) {
#pragma unroll
        for (int i = 0; i < 16; i++) { cam.view_inv[i] = P.view_inv[i]; cam.proj_inv[i] = P.proj_inv[i]; }
        cam.width = P.width; cam.height = P.height; cam.focus_distance = P.focus_distance; cam.dof_strength = P.dof_strength;
    }
#else
    const RenderParams& cam = P;
#endif
#if VPT_WHOLE_ARGS_AT_USE
    // the loop's view of the arguments (whole_args.hpp): `a` again, where it lies in memory
    const VPT_KERNARG WholeArgs* ka = (const VPT_KERNARG WholeArgs*)__builtin_amdgcn_kernarg_segment_ptr();
#else
    const DeviceScene& usc = sc;
    const RenderParams& uP = P;
    const PathState& ups = ps;
#endif
    stage_scene<true>(sc, lds_nodes, lds_tris);
    constexpr uint32_t kWaves = kTraverseBlock / 64u;
    __shared__ uint32_t r_slot[kWaves][128], r_prim[kWaves][128], r_inst[kWaves][128];
    __shared__ float r_t[kWaves][128], r_u[kWaves][128], r_v[kWaves][128];
    __shared__ float4 r_ra[kWaves][128], r_rb[kWaves][128], r_rt[kWaves][128];
    // the wave's fresh camera rays (whole_refill.hpp): slot, origin, direction, RNG state behind camera_ray; dword arrays, lane = bank
    __shared__ uint32_t f_slot[kWaves][refill::kTile], f_rng[kWaves][refill::kTile];
    __shared__ float f_ox[kWaves][refill::kTile], f_oy[kWaves][refill::kTile], f_oz[kWaves][refill::kTile];
    __shared__ float f_dx[kWaves][refill::kTile], f_dy[kWaves][refill::kTile], f_dz[kWaves][refill::kTile];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (uniform: the rings' and the buffer's rows are addressed from a scalar base)
    // tile cursor and fresh-ray buffer, wave-uniform by construction (kernels_trace.hip k_trace_vote)
    const refill::Shape shape{n_slots, gridDim.x * kWaves, static_rounds, chunk_tiles};
    refill::Cursor cur = refill::make_cursor(shape, blockIdx.x * kWaves + wave);
    refill::Fresh fresh = refill::make_fresh();
    uint32_t hit_head = 0u, hit_count = 0u;   // wave-uniform
#if VPT_DIAG_REFILL_LANES
    uint32_t d_passes = 0u, d_lanes = 0u;
#endif
#if VPT_DIAG_LIGHT_REFR
    uint32_t d_steps = 0u, d_refr = 0u, d_refr_dead_only = 0u;
#endif
    TravStats st, sst; st.nodes = 0; st.tris = 0; sst.nodes = 0; sst.tris = 0;
    uint32_t w_paths = 0u, w_rays = 0u, w_hits0 = 0u, w_alive0 = 0u, w_rays0 = 0u, w_parked = 0u;   // wave totals (uniform); *0: bounce 0 only; parked: hits of later bounces (their pathLight waits in ACC)
    // the lane's path between two steps
    bool has_ray = false;
    uint32_t slot = 0u, rng_s = 0u, depth = 0u;
    bool in_medium = false;
    V3 porg = v3s(0.0f), pdir = v3s(0.0f), thr = v3s(1.0f), lightp = v3s(0.0f);
    float pdf = 1.0f;
    for (;;) {
#if VPT_WHOLE_ARGS_AT_USE
        // The compiler knows that argument memory does not change and would load every word once, ahead of the loop — the registers this is about.
        // Behind this statement it no longer knows where `ka` points, so what a round of the loop reads through it is loaded in that round.
        asm volatile("" : "+s"(ka));
        const VPT_KERNARG WholeScene<STRICT, PLAIN>& usc = static_cast<const VPT_KERNARG WholeScene<STRICT, PLAIN>&>(ka->sc);
        const VPT_KERNARG WholeParams& uP = static_cast<const VPT_KERNARG WholeParams&>(ka->P);
        const VPT_KERNARG PathState& ups = ka->ps;
#endif
        // ---- shade: a chunk of parked hits (a partial one only when nothing can be added to it any more: no lane holds a ray here)
        if (hit_count >= 64u || (refill::exhausted(cur, fresh) && hit_count > 0u)) {
            const uint32_t cnt = hit_count < 64u ? hit_count : 64u;
            const bool valid = lane_id() < cnt;
            uint32_t nrays = 0u;
            bool first = false, alive = false;
#if VPT_DIAG_LIGHT_REFR
            bool l_refr = false, l_dead = false;
#endif
            if (valid) {
                const uint32_t q = (hit_head + lane_id()) & 127u;
                ShadeIn in_;
                const float4 a = r_ra[wave][q], b = r_rb[wave][q], t = r_rt[wave][q];
                slot = r_slot[wave][q];
                in_.rng = __float_as_uint(a.w);
                in_.porg = xyz(a); in_.pdir = xyz(b);
                const uint32_t dw = __float_as_uint(b.w);
                in_.depth = dw & 0x7fffffffu; in_.in_medium = (dw >> 31) != 0u;
                in_.thr_prev = xyz(t); in_.prev_pdf = t.w;
                in_.vdepth = 0u; in_.cchan = -1; in_.vol_index = -1; in_.vol_t = 0.0f; in_.atm_comp = -1;
                in_.h = make_float4(r_t[wave][q], r_u[wave][q], r_v[wave][q], __uint_as_float(r_prim[wave][q]));
                in_.inst = r_inst[wave][q];
                first = in_.depth == 0u;   // (only a camera ray has depth 0: the in-medium walk that leaves the depth alone starts behind a refraction)
                ShadeOut o;
                shade_core<false, (int)kShadeTextured>(usc, uP, ups, slot, in_, o);   // "all of these hit something"
#if VPT_DIAG_LIGHT_REFR
                l_refr = o.diag_light_refr; l_dead = o.diag_light_refr_dead;
#endif
                // pathLight so far: fetched behind the shader (three registers less across its peak), in flight during the shadow queries
                const V3 light_prev = first ? v3s(0.0f) : xyz(ups.ACC[slot]);
                // connect, inline (RayGen.slang:92-102)
                V3 E = o.emitted;
                constexpr bool kVote = VPT_WHOLE_VOTE != 0 && !STRICT;   // vote-scheduled searches on the tree in LDS (above); the validating instantiations keep the per-lane loops
                if (o.want_sky) {
                    bool vis;
#if VPT_WHOLE_ARGS_AT_USE
                    const bool rq = (uP.flags & VPT_FLAG_RAY_QUERIES) != 0u;
#endif
                    if constexpr (kVote) vis = sky_visible_vote<COUNT>(usc, lds_nodes, lds_tris, o.sky_o, o.sky_d, stack, sst, rq);
                    else vis = sky_visible<true, COUNT>(usc, lds_nodes, lds_tris, o.sky_o, o.sky_d, stack, sst, rq);
                    if (vis) E = E + o.csky;
                    nrays++;
                }
                if (o.want_light) {
                    bool vis;
#if VPT_DIAG_NO_LIGHT_SEARCH   // measuring build only (tests/tools/build_variant.py): what the kernel costs WITHOUT its light-identity searches (wrong images)
                    vis = true;
#else
                    if constexpr (kVote) vis = light_visible_vote<COUNT>(usc, lds_nodes, lds_tris, o.light_o, o.light_d, o.light_gid, stack, sst);
                    else vis = light_visible<true, COUNT>(usc, lds_nodes, lds_tris, o.light_o, o.light_d, o.light_gid, stack, sst);
#endif
                    if (vis) E = E + o.clight;
                    nrays++;
                }
                // contribution and the survivor's registers: the same statements as a closure called once.  Nothing else differs, and why the compiler
                // then allocates better is not understood: the PLAIN instantiation keeps 232 instead of 270 scalar-spill lane operations and 1584 instead
                // of 1703 SALU instructions (VALU 5491 / 5486), and Cornell 1080p runs at 8926-8945 against 8818-8831 Msamples/s, same box, alternating
                // (profiles/r12_whole_walk_ab.md; a compiler update may take it back: tests/tools/spill_report.py shows the counts)
                auto finish = [&]() {
                    const V3 light = whole_finish(uP, ups, slot, E, in_.thr_prev, light_prev, o);
                    alive = o.alive;
                    if (alive) {
                        has_ray = true;
                        rng_s = o.rng; porg = o.new_o; pdir = o.new_d; depth = o.new_depth; in_medium = o.in_medium; thr = o.thr; pdf = o.new_pdf; lightp = light;
                    }
                };
                finish();
            }
            hit_head += cnt; hit_count -= cnt;
#if VPT_DIAG_LIGHT_REFR   // steps in which the lobe ran on some lane | in which every lane that ran it has pg == 0 (the steps a sign-only evaluation would spare)
            d_steps++;
            if (__ballot(l_refr) != 0ull) { d_refr++; if (__ballot(l_refr && !l_dead) == 0ull) d_refr_dead_only++; }
#endif
            w_rays += (uint32_t)__popcll(__ballot(nrays >= 1u)) + (uint32_t)__popcll(__ballot(nrays >= 2u));
            w_rays0 += (uint32_t)__popcll(__ballot(first && nrays >= 1u)) + (uint32_t)__popcll(__ballot(first && nrays >= 2u));
            w_alive0 += (uint32_t)__popcll(__ballot(first && alive));
        }
        // ---- refill: free lanes take the next unstarted samples from the front of the wave's buffer; when it runs out, ALL lanes generate the next
        // tile of camera rays into it (a second pass when the buffer ran out half-way)
        if (!refill::exhausted(cur, fresh)) {
#pragma unroll 1
            for (int pass = 0; pass < 2; pass++) {
                const unsigned long long m_free = __ballot(!has_ray);
                if (m_free == 0ull) break;
                if (fresh.count == 0u) {
                    if (refill::range_empty(cur) && !refill::take_static(shape, cur)) {   // the next tile(s) through the counter
                        const uint32_t take = refill::dyn_take(shape, cur);
                        uint32_t k = 0u;
                        if (lane_id() == 0u) k = atomicAdd(&ctr->extend_head, take);
                        refill::take_dynamic(shape, cur, __builtin_amdgcn_readfirstlane(k), take);
                    }
                    if (refill::exhausted(cur, fresh)) break;
                    const uint32_t g = refill::gen_count(cur);
#if VPT_DIAG_REFILL_LANES
                    d_passes++; d_lanes += g;
#endif
                    if (lane_id() < g) {
                        uint32_t gslot, x, y, f;
#if VPT_WHOLE_ARGS_AT_USE
                        const uint32_t dispatch_base = uP.dispatch_base_dev ? *uP.dispatch_base_dev : ka->dispatch_base;   // (a replayed graph: as above)
#endif
                        launch_pixel(uP, cur.w_next + lane_id(), dispatch_base, gslot, x, y, f);
                        const uint32_t seed = pcg_hash(uP.base_seed + dispatch_base + f);  // PathTracer.cpp:139 with an explicit seed
                        Rng r; r.s = y + uP.width * x + seed;                              // RayGen.slang:28
                        V3 go, gd;
                        camera_ray(cam, r, x, y, go, gd);
                        const uint32_t j = lane_id();
                        f_slot[wave][j] = gslot; f_rng[wave][j] = r.s;
                        f_ox[wave][j] = go.x; f_oy[wave][j] = go.y; f_oz[wave][j] = go.z;
                        f_dx[wave][j] = gd.x; f_dy[wave][j] = gd.y; f_dz[wave][j] = gd.z;
                    }
                    refill::generated(cur, fresh, g);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                }
                const uint32_t q = fresh.head + lanes_below(m_free);
                refill::pop(fresh, (uint32_t)__popcll(m_free));
                if (!has_ray && q < fresh.head) {
                    slot = f_slot[wave][q]; rng_s = f_rng[wave][q];
                    porg = v3(f_ox[wave][q], f_oy[wave][q], f_oz[wave][q]);
                    pdir = v3(f_dx[wave][q], f_dy[wave][q], f_dz[wave][q]);
                    depth = 0u; in_medium = false; thr = v3s(1.0f); pdf = 1.0f; lightp = v3s(0.0f);
                    has_ray = true;
                }
            }
        }
        if (__ballot(has_ray) == 0ull) {
            if (refill::exhausted(cur, fresh) && hit_count == 0u) break;
            continue;
        }
        // ---- trace: closest hits; park the hits, finish the misses
        {
            HitRec hr;
            bool hit = false;
            if (has_ray) {
                if constexpr (VPT_WHOLE_VOTE != 0 && !STRICT) { LdsSceneSrc src{lds_nodes, lds_tris, false, kSlabFmaReach * usc.scene_extent}; hit = lds_closest_vote<COUNT>(src, porg, normalize(pdir), 0.01f, 100000.0f, stack, hr, st); }
                else hit = trace_any<true, COUNT>(usc, lds_nodes, lds_tris, porg, normalize(pdir), 0.01f, 100000.0f, stack, hr, st);
            }
            const unsigned long long mh = __ballot(has_ray && hit);
            if (has_ray && hit) {
                const uint32_t q = (hit_head + hit_count + lanes_below(mh)) & 127u;
                r_slot[wave][q] = slot; r_t[wave][q] = hr.t; r_u[wave][q] = hr.u; r_v[wave][q] = hr.v; r_prim[wave][q] = hr.gid; r_inst[wave][q] = hr.inst;
                r_ra[wave][q] = f4u(porg, rng_s);
                r_rb[wave][q] = f4u(pdir, depth | (in_medium ? 0x80000000u : 0u));
                r_rt[wave][q] = f4(thr, pdf);
                if (depth != 0u) ups.ACC[slot] = f4(lightp, 0.0f);   // pathLight so far (a camera ray's is 0)
            }
            hit_count += (uint32_t)__popcll(mh);
            w_paths += (uint32_t)__popcll(__ballot(has_ray));
            w_hits0 += (uint32_t)__popcll(__ballot(has_ray && hit && depth == 0u));
            w_parked += (uint32_t)__popcll(__ballot(has_ray && hit && depth != 0u));
            if (has_ray && !hit) {   // Miss.slang; the path ends here
                ShadeIn in_;
                in_.rng = rng_s; in_.porg = porg; in_.pdir = pdir; in_.depth = depth; in_.in_medium = in_medium; in_.thr_prev = thr; in_.prev_pdf = pdf;
                in_.vdepth = 0u; in_.cchan = -1; in_.vol_index = -1; in_.vol_t = 0.0f; in_.atm_comp = -1;
                in_.h = make_float4(-1.0f, 0.0f, 0.0f, 0.0f); in_.inst = 0u;
                ShadeOut o;
                shade_core<false, (int)kShadeMiss>(usc, uP, ups, slot, in_, o);
                (void)whole_finish(uP, ups, slot, o.emitted, thr, lightp, o);
            }
            has_ray = false;
            // nothing of the lane's path is live across the shade step (hits wait in the ring): say so, or its 17 registers stay allocated through shade_core
            porg = v3s(0.0f); pdir = v3s(0.0f); thr = v3s(1.0f); lightp = v3s(0.0f); pdf = 1.0f; rng_s = 0u; depth = 0u; in_medium = false;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    if (lane_id() == 0) {
        if (w_paths) atomicAdd(&ctr->stat_closest, (unsigned long long)w_paths);
        if (w_rays) atomicAdd(&ctr->stat_shadow, (unsigned long long)w_rays);
        if (w_hits0) atomicAdd(&ctr->stat_primary_hits, (unsigned long long)w_hits0);
        if (w_alive0) atomicAdd(&ctr->stat_primary_alive, (unsigned long long)w_alive0);
        if (w_rays0) atomicAdd(&ctr->stat_primary_rays, (unsigned long long)w_rays0);
        if (w_parked) atomicAdd(&ctr->stat_connect, (unsigned long long)w_parked);   // vpt_stats.connect_paths: here, the hits whose pathLight made the round trip through ACC
    }
#if VPT_DIAG_REFILL_LANES   // measuring build only: passes of camera_ray and the lanes that ran them, reported IN PLACE of a counting context's closest-hit visits
    if (lane_id() == 0) { atomicAdd(&ctr->stat_nodes, (unsigned long long)d_passes); atomicAdd(&ctr->stat_tris, (unsigned long long)d_lanes); }
    constexpr bool kReportVisits = false;
#elif VPT_DIAG_LIGHT_REFR   // measuring build only, IN PLACE of a counting context's visits: shade steps | those whose light evaluation ran the refraction lobe |
                            // of these, the steps in which only lanes with pg == 0 ran it
    if (lane_id() == 0) {
        atomicAdd(&ctr->stat_nodes, (unsigned long long)d_steps); atomicAdd(&ctr->stat_tris, (unsigned long long)d_refr);
        atomicAdd(&ctr->stat_shadow_nodes, (unsigned long long)d_refr_dead_only);
    }
    constexpr bool kReportVisits = false;
#else
    constexpr bool kReportVisits = COUNT;
#endif
    if (kReportVisits) {
        atomicAdd(&ctr->stat_nodes, (unsigned long long)st.nodes);
        atomicAdd(&ctr->stat_tris, (unsigned long long)st.tris);
        atomicAdd(&ctr->stat_shadow_nodes, (unsigned long long)sst.nodes);
        atomicAdd(&ctr->stat_shadow_tris, (unsigned long long)sst.tris);
    }
}

// Whole paths in one launch (k_whole): LDS-resident scenes without media, one sample per pixel and frame.
void launch_whole(hipStream_t s, uint32_t blocks, bool count, const DeviceScene& sc, const RenderParams& P, const PathState& ps, Counters* ctr, uint32_t n_slots,
                  uint32_t dispatch_base, bool plain, uint32_t static_rounds, uint32_t chunk_tiles) {
    const size_t lds = traverse_lds_bytes(sc, true, kWholeStackRows);
    const dim3 g(blocks), b(kTraverseBlock);
    // one launch site for the five instantiations (the argument marshalling is host code the library's size bound pays for five times otherwise)
#if VPT_WHOLE_ARGS_AT_USE
    void (*k)(WholeArgs);
#else
    void (*k)(DeviceScene, RenderParams, PathState, Counters*, uint32_t, uint32_t, uint32_t, uint32_t);
#endif
    if (plain && !count && !sc.strict_hits && sc.env_black) k = k_whole<false, false, true>;
    else if (sc.strict_hits) k = count ? k_whole<true, true, false> : k_whole<false, true, false>;
    else k = count ? k_whole<true, false, false> : k_whole<false, false, false>;
#if VPT_WHOLE_ARGS_AT_USE
    hipLaunchKernelGGL(k, g, b, lds, s, WholeArgs{sc, P, ps, ctr, n_slots, dispatch_base, static_rounds, chunk_tiles});
#else
    hipLaunchKernelGGL(k, g, b, lds, s, sc, P, ps, ctr, n_slots, dispatch_base, static_rounds, chunk_tiles);
#endif
}
int whole_blocks_per_cu(const DeviceScene& sc, bool plain) {
    int nb = 0;
    const size_t lds = traverse_lds_bytes(sc, true, kWholeStackRows);
    if (plain) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_whole<false, false, true>, kTraverseBlock, lds);
    else (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_whole<false, false, false>, kTraverseBlock, lds);
    return nb > 0 ? nb : 1;
}

}  // namespace vpt
