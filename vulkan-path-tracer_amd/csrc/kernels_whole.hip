// kernels_whole.hip — k_whole: whole paths in one launch, for scenes whose BVH rides in LDS (VPT_PIPELINE_WHOLE; the headline kernel).
// A launch runs a batch, or one PART of a large one — consecutive frames, its slot 0 the part's first sample (api_render.hip part_state) — while the
// resolve of the part before runs beside it on the lane's second stream (path_plan.hpp Schedule::parts); the kernel does not know the difference.
// With it: launch_whole and whole_blocks_per_cu.  A wave is 64 lanes.  (Variants of this kernel that were measured and not taken: profiles/REJECTED.md.)
#include "kernels.hpp"
#include "traverse.hpp"
#include "wave.hpp"
#include "shade_core.hpp"
#include "whole_refill.hpp"
#include "whole_args.hpp"
#include "camera_cull.hpp"

namespace vpt {

#define VPT_KERNARG __attribute__((address_space(4)))   // the constant address space: where a kernel's arguments lie
template <> struct OneSampleFrames<VPT_KERNARG WholeParams> { static constexpr bool value = true; };

// ------------------------------------------------------------------ whole paths in one launch
// The reference's RayGen invocation IS a whole path: one thread runs the bounce loop of its pixel's sample to the end
// (RayGen.slang:66-114).  k_whole is that loop on persistent waves, for scenes whose BVH rides in LDS and which have no media:
// a lane keeps its path in registers from bounce to bounce, and a lane whose path has ended takes the next unstarted sample of the
// batch, so a launch runs until the batch's samples are used up and no path record, queue or counter crosses HBM in between —
// only the per-sample frame sums (ACC) do.  One launch per batch (or part of one) instead of max_depth: what a 1-frame batch at 1080p needs (its
// later bounces are launches of 10^5 paths that do not fill the chip, vpt_render_async).
// A sample whose pixel lies outside the launch's screen rectangle of the scene's box (camera_cull.hpp; the host bounds the box per batch:
// api_render.hip batch_begin) never becomes a path, and the kernel never sees it: its camera ray could only miss, so the launch's indices are
// dealt over the samples inside the rectangle alone (whole_deal.hpp), the zero frame sums of the others are written in runs of whole-wave stores
// by the waves that deal the rectangle's rows, and their one ray each is a constant the launch adds to its count (53.8 % of the samples of Cornell
// 1080p: profiles/r18_whole_camera_cull_ab.md, profiles/r21_whole_deal_ab.md).
// A wave alternates two steps, each on full lanes:
//   trace   every lane holds a ray — a survivor of the shade step or a fresh camera ray — and finds its closest hit; misses run the
//           miss shader and end there, hits are parked in a wave-private ring in LDS (hit record + the path's registers);
//   shade   once the ring holds 64 hits: closest-hit shader, the <= 2 shadow queries, contribution, Russian roulette for those 64;
//           survivors keep their lanes for the next trace step.
// Per path this is k_bounce's arithmetic in k_bounce's order (same shade_core, same connect code), and which lane or wave runs a
// sample cannot matter: seeds come from (pixel, frame), results go to ACC[slot].  pathLight of a parked hit waits in ACC[slot].
template <class Pm, class Ps>
__device__ __forceinline__ V3 whole_finish(const Pm& P, const Ps& ps, uint32_t slot, V3 E, V3 thr_prev, V3 light_prev, const ShadeOut& o) {
    const V3 light = light_prev + path_contribution(E, thr_prev, o.cflags, P.max_luminance);
    if (o.terminated) ps.ACC[slot] = finite3(light) ? f4(v3s(0.0f) + light, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // end of the sample: the frame sum
    return light;
}
// Zero frame sums for slots [first, end), every lane of the wave storing (wave-uniform arguments).  A function of its own, not inlined: inlined, its
// registers raised the headline instantiation from 160 to 167 VGPRs, k_resolve (24) no longer fitted beside three of its waves on a SIMD, and a
// part's resolve ran past the next launch (profiles/r21_whole_deal_ab.md).  The margin is thin — 158 VGPRs reported, 160 allocated, and 8 B of
// scratch reserved for the call — and a compiler update can take it back without a word: tests/tools/spill_report.py shows the figure
// (k_whole<false, false, true> must stay at or below 160 VGPRs).
__device__ __attribute__((noinline)) void whole_zero_run(float4* acc, uint32_t first, uint32_t end) {
    for (uint32_t i = first + lane_id(); i < end; i += 64u) acc[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// Samples are dealt in tiles of 64 (consecutive pixels of a row).  Wave w of W takes tiles w, w + W, ... for the first `static_rounds` rounds
// without an atomic, and the tiles behind them `chunk_tiles` at a time through ctr->extend_head (the host picks both: api_render.hip batch_begin).
// (Measured and not kept: one-wave blocks, which leave the CU as soon as THEIR paths have ended and so let the next frame's launch in earlier —
// a 1-frame launch at 1080p 542 us against 509 us, and slower with two or three frames in flight too: profiles/r04_whole_lanes.json.)
template <bool COUNT, bool STRICT, bool PLAIN>
__global__ __launch_bounds__(kTraverseBlock, 3) void k_whole(WholeLaunch wl) {   // (ONE parameter: the argument segment is a WholeLaunch, a WholeArgs at its start)
    const WholeArgs& a = wl.a;
    // what runs once, before the loop, reads the arguments as any kernel does
    const DeviceScene sc = a.sc;
    const RenderParams P = a.P;
    Counters* const ctr = a.ctr;
    extern __shared__ __align__(16) unsigned char smem[];
    const TravStackT<kWholeStackRows> stack = make_stack<kWholeStackRows>(smem, sc.stack_overflow);
    float4* lds_nodes = reinterpret_cast<float4*>(smem + kWholeStackRows * kTraverseBlock * 4);
    float4* lds_tris = lds_nodes + sc.node_count * 8;
    // The camera lives in LDS between two refills and in no register.  camera_ray's part of P is read once per tile of 64 samples: from LDS there (a
    // uniform address broadcasts) instead of ~40 scalar registers held across the shade and trace steps; staged behind stage_scene's barrier.  Its
    // only other reader, shade_core's "next sample of the pixel" branch, is not compiled: the planner gives this kernel one-sample frames only
    // (path_plan.hpp whole_possible), a compile-time fact of WholeParams.  Cornell 1080p, same box, alternating: 8827-8833 Msamples/s against
    // 8641-8658 with the camera in scalar registers (profiles/r11_whole_uniform_ab.md).
    // The block (camera.hpp) also holds what camera_ray would compute alike for every sample of the launch: the camera's position, and whether the
    // lens sample can move it — with depth of field off it cannot, and camera_ray only draws it: 9374-9398 against 9266-9295 (profiles/r16_whole_camera_ab.md).
    __shared__ CameraBlock cam;
    if (threadIdx.x == 0u) fill_camera_block(cam, P.view_inv, P.proj_inv, P.width, P.height, P.focus_distance, P.dof_strength);
    // The loop's view of the arguments (whole_args.hpp): `a` again, where it lies in memory.  The loop reads the words of the scene, the parameters
    // and the path buffers from the kernel's argument segment where it uses them and holds none of them in registers across the trace loops.
    // Cornell 1080p, same box, alternating: 9250-9269 Msamples/s against 9100-9109 with the arguments held in registers and VGPR lanes
    // (profiles/r14_whole_uniforms_ab.md).
    const VPT_KERNARG WholeArgs* ka = (const VPT_KERNARG WholeArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    // The PLAIN instantiation's closest-hit search takes the two-slot step at half-empty nodes (node_step.hpp; the Cornell tree's nodes 1 and 2): their
    // child words are flagged here, in the LDS copy.  The other four keep the four-wide step and compile as they did — the counting and validating ones
    // make the same visits by construction, and the general one lost 0.4 % on the compact scene, whose tree has one such node in seven
    // (profiles/r22_narrow_node_ab.md).  In the light query the step was measured slower, and issued MORE instructions (profiles/REJECTED.md).
    constexpr bool NARROW = PLAIN && !COUNT && !STRICT;
#if VPT_LAB
    stage_scene<true, NARROW>(sc, lds_nodes, lds_tris, (a.chunk_tiles & kWholeNarrowOff) == 0u);   // (VPT_LAB_NARROW_OFF: no word is flagged, every step four-wide)
#else
    stage_scene<true, NARROW>(sc, lds_nodes, lds_tris);
#endif
    constexpr uint32_t kWaves = kTraverseBlock / 64u;
    __shared__ uint32_t r_slot[kWaves][128], r_prim[kWaves][128], r_inst[kWaves][128];
    __shared__ float r_t[kWaves][128], r_u[kWaves][128], r_v[kWaves][128];
    __shared__ float4 r_ra[kWaves][128], r_rb[kWaves][128], r_rt[kWaves][128];
    // the wave's fresh camera rays (whole_refill.hpp): slot, origin, direction, RNG state behind camera_ray; dword arrays, lane = bank
    __shared__ uint32_t f_slot[kWaves][refill::kTile], f_rng[kWaves][refill::kTile];
    __shared__ float f_ox[kWaves][refill::kTile], f_oy[kWaves][refill::kTile], f_oz[kWaves][refill::kTile];
    __shared__ float f_dx[kWaves][refill::kTile], f_dy[kWaves][refill::kTile], f_dz[kWaves][refill::kTile];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (uniform: the rings' and the buffer's rows are addressed from a scalar base)
    // tile cursor and fresh-ray buffer, wave-uniform by construction (wave_cursor.hpp DealCursor)
    const refill::Shape shape{a.n_slots, gridDim.x * kWaves, a.static_rounds, a.chunk_tiles};
    refill::Cursor cur = refill::make_cursor(shape, blockIdx.x * kWaves + wave);
    refill::Fresh fresh = refill::make_fresh();
    uint32_t hit_head = 0u, hit_count = 0u;   // wave-uniform
    TravStats st, sst; st.nodes = 0; st.tris = 0; sst.nodes = 0; sst.tris = 0;
    uint32_t w_paths = 0u, w_rays = 0u, w_hits0 = 0u, w_alive0 = 0u, w_rays0 = 0u, w_parked = 0u;   // wave totals (uniform); *0: bounce 0 only; parked: hits of later bounces (their pathLight waits in ACC)
    // the lane's path between two steps
    bool has_ray = false;
    uint32_t slot = 0u, rng_s = 0u, depth = 0u;
    bool in_medium = false;
    V3 porg = v3s(0.0f), pdir = v3s(0.0f), thr = v3s(1.0f), lightp = v3s(0.0f);
    float pdf = 1.0f;
    for (;;) {
        // The compiler knows that argument memory does not change and would load every word once, ahead of the loop — the registers this is about.
        // Behind this statement it no longer knows where `ka` points, so what a round of the loop reads through it is loaded in that round.
        asm volatile("" : "+s"(ka));
        const VPT_KERNARG WholeScene<STRICT, PLAIN>& usc = static_cast<const VPT_KERNARG WholeScene<STRICT, PLAIN>&>(ka->sc);
        const VPT_KERNARG WholeParams& uP = static_cast<const VPT_KERNARG WholeParams&>(ka->P);
        const VPT_KERNARG PathState& ups = ka->ps;
        // ---- shade: a chunk of parked hits (a partial one only when nothing can be added to it any more: no lane holds a ray here)
        if (hit_count >= 64u || (refill::exhausted(cur, fresh) && hit_count > 0u)) {
            const uint32_t cnt = hit_count < 64u ? hit_count : 64u;
            const bool valid = lane_id() < cnt;
            uint32_t nrays = 0u;
            bool first = false, alive = false;
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
                // pathLight so far: fetched behind the shader (three registers less across its peak), in flight during the shadow queries
                const V3 light_prev = first ? v3s(0.0f) : xyz(ups.ACC[slot]);
                // connect, inline (RayGen.slang:92-102)
                V3 E = o.emitted;
                if (o.want_sky) {
                    const bool rq = (uP.flags & VPT_FLAG_RAY_QUERIES) != 0u;
                    if (sky_visible<true, COUNT, NARROW>(usc, lds_nodes, lds_tris, o.sky_o, o.sky_d, stack, sst, rq)) E = E + o.csky;
                    nrays++;
                }
                if (o.want_light) {
                    if (light_visible<true, COUNT, NARROW>(usc, lds_nodes, lds_tris, o.light_o, o.light_d, o.light_gid, stack, sst)) E = E + o.clight;
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
            w_rays += (uint32_t)__popcll(__ballot(nrays >= 1u)) + (uint32_t)__popcll(__ballot(nrays >= 2u));
            w_rays0 += (uint32_t)__popcll(__ballot(first && nrays >= 1u)) + (uint32_t)__popcll(__ballot(first && nrays >= 2u));
            w_alive0 += (uint32_t)__popcll(__ballot(first && alive));
        }
        // ---- refill: free lanes take the next unstarted samples from the front of the wave's buffer; when it runs out, ALL lanes take the next
        // tile of launch indices and write their camera rays into the buffer.  A launch with a rectangle (camera_cull.hpp) deals its indices over
        // the samples inside it (whole_deal.hpp): a lane takes its index apart by the rectangle's size and width, where a launch without one divides
        // by shard_pixels and width (pixel_of_slot).  Either way every index is a path.
        if (!refill::exhausted(cur, fresh)) {
#pragma unroll 1
            for (;;) {
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
                    const uint32_t dispatch_base = uP.dispatch_base_dev ? *uP.dispatch_base_dev : ka->dispatch_base;   // (a replayed graph: the batch's first dispatch index lives in device memory)
                    uint32_t gslot = 0u, x = 0u, y = 0u, f = 0u;
                    // (a launch without a rectangle pays nothing for the other decode: `bounded` comes from two argument words, a scalar branch)
                    const VPT_KERNARG WholeLaunch* kl = (const VPT_KERNARG WholeLaunch*)ka;
                    const cull::Packed rect{kl->cull_x, kl->cull_y};
                    // The counting instantiations have one decode only — the library's size bound (tests/test_abi.py) has no room for the other five times —
                    // and the host gives their launches no rectangle (api_render.hip whole_cull_rect): their figures are those of the search itself.
                    const bool bounded = !COUNT && (rect.x != cull::kAxisAll || rect.y != cull::kAxisAll);
                    bool row_end = false, at_frame_end = false;
                    if (lane_id() < g) {
                        const uint32_t li = cur.w_next + lane_id();
                        if (uP.split != 1u) {   // split-screen dispatch: one decode, over the rectangle or the image (not what anything is timed on)
                            const uint32_t x0 = bounded ? cull::axis_first(rect.x) : 0u, y0 = bounded ? cull::axis_first(rect.y) : 0u;
                            deal::decode_split(x0, bounded ? x0 + cull::axis_span(rect.x) : uP.width - 1u, y0, bounded ? y0 + cull::axis_span(rect.y) : uP.height - 1u,
                                               uP.split, uP.width, uP.shard_pixels, uP.launch_off, dispatch_base, li, gslot, x, y, f);
                        } else if (bounded) {
                            const deal::Deal d{kl->deal.x0, kl->deal.rw, kl->deal.ys0, kl->deal.rect_px, 0u, kl->deal.last_in_frame, 0u, 0u};   // (argument words: scalar loads)
                            deal::decode(d, uP.shard_pixels, uP.width, uP.shard_rank, uP.shard_count, li, gslot, x, y, f);
                            row_end = x == kl->deal.x0 + kl->deal.rw - 1u; at_frame_end = deal::frame_end(d, uP.shard_pixels, f, gslot);
                        } else { gslot = li; pixel_of_slot(uP, li, x, y, f); }
                        const uint32_t seed = pcg_hash(uP.base_seed + dispatch_base + f);  // PathTracer.cpp:139 with an explicit seed
                        Rng r; r.s = y + uP.width * x + seed;                              // RayGen.slang:28
                        V3 go, gd;
                        camera_ray(cam, r, x, y, go, gd);
                        const uint32_t j = lane_id();
                        f_slot[wave][j] = gslot; f_rng[wave][j] = r.s;
                        f_ox[wave][j] = go.x; f_oy[wave][j] = go.y; f_oz[wave][j] = go.z;
                        f_dx[wave][j] = gd.x; f_dy[wave][j] = gd.y; f_dz[wave][j] = gd.z;
                    }
                    const bool first_tile = cur.w_next == 0u;
                    refill::generated(cur, fresh, g);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    // The samples outside the rectangle: their zero frame sums, in the runs between the rectangle's rows (whole_deal.hpp frame_end and run_after, on
                    // wave-uniform values).  The wave that deals a row's last sample writes the run behind it, and the one that deals index 0 the slots before.
                    if (bounded && uP.split == 1u) {
                        unsigned long long m_end = __ballot(row_end);
                        const unsigned long long m_last = __ballot(at_frame_end);
                        if (first_tile)
                            whole_zero_run(ups.ACC, 0u, kl->deal.head);
                        const deal::Deal dz{kl->deal.x0, kl->deal.rw, kl->deal.ys0, kl->deal.rect_px, kl->deal.gap, kl->deal.last_in_frame, kl->deal.head, kl->deal.slots};
                        while (m_end != 0ull) {
                            const uint32_t b = (uint32_t)__builtin_ctzll(m_end);
                            uint32_t first, end;
                            deal::run_after(dz, uP.shard_pixels, __builtin_amdgcn_readfirstlane(f_slot[wave][b]), ((m_last >> b) & 1ull) != 0ull, first, end);
                            m_end &= m_end - 1ull;
                            whole_zero_run(ups.ACC, first, end);
                        }
                    }
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
            if (has_ray) hit = trace_any<true, COUNT, NARROW>(usc, lds_nodes, lds_tris, porg, normalize(pdir), 0.01f, 100000.0f, stack, hr, st);
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
    // The samples outside the launch's rectangle, which no lane ever saw: one closest-hit ray each, as the paths they would have been.  The host
    // counted them (whole_deal.hpp culled); one lane of the launch adds the figure.
    if (!COUNT && blockIdx.x == 0u && threadIdx.x == 0u) {
        const unsigned long long culled = ((const VPT_KERNARG WholeLaunch*)ka)->culled;
        if (culled) {
            atomicAdd(&ctr->stat_closest, culled);
#if VPT_LAB
            atomicAdd(&ctr->whole_culled, (uint32_t)culled);   // (the laboratory reports them: vpt_lab_whole_culled)
#endif
        }
    }
    if (COUNT) {
        atomicAdd(&ctr->stat_nodes, (unsigned long long)st.nodes);
        atomicAdd(&ctr->stat_tris, (unsigned long long)st.tris);
        atomicAdd(&ctr->stat_shadow_nodes, (unsigned long long)sst.nodes);
        atomicAdd(&ctr->stat_shadow_tris, (unsigned long long)sst.tris);
    }
}

// Whole paths in one launch (k_whole): LDS-resident scenes without media, one sample per pixel and frame.
void launch_whole(hipStream_t s, uint32_t blocks, bool count, const DeviceScene& sc, const RenderParams& P, const PathState& ps, Counters* ctr, uint32_t n_slots,
                  uint32_t dispatch_base, bool plain, uint32_t static_rounds, uint32_t chunk_tiles, cull::Packed rect, const deal::Deal& deal, uint64_t culled) {
    const size_t lds = traverse_lds_bytes(sc, true, kWholeStackRows);
    const dim3 g(blocks), b(kTraverseBlock);
    // one launch site for the five instantiations (the argument marshalling is host code the library's size bound pays for five times otherwise)
    void (*k)(WholeLaunch);
    if (plain && !count && !sc.strict_hits && sc.env_black) k = k_whole<false, false, true>;
    else if (sc.strict_hits) k = count ? k_whole<true, true, false> : k_whole<false, true, false>;
    else k = count ? k_whole<true, false, false> : k_whole<false, false, false>;
    hipLaunchKernelGGL(k, g, b, lds, s, WholeLaunch{WholeArgs{sc, P, ps, ctr, n_slots, dispatch_base, static_rounds, chunk_tiles}, rect.x, rect.y, deal, culled});
}
int whole_blocks_per_cu(const DeviceScene& sc, bool plain) {
    int nb = 0;
    const size_t lds = traverse_lds_bytes(sc, true, kWholeStackRows);
    if (plain) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_whole<false, false, true>, kTraverseBlock, lds);
    else (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_whole<false, false, false>, kTraverseBlock, lds);
    return nb > 0 ? nb : 1;
}

}  // namespace vpt
