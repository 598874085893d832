// kernels_bounce.hip — k_bounce: one whole bounce per launch (camera ray or queued path, closest hit, shader, shadow queries, contribution, roulette),
// with and without media (VPT_PIPELINE_FUSED); launch_bounce and bounce_blocks_per_cu.
#include "kernels.hpp"
#include "traverse.hpp"
#include "wave.hpp"
#include "shade_core.hpp"
#include "vote.hpp"

namespace vpt {

// ------------------------------------------------------------------ primary: bounce 0, fully fused
// Bounce 0 is ~60 % of all path-bounces of a frame (every pixel has one; later bounces only see the
// survivors), its rays are coherent, and nothing about it has to be read from memory: the slot id gives
// pixel and frame, hence seed, RNG state and camera ray (RayGen.slang:12-64).  So the first bounce runs as one
// kernel — camera ray, closest hit, miss/closest-hit shader, the <= 2 shadow rays, contribution, Russian
// roulette — and only survivors write their records (A, B, T, L) and enter the wavefront queues.
// Finished paths write just the frame sum.  pathThroughput is 1 and pathLight is 0 on entry.
// The same kernel with FIRST = false runs every later bounce of scenes whose BVH rides in LDS (traversal is
// then a handful of LDS reads, so a separate extend/connect stage would only move records through HBM):
// it reads a queued path's records A, B, T, L, does the whole bounce, and writes them back for survivors.
// PLAIN: the scene class set this instantiation serves — every material's textures are 1x1 and the environment is black (the Cornell
// box; chosen by vpt_set_scene / vpt_set_material / vpt_set_environment, api_scene.hip update_depth_bounded by scene_prep.hpp plain).  The general kernel skips the texture taps and the
// environment sampler through uniform branches; here they are not compiled in at all (a quarter of the general kernel's instructions).
template <bool LDS_SCENE, bool COUNT, bool FIRST, bool VOL, bool STRICT, bool PLAIN = false>
__global__ __launch_bounds__(kTraverseBlock, 3) void k_bounce(DeviceScene sc, RenderParams P, PathState ps, StreamState ss, const uint32_t* queue,
                                                             uint32_t* queue_next, Counters* ctr, uint32_t parity, uint32_t n_slots,
                                                             uint32_t dispatch_base, uint32_t k3) {
    // compile-time constant from here on (VPT_FLAG_LOCAL_HITS picks the instantiation) — except in the media kernels (180 KB of code each, 688-720 B of
    // scratch per lane) and in the fused kernel on a tree in memory (VPT_PIPELINE_FUSED forced on a scene AUTO gives to the streams: half their rate),
    // which read the flag at run time: neither is near the speed of light, so one instantiation serves both hit rules
    if (!VOL && LDS_SCENE) sc.strict_hits = STRICT ? 1u : 0u;
    if (PLAIN) { sc.all_plain = 1u; sc.env_black = 1u; } else sc.all_plain = 0u;   // likewise
    if (FIRST && P.dispatch_base_dev) dispatch_base = *P.dispatch_base_dev;   // a replayed graph: the batch's first dispatch index lives in device memory
    const bool rq = (P.flags & VPT_FLAG_RAY_QUERIES) != 0u;   // USE_RAY_QUERIES (RTCommon.slang:52 / :64): which interval and direction the shadow and distance queries use
    extern __shared__ __align__(16) unsigned char smem[];
    const TravStack stack = make_stack(smem, sc.stack_overflow);
    float4* lds_nodes = reinterpret_cast<float4*>(smem + kStackDepth * kTraverseBlock * 4);
    float4* lds_tris = lds_nodes + sc.node_count * 8;
    stage_scene<LDS_SCENE>(sc, lds_nodes, lds_tris);
    // Queue k3 (= bounce index % 3) is read, queue k3 + 1 appended to, the words of queue k3 + 2 zeroed for the bounce after the
    // next: no reset kernel between two bounces.  A queue's length (holes included) is its static part — one chunk per wave
    // that took part in the producing launch, or nothing when that launch appended exactly — plus the dynamically reserved part.
    const uint32_t kn = (k3 + 1u) % 3u, kz = (k3 + 2u) % 3u;
    const uint32_t n = FIRST ? n_slots : ctr->rc3_static[k3] + ctr->rc3[k3];
    const uint32_t waves = gridDim.x * (kTraverseBlock / 64u);
    const uint32_t need = (n + 63u) / 64u, active = need < waves ? need : waves;
    const bool exact = n < kFusedExactBelow;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctr->rc3_static[kn] = exact ? 0u : active * kAppendChunk;
        ctr->rc3[kz] = 0u; ctr->alive3[kz] = 0u;
    }
    // Long queues: wave-private chunked appends (vote.hpp).  Short ones (< kFusedExactBelow entries): the block's four waves
    // add up their survivors in LDS and reserve them with ONE atomic per 256 paths, exactly — no holes, and few enough atomics
    // for a kernel whose whole launch takes ~0.1 ms at that size (one per wave would saturate the counter, ~88 / us).
    __shared__ uint32_t s_cnt[kTraverseBlock / 64u];
    __shared__ uint32_t s_base[kTraverseBlock / 64u];
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t gw = blockIdx.x * (kTraverseBlock / 64u) + wave;
    if (!exact && gw >= active) return;   // (after the block-wide staging above) this wave owns no chunk and no work
    WaveAppender a_next;
    a_next.init(gw, false, active * kAppendChunk);   // chunked mode: the counter rc3[kn] counts what is reserved beyond the static chunks
    TravStats st, sst; st.nodes = 0; st.tris = 0; sst.nodes = 0; sst.tris = 0;
    uint32_t w_paths = 0u, w_alive = 0u, w_rays = 0u, w_hits = 0u;  // wave totals (uniform)
    // Regrouping (long queues of the plain later bounces): a wave does not run the closest-hit shader on the 64 paths it has just
    // traced.  Its misses are finished at once (the miss shader is short), its hits are parked — hit record, ray and throughput
    // records — in a wave-private ring in LDS, and the closest-hit shader and the shadow queries run on FULL chunks of 64 hits
    // whenever the ring has that many (the partial last chunk is flushed at the end).  Queue holes vanish on the way.  Without it
    // a wave drags its misses and holes through the whole closest-hit shader as idle lanes (Cornell bounces: 41 of 64 lanes
    // active, 49 with it).  Every record is still read once, as a coalesced stream, except pathLight, which a parked hit fetches
    // when its chunk runs.  Results cannot change: every path gets exactly its own records and hit.
    const bool regroup = !FIRST && !VOL && !exact;   // (bounce 0: its camera rays are coherent; regrouping them measured 12 % slower)
    __shared__ uint32_t r_idx[kTraverseBlock / 64u][128], r_prim[kTraverseBlock / 64u][128], r_inst[kTraverseBlock / 64u][128];
    __shared__ float r_t[kTraverseBlock / 64u][128], r_u[kTraverseBlock / 64u][128], r_v[kTraverseBlock / 64u][128];
    __shared__ float4 r_ra[kTraverseBlock / 64u][128], r_rb[kTraverseBlock / 64u][128], r_rt[kTraverseBlock / 64u][128];
    uint32_t hit_head = 0u, hit_count = 0u;   // wave-uniform
    uint32_t tile = blockIdx.x;
    for (;;) {
        {
            const bool tiles_done = tile * kTraverseBlock >= n;
            uint32_t idx = 0u, slot = kHole;
            bool alive = false, hit = false, valid = false;
            uint32_t nrays = 0u;
            ShadeOut o;
            V3 light = v3s(0.0f);
            ShadeIn in_;
            V3 light_prev = v3s(0.0f);
            bool aborted = false;
            const bool pop_hits = regroup && (hit_count >= 64u || (tiles_done && hit_count > 0u));
            if (pop_hits) {   // a chunk of parked hits
                const uint32_t cnt = hit_count < 64u ? hit_count : 64u;
                valid = lane_id() < cnt;
                if (valid) {
                    const uint32_t q = (hit_head + lane_id()) & 127u;
                    idx = r_idx[wave][q];
                    const float4 a = r_ra[wave][q], b = r_rb[wave][q], t = r_rt[wave][q];
                    slot = queue[idx];
                    in_.rng = __float_as_uint(a.w);
                    in_.porg = xyz(a); in_.pdir = xyz(b);
                    const uint32_t dw = __float_as_uint(b.w);
                    in_.depth = dw & 0x7fffffffu; in_.in_medium = (dw >> 31) != 0u;
                    in_.thr_prev = xyz(t); in_.prev_pdf = t.w;
                    light_prev = xyz(ss.RL[parity][idx]);
                    in_.vdepth = 0u; in_.cchan = -1;
                    in_.vol_index = -1; in_.vol_t = 0.0f; in_.atm_comp = -1;
                    hit = true;
                    in_.h = make_float4(r_t[wave][q], r_u[wave][q], r_v[wave][q], __uint_as_float(r_prim[wave][q]));
                    in_.inst = r_inst[wave][q];
                }
                hit_head += cnt; hit_count -= cnt;
            } else if (!tiles_done) {
                idx = tile * kTraverseBlock + threadIdx.x;
                tile += gridDim.x;
                slot = FIRST ? idx : (idx < n ? queue[idx] : kHole);
                valid = idx < n && slot != kHole;
                HitRec hr;
                float4 rec_a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rec_b = rec_a, rec_t = rec_a;
                if (valid) {
                    if (FIRST) {
                        uint32_t x, y, f;
                        launch_pixel(P, idx, dispatch_base, slot, x, y, f);
                        uint32_t seed = pcg_hash(P.base_seed + dispatch_base + f);  // PathTracer.cpp:139 with an explicit seed
                        Rng r; r.s = y + P.width * x + seed;                        // RayGen.slang:28
                        camera_ray(P, r, x, y, in_.porg, in_.pdir);
                        in_.rng = r.s; in_.depth = 0u; in_.in_medium = false; in_.thr_prev = v3s(1.0f); in_.prev_pdf = 1.0f;
                        in_.vdepth = 0u; in_.cchan = -1;
                        if (P.samples_per_frame > 1) ps.sidx[slot] = 0u;
                    } else {   // the path's records, in queue order
                        const float4 a = ss.RA[parity][idx], b = ss.RB[parity][idx], t = ss.RT[parity][idx];
                        rec_a = a; rec_b = b; rec_t = t;
                        in_.rng = __float_as_uint(a.w);
                        in_.porg = xyz(a); in_.pdir = xyz(b);
                        uint32_t dw = __float_as_uint(b.w);
                        in_.depth = dw & 0x7fffffffu; in_.in_medium = (dw >> 31) != 0u;
                        in_.vdepth = VOL ? ps.vdepth[slot] : 0u;
                        in_.cchan = (VOL && sc.atm_on) ? ps.cchan[slot] : -1;
                        in_.thr_prev = xyz(t); in_.prev_pdf = t.w;
                        light_prev = xyz(ss.RL[parity][idx]);
                    }
                    in_.vol_index = -1; in_.vol_t = 0.0f; in_.atm_comp = -1;
                    // RayGen.slang:76-84: a path whose origin is below the planet's surface leaves the loop at once
                    aborted = VOL && sc.atm_on && atmosphere_height(sc, in_.porg) < 0.0f;
                    if (VOL && !aborted) {  // ScatteredInVolume (RayGen.slang:86): GetDistanceToGeometry uses the payload direction as is,
                                            // TMin 1e-5, TMax 1e6 (RTCommon.slang:86-101)
                        // (without USE_RAY_QUERIES: RTCommon.slang:103-117 — normalised direction, TMax 1000)
                        bool g = trace_any<LDS_SCENE, COUNT>(sc, lds_nodes, lds_tris, in_.porg, rq ? in_.pdir : normalize(in_.pdir), 0.00001f, rq ? 1000000.0f : 1000.0f, stack, hr, st);
                        Rng vr; vr.s = in_.rng;
                        int cc;
                        in_.vol_index = scattered_in_media(sc, in_.porg, in_.pdir, vr, g ? hr.t : -1.0f, (float)in_.depth, in_.cchan, in_.vol_t, in_.atm_comp, cc);
                        if (in_.vol_index == -2) in_.cchan = cc;  // the path now tracks this colour channel only (:242-247)
                        in_.rng = vr.s;
                    }
                    if (!VOL || (!aborted && in_.vol_index == -1))
                        hit = trace_any<LDS_SCENE, COUNT>(sc, lds_nodes, lds_tris, in_.porg, normalize(in_.pdir), 0.01f, 100000.0f, stack, hr, st);
                    in_.h = make_float4(hit ? hr.t : -1.0f, hr.u, hr.v, __uint_as_float(hr.gid));
                    in_.inst = hr.inst;
                }
                if (regroup) {   // park the hits (the ring holds < 64 entries here, so 128 slots are enough); the misses go on below
                    const unsigned long long mh = __ballot(valid && hit);
                    if (valid && hit) {
                        const uint32_t q = (hit_head + hit_count + lanes_below(mh)) & 127u;
                        r_idx[wave][q] = idx; r_t[wave][q] = hr.t; r_u[wave][q] = hr.u; r_v[wave][q] = hr.v; r_prim[wave][q] = hr.gid; r_inst[wave][q] = hr.inst;
                        r_ra[wave][q] = rec_a; r_rb[wave][q] = rec_b; r_rt[wave][q] = rec_t;
                    }
                    hit_count += (uint32_t)__popcll(mh);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    valid = valid && !hit;
                    if (__ballot(valid) == 0ull) continue;
                }
            } else {
                break;
            }
            if (valid) {
                if (VOL && aborted) {
                    o.want_sky = false; o.want_light = false; o.emitted = v3s(0.0f); o.csky = v3s(0.0f); o.clight = v3s(0.0f);
                    o.rng = in_.rng; o.new_depth = in_.depth; o.new_o = in_.porg; o.new_d = in_.pdir; o.new_pdf = in_.prev_pdf; o.bxdf = v3s(1.0f);
                    o.in_medium = in_.in_medium; o.vdepth = in_.vdepth; o.cchan = in_.cchan; o.light_gid = 0xffffffffu; o.light_miss_ok = false;
                } else {
                    shade_core<VOL>(sc, P, ps, slot, in_, o);
                }
            // connect, inline (RayGen.slang:92-102; FIRST: pathThroughput == 1, pathLight == 0)
                V3 E = o.emitted;
                if (!VOL && o.want_sky) {
                    if (sky_visible<LDS_SCENE, COUNT>(sc, lds_nodes, lds_tris, o.sky_o, o.sky_d, stack, sst, rq)) E = E + o.csky;
                    nrays++;
                }
                if (VOL && o.want_sky) {  // the sky term is assembled now: its transmittance draws come after the visibility test
                    nrays++;
                    if (sky_visible<LDS_SCENE, COUNT>(sc, lds_nodes, lds_tris, o.sky_o, o.sky_d, stack, sst, rq)) {
                        Rng tr_rng; tr_rng.s = o.rng;
                        V3 csky;
                        if (o.sky_kind == 2) {        // RayGen.slang:405-424: (phase * T_atm * T_boxes) * (sun / pdf)
                            V3 tr = atmosphere_transmittance(sc, tr_rng, o.sky_o, o.sky_d, o.cchan);
                            tr = tr * volumes_transmittance(sc, tr_rng, o.sky_o, o.sky_d, o.sky_tdepth);
                            csky = (o.sky_f * tr) * (o.sky_rgb / o.sky_w);
                        } else {
                            V3 tr = v3s(volumes_transmittance(sc, tr_rng, o.new_o, o.sky_d, o.sky_tdepth));  // from the new origin (ClosestHit.slang:332-349, RayGen.slang:325-343)
                            if (sc.atm_on) tr = nee_atmosphere_transmittance(sc, tr_rng, tr, o.new_o, o.sky_d, o.cchan);
                            if (o.sky_kind == 0) csky = ((o.sky_f * tr) * o.sky_rgb / o.sky_w) * o.sky_mis;
                            else csky = ((tr * o.sky_f) * (o.sky_rgb / o.sky_w)) * o.sky_mis;
                        }
                        o.rng = tr_rng.s;
                        if (o.sky_add) E = E + csky;
                    }
                }
                if (o.want_light) {
                    bool vis = light_visible<LDS_SCENE, COUNT>(sc, lds_nodes, lds_tris, o.light_o, o.light_d, o.light_gid, stack, sst);
                    if (VOL && !vis && o.light_miss_ok) vis = sky_visible<LDS_SCENE, COUNT>(sc, lds_nodes, lds_tris, o.light_o, o.light_d, stack, sst, true);   // (light rays exist with USE_RAY_QUERIES only)
                    if (VOL) {
                        if (vis) {  // ClosestHit.slang:361-370, RayGen.slang:348-361: the light term with the box transmittance
                            Rng tr_rng; tr_rng.s = o.rng;
                            V3 tr = v3s(volumes_transmittance(sc, tr_rng, o.new_o, o.light_d, o.light_tdepth));
                            o.rng = tr_rng.s;
                            V3 cl = o.light_kind == 0 ? ((o.light_f * tr) * o.light_rgb / o.light_w) * o.light_mis
                                                      : ((tr * o.light_f) * (o.light_rgb / o.light_w)) * o.light_mis;
                            if (o.light_add) E = E + cl;
                        }
                    } else if (vis) {
                        E = E + o.clight;
                    }
                    nrays++;
                }
                const int fin_chan = VOL ? o.cchan : -1;  // the channel this sample is accumulated in (RayGen.slang:118-128)
                if (VOL) shade_tail_media(P, ps, slot, in_.thr_prev, aborted, o);
                light = light_prev + path_contribution(E, in_.thr_prev, o.cflags, P.max_luminance);
                if (VOL && aborted) light = light_prev;  // the loop was left before anything was added
                if (o.terminated) {  // end of a sample: NaN/Inf guard, frame sum (RayGen.slang:116-128)
                    const bool ok = finite3(light);
                    if (VOL && fin_chan != -1) light = v3(fin_chan == 0 ? light.x : 0.0f, fin_chan == 1 ? light.y : 0.0f, fin_chan == 2 ? light.z : 0.0f);
                    if (FIRST || P.samples_per_frame == 1) {  // first (or only) finalisation of the slot: 0 + pathLight
                        ps.ACC[slot] = ok ? f4(v3s(0.0f) + light, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    } else if (ok) {
                        float4 acc = ps.ACC[slot]; ps.ACC[slot] = f4(xyz(acc) + light, 0.0f);
                    }
                    light = v3s(0.0f);
                } else if (FIRST && P.samples_per_frame > 1) {
                    ps.ACC[slot] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // later finalisations add to it
                }
                alive = o.alive;
                if (alive && VOL) { ps.vdepth[slot] = o.vdepth; if (sc.atm_on) ps.cchan[slot] = o.cchan; }
            }
            // survivors: the queue entry and, with it, the path's records go to the next queue (wave-private chunked append)
            uint32_t pn;
            if (!exact) pn = a_next.append(alive, &ctr->rc3[kn]);
            else {
                const unsigned long long ma = __ballot(alive);
                if (lane_id() == 0) s_cnt[wave] = (uint32_t)__popcll(ma);
                __syncthreads();
                if (threadIdx.x == 0) {
                    uint32_t sum = 0u, pre[kTraverseBlock / 64u];
                    for (uint32_t w = 0; w < kTraverseBlock / 64u; w++) { pre[w] = sum; sum += s_cnt[w]; }
                    const uint32_t b = sum ? atomicAdd(&ctr->rc3[kn], sum) : 0u;
                    for (uint32_t w = 0; w < kTraverseBlock / 64u; w++) s_base[w] = b + pre[w];
                }
                __syncthreads();
                pn = s_base[wave] + lanes_below(ma);
            }
            if (alive) {
                queue_next[pn] = slot;
                ss.RA[parity ^ 1u][pn] = f4u(o.new_o, o.rng);
                ss.RB[parity ^ 1u][pn] = f4u(o.new_d, o.new_depth | (o.in_medium ? 0x80000000u : 0u));
                ss.RT[parity ^ 1u][pn] = f4(o.thr, o.new_pdf);
                ss.RL[parity ^ 1u][pn] = f4(light, 0.0f);
            }
            w_paths += (uint32_t)__popcll(__ballot(valid));
            w_alive += (uint32_t)__popcll(__ballot(alive));
            w_rays += (uint32_t)__popcll(__ballot(nrays >= 1u)) + (uint32_t)__popcll(__ballot(nrays >= 2u));
            w_hits += (uint32_t)__popcll(__ballot(hit));
        }
    }
    if (!exact) for (uint32_t j = lane_id(); j < a_next.tail_count(); j += 64u) queue_next[a_next.tail_first() + j] = kHole;  // the unwritten tail of the wave's last chunk
    if (lane_id() == 0) {
        if (w_alive) atomicAdd(&ctr->alive3[kn], w_alive);
        if (w_paths) atomicAdd(&ctr->stat_closest, (unsigned long long)w_paths);
        if (w_rays) atomicAdd(&ctr->stat_shadow, (unsigned long long)w_rays);
        if (FIRST) {
            if (w_hits) atomicAdd(&ctr->stat_primary_hits, (unsigned long long)w_hits);
            if (w_alive) atomicAdd(&ctr->stat_primary_alive, (unsigned long long)w_alive);
            if (w_rays) atomicAdd(&ctr->stat_primary_rays, (unsigned long long)w_rays);
        }
    }
    if (COUNT) {
        atomicAdd(&ctr->stat_nodes, (unsigned long long)st.nodes);
        atomicAdd(&ctr->stat_tris, (unsigned long long)st.tris);
        atomicAdd(&ctr->stat_shadow_nodes, (unsigned long long)sst.nodes);
        atomicAdd(&ctr->stat_shadow_tris, (unsigned long long)sst.tris);
    }
}

// first == true: bounce 0 of n_slots fresh slots (queue unused); otherwise one fused bounce of queue[parity].
void launch_bounce(hipStream_t s, uint32_t blocks, bool lds_scene, bool count, bool first, const DeviceScene& sc, const RenderParams& P,
                   const PathState& ps, const StreamState& ss, const uint32_t* queue, uint32_t* queue_next, Counters* ctr, uint32_t parity, uint32_t n_slots,
                   uint32_t dispatch_base, uint32_t k3, bool plain) {
    const size_t lds = traverse_lds_bytes(sc, lds_scene, kStackDepth);
    const dim3 g(blocks), b(kTraverseBlock);
    // one launch site for the sixteen instantiations: each site copies the scene, the parameters and both path states by value, host code the library's
    // size bound (DESIGN.md "Library size") would pay for sixteen times
    void (*k)(DeviceScene, RenderParams, PathState, StreamState, const uint32_t*, uint32_t*, Counters*, uint32_t, uint32_t, uint32_t, uint32_t);
    if (plain && lds_scene && !count && !sc.strict_hits && sc.volume_count == 0u && !sc.atm_on && sc.env_black) {   // the scene-class instantiation
        k = first ? k_bounce<true, false, true, false, false, true> : k_bounce<true, false, false, false, false, true>;
    } else if (sc.volume_count > 0u || sc.atm_on) {  // the media variants carry no traversal counters and read VPT_FLAG_LOCAL_HITS at run time
        if (lds_scene) k = first ? k_bounce<true, false, true, true, false> : k_bounce<true, false, false, true, false>;
        else k = first ? k_bounce<false, false, true, true, false> : k_bounce<false, false, false, true, false>;
    } else if (lds_scene) {
        const bool strict = sc.strict_hits;
        if (count) {
            if (first) k = strict ? k_bounce<true, true, true, false, true> : k_bounce<true, true, true, false, false>;
            else k = strict ? k_bounce<true, true, false, false, true> : k_bounce<true, true, false, false, false>;
        } else {
            if (first) k = strict ? k_bounce<true, false, true, false, true> : k_bounce<true, false, true, false, false>;
            else k = strict ? k_bounce<true, false, false, false, true> : k_bounce<true, false, false, false, false>;
        }
    } else {   // a tree in memory: the hit rule is read at run time (above), and the visit counters always run (two adds per visit in a kernel
               // that is the slow side of an A/B anyway: one instantiation per bounce kind instead of four)
        k = first ? k_bounce<false, true, true, false, false> : k_bounce<false, true, false, false, false>;
    }
    hipLaunchKernelGGL(k, g, b, lds, s, sc, P, ps, ss, queue, queue_next, ctr, parity, n_slots, dispatch_base, k3);
}
int bounce_blocks_per_cu(bool lds_scene, const DeviceScene& sc, bool plain) {
    int nb = 0;
    size_t lds = traverse_lds_bytes(sc, lds_scene, kStackDepth);
    if (lds_scene && plain) {   // the smaller of the two instantiations a batch launches
        int a = 0, b = 0;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_bounce<true, false, true, false, false, true>, kTraverseBlock, lds);
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_bounce<true, false, false, false, false, true>, kTraverseBlock, lds);
        nb = a < b ? a : b;
        return nb > 0 ? nb : 1;
    }
    if (lds_scene) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_bounce<true, false, false, false, false>, kTraverseBlock, lds);
    else (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_bounce<false, true, false, false, false>, kTraverseBlock, lds);
    return nb > 0 ? nb : 1;
}

}  // namespace vpt

// The media stages' kernels ride in this translation unit (same flags; one fat binary and its page padding less: DESIGN.md "Library size").
#include "kernels_media.hip"
