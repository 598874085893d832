// kernels_lab_r1.hip — round 1's stage kernels (VPT_PIPELINE_STAGED_R1): raygen, extend, shade, connect and the two counter kernels between them, with their
// launchers and occupancy helpers.  Laboratory library only (_build.LAB_SOURCES): the product neither compiles nor declares any of it.
#include "kernels.hpp"
#include "traverse.hpp"
#include "wave_cursor.hpp"
#include "shade_core.hpp"

namespace vpt {

static inline uint32_t cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// ------------------------------------------------------------------ raygen (round 1's staged pipeline only)
// Scenes whose BVH does not fit in LDS run bounce 0 through the same extend / shade / connect stages as every
// other bounce, so the camera rays are written out as ordinary path records.
__global__ __launch_bounds__(256) void k_raygen(RenderParams P, PathState ps, uint32_t* queue, Counters* ctr, uint32_t n_slots, uint32_t dispatch_base) {
    uint32_t li = blockIdx.x * blockDim.x + threadIdx.x;
    if (li == 0u) ctr->ray_count[0] = n_slots;  // the counters were zeroed at the start of the batch
    if (li >= n_slots) return;
    uint32_t slot, x, y, f;
    launch_pixel(P, li, dispatch_base, slot, x, y, f);
    uint32_t seed = pcg_hash(P.base_seed + dispatch_base + f);  // PathTracer.cpp:139 with an explicit seed
    Rng r; r.s = y + P.width * x + seed;                        // RayGen.slang:28
    V3 o, d;
    camera_ray(P, r, x, y, o, d);
    ps.A[slot] = f4u(o, r.s);
    ps.B[slot] = f4u(d, 0u);
    ps.T[0][slot] = make_float4(1.0f, 1.0f, 1.0f, 1.0f);  // pathThroughput = 1, payload.PDF = 1
    ps.L[slot] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (P.samples_per_frame > 1) { ps.ACC[slot] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); ps.sidx[slot] = 0u; }
    queue[li] = slot;
}
void launch_raygen(hipStream_t s, const RenderParams& P, const PathState& ps, uint32_t* queue, Counters* ctr, uint32_t n_slots, uint32_t dispatch_base) {
    hipLaunchKernelGGL(k_raygen, dim3(cdiv(n_slots, 256)), dim3(256), 0, s, P, ps, queue, ctr, n_slots, dispatch_base);
}

// ------------------------------------------------------------------ extend: closest hit of every queued path (round 1's stage kernels)
template <bool LDS_SCENE, bool COUNT, bool STRICT>
__global__ __launch_bounds__(kTraverseBlock, 8) void k_extend(DeviceScene sc, PathState ps, const uint32_t* queue,
                                                          Counters* ctr, uint32_t parity) {
    sc.strict_hits = STRICT ? 1u : 0u;  // compile-time constant from here on (VPT_FLAG_LOCAL_HITS picks the instantiation)
    extern __shared__ __align__(16) unsigned char smem[];
    const TravStack stack = make_stack(smem, sc.stack_overflow);
    float4* lds_nodes = reinterpret_cast<float4*>(smem + kStackDepth * kTraverseBlock * 4);
    float4* lds_tris = lds_nodes + sc.node_count * 8;
    stage_scene<LDS_SCENE>(sc, lds_nodes, lds_tris);
    const uint32_t n = ctr->ray_count[parity];
    const uint32_t chunk = fetch_chunk(n);
    TravStats st; st.nodes = 0; st.tris = 0;
    while (true) {
        uint32_t base = 0;
        if (lane_id() == 0) base = atomicAdd(&ctr->extend_head, chunk);
        base = __shfl(base, 0);
        if (base >= n) break;
        for (uint32_t k = 0; k < chunk; k += 64) {
            uint32_t i = base + k + lane_id();
            if (i >= n) break;
            uint32_t slot = queue[i];
            float4 a = ps.A[slot], b = ps.B[slot];
            V3 d = normalize(xyz(b));  // RayGen.slang:70
            HitRec h;
            bool found = trace_any<LDS_SCENE, COUNT>(sc, lds_nodes, lds_tris, xyz(a), d, 0.01f, 100000.0f, stack, h, st);
            ps.H[slot] = make_float4(found ? h.t : -1.0f, h.u, h.v, __uint_as_float(h.gid));   // the shade stage addresses the triangle's shading record by global id
            ps.hinst[slot] = h.inst;
        }
    }
    if (COUNT) {
        atomicAdd(&ctr->stat_nodes, (unsigned long long)st.nodes);
        atomicAdd(&ctr->stat_tris, (unsigned long long)st.tris);
    }
}
void launch_extend(hipStream_t s, uint32_t blocks, bool lds_scene, bool count, const DeviceScene& sc, const PathState& ps,
                   const uint32_t* queue, Counters* ctr, uint32_t parity) {
    size_t lds = traverse_lds_bytes(sc, lds_scene, kStackDepth);
    const bool strict = sc.strict_hits != 0u;
    void (*k)(DeviceScene, PathState, const uint32_t*, Counters*, uint32_t);
    if (lds_scene) k = count ? (strict ? k_extend<true, true, true> : k_extend<true, true, false>) : (strict ? k_extend<true, false, true> : k_extend<true, false, false>);
    else k = count ? (strict ? k_extend<false, true, true> : k_extend<false, true, false>) : (strict ? k_extend<false, false, true> : k_extend<false, false, false>);
    hipLaunchKernelGGL(k, dim3(blocks), dim3(kTraverseBlock), lds, s, sc, ps, queue, ctr, parity);
}

// ------------------------------------------------------------------ shade (round 1's stage kernels)
// One path per lane: miss shader or closest-hit shader, then the tail of the reference's bounce loop that
// does not depend on visibility (throughput update, Russian roulette, termination, next-sample
// regeneration).  Survivors are ballot-compacted into the next ray queue; paths with anything pending
// (emission, NEE candidates, end of sample) are compacted into the connect queue — entries that carry
// shadow rays from the front, the others from the back, so a wave of the connect kernel is homogeneous.
// Result bits of shade_path()
constexpr uint32_t kSP_Alive = 1u, kSP_Front = 2u, kSP_Back = 4u;  // bits 3-4: number of shadow rays queued

__device__ __forceinline__ uint32_t shade_path(const DeviceScene& sc, const RenderParams& P, const PathState& ps,
                                               const float4* Tin, float4* Tout, uint32_t slot) {
    float4 a = ps.A[slot], b = ps.B[slot], t = Tin[slot];
    ShadeIn in_;
    in_.h = ps.H[slot];
    in_.inst = in_.h.x < 0.0f ? 0u : ps.hinst[slot];
    in_.rng = __float_as_uint(a.w);
    in_.porg = xyz(a); in_.pdir = xyz(b);
    uint32_t dw = __float_as_uint(b.w);
    in_.depth = dw & 0x7fffffffu; in_.in_medium = (dw >> 31) != 0u;
    in_.thr_prev = xyz(t); in_.prev_pdf = t.w;
    in_.vol_index = -1; in_.vol_t = 0.0f; in_.vdepth = 0u; in_.cchan = -1; in_.atm_comp = -1;
    ShadeOut o;
    shade_core<false>(sc, P, ps, slot, in_, o);
    if (o.alive) {
        ps.A[slot] = f4u(o.new_o, o.rng);
        ps.B[slot] = f4u(o.new_d, o.new_depth | (o.in_medium ? 0x80000000u : 0u));
        Tout[slot] = f4(o.thr, o.new_pdf);
    }
    const V3 tp = in_.thr_prev;
    bool thr_finite = !isinf_(tp.x) && !isinf_(tp.y) && !isinf_(tp.z) && !isnan_(tp.x) && !isnan_(tp.y) && !isnan_(tp.z);
    // 0 * inf = NaN must still reach pathLight, so a non-finite throughput always goes through connect
    bool pending = o.want_sky || o.want_light || o.terminated || o.emitted.x != 0.0f || o.emitted.y != 0.0f || o.emitted.z != 0.0f || !thr_finite;
    if (pending) {
        ps.CE[slot] = f4u(o.emitted, o.cflags);
        if (o.want_sky) {
            ps.CS[slot] = f4(o.csky, 0.0f);
            ps.CSO[slot] = f4(o.sky_o, o.sky_d.x);
            ps.CSD[slot] = make_float4(o.sky_d.y, o.sky_d.z, 0.0f, 0.0f);
        }
        if (o.want_light) {
            ps.CL[slot] = f4u(o.clight, o.light_gid);
            ps.CLO[slot] = f4(o.light_o, o.light_d.x);
            ps.CLD[slot] = make_float4(o.light_d.y, o.light_d.z, 0.0f, 0.0f);
        }
    }
    bool has_rays = o.want_sky || o.want_light;
    return (o.alive ? kSP_Alive : 0u) | ((pending && has_rays) ? kSP_Front : 0u) | ((pending && !has_rays) ? kSP_Back : 0u) |
           (((o.want_sky ? 1u : 0u) + (o.want_light ? 1u : 0u)) << 3);
}

// A block shades tiles of cpt x 256 paths (cpt = 1..4 per thread) and reserves queue space with ONE atomic
// per counter per tile; cpt grows with the queue so a launch issues at most ~8k atomics per counter.

__global__ __launch_bounds__(256, 3) void k_shade(DeviceScene sc, RenderParams P, PathState ps, const uint32_t* queue,
                                               uint32_t* queue_next, uint32_t* cqueue, Counters* ctr, uint32_t parity) {
    __shared__ uint32_t s_cnt[4][4];
    __shared__ uint32_t s_base[4][3];
    const uint32_t n = ctr->ray_count[parity];
    const float4* Tin = ps.T[parity];
    float4* Tout = ps.T[parity ^ 1u];
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t cpt = (n + (1u << 21) - 1u) >> 21;
    cpt = cpt < 1u ? 1u : (cpt > 4u ? 4u : cpt);
    const uint32_t tile_size = cpt * 256u;
    for (uint32_t tile = blockIdx.x * tile_size; tile < n; tile += gridDim.x * tile_size) {
        uint32_t s0 = 0u, s1 = 0u, s2 = 0u, s3 = 0u, res = 0u;  // slots and 5-bit results of this lane's 4 paths
        uint32_t tot_alive = 0u, tot_front = 0u, tot_back = 0u, tot_rays = 0u;  // wave totals
#pragma unroll 1
        for (uint32_t c = 0; c < cpt; c++) {
            uint32_t i = tile + c * 256u + threadIdx.x;
            uint32_t r = 0u, slot = 0u;
            if (i < n) {
                slot = queue[i];
                r = shade_path(sc, P, ps, Tin, Tout, slot);
            }
            s0 = (c == 0u) ? slot : s0; s1 = (c == 1u) ? slot : s1; s2 = (c == 2u) ? slot : s2; s3 = (c == 3u) ? slot : s3;
            res |= r << (c * 5u);
            tot_alive += (uint32_t)__popcll(__ballot((r & kSP_Alive) != 0u));
            tot_front += (uint32_t)__popcll(__ballot((r & kSP_Front) != 0u));
            tot_back += (uint32_t)__popcll(__ballot((r & kSP_Back) != 0u));
            tot_rays += (uint32_t)__popcll(__ballot((r & 8u) != 0u)) + 2u * (uint32_t)__popcll(__ballot((r & 16u) != 0u));
        }
        // block-level reservation: one atomic per counter per 1024 paths
        if (lane_id() == 0) { s_cnt[wave][0] = tot_alive; s_cnt[wave][1] = tot_front; s_cnt[wave][2] = tot_back; s_cnt[wave][3] = tot_rays; }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t sum[4] = {0u, 0u, 0u, 0u};
            uint32_t pre[4][3];
            for (uint32_t w = 0; w < 4; w++)
                for (uint32_t q = 0; q < 4; q++) { if (q < 3) pre[w][q] = sum[q]; sum[q] += s_cnt[w][q]; }
            uint32_t b_alive = sum[0] ? atomicAdd(&ctr->ray_count[parity ^ 1u], sum[0]) : 0u;
            uint32_t b_front = sum[1] ? atomicAdd(&ctr->connect_front, sum[1]) : 0u;
            uint32_t b_back = sum[2] ? atomicAdd(&ctr->connect_back, sum[2]) : 0u;
            if (sum[3]) atomicAdd(&ctr->shadow_rays, sum[3]);
            for (uint32_t w = 0; w < 4; w++) { s_base[w][0] = b_alive + pre[w][0]; s_base[w][1] = b_front + pre[w][1]; s_base[w][2] = b_back + pre[w][2]; }
        }
        __syncthreads();
        uint32_t o_alive = s_base[wave][0], o_front = s_base[wave][1], o_back = s_base[wave][2];
#pragma unroll
        for (uint32_t c = 0; c < 4; c++) {
            uint32_t r = (res >> (c * 5u)) & 31u;
            uint32_t slot = c == 0u ? s0 : (c == 1u ? s1 : (c == 2u ? s2 : s3));
            unsigned long long ma = __ballot((r & kSP_Alive) != 0u), mf = __ballot((r & kSP_Front) != 0u), mb = __ballot((r & kSP_Back) != 0u);
            if (r & kSP_Alive) queue_next[o_alive + lanes_below(ma)] = slot;
            if (r & kSP_Front) cqueue[o_front + lanes_below(mf)] = slot;
            if (r & kSP_Back) cqueue[ps.capacity - 1u - (o_back + lanes_below(mb))] = slot;
            o_alive += (uint32_t)__popcll(ma); o_front += (uint32_t)__popcll(mf); o_back += (uint32_t)__popcll(mb);
        }
    }
}
void launch_shade(hipStream_t s, uint32_t blocks, const DeviceScene& sc, const RenderParams& P, const PathState& ps,
                  const uint32_t* queue, uint32_t* queue_next, uint32_t* cqueue, Counters* ctr, uint32_t parity) {
    hipLaunchKernelGGL(k_shade, dim3(blocks), dim3(256), 0, s, sc, P, ps, queue, queue_next, cqueue, ctr, parity);
}
int shade_blocks_per_cu() {
    int nb = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_shade, 256, 0);
    return nb > 0 ? nb : 1;
}

// ------------------------------------------------------------------ connect (round 1's stage kernels)
// Per pending path: trace its (<= 2) shadow rays (RTCommon.slang:47-64: closest committed hit), join the
// visible NEE contributions with the emission BEFORE the luminance clamp (RayGen.slang:92-102), add to
// pathLight, and at the end of a sample apply the NaN/Inf guard and add to the frame sum (:116-128).
//
// A block works on tiles of up to kConnectTile paths.  The shadow rays of a tile are first listed in LDS (sky
// rays from the front, light rays from the back, one entry = owning path of the tile), then traced ONE RAY PER
// LANE — a path with two rays does not hold a lane twice as long while its neighbours idle, and waves see one
// ray kind — and the visibility bits go back to the owners through LDS, which add the contributions in the
// reference's order.
constexpr uint32_t kConnectTile = 512;
constexpr uint32_t kConnectScratch = kConnectTile * 4 + kConnectTile * 2 * 2 + kConnectTile * 2 + 16;  // slots, ray list, visibility, counters
__device__ inline uint32_t connect_tile(uint32_t n) { return n >= (1u << 19) ? 512u : n >= (1u << 17) ? 256u : n >= (1u << 15) ? 128u : 64u; }

template <bool LDS_SCENE, bool COUNT, bool STRICT>
__global__ __launch_bounds__(kTraverseBlock, 8) void k_connect(DeviceScene sc, RenderParams P, PathState ps, const uint32_t* cqueue,
                                                           Counters* ctr, uint32_t parity) {
    sc.strict_hits = STRICT ? 1u : 0u;
    extern __shared__ __align__(16) unsigned char smem[];
    const TravStack stack = make_stack(smem, sc.stack_overflow);
    unsigned char* scratch = smem + kStackDepth * kTraverseBlock * 4;
    uint32_t* t_slot = reinterpret_cast<uint32_t*>(scratch);                                   // [kConnectTile]
    uint16_t* t_list = reinterpret_cast<uint16_t*>(scratch + kConnectTile * 4);                // [2 * kConnectTile]
    unsigned char* t_vis = scratch + kConnectTile * 8;                                         // [2 * kConnectTile]
    uint32_t* t_misc = reinterpret_cast<uint32_t*>(scratch + kConnectTile * 10);               // tile base, #sky, #light
    float4* lds_nodes = reinterpret_cast<float4*>(scratch + kConnectScratch);
    float4* lds_tris = lds_nodes + sc.node_count * 8;
    stage_scene<LDS_SCENE>(sc, lds_nodes, lds_tris);
    const uint32_t nf = ctr->connect_front, nb = ctr->connect_back, n = nf + nb;
    const float4* Tprev = ps.T[parity];
    const uint32_t tile = connect_tile(n);
    const uint32_t tid = threadIdx.x;
    constexpr uint32_t kOwn = kConnectTile / kTraverseBlock;  // paths a thread owns per tile
    TravStats st; st.nodes = 0; st.tris = 0;
    while (true) {
        __syncthreads();  // the previous tile is fully consumed
        if (tid == 0) { t_misc[0] = atomicAdd(&ctr->connect_head, tile); t_misc[1] = 0u; t_misc[2] = 0u; }
        __syncthreads();
        const uint32_t base = t_misc[0];
        if (base >= n) break;
        uint32_t slot[kOwn], flags[kOwn];
#pragma unroll
        for (uint32_t q = 0; q < kOwn; q++) {
            const uint32_t j = tid + q * kTraverseBlock, i = base + j;
            const bool valid = j < tile && i < n;
            slot[q] = 0u; flags[q] = 0u;
            if (valid) {
                slot[q] = (i < nf) ? cqueue[i] : cqueue[ps.capacity - 1u - (i - nf)];
                flags[q] = __float_as_uint(ps.CE[slot[q]].w) | 0x80000000u;  // bit 31: this thread owns a path here
                t_slot[j] = slot[q];
            }
            const bool sky = (flags[q] & kCF_Sky) != 0u, light = (flags[q] & kCF_Light) != 0u;
            const uint32_t ps_ = wave_append(sky, &t_misc[1]);
            if (sky) t_list[ps_] = (uint16_t)j;
            const uint32_t pl_ = wave_append(light, &t_misc[2]);
            if (light) t_list[2u * kConnectTile - 1u - pl_] = (uint16_t)j;
        }
        __syncthreads();
        const uint32_t ns = t_misc[1], nr = ns + t_misc[2];
        for (uint32_t r = tid; r < nr; r += kTraverseBlock) {
            if (r < ns) {  // ClosestHit.slang:139, 344-353
                const uint32_t j = t_list[r], sl = t_slot[j];
                float4 so = ps.CSO[sl], sd = ps.CSD[sl];
                t_vis[2u * j] = sky_visible<LDS_SCENE, COUNT>(sc, lds_nodes, lds_tris, xyz(so), v3(so.w, sd.x, sd.y), stack, st, (P.flags & VPT_FLAG_RAY_QUERIES) != 0u) ? 1 : 0;
            } else {       // ClosestHit.slang:171-176, 358-370
                const uint32_t j = t_list[2u * kConnectTile - 1u - (r - ns)], sl = t_slot[j];
                float4 lo = ps.CLO[sl], ld = ps.CLD[sl];
                const uint32_t expect = __float_as_uint(ps.CL[sl].w);
                t_vis[2u * j + 1u] = light_visible<LDS_SCENE, COUNT>(sc, lds_nodes, lds_tris, xyz(lo), v3(lo.w, ld.x, ld.y), expect, stack, st) ? 1 : 0;
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t q = 0; q < kOwn; q++) {
            if (flags[q] & 0x80000000u) {
                const uint32_t j = tid + q * kTraverseBlock, sl = slot[q], fl = flags[q];
                V3 E = xyz(ps.CE[sl]);
                if ((fl & kCF_Sky) && t_vis[2u * j]) E = E + xyz(ps.CS[sl]);
                if ((fl & kCF_Light) && t_vis[2u * j + 1u]) E = E + xyz(ps.CL[sl]);
                const V3 contrib = path_contribution(E, xyz(Tprev[sl]), fl, P.max_luminance);
                V3 light = xyz(ps.L[sl]) + contrib;
                if (fl & kCF_Finalize) {
                    const bool ok = finite3(light);
                    if (P.samples_per_frame == 1) {  // the only finalisation of this slot: 0 + pathLight
                        ps.ACC[sl] = ok ? f4(v3s(0.0f) + light, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    } else if (ok) {
                        float4 acc = ps.ACC[sl]; ps.ACC[sl] = f4(xyz(acc) + light, 0.0f);
                    }
                    light = v3s(0.0f);  // the pixel's next sample of the frame starts from pathLight = 0
                }
                ps.L[sl] = f4(light, 0.0f);
            }
        }
    }
    if (COUNT) {
        atomicAdd(&ctr->stat_shadow_nodes, (unsigned long long)st.nodes);
        atomicAdd(&ctr->stat_shadow_tris, (unsigned long long)st.tris);
    }
}
void launch_connect(hipStream_t s, uint32_t blocks, bool lds_scene, bool count, const DeviceScene& sc, const RenderParams& P,
                    const PathState& ps, const uint32_t* cqueue, Counters* ctr, uint32_t parity) {
    size_t lds = traverse_lds_bytes(sc, lds_scene, kStackDepth) + kConnectScratch;
    const bool strict = sc.strict_hits != 0u;
    void (*k)(DeviceScene, RenderParams, PathState, const uint32_t*, Counters*, uint32_t);
    if (lds_scene) k = count ? (strict ? k_connect<true, true, true> : k_connect<true, true, false>) : (strict ? k_connect<true, false, true> : k_connect<true, false, false>);
    else k = count ? (strict ? k_connect<false, true, true> : k_connect<false, true, false>) : (strict ? k_connect<false, false, true> : k_connect<false, false, false>);
    hipLaunchKernelGGL(k, dim3(blocks), dim3(kTraverseBlock), lds, s, sc, P, ps, cqueue, ctr, parity);
}
int traverse_blocks_per_cu(bool lds_scene, const DeviceScene& sc) {
    int nb = 0;
    size_t lds = traverse_lds_bytes(sc, lds_scene, kStackDepth) + kConnectScratch;
    if (lds_scene) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_connect<true, false, false>, kTraverseBlock, lds);
    else (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_connect<false, false, false>, kTraverseBlock, lds);
    return nb > 0 ? nb : 1;
}

// Start of a bounce (round 1's stage kernels): fold the statistics of the previous one, reset cursors and the output queue sizes.
__global__ void k_prepare(Counters* ctr, uint32_t parity) {
    ctr->stat_closest += ctr->ray_count[parity];
    ctr->stat_shadow += ctr->shadow_rays;
    ctr->stat_connect += ctr->connect_front + ctr->connect_back;
    ctr->shadow_rays = 0u;
    ctr->extend_head = 0u; ctr->connect_head = 0u; ctr->connect_front = 0u; ctr->connect_back = 0u;
    ctr->ray_count[parity ^ 1u] = 0u;
}
__global__ void k_fold(Counters* ctr) {
    ctr->stat_shadow += ctr->shadow_rays; ctr->shadow_rays = 0u;
    ctr->stat_connect += ctr->connect_front + ctr->connect_back; ctr->connect_front = 0u; ctr->connect_back = 0u;
}
void launch_prepare(hipStream_t s, Counters* ctr, uint32_t parity) { hipLaunchKernelGGL(k_prepare, dim3(1), dim3(1), 0, s, ctr, parity); }
void launch_fold(hipStream_t s, Counters* ctr) { hipLaunchKernelGGL(k_fold, dim3(1), dim3(1), 0, s, ctr); }

}  // namespace vpt
