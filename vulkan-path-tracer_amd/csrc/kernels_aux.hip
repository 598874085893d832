// kernels_aux.hip — one-pass kernels beside the integrators: the resolve (running mean over a batch's frames), shard rows -> full image, the derived scene
// tables (k_precompute_*, k_classify_instances), the refit behind vpt_set_instance_transforms (k_retransform_tris, k_refit_level), k_first_hit (the closest hit of caller-supplied or camera rays and the guide buffers there: vpt_trace_rays, vpt_render_features, vpt_pick), the test hook k_read_density_grid (a density grid's lookup), the LDS / stack-overflow size helpers every launcher shares, and the count of spilled stack words (k_count_spilled).
#include "bvh_refit.hpp"
#include "kernels.hpp"
#include "shade_core.hpp"
#include "traverse.hpp"

namespace vpt {

static inline uint32_t cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// ------------------------------------------------------------------ resolve: running mean, frames applied in order
// frame_base = index of the first dispatch of the batch (== FrameCount when ScreenSplitCount is 1).
// `guard`: queue size word that must be 0 (every path of the batch has finished) — the host enqueues the resolve right
// behind the bounces it expects to be the last ones and only then looks at the counter; if paths were still alive the
// launch does nothing and is repeated after more bounces.
__global__ __launch_bounds__(256) void k_resolve(RenderParams P, PathState ps, float4* image, uint32_t frames, uint32_t frame_base, const uint32_t* guard) {
    if (guard && *guard != 0u) return;
    if (P.dispatch_base_dev) frame_base = *P.dispatch_base_dev;   // a replayed graph (see k_bounce)
    uint32_t sp = blockIdx.x * blockDim.x + threadIdx.x;
    if (sp >= P.shard_pixels) return;
    float4 px = image[sp];
    V3 color = v3(px.x, px.y, px.z);
    if (P.split == 1u) {
        for (uint32_t f = 0; f < frames; f++) {
            V3 acc = xyz(ps.ACC[f * P.shard_pixels + sp]) / (float)P.samples_per_frame;
            uint32_t fc = frame_base + f;
            if (fc > 0) color = lerp(color, acc, 1.0f / (float)(fc + 1u));
            else color = acc;
        }
    } else {
        // split-screen (RayGen.slang:16-25, 143-157): dispatch d touches only the pixels of its chunk; the very
        // first dispatch also copies each rendered pixel into its whole S x S cell ("pixels that aren't rendered")
        const uint32_t S = P.split, y = sp / P.width, x = sp - y * P.width;
        for (uint32_t f = 0; f < frames; f++) {
            uint32_t d = frame_base + f, c = d % (S * S), fc = d / (S * S);
            if (x % S == c % S && y % S == c / S) {
                V3 acc = xyz(ps.ACC[f * P.shard_pixels + sp]) / (float)P.samples_per_frame;
                if (fc > 0) color = lerp(color, acc, 1.0f / (float)(fc + 1u));
                else color = acc;
            } else if (d == 0u) {
                uint32_t ax = x - x % S, ay = y - y % S;
                color = xyz(ps.ACC[f * P.shard_pixels + ay * P.width + ax]) / (float)P.samples_per_frame;
            }
        }
    }
    image[sp] = make_float4(color.x, color.y, color.z, 1.0f);
}
void launch_resolve(hipStream_t s, const RenderParams& P, const PathState& ps, float* image, uint32_t frames, uint32_t frame_base, const uint32_t* guard) {
    hipLaunchKernelGGL(k_resolve, dim3(cdiv(P.shard_pixels, 256)), dim3(256), 0, s, P, ps, reinterpret_cast<float4*>(image), frames, frame_base, guard);
}

// shard rows <-> full image
__global__ __launch_bounds__(256) void k_scatter_rows(const float4* gathered, float4* full, uint32_t width, uint32_t height,
                                                      uint32_t shard_count, uint32_t shard_stride_px) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= width * height) return;
    uint32_t y = i / width, x = i - y * width;
    uint32_t r = y % shard_count, ys = y / shard_count;
    full[i] = gathered[(size_t)r * shard_stride_px + (size_t)ys * width + x];
}
void launch_scatter_rows(hipStream_t s, const float* gathered, float* full, uint32_t w, uint32_t h, uint32_t shard_count, uint32_t stride_px) {
    hipLaunchKernelGGL(k_scatter_rows, dim3(cdiv(w * h, 256)), dim3(256), 0, s, reinterpret_cast<const float4*>(gathered),
                       reinterpret_cast<float4*>(full), w, h, shard_count, stride_px);
}

// ------------------------------------------------------------------ derived scene tables
__global__ __launch_bounds__(256) void k_precompute_materials(DeviceScene sc, uint32_t flags, MatResolved* out, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const vpt_material& m = sc.materials[i];
    MatResolved r;
    V2 uv; uv.x = 0.0f; uv.y = 0.0f;
    material_resolve(sc, m, uv, flags, r);   // a field whose texture is not 1x1 holds a value nobody reads (its flag stays clear)
    auto one = [&](uint32_t t) { return sc.textures[t].w == 1 && sc.textures[t].h == 1; };
    r.flags = (one(m.base_color_texture) ? kMatBase : 0u) | (one(m.roughness_texture) ? kMatRoughness : 0u) |
              (one(m.metallic_texture) ? kMatMetallic : 0u) | (one(m.emissive_texture) ? kMatEmissive : 0u);
    if ((r.flags & (kMatBase | kMatRoughness | kMatMetallic | kMatEmissive)) == (kMatBase | kMatRoughness | kMatMetallic | kMatEmissive)) r.flags |= kMatAllValues;
    if (one(m.normal_texture)) {
        V4 nm = tex_sample(sc, m.normal_texture, 0.0f, 0.0f);
        r.nmap[0] = nm.x * 2.0f - 1.0f; r.nmap[1] = nm.y * 2.0f - 1.0f; r.nmap[2] = nm.z * 2.0f - 1.0f;
        r.flags |= kMatNormal;
    } else { r.nmap[0] = r.nmap[1] = r.nmap[2] = 0.0f; }
    r.pad1 = r.pad2 = 0.0f;
    r.tex[0] = sc.textures[m.normal_texture]; r.tex[1] = sc.textures[m.base_color_texture]; r.tex[2] = sc.textures[m.roughness_texture];
    r.tex[3] = sc.textures[m.metallic_texture]; r.tex[4] = sc.textures[m.emissive_texture];
    out[i] = r;
}
// One LightSampler per emissive mesh (device_types.hpp): the fields SampleEmissiveTriangle reads through four tables, side by side.
__global__ __launch_bounds__(64) void k_precompute_lights(DeviceScene sc, LightSampler* out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= sc.emissive_count) return;
    const EmissiveDesc& em = sc.emissive[i];
    const vpt_material& m = sc.materials[em.material];
    LightSampler ls;
    ls.tri_count = em.tri_count; ls.gid_base = sc.instances[em.instance].tri_offset; ls.tri_base = sc.emissive_tri_offset[i];
    ls.tex = sc.textures[m.emissive_texture];
    ls.uniform = (ls.tex.w == 1 && ls.tex.h == 1) ? 1u : 0u;
    ls.emissive_color[0] = m.emissive_color[0]; ls.emissive_color[1] = m.emissive_color[1]; ls.emissive_color[2] = m.emissive_color[2];
    V4 te = tex_sample(sc, m.emissive_texture, 0.0f, 0.0f);
    ls.radiance[0] = m.emissive_color[0] * te.x; ls.radiance[1] = m.emissive_color[1] * te.y; ls.radiance[2] = m.emissive_color[2] * te.z;
    ls.pad0 = ls.pad1 = 0.0f;
    out[i] = ls;
}
__global__ __launch_bounds__(256) void k_precompute_tri_ng(DeviceScene sc, float4* out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= sc.tri_count) return;
    const BvhTri& t = sc.tris[i];
    V3 ng = triangle_ng(sc, sc.instances[t.inst], t.prim);
    out[t.gid] = make_float4(ng.x, ng.y, ng.z, 0.0f);
}
__global__ __launch_bounds__(256) void k_precompute_tri_shade(DeviceScene sc, float4* out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= sc.tri_count) return;
    const BvhTri& t = sc.tris[i];
    const InstanceDesc in = sc.instances[t.inst];
    const MeshDesc me = sc.meshes[in.mesh];
    const uint32_t* idx = sc.indices + me.index_offset + t.prim * 3;
    const vpt_vertex* vb = sc.vertices + me.vertex_offset;
    float4* q = out + (size_t)t.gid * 8;
    for (int k = 0; k < 3; k++) {
        const float4* v = reinterpret_cast<const float4*>(vb + idx[k]);
        q[2 * k] = v[0]; q[2 * k + 1] = v[1];
    }
    V3 ng = triangle_ng(sc, in, t.prim);
    q[6] = make_float4(ng.x, ng.y, ng.z, 0.0f);
    q[7] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
__global__ __launch_bounds__(256) void k_precompute_emissive(DeviceScene sc, EmissiveTri* out, uint32_t total) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    uint32_t k = 0;
    while (k + 1 < sc.emissive_count && sc.emissive_tri_offset[k + 1] <= i) k++;
    EmissiveTri t;
    emissive_tri_compute(sc, sc.emissive[k], i - sc.emissive_tri_offset[k], t);
    out[i] = t;
}
// Shade class of every instance (device_types.hpp kShade*), from the resolved material table.
__global__ __launch_bounds__(256) void k_classify_instances(DeviceScene sc, unsigned char* out, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t mi = sc.instances[i].material;
    const vpt_material& m = sc.materials[mi];
    const MatResolved& r = sc.mat_resolved[mi];
    const bool emissive = (r.flags & kMatEmissive) ? (r.emissive[0] > 0.0f || r.emissive[1] > 0.0f || r.emissive[2] > 0.0f)
                                         : (m.emissive_color[0] != 0.0f || m.emissive_color[1] != 0.0f || m.emissive_color[2] != 0.0f);
    uint32_t c = kShadeTextured;
    if (emissive) c = kShadeEmissive;
    else if (m.transmission > 0.0f) c = kShadeGlass;
    else if ((r.flags & (kMatAllValues | kMatNormal)) == (kMatAllValues | kMatNormal)) c = kShadePlain;   // the promise k_shade_stream<kShadePlain> relies on: no texture of this material is ever sampled
    out[i] = (unsigned char)c;
}
void launch_classify_instances(hipStream_t s, const DeviceScene& sc, unsigned char* out, uint32_t n) {
    if (n) hipLaunchKernelGGL(k_classify_instances, dim3((n + 255) / 256), dim3(256), 0, s, sc, out, n);
}
// (the light table reads materials and textures too: every caller that refreshes one refreshes the other)
void launch_precompute_materials(hipStream_t s, const DeviceScene& sc, uint32_t flags, MatResolved* out, uint32_t n) {
    if (n) hipLaunchKernelGGL(k_precompute_materials, dim3((n + 255) / 256), dim3(256), 0, s, sc, flags, out, n);
    if (sc.emissive_count) hipLaunchKernelGGL(k_precompute_lights, dim3((sc.emissive_count + 63) / 64), dim3(64), 0, s, sc, const_cast<LightSampler*>(sc.lights));
}
void launch_precompute_tri_ng(hipStream_t s, const DeviceScene& sc, float4* out) {
    if (sc.tri_count) hipLaunchKernelGGL(k_precompute_tri_ng, dim3((sc.tri_count + 255) / 256), dim3(256), 0, s, sc, out);
}
void launch_precompute_tri_shade(hipStream_t s, const DeviceScene& sc, float4* out) {
    if (sc.tri_count) hipLaunchKernelGGL(k_precompute_tri_shade, dim3((sc.tri_count + 255) / 256), dim3(256), 0, s, sc, out);
}
void launch_precompute_emissive(hipStream_t s, const DeviceScene& sc, EmissiveTri* out, uint32_t total) {
    if (total) hipLaunchKernelGGL(k_precompute_emissive, dim3((total + 255) / 256), dim3(256), 0, s, sc, out, total);
}

// ------------------------------------------------------------------ moved instances: triangles re-transformed, boxes refitted (bvh_refit.hpp)
// Instances [first, first + count) take the matrices at xf (16 floats each), the others keep InstanceDesc's: the installed tables are only read.
__device__ inline void moved_triangle(const DeviceScene& sc, uint32_t inst, uint32_t prim, uint32_t first, uint32_t count, const float* xf, BvhTri& t) {
    const InstanceDesc& in = sc.instances[inst];
    const MeshDesc me = sc.meshes[in.mesh];
    const uint32_t* idx = sc.indices + me.index_offset + prim * 3;
    const vpt_vertex* vb = sc.vertices + me.vertex_offset;
    refit::world_triangle(inst - first < count ? xf + (size_t)(inst - first) * 16 : in.xform, vb[idx[0]].position, vb[idx[1]].position, vb[idx[2]].position, t);
}
// Thread i: leaf slot i gets its world triangle under the new matrices (prim / inst / gid kept), and global triangle i, if it has no slot (a sliver
// the tree was built without), is looked at too.  words[0] is raised when the sliver set would change — a slot's triangle is degenerate now, or a
// sliver no longer is: the tree has no place for either — and words[1] takes the bits of the largest |coordinate| of the slots' triangles.
__global__ __launch_bounds__(256) void k_retransform_tris(DeviceScene sc, uint32_t total_tris, uint32_t n_inst, uint32_t first, uint32_t count, const float* xf, BvhTri* out, uint32_t* words) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t flag = 0u, extent = 0u;
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {   // 0: leaf slot i; 1: global triangle i, when it has no slot
        BvhTri t;
        if (pass == 0) {
            if (i >= sc.tri_count) continue;
            t = sc.tris[i];
        } else {
            if (i >= total_tris || sc.tri_slot_of_gid[i] != 0xffffffffu) continue;
            uint32_t lo = 0u, hi = n_inst;   // the last instance whose first triangle id is <= i
            while (hi - lo > 1u) { const uint32_t mid = (lo + hi) / 2u; if (sc.instances[mid].tri_offset <= i) lo = mid; else hi = mid; }
            t.inst = lo; t.prim = i - sc.instances[lo].tri_offset;
        }
        moved_triangle(sc, t.inst, t.prim, first, count, xf, t);
        const bool sliver = refit::degenerate(t);
        if (pass == 0) { out[i] = t; extent = vptfp::f2u(refit::max_abs_coord(t)); }
        if (sliver == (pass == 0)) flag = 1u;
    }
    for (int o = 32; o > 0; o >>= 1) { const uint32_t e = __shfl_down(extent, o), f = __shfl_down(flag, o); extent = e > extent ? e : extent; flag |= f; }
    if ((threadIdx.x & 63u) == 0u) { if (flag) atomicOr(&words[0], 1u); if (extent) atomicMax(&words[1], extent); }
}
// One height of the tree, one thread per node (bvh_refit.hpp refit_node); the launch before this one wrote the boxes of every lower node.
__global__ __launch_bounds__(256) void k_refit_level(DeviceScene sc, const uint32_t* order, uint32_t begin, uint32_t end, const BvhTri* tris, float pad, float* boxes, BvhNode* nodes_out, BvhNodeWide* wide_out) {
    const uint32_t j = begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= end) return;
    const uint32_t i = order[j];
    if (i < sc.node_count) refit::refit_node(i, sc.nodes, sc.nodes_wide, sc.node_count, tris, sc.tri_count, pad, boxes, nodes_out, wide_out);
}
void launch_retransform_tris(hipStream_t s, const DeviceScene& sc, uint32_t total_tris, uint32_t n_inst, uint32_t first, uint32_t count, const float* xf, BvhTri* out, uint32_t* words) {
    const uint32_t n = sc.tri_count > total_tris ? sc.tri_count : total_tris;
    if (n) hipLaunchKernelGGL(k_retransform_tris, dim3(cdiv(n, 256)), dim3(256), 0, s, sc, total_tris, n_inst, first, count, xf, out, words);
}
void launch_refit_level(hipStream_t s, const DeviceScene& sc, const uint32_t* order, uint32_t begin, uint32_t end, const BvhTri* tris, float pad, float* boxes, BvhNode* nodes_out, BvhNodeWide* wide_out) {
    if (end > begin) hipLaunchKernelGGL(k_refit_level, dim3(cdiv(end - begin, 256)), dim3(256), 0, s, sc, order, begin, end, tris, pad, boxes, nodes_out, wide_out);
}

// (camera_ray_with, the camera ray with its four draws handed in: camera.hpp)
// The closest hit of a ray and, for a camera ray, what lies there (kernels.hpp FirstHitArgs): vpt_trace_rays' test hook on caller-supplied rays, and the
// guide buffers of vpt_render_features / vpt_pick — the integrator's camera-ray query (RayGen.slang:70: direction normalised, tmin 0.01, tmax 100000)
// followed by the head of ClosestHit.slang (SurfaceFrame, :45-71; Material.Initialize's base colour, Material.slang:44) and nothing after it.  In camera
// mode work item i is lane i % 64 of tile i / 64 and a tile is 8 x 8 pixels: a wave's rays stay together in the tree and its texel taps in a few lines.
// The in-memory tree serves every scene (an LDS-resident one has it too).  One traversal is compiled in for both ray sources: a second kernel would
// carry a second copy of it.  No barrier in the loop: lanes outside the image skip their item.
__global__ __launch_bounds__(kTraverseBlock) void k_first_hit(DeviceScene sc, RenderParams P, FirstHitArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const TravStack stack = make_stack(smem, sc.stack_overflow);
    GlobalSceneSrc src{sc.nodes, sc.tris, sc.strict_hits != 0u};
    const uint32_t tiles_x = (P.width + 7u) / 8u;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x) {
        V3 o, d; float tmin = 0.01f, tmax = 100000.0f;
        uint32_t px = 0u;
        if (a.rays) {
            vpt_ray r = a.rays[i];
            o = v3(r.origin[0], r.origin[1], r.origin[2]); d = v3(r.direction[0], r.direction[1], r.direction[2]); tmin = r.tmin; tmax = r.tmax;
        } else {
            uint32_t x, y;
            if (a.pick) { y = a.pixel / P.width; x = a.pixel - y * P.width; }
            else {
                const uint32_t tile = i >> 6, ty = tile / tiles_x;
                x = (tile - ty * tiles_x) * 8u + (i & 7u); y = ty * 8u + ((i >> 3) & 7u);
                if (x >= P.width || y >= P.height) continue;
                px = y * P.width + x;
            }
            float j0 = 0.5f, j1 = 0.5f; V2 rc; rc.x = 0.0f; rc.y = 0.0f;
            if (a.mode == VPT_FEATURES_SAMPLE) {
                Rng r; r.s = y + P.width * x + pcg_hash(P.base_seed + a.frame);   // RayGen.slang:28, PathTracer.cpp:139: sample 0 of the pixel in dispatch `frame`
                j0 = r.uf(); j1 = r.uf(); rc = random_circle(r);
            }
            camera_ray_with(P, j0, j1, rc, x, y, o, d);
            d = normalize(d);
        }
        HitRec h; TravStats st;
        bool found = trace_closest<false>(src, o, d, tmin, tmax, stack, h, st);
        if (a.rays) {
            vpt_hit q; q.t = found ? h.t : -1.0f; q.u = found ? h.u : 0.0f; q.v = found ? h.v : 0.0f; q.primitive = h.prim; q.instance = h.inst;
            a.hits[i] = q;
            continue;
        }
        float t = -1.0f;
        uint4 id = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
        float4 nrm = make_float4(0.0f, 0.0f, 0.0f, 0.0f), alb = nrm, uv = nrm, pos = nrm;
        if (found) {
            const InstanceDesc& in = sc.instances[h.inst];
            const vpt_material& m = sc.materials[in.material];
            const MatResolved& mr = sc.mat_resolved[in.material];
            const bool geo_only = (P.flags & VPT_FLAG_GEOMETRY_NORMALS) != 0;
            t = h.t; id = make_uint4(h.inst, h.prim, in.material, in.mesh);
            uv.x = h.u; uv.y = h.v;
            V3 at = o + h.t * d; pos = make_float4(at.x, at.y, at.z, 0.0f);
            SurfaceFrame s;
            surface_geom(sc, s, in, h.gid, h.u, h.v, d, geo_only);
            TexTaps nt, bt;   // the two taps in flight together
            const bool base_tap = a.albedo && !(mr.flags & kMatBase);
            if (!geo_only && !(mr.flags & kMatNormal)) tex_issue(sc.texels, mr.tex[0], s.uv.x, s.uv.y, nt);
            if (base_tap) tex_issue(sc.texels, mr.tex[1], s.uv.x, s.uv.y, bt);
            surface_frame(s, d, geo_only, mr, nt);
            nrm = make_float4(s.N.x, s.N.y, s.N.z, s.inside ? 1.0f : 0.0f);
            float b[3] = {mr.base[0], mr.base[1], mr.base[2]};   // 1x1 texture: material_resolve's value (VPT_FLAG_FURNACE included), from the table
            if (base_tap) {                                       // otherwise its expression on this hit's texels (material_finish)
                const V4 tb = tex_finish(bt);
                const float c[3] = {tb.x, tb.y, tb.z};
#pragma unroll 1
                for (int k = 0; k < 3; k++) b[k] = (P.flags & VPT_FLAG_FURNACE) ? 1.0f : m.base_color[k] * pow_(c[k], 2.2f);
            }
            alb = make_float4(b[0], b[1], b[2], m.transmission);
        }
        if (a.depth) a.depth[px] = t;
        if (a.ids) a.ids[px] = id;
        if (a.normal) a.normal[px] = nrm;
        if (a.albedo) a.albedo[px] = alb;
        if (a.pick) { a.pick[0] = uv; a.pick[1] = pos; }
    }
}
void launch_first_hit(hipStream_t s, uint32_t blocks, const DeviceScene& sc, const RenderParams& P, const FirstHitArgs& a) {
    uint32_t g = cdiv(a.n, kTraverseBlock);
    hipLaunchKernelGGL(k_first_hit, dim3(g < blocks ? g : blocks), dim3(kTraverseBlock), (size_t)kStackDepth * kTraverseBlock * 4, s, sc, P, a);
}
void launch_trace_rays(hipStream_t s, uint32_t blocks, const DeviceScene& sc, const vpt_ray* rays, uint32_t n, vpt_hit* hits) {
    FirstHitArgs a{}; a.rays = rays; a.hits = hits; a.n = n;
    launch_first_hit(s, blocks, sc, RenderParams{}, a);   // (the camera is not looked at)
}

// Test hook: the samplers' lookup (grid_prep.hpp grid_value) at caller-supplied voxels, clamped to the index box as sample_density_grid clamps.
__global__ __launch_bounds__(256) void k_read_density_grid(DensityGrid g, const int32_t* ijk, uint32_t n, float* out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int cx = min(max(ijk[(size_t)i * 3], 0), (int)g.dim[0] - 1), cy = min(max(ijk[(size_t)i * 3 + 1], 0), (int)g.dim[1] - 1), cz = min(max(ijk[(size_t)i * 3 + 2], 0), (int)g.dim[2] - 1);
        out[i] = grid::grid_value(g, (uint32_t)cx, (uint32_t)cy, (uint32_t)cz);
    }
}
void launch_read_density_grid(hipStream_t s, const DensityGrid& g, const int32_t* ijk, uint32_t n, float* out) {
    const uint32_t b = cdiv(n, 256);
    hipLaunchKernelGGL(k_read_density_grid, dim3(b < 1024u ? b : 1024u), dim3(256), 0, s, g, ijk, n, out);
}

size_t traverse_lds_bytes(const DeviceScene& sc, bool lds_scene, int stack_rows) {
    size_t b = (size_t)stack_rows * kTraverseBlock * 4;
    if (lds_scene) b += (size_t)sc.node_count * sizeof(BvhNodeWide) + (size_t)sc.tri_count * sizeof(BvhTri);
    return b;
}
size_t stack_overflow_bytes(uint32_t blocks) { return (size_t)blocks * kTraverseBlock * kOverflowStride * 4; }   // (traverse.hpp: the longest per-thread region of any kernel)
// What the traversal kernels have written into a spill region (vpt_get_stats).
__global__ __launch_bounds__(256) void k_count_spilled(const uint32_t* p, uint32_t n, unsigned long long* out) {
    unsigned long long cnt = 0ull;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) cnt += p[i] != kSpillPattern ? 1ull : 0ull;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
    if ((threadIdx.x & 63u) == 0u && cnt) atomicAdd(out, cnt);
}
void launch_count_spilled(hipStream_t s, const uint32_t* region, uint32_t words, unsigned long long* out) {
    hipLaunchKernelGGL(k_count_spilled, dim3(1024), dim3(256), 0, s, region, words, out);
}

}  // namespace vpt
