// scene_prep.hpp — everything vpt_set_scene / vpt_set_material / vpt_set_environment / vpt_set_instance_transforms decide and compute on the host before a byte reaches the device: the checks
// of a scene description, the pooled and flattened geometry, the texel pool, the environment's alias table and pdf, the emissive-mesh
// list, and the predicates the grids are picked by (host arithmetic of PathTracer.cpp restated).  Plain C++ on plain values, no context and
// no HIP call: api_scene.hip uploads what this prepares, and tests/test_scene_prep_cpu.py holds every rejection to its code and message and
// every table to the oracle's own writing of it (oracle.cpp build_tris / build_env / build_emissive), bit for bit, without a device.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "device_types.hpp"   // (+ vpt.h, vpt_fp32.h)

namespace vpt {
namespace scene {

struct Verdict {
    int code;          // VPT_OK or the VPT_ERR_* vpt_set_scene returns
    const char* msg;   // static; what vpt_last_error then says
};
constexpr Verdict kAccepted{VPT_OK, ""};

// Totals of the pools a description is flattened into, against the 32-bit offsets that address them.
struct PoolTotals {
    uint64_t vertices = 0, indices = 0, texel_bytes = 0;
    void add_mesh(uint32_t vertex_count, uint32_t index_count) { vertices += vertex_count; indices += index_count; }
    void add_texture(uint32_t w, uint32_t h, uint32_t channels) { texel_bytes += (uint64_t)w * h * channels + 3; }   // (+ 3: every texture starts 4-byte aligned)
    Verdict geometry() const {
        if (vertices > 0xffffffffull || indices > 0xffffffffull) return {VPT_ERR_LIMIT, "more than 2^32 pooled vertices / indices"};
        return kAccepted;
    }
    Verdict texels() const {
        if (texel_bytes > 0xffffffffull) return {VPT_ERR_LIMIT, "texel pool over 4 GiB (TexDesc offsets are 32-bit)"};
        return kAccepted;
    }
};

// The shade stage indexes textures[] unchecked.
inline bool material_textures_ok(const vpt_material& m, uint32_t texture_count) {
    return m.base_color_texture < texture_count && m.normal_texture < texture_count && m.roughness_texture < texture_count &&
           m.metallic_texture < texture_count && m.emissive_texture < texture_count;
}
inline bool is_emissive(const vpt_material& m) { return m.emissive_color[0] != 0.0f || m.emissive_color[1] != 0.0f || m.emissive_color[2] != 0.0f; }

// What vpt_set_scene and vpt_set_instance_transforms demand of ONE instance matrix (float[16], column-major): nothing.  Any sixteen floats are
// accepted, a singular matrix included (its triangles are slivers and are dropped, its inverse is whatever inverse3x3_from_mat4 makes of it), as
// vpt_set_scene always has.  The one place a demand would go, so that both callers refuse the same matrices with the same message.
inline Verdict check_instance_transform(const float* /*m*/) { return kAccepted; }
// Every reason vpt_set_instance_transforms rejects its arguments for, in the order it reports them (instance_count: of the installed scene).
// count == 0 passes whatever the rest says: such a call changes nothing.
inline Verdict check_instance_transforms(uint32_t first, uint32_t count, const float* transforms, uint32_t instance_count) {
    if (count == 0) return kAccepted;
    if (!transforms) return {VPT_ERR_INVALID_ARGUMENT, "no instance transforms"};
    if (first > instance_count || count > instance_count - first) return {VPT_ERR_INVALID_ARGUMENT, "instance range out of bounds"};   // (first + count may wrap)
    for (uint32_t i = 0; i < count; i++) { const Verdict v = check_instance_transform(transforms + (size_t)i * 16); if (v.code) return v; }
    return kAccepted;
}

// Every reason vpt_set_scene rejects a description for, in the order it reports them.  What passes here can only fail on the device.
inline Verdict check(const vpt_scene_desc& sd) {
    if (sd.mesh_count == 0 || !sd.meshes) return {VPT_ERR_INVALID_ARGUMENT, "No meshes found in scene"};  // PathTracer.cpp:180
    if (sd.mesh_count >= VPT_MAX_ENTITIES || sd.material_count >= VPT_MAX_ENTITIES) return {VPT_ERR_LIMIT, "too many meshes/materials"};
    if (sd.instance_count >= VPT_MAX_INSTANCES) return {VPT_ERR_LIMIT, "too many mesh instances"};
    if (!sd.materials || sd.material_count == 0 || !sd.instances || !sd.textures || sd.texture_count == 0 || !sd.env_rgba ||
        sd.env_width == 0 || sd.env_height == 0 || !sd.lut_reflection || !sd.lut_refraction_outside || !sd.lut_refraction_inside)
        return {VPT_ERR_INVALID_ARGUMENT, "incomplete scene description"};
    PoolTotals pools;
    for (uint32_t m = 0; m < sd.mesh_count; m++) {
        const vpt_mesh& me = sd.meshes[m];
        if (!me.vertices || !me.indices || me.index_count % 3 != 0) return {VPT_ERR_INVALID_ARGUMENT, "bad mesh"};
        for (uint32_t k = 0; k < me.index_count; k++) if (me.indices[k] >= me.vertex_count) return {VPT_ERR_INVALID_ARGUMENT, "mesh index out of range"};
        pools.add_mesh(me.vertex_count, me.index_count);
    }
    if (pools.geometry().code) return pools.geometry();
    for (uint32_t i = 0; i < sd.material_count; i++)
        if (!material_textures_ok(sd.materials[i], sd.texture_count)) return {VPT_ERR_INVALID_ARGUMENT, "material texture index out of range"};
    for (uint32_t i = 0; i < sd.instance_count; i++) {
        if (sd.instances[i].mesh_index >= sd.mesh_count) return {VPT_ERR_INVALID_ARGUMENT, "instance mesh index out of range"};
        if (sd.instances[i].material_index >= sd.material_count) return {VPT_ERR_INVALID_ARGUMENT, "Mesh instance has invalid material index"};  // PathTracer.cpp:454
        { const Verdict v = check_instance_transform(sd.instances[i].transform); if (v.code) return v; }
    }
    for (uint32_t t = 0; t < sd.texture_count; t++) {
        const vpt_texture& tx = sd.textures[t];
        if (!tx.data || tx.width == 0 || tx.height == 0 || (tx.channels != 1 && tx.channels != 4)) return {VPT_ERR_INVALID_ARGUMENT, "bad texture"};
        pools.add_texture(tx.width, tx.height, tx.channels);
    }
    if (pools.texels().code) return pools.texels();
    uint32_t emissive = 0;   // one entry of the emissive-mesh list per instance of an emissive material (emissive_list)
    for (uint32_t i = 0; i < sd.instance_count; i++) emissive += is_emissive(sd.materials[sd.instances[i].material_index]) ? 1u : 0u;
    if (emissive > VPT_MAX_EMISSIVE_MESHES) return {VPT_ERR_LIMIT, "too many emissive meshes"};
    return kAccepted;
}

// Every reason vpt_set_environment rejects a map for, in the order it reports them (vpt_set_scene's own checks of a description's
// environment are in check() above and stay as they are).
inline Verdict check_environment(const float* rgba, uint32_t w, uint32_t h) {
    if (!rgba || w == 0 || h == 0) return {VPT_ERR_INVALID_ARGUMENT, "incomplete environment map"};
    // the alias table's entries and sample_env's texel index are 32-bit (shading.hpp sample_env: size = w * h)
    if ((uint64_t)w * h > 0xffffffffull) return {VPT_ERR_LIMIT, "environment map of 2^32 texels or more"};
    return kAccepted;
}

// LoadEnvironmentMap, PathTracer.cpp:1161-1296: per-texel importance = solid angle * max(rgb), alias
// table (Vose-style pairing with the reference's pre-increment partition quirk), pdf into alpha.
inline void env_tables(const float* rgba, uint32_t w, uint32_t h, std::vector<float>& env, std::vector<AliasEntry>& alias) {
    const uint64_t size = (uint64_t)w * h;
    env.assign(rgba, rgba + size * 4);
    std::vector<float> importance(size);
    float cos_prev = 1.0f;
    const float step_phi = 2.0f * 3.14159265358979323846f / (float)w;
    const float step_theta = 3.14159265358979323846f / (float)h;
    for (uint32_t y = 0; y < h; y++) {
        float cos_next = vptfp::cos_((float)(y + 1) * step_theta);
        float area = (cos_prev - cos_next) * step_phi;
        cos_prev = cos_next;
        const float* row = &env[(size_t)y * w * 4];
        for (uint32_t x = 0; x < w; x++) importance[(size_t)y * w + x] = area * std::max(row[x * 4], std::max(row[x * 4 + 1], row[x * 4 + 2]));
    }
    float sum = 0.0f;
    for (uint64_t i = 0; i < size; i++) sum = sum + importance[i];  // std::accumulate in fp32, in order
    const float average = sum / (float)size;
    alias.resize(size);
    for (uint64_t i = 0; i < size; i++) { alias[i].importance = (average == 0.0f) ? 0.0f : importance[i] / average; alias[i].alias = (uint32_t)i; }
    std::vector<uint32_t> table(size + 1, 0u);
    uint32_t lo = 0, hi = (uint32_t)size;
    for (uint32_t i = 0; i < size; i++) {
        if (alias[i].importance < 1.0f) table[++lo] = i;  // upstream pre-increments: slot 0 stays 0
        else table[--hi] = i;
    }
    for (lo = 0; lo < hi && hi < size; lo++) {
        const uint32_t l = table[lo], g = table[hi];
        alias[l].alias = g;
        alias[g].importance -= 1.0f - alias[l].importance;
        if (alias[g].importance < 1.0f) hi++;
    }
    for (uint64_t i = 0; i < size; i++) {
        float m = std::max(env[i * 4], std::max(env[i * 4 + 1], env[i * 4 + 2]));
        env[i * 4 + 3] = (sum == 0.0f) ? 0.0f : m / sum;
    }
}

// Every float of the finished table (pdf included) is exactly 0: DeviceScene::env_black, and one of the conditions of plain() below.
inline bool env_is_black(const std::vector<float>& env) {
    for (size_t i = 0; i < env.size(); i++) if (env[i] != 0.0f) return false;
    return true;
}

// Emissive-mesh list, PathTracer.cpp:449-469 (and SetMaterial's rebuild, 712-794: same resulting order
// only for additions at the end; we rebuild from instance order, which is what SetScene produces).
struct EmissiveList {
    std::vector<EmissiveDesc> list;
    uint32_t tris = 0;                  // light triangles of the whole list
    std::vector<uint32_t> tri_offset;   // per entry: its first light triangle (never empty: one 0 for an empty list)
};
inline EmissiveList emissive_list(const std::vector<MeshDesc>& meshes, const std::vector<InstanceDesc>& instances, const std::vector<vpt_material>& materials) {
    EmissiveList out;
    for (uint32_t i = 0; i < instances.size(); i++) {
        if (is_emissive(materials[instances[i].material])) {
            EmissiveDesc e;
            e.mesh = instances[i].mesh; e.material = instances[i].material;
            e.tri_count = meshes[e.mesh].tri_count; e.instance = i;
            memcpy(e.xform, instances[i].xform, 64);
            out.tri_offset.push_back(out.tris);
            out.list.push_back(e); out.tris += e.tri_count;
        }
    }
    if (out.tri_offset.empty()) out.tri_offset.push_back(0u);
    return out;
}

// Does every path end within max_depth * samples_per_frame bounces?  A bounce either raises payload.Depth or ends the path — except a
// scattering event INSIDE a medium (ClosestHit.slang:80-116: depth unchanged), which needs a transmissive material whose medium has a
// density and an anisotropy other than 1 (shade_core.hpp); media (volumes / atmosphere) raise the depth per event but their batches
// run stages with host-visible fallbacks, so they count as unbounded too.
inline bool depth_bounded(const std::vector<vpt_material>& materials) {
    for (const vpt_material& m : materials)
        if (m.transmission > 0.0f && m.medium_density != 0.0f && m.medium_anisotropy != 1.0f) return false;
    return true;
}
// The scene class the fused kernel is specialised for (kernels_bounce.hip k_bounce<PLAIN>): every material's five textures are 1x1 and the
// environment is black — what k_precompute_materials turns into MatResolved.flags == 63 for every material, and k_precompute_lights into
// uniform light samplers.
inline bool plain(const std::vector<vpt_material>& materials, const std::vector<unsigned char>& tex_1x1, bool env_black, uint32_t build_flags) {
    if (!env_black || (build_flags & VPT_BUILD_GENERAL_KERNELS)) return false;
    auto one = [&](uint32_t t) { return t < tex_1x1.size() && tex_1x1[t] != 0; };
    for (const vpt_material& m : materials)
        if (!(one(m.base_color_texture) && one(m.normal_texture) && one(m.roughness_texture) && one(m.metallic_texture) && one(m.emissive_texture))) return false;
    return true;
}

// Small scenes ride in LDS next to the traversal stacks, in the fp32 node form: up to 3 KB, so that three blocks of the fused
// kernel (14 KB of stacks + 36 KB of regrouping ring + the scene each) still fit the 160 KB of a CU.
inline bool fits_lds(size_t scene_bytes) { return scene_bytes <= 3072; }
inline bool rides_in_lds(size_t nodes, size_t leaf_tris) { return fits_lds(nodes * sizeof(BvhNodeWide) + leaf_tris * sizeof(BvhTri)); }

// Per global triangle id: its position in the leaf-ordered triangle array.  0xffffffff: a sliver, in no leaf.
inline std::vector<uint32_t> slot_of_gid(const std::vector<BvhTri>& leaf_tris, uint32_t total_tris) {
    std::vector<uint32_t> slot_of(total_tris, 0xffffffffu);
    for (size_t i = 0; i < leaf_tris.size(); i++) slot_of[leaf_tris[i].gid] = (uint32_t)i;
    return slot_of;
}

// A checked description, flattened into the tables the device reads (all but the BVH, which bvh_build.hpp builds over `tris`).
struct HostScene {
    std::vector<vpt_vertex> verts;          // pooled, mesh after mesh
    std::vector<uint32_t> idx;
    std::vector<MeshDesc> meshes;
    uint64_t total_vertices = 0, total_indices = 0;
    std::vector<InstanceDesc> instances;
    std::vector<BvhTri> tris;               // world space, instance-major, slivers dropped: the builder's input
    uint32_t total_tris = 0;                // slivers included: global triangle ids are below this
    std::vector<vpt_material> materials;
    uint32_t texture_count = 0;
    std::vector<TexDesc> textures;
    std::vector<uint8_t> texels;            // every texture 4-byte aligned
    std::vector<unsigned char> tex_1x1;     // per texture
    std::vector<float> env;                 // RGBA32F, alpha = pdf
    std::vector<AliasEntry> alias;
    bool env_black = true;                  // every float of env is exactly 0
};
inline HostScene prepare(const vpt_scene_desc& sd) {
    HostScene s;
    // ---- geometry pools
    for (uint32_t m = 0; m < sd.mesh_count; m++) {
        const vpt_mesh& me = sd.meshes[m];
        MeshDesc d; d.vertex_offset = (uint32_t)s.verts.size(); d.index_offset = (uint32_t)s.idx.size(); d.tri_count = me.index_count / 3; d.pad = 0;
        s.verts.insert(s.verts.end(), me.vertices, me.vertices + me.vertex_count);
        s.idx.insert(s.idx.end(), me.indices, me.indices + me.index_count);
        s.meshes.push_back(d);
        s.total_vertices += me.vertex_count; s.total_indices += me.index_count;
    }
    s.materials.assign(sd.materials, sd.materials + sd.material_count);
    s.texture_count = sd.texture_count;
    // ---- instances, flattened world-space triangles (instance-major global ids)
    for (uint32_t i = 0; i < sd.instance_count; i++) {
        const vpt_instance& in = sd.instances[i];
        InstanceDesc d; memset(&d, 0, sizeof(d));
        d.mesh = in.mesh_index; d.material = in.material_index; d.tri_offset = s.total_tris;
        memcpy(d.xform, in.transform, 64);
        vptfp::inverse3x3_from_mat4(in.transform, d.inv3);
        s.instances.push_back(d);
        const MeshDesc& me = s.meshes[d.mesh];
        for (uint32_t t = 0; t < me.tri_count; t++) {
            const uint32_t* ii = &s.idx[me.index_offset + t * 3];
            vptfp::V3 p[3];
            for (int k = 0; k < 3; k++) {
                const vpt_vertex& v = s.verts[me.vertex_offset + ii[k]];
                p[k] = vptfp::mat_point(d.xform, vptfp::v3(v.position[0], v.position[1], v.position[2]));
            }
            vptfp::V3 e1 = p[1] - p[0], e2 = p[2] - p[0];
            BvhTri bt;
            bt.v0[0] = p[0].x; bt.v0[1] = p[0].y; bt.v0[2] = p[0].z;
            bt.e1[0] = e1.x; bt.e1[1] = e1.y; bt.e1[2] = e1.z;
            bt.e2[0] = e2.x; bt.e2[1] = e2.y; bt.e2[2] = e2.z;
            bt.prim = t; bt.inst = i; bt.gid = s.total_tris++;  // instance-major id over ALL triangles (tie-break key)
            if (!vptfp::triangle_degenerate(e1, e2)) s.tris.push_back(bt);  // slivers are not intersectable (vpt_fp32.h)
        }
    }
    // ---- textures: TexDesc.offset and the shade stage's texel addresses are 32-bit byte offsets into the pool (check bounds it)
    for (uint32_t t = 0; t < sd.texture_count; t++) {
        const vpt_texture& tx = sd.textures[t];
        while (s.texels.size() % 4) s.texels.push_back(0);
        TexDesc d; d.offset = (uint32_t)s.texels.size(); d.w = tx.width; d.h = tx.height; d.c = tx.channels;
        s.tex_1x1.push_back(tx.width == 1 && tx.height == 1 ? 1 : 0);
        s.texels.insert(s.texels.end(), tx.data, tx.data + (size_t)tx.width * tx.height * tx.channels);
        s.textures.push_back(d);
    }
    // ---- environment + tables
    env_tables(sd.env_rgba, sd.env_width, sd.env_height, s.env, s.alias);
    s.env_black = env_is_black(s.env);
    return s;
}

}  // namespace scene
}  // namespace vpt
