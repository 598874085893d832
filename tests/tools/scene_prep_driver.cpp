// Host driver of vulkan-path-tracer_amd/csrc/scene_prep.hpp for tests/test_scene_prep_cpu.py: scene::check, scene::prepare and the
// predicates behind a C interface, in the layouts oracle/oracle_py.py returns the oracle's own tables in.  Built as a shared library
// with g++ (no HIP runtime is linked or called) and driven through ctypes with the package's _abi.SceneDesc.
#include <cstdint>
#include <cstring>

#include "scene_prep.hpp"

using namespace vpt;

namespace {
struct Prepared {
    scene::HostScene hs;
    scene::EmissiveList em;
};
const char* verdict(scene::Verdict v, int* code) { *code = v.code; return v.msg; }
}  // namespace

extern "C" {

const char* sp_check(const vpt_scene_desc* sd, int* code) { return verdict(scene::check(*sd), code); }
// The pool bounds of scene::check from counts alone: vertex / index counts per mesh, (w, h, channels) per texture.
const char* sp_check_pools(const uint32_t* vertex_counts, const uint32_t* index_counts, uint32_t meshes, const uint32_t* whc, uint32_t textures, int* code) {
    scene::PoolTotals p;
    for (uint32_t i = 0; i < meshes; i++) p.add_mesh(vertex_counts[i], index_counts[i]);
    for (uint32_t i = 0; i < textures; i++) p.add_texture(whc[i * 3], whc[i * 3 + 1], whc[i * 3 + 2]);
    if (p.geometry().code) return verdict(p.geometry(), code);
    return verdict(p.texels(), code);
}
int sp_material_textures_ok(const vpt_material* m, uint32_t texture_count) { return scene::material_textures_ok(*m, texture_count) ? 1 : 0; }

void* sp_prepare(const vpt_scene_desc* sd) {
    Prepared* p = new Prepared();
    p->hs = scene::prepare(*sd);
    p->em = scene::emissive_list(p->hs.meshes, p->hs.instances, p->hs.materials);
    return p;
}
void sp_destroy(void* h) { delete (Prepared*)h; }
// kept triangles, all triangles, pooled vertices, pooled indices, env texels, instances, textures, texel bytes, env_black, materials
void sp_counts(void* h, uint64_t* out10) {
    const scene::HostScene& s = ((Prepared*)h)->hs;
    const uint64_t v[10] = {s.tris.size(), s.total_tris, s.total_vertices, s.total_indices, s.alias.size(), s.instances.size(), s.textures.size(), s.texels.size(), s.env_black ? 1u : 0u, s.materials.size()};
    memcpy(out10, v, sizeof(v));
    // the pools hold what the totals say
    if (s.verts.size() != s.total_vertices || s.idx.size() != s.total_indices || s.texture_count != s.textures.size() || s.tex_1x1.size() != s.textures.size()) out10[0] = ~0ull;
}
// Oracle.triangles(): 12 floats per kept triangle = v0, e1, e2, then prim / inst / gid as uint32 bits
void sp_get_triangles(void* h, float* out) {
    const scene::HostScene& s = ((Prepared*)h)->hs;
    for (size_t i = 0; i < s.tris.size(); i++) memcpy(out + i * 12, &s.tris[i], 48);
}
// orc_get_env_tables
void sp_get_env_tables(void* h, uint32_t* alias_out, float* importance_out, float* pdf_out) {
    const scene::HostScene& s = ((Prepared*)h)->hs;
    for (size_t i = 0; i < s.alias.size(); i++) { alias_out[i] = s.alias[i].alias; importance_out[i] = s.alias[i].importance; pdf_out[i] = s.env[i * 4 + 3]; }
}
// per texture: offset, w, h, c, 1x1; then the pool
void sp_get_textures(void* h, uint32_t* desc5, uint8_t* texels) {
    const scene::HostScene& s = ((Prepared*)h)->hs;
    for (size_t t = 0; t < s.textures.size(); t++) {
        const uint32_t v[5] = {s.textures[t].offset, s.textures[t].w, s.textures[t].h, s.textures[t].c, s.tex_1x1[t]};
        memcpy(desc5 + t * 5, v, sizeof(v));
    }
    if (!s.texels.empty()) memcpy(texels, s.texels.data(), s.texels.size());
}
// per instance: mesh, material, tri_offset, then xform (16) and inv3 (9) as float bits: 28 words
void sp_get_instances(void* h, uint32_t* out28) {
    const scene::HostScene& s = ((Prepared*)h)->hs;
    for (size_t i = 0; i < s.instances.size(); i++) {
        const InstanceDesc& d = s.instances[i];
        uint32_t* q = out28 + i * 28;
        q[0] = d.mesh; q[1] = d.material; q[2] = d.tri_offset;
        memcpy(q + 3, d.xform, 64); memcpy(q + 19, d.inv3, 36);
    }
}
// vpt_set_material's part of the preparation: the emissive list of the changed materials
void sp_set_material(void* h, uint32_t index, const vpt_material* m) {
    Prepared* p = (Prepared*)h;
    p->hs.materials[index] = *m;
    p->em = scene::emissive_list(p->hs.meshes, p->hs.instances, p->hs.materials);
}
// out2 = entries, light triangles; per entry (when asked for): mesh, material, tri_count, instance, tri_offset
void sp_get_emissive(void* h, uint32_t* out2, uint32_t* entries5) {
    const scene::EmissiveList& em = ((Prepared*)h)->em;
    out2[0] = (uint32_t)em.list.size(); out2[1] = em.tris;
    for (size_t k = 0; entries5 && k < em.list.size(); k++) {
        const uint32_t v[5] = {em.list[k].mesh, em.list[k].material, em.list[k].tri_count, em.list[k].instance, em.tri_offset[k]};
        memcpy(entries5 + k * 5, v, sizeof(v));
    }
    if (em.tri_offset.size() != (em.list.empty() ? 1u : em.list.size())) out2[0] = ~0u;
}

int sp_depth_bounded(const vpt_material* m, uint32_t n) { return scene::depth_bounded(std::vector<vpt_material>(m, m + n)) ? 1 : 0; }
int sp_plain(const vpt_material* m, uint32_t n, const unsigned char* tex_1x1, uint32_t textures, int env_black, uint32_t build_flags) {
    return scene::plain(std::vector<vpt_material>(m, m + n), std::vector<unsigned char>(tex_1x1, tex_1x1 + textures), env_black != 0, build_flags) ? 1 : 0;
}
int sp_rides_in_lds(uint64_t nodes, uint64_t leaf_tris) { return scene::rides_in_lds(nodes, leaf_tris) ? 1 : 0; }
int sp_fits_lds(uint64_t bytes) { return scene::fits_lds(bytes) ? 1 : 0; }
uint32_t sp_node_bytes() { return sizeof(BvhNodeWide); }
uint32_t sp_tri_bytes() { return sizeof(BvhTri); }
void sp_slot_of_gid(const uint32_t* leaf_gids, uint32_t leaves, uint32_t total_tris, uint32_t* out) {
    std::vector<BvhTri> lt(leaves);
    for (uint32_t i = 0; i < leaves; i++) { memset(&lt[i], 0, sizeof(BvhTri)); lt[i].gid = leaf_gids[i]; }
    const std::vector<uint32_t> s = scene::slot_of_gid(lt, total_tris);
    if (total_tris) memcpy(out, s.data(), (size_t)total_tris * 4);
}

}  // extern "C"
