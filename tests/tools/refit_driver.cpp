// Host driver of the BVH refit behind vpt_set_instance_transforms for tests/test_refit_cpu.py: a stand-alone program (g++, no HIP runtime linked or
// called; it may be built with -fsanitize=address,undefined) that prepares a description (scene_prep.hpp), builds its tree (bvh_build.hpp) and refits
// it under a second set of instance matrices through the functions the kernels call (bvh_refit.hpp), in the kernels' order: every leaf slot and every
// slot-less triangle first (kernels_aux.hip k_retransform_tris), then the nodes height by height, lowest first (k_refit_level).
//
//   refit_driver refit IN OUT      IN:  u32 meshes, instances, spatial_splits; per mesh u32 vertices, indices, float3 positions, u32 indices;
//                                       per instance u32 mesh, float[16] matrix the tree is built with, float[16] matrix it is refitted with
//                                  OUT: u32[12] header (see main), then the arrays it names, back to back
//   refit_driver check FIRST COUNT NULL INSTANCES     prints "<code>|<message>" of scene::check_instance_transforms
//   refit_driver matrix F0 .. F15                     prints the verdicts of scene::check (an instance with this matrix) and of
//                                                     scene::check_instance_transforms (the same matrix), one per line
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bvh_build.hpp"
#include "bvh_refit.hpp"
#include "scene_prep.hpp"

using namespace vpt;

namespace {

struct Input {
    std::vector<std::vector<vpt_vertex>> verts;
    std::vector<std::vector<uint32_t>> idx;
    std::vector<vpt_mesh> meshes;
    std::vector<vpt_instance> inst[2];   // the matrices the tree is built with | refitted with
    uint32_t spatial = 0;
    // what scene::prepare reads besides the geometry: one material, one 1x1 texture, a 1x1 environment
    vpt_material material;
    vpt_texture texture;
    uint8_t texel[4] = {255, 255, 255, 255};
    float env[4] = {0, 0, 0, 0};
    float lut[1] = {0};
    vpt_scene_desc desc(int which) {
        vpt_scene_desc sd; memset(&sd, 0, sizeof(sd));
        sd.meshes = meshes.data(); sd.mesh_count = (uint32_t)meshes.size();
        sd.materials = &material; sd.material_count = 1;
        sd.instances = inst[which].data(); sd.instance_count = (uint32_t)inst[which].size();
        sd.textures = &texture; sd.texture_count = 1;
        sd.env_rgba = env; sd.env_width = 1; sd.env_height = 1;
        sd.lut_reflection = sd.lut_refraction_outside = sd.lut_refraction_inside = lut;
        return sd;
    }
};

bool read_all(const char* path, std::vector<unsigned char>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
    out.resize((size_t)n);
    const bool ok = n == 0 || fread(out.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    return ok;
}
struct Reader {
    const std::vector<unsigned char>& b; size_t at = 0; bool ok = true;
    void get(void* dst, size_t n) { if (at + n > b.size()) { ok = false; memset(dst, 0, n); return; } memcpy(dst, b.data() + at, n); at += n; }
    uint32_t u32() { uint32_t v; get(&v, 4); return v; }
};
template <class T>
void put(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

int run_refit(const char* in_path, const char* out_path) {
    std::vector<unsigned char> bytes;
    if (!read_all(in_path, bytes)) { fprintf(stderr, "cannot read %s\n", in_path); return 2; }
    Reader r{bytes};
    Input in;
    memset(&in.material, 0, sizeof(in.material));
    in.texture.width = in.texture.height = 1; in.texture.channels = 4; in.texture.data = in.texel;
    const uint32_t n_meshes = r.u32(), n_inst = r.u32();
    in.spatial = r.u32();
    in.verts.resize(n_meshes); in.idx.resize(n_meshes);
    for (uint32_t m = 0; m < n_meshes && r.ok; m++) {
        const uint32_t nv = r.u32(), ni = r.u32();
        if ((size_t)nv * 12 + (size_t)ni * 4 > bytes.size()) { r.ok = false; break; }
        in.verts[m].resize(nv); in.idx[m].resize(ni);
        for (uint32_t v = 0; v < nv; v++) { memset(&in.verts[m][v], 0, sizeof(vpt_vertex)); r.get(in.verts[m][v].position, 12); }
        r.get(in.idx[m].data(), (size_t)ni * 4);
        vpt_mesh me; me.vertices = in.verts[m].data(); me.vertex_count = nv; me.indices = in.idx[m].data(); me.index_count = ni;
        in.meshes.push_back(me);
    }
    for (uint32_t i = 0; i < n_inst && r.ok; i++) {
        vpt_instance a; a.mesh_index = r.u32(); a.material_index = 0;
        vpt_instance b = a;
        r.get(a.transform, 64); r.get(b.transform, 64);
        in.inst[0].push_back(a); in.inst[1].push_back(b);
    }
    if (!r.ok) { fprintf(stderr, "short input\n"); return 2; }
    const vpt_scene_desc sd0 = in.desc(0), sd1 = in.desc(1);
    const scene::Verdict v0 = scene::check(sd0);
    if (v0.code) { fprintf(stderr, "scene::check: %s\n", v0.msg); return 2; }

    // ---- what vpt_set_scene does: the tables, the tree, the order of a refit
    scene::HostScene hs = scene::prepare(sd0);
    std::vector<BvhNode> nodes; std::vector<BvhNodeWide> wide; std::vector<BvhTri> leaf; int depth = 0;
    build_bvh(hs.tris, nodes, wide, leaf, &depth, nullptr, in.spatial != 0u);
    const float extent0 = bvh_max_abs_coord(hs.tris);
    const std::vector<uint32_t> slot_of = scene::slot_of_gid(leaf, hs.total_tris);
    std::vector<uint32_t> order, level_off;
    refit::levels(nodes, order, level_off);
    uint32_t parents_first = 1u;
    for (size_t i = 0; i < nodes.size(); i++) for (int k = 0; k < 4; k++) if (nodes[i].child[k] >= 0 && (size_t)nodes[i].child[k] <= i) parents_first = 0u;

    // ---- what vpt_set_instance_transforms does (the new matrices: sd1's)
    auto moved_triangle = [&](uint32_t inst, uint32_t prim, BvhTri& t) {
        const InstanceDesc& d = hs.instances[inst];
        const MeshDesc& me = hs.meshes[d.mesh];
        const uint32_t* ii = &hs.idx[me.index_offset + prim * 3];
        const vpt_vertex* vb = &hs.verts[me.vertex_offset];
        refit::world_triangle(sd1.instances[inst].transform, vb[ii[0]].position, vb[ii[1]].position, vb[ii[2]].position, t);
    };
    uint32_t flag = 0u, extent_bits = 0u;
    std::vector<BvhTri> staged(leaf.size());
    for (size_t i = 0; i < leaf.size(); i++) {
        BvhTri t = leaf[i];
        moved_triangle(t.inst, t.prim, t);
        staged[i] = t;
        if (refit::degenerate(t)) flag = 1u;
        extent_bits = std::max(extent_bits, vptfp::f2u(refit::max_abs_coord(t)));
    }
    for (uint32_t g = 0; g < hs.total_tris; g++) {
        if (slot_of[g] != 0xffffffffu) continue;
        uint32_t lo = 0u, hi = (uint32_t)hs.instances.size();
        while (hi - lo > 1u) { const uint32_t mid = (lo + hi) / 2u; if (hs.instances[mid].tri_offset <= g) lo = mid; else hi = mid; }
        BvhTri t;
        moved_triangle(lo, g - hs.instances[lo].tri_offset, t);
        if (!refit::degenerate(t)) flag = 1u;
    }
    const float pad = refit::pad_of(vptfp::u2f(extent_bits));
    std::vector<BvhNode> nodes1(nodes.size()); std::vector<BvhNodeWide> wide1(wide.size());
    std::vector<float> boxes(nodes.size() * 6, 0.0f);
    for (size_t h = 0; h + 1 < level_off.size(); h++)
        for (uint32_t j = level_off[h]; j < level_off[h + 1]; j++)
            refit::refit_node(order[j], nodes.data(), wide.data(), (uint32_t)nodes.size(), staged.data(), (uint32_t)staged.size(), pad, boxes.data(), nodes1.data(), wide1.data());

    // ---- the yardstick: scene::prepare of the moved description
    scene::HostScene hs1 = scene::prepare(sd1);
    const float extent1 = bvh_max_abs_coord(hs1.tris);

    FILE* f = fopen(out_path, "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", out_path); return 2; }
    // slots, nodes, triangles (slivers included), kept triangles of the moved description, sliver flag, extent after the refit, extent of the
    // moved description, extent the tree was built with, levels, parents numbered below their children, depth, wide nodes
    const uint32_t header[12] = {(uint32_t)leaf.size(), (uint32_t)nodes.size(), hs.total_tris, (uint32_t)hs1.tris.size(), flag, extent_bits, vptfp::f2u(extent1), vptfp::f2u(extent0),
                                 (uint32_t)level_off.size() - 1u, parents_first, (uint32_t)depth, (uint32_t)wide.size()};
    fwrite(header, 4, 12, f);
    put(f, leaf); put(f, nodes); put(f, wide); put(f, staged); put(f, nodes1); put(f, wide1); put(f, hs1.tris); put(f, order); put(f, level_off);
    fclose(f);
    return 0;
}

void print_verdict(const scene::Verdict& v) { printf("%d|%s\n", v.code, v.msg); }

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "refit" && argc == 4) return run_refit(argv[2], argv[3]);
    if (mode == "check" && argc == 6) {
        const uint32_t first = (uint32_t)strtoul(argv[2], nullptr, 0), count = (uint32_t)strtoul(argv[3], nullptr, 0), instances = (uint32_t)strtoul(argv[5], nullptr, 0);
        const bool null = atoi(argv[4]) != 0;
        const float one[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        std::vector<float> m;   // (a range that passes holds at most `instances` matrices; one that does not is refused before a matrix is read)
        for (uint32_t i = 0; i < std::max(1u, std::min(count, instances)); i++) m.insert(m.end(), one, one + 16);
        print_verdict(scene::check_instance_transforms(first, count, null ? nullptr : m.data(), instances));
        return 0;
    }
    if (mode == "matrix" && argc == 18) {
        vpt_vertex v[3]; memset(v, 0, sizeof(v)); v[1].position[0] = 1.0f; v[2].position[1] = 1.0f;
        uint32_t idx[3] = {0, 1, 2};
        vpt_mesh me; me.vertices = v; me.vertex_count = 3; me.indices = idx; me.index_count = 3;
        vpt_material mat; memset(&mat, 0, sizeof(mat));
        uint8_t texel[4] = {0, 0, 0, 0};
        vpt_texture tx; tx.width = tx.height = 1; tx.channels = 4; tx.data = texel;
        float env[4] = {0, 0, 0, 0}, lut[1] = {0};
        vpt_instance in; in.mesh_index = 0; in.material_index = 0;
        for (int k = 0; k < 16; k++) in.transform[k] = strtof(argv[2 + k], nullptr);
        vpt_scene_desc sd; memset(&sd, 0, sizeof(sd));
        sd.meshes = &me; sd.mesh_count = 1; sd.materials = &mat; sd.material_count = 1; sd.instances = &in; sd.instance_count = 1;
        sd.textures = &tx; sd.texture_count = 1; sd.env_rgba = env; sd.env_width = sd.env_height = 1;
        sd.lut_reflection = sd.lut_refraction_outside = sd.lut_refraction_inside = lut;
        print_verdict(scene::check(sd));
        print_verdict(scene::check_instance_transforms(0, 1, in.transform, 1));
        return 0;
    }
    fprintf(stderr, "usage: refit_driver refit IN OUT | check FIRST COUNT NULL INSTANCES | matrix F0 .. F15\n");
    return 2;
}
