// api_scene.hip — everything that installs or edits what a batch only reads: vpt_set_scene (what scene_prep.hpp prepares on the host and
// bvh_build.cpp builds, uploaded), its partial updates (material, environment, instance transforms by a device refit: bvh_refit.hpp), the media
// (density grids as grid_prep.hpp prepares them), and the test hooks.
#include <chrono>

#include "api_ctx.hpp"
#include "bvh_build.hpp"
#include "bvh_refit.hpp"
#include "grid_prep.hpp"

using namespace vpt::api;

// ---- helpers of this file alone
namespace {

// A scene table of n (at least one) elements, freed with the scene: DeviceScene's pointer to it and, for a table that is written after the
// upload, the writable one (vpt_ctx::Writable) are set here, from one allocation sized by their own element type.
// (the work is done once, on bytes; the template below, and api_ctx.hpp's upload, only size and type it)
int alloc_bytes(vpt_ctx* c, size_t bytes, void** out) {
    void* d = nullptr;
    HIPCHK(c, hipMalloc(&d, bytes));
    c->scene_allocs.push_back(d);
    *out = d;
    return VPT_OK;
}
template <class T>
int alloc_table(vpt_ctx* c, size_t n, const T** out, T** writable = nullptr) {
    void* d = nullptr;
    int rc = alloc_bytes(c, std::max<size_t>(n, 1) * sizeof(T), &d);
    if (d) { *out = (T*)d; if (writable) *writable = (T*)d; }
    return rc;
}

// Tables of the scene that have been replaced: freed now and taken out of scene_allocs (whose order means nothing: free_scene frees them all).
void release_tables(vpt_ctx* c, std::initializer_list<const void*> gone) {
    for (size_t i = 0; i < c->scene_allocs.size();) {
        void*& p = c->scene_allocs[i];
        if (p && std::find(gone.begin(), gone.end(), (const void*)p) != gone.end()) { (void)hipFree(p); p = c->scene_allocs.back(); c->scene_allocs.pop_back(); } else i++;
    }
}
// Staged tables: allocated behind the first `held` entries of scene_allocs by an update that installs them only once all of them are whole.  The
// update failed: they are freed and the scene is as it was.
void drop_staged(vpt_ctx* c, size_t held) {
    while (c->scene_allocs.size() > held) { (void)hipFree(c->scene_allocs.back()); c->scene_allocs.pop_back(); }
}

// The emissive-mesh list of the scene's current materials (scene_prep.hpp emissive_list) ...
void build_emissive(vpt_ctx* c) { c->emissive = scene::emissive_list(c->meshes, c->instances, c->materials); }
// ... and its tables on the device.
int upload_emissive(vpt_ctx* c) {
    const scene::EmissiveList& em = c->emissive;
    // (vpt_set_scene never gets here with such a list: scene::check refuses the description; this guards vpt_set_material's rebuild)
    if (em.list.size() > VPT_MAX_EMISSIVE_MESHES) return fail(c, VPT_ERR_LIMIT, "too many emissive meshes");
    if (!em.list.empty())
        HIPCHK(c, hipMemcpy(c->dw.emissive, em.list.data(), em.list.size() * sizeof(EmissiveDesc), hipMemcpyHostToDevice));
    c->dsc.emissive_count = (uint32_t)em.list.size();
    c->dsc.emissive_tris = em.tris;
    // per-light-triangle table (world-space corners, normal, area)
    HIPCHK(c, hipMemcpy(c->dw.emissive_tri_offset, em.tri_offset.data(), em.tri_offset.size() * 4, hipMemcpyHostToDevice));
    launch_precompute_emissive(c->main.stream, c->dsc, c->dw.emissive_tri, em.tris);
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return VPT_OK;
}

// The grid of the fused kernel's instantiation that serves the scene's current materials (scene_prep.hpp depth_bounded / plain).
void update_depth_bounded(vpt_ctx* c) {
    c->depth_bounded = scene::depth_bounded(c->materials);
    c->scene_plain = scene::plain(c->materials, c->tex_1x1, c->dsc.env_black != 0u, c->cfg.build_flags);
    c->primary_blocks = (c->scene_plain && c->lds_scene) ? c->primary_blocks_plain : c->primary_blocks_general;
}

// Which shade classes occur in the scene: the staged pipeline launches the shade stage once per class that does.
int update_class_present(vpt_ctx* c) {
    std::vector<unsigned char> cls(c->instances.size());
    if (!cls.empty()) HIPCHK(c, hipMemcpy(cls.data(), c->dw.inst_class, cls.size(), hipMemcpyDeviceToHost));
    c->class_present = 1u << kShadeMiss;
    for (unsigned char k : cls) if (k < kShadeClasses) c->class_present |= 1u << k;
    return VPT_OK;
}

// The box camera_cull.hpp bounds on the screen: the union of the root's used child boxes as nodes_wide holds them (padded fp32).
cull::WorldBox root_box(const BvhNodeWide& n) {
    cull::WorldBox b{{3.0e38f, 3.0e38f, 3.0e38f}, {-3.0e38f, -3.0e38f, -3.0e38f}, false};
    for (int k = 0; k < 4; k++)
        if (refit::slot_used(n, k)) {
            const float* f = n.minx;   // minx, miny, minz, maxx, maxy, maxz: four floats each, back to back
            for (int a = 0; a < 3; a++) { b.lo[a] = std::min(b.lo[a], f[a * 4 + k]); b.hi[a] = std::max(b.hi[a], f[12 + a * 4 + k]); }
            b.valid = true;
        }
    return b;
}

// The tree build_bvh makes of a prepared scene's triangles.
struct SceneBvh {
    std::vector<BvhNode> nodes; std::vector<BvhNodeWide> wide; std::vector<BvhTri> leaf_tris; int depth = 0;
};
// The environment's tables (scene_prep.hpp env_tables) on the device and DeviceScene's fields for them: both tables or, after a failure,
// neither, with DeviceScene as it was.  Whatever DeviceScene pointed to before is the caller's to free.
int upload_environment(vpt_ctx* c, const std::vector<float>& env, const std::vector<AliasEntry>& alias, uint32_t w, uint32_t h, bool black) {
    DeviceScene& D = c->dsc;
    const size_t held = c->scene_allocs.size();
    const float* e = nullptr;
    const AliasEntry* a = nullptr;
    int rc = upload(c, env, &e);
    if (rc == VPT_OK) rc = upload(c, alias, &a);
    if (rc) {
        drop_staged(c, held);
        return rc;
    }
    D.env = e; D.alias = a;
    D.env_w = w; D.env_h = h;
    D.env_black = black ? 1u : 0u;
    return VPT_OK;
}
// Uploads a prepared scene and its tree (the previous scene's tables are gone: free_scene), and takes over the host copies later calls
// work from (vpt_set_material, vpt_get_stats, the trace lab).
int upload_scene(vpt_ctx* c, const vpt_scene_desc& sd, scene::HostScene& hs, const SceneBvh& bvh) {
    DeviceScene& D = c->dsc;
    vpt_ctx::Writable& W = c->dw;
    int rc;
    c->lds_scene = scene::rides_in_lds(bvh.nodes.size(), bvh.leaf_tris.size());
    c->whole_box = c->lds_scene && !bvh.wide.empty() ? root_box(bvh.wide[0]) : cull::WorldBox{};
    c->bvh_depth = (uint32_t)bvh.depth;
    D.nodes_wide = nullptr; D.nodes8 = nullptr; D.nodes4s = nullptr;
    if ((rc = upload(c, bvh.nodes, &D.nodes))) return rc;
    if (c->lds_scene && (rc = upload(c, bvh.wide, &D.nodes_wide))) return rc;
    if ((rc = upload(c, bvh.leaf_tris, &D.tris))) return rc;
    D.node_count = (uint32_t)bvh.nodes.size(); D.tri_count = (uint32_t)bvh.leaf_tris.size();
    D.scene_extent = bvh_max_abs_coord(hs.tris);   // the number the builder padded the boxes by (slab.hpp: the reach of the fma box test)
    if ((rc = upload(c, scene::slot_of_gid(bvh.leaf_tris, hs.total_tris), &D.tri_slot_of_gid))) return rc;
    {   // the order vpt_set_instance_transforms refits the nodes in
        std::vector<uint32_t> order;
        refit::levels(bvh.nodes, order, c->refit_level_off);
        if ((rc = upload(c, order, &c->refit_order))) return rc;
    }
    c->total_tris = hs.total_tris; c->lab_trees_stale = false;
    if ((rc = upload(c, hs.verts, &D.vertices))) return rc;
    if ((rc = upload(c, hs.idx, &D.indices))) return rc;
    if ((rc = upload(c, hs.meshes, &D.meshes))) return rc;
    if ((rc = upload(c, hs.instances, &D.instances))) return rc;
    if ((rc = upload(c, hs.materials, &D.materials, 1, &W.materials))) return rc;
    if ((rc = upload(c, hs.textures, &D.textures))) return rc;
    if ((rc = upload(c, hs.texels, &D.texels, 4))) return rc;
    // filled on the device (kernels_aux.hip k_precompute_*) or by upload_emissive; per instance: an emissive mesh is an instance of an emissive material
    const size_t n_inst = hs.instances.size(), n_tris = hs.total_tris;
    if ((rc = alloc_table(c, n_inst, &D.emissive, &W.emissive))) return rc;
    if ((rc = alloc_table(c, hs.materials.size(), &D.mat_resolved, &W.mat_resolved))) return rc;
    if ((rc = alloc_table(c, n_tris, &D.emissive_tri, &W.emissive_tri))) return rc;
    if ((rc = alloc_table(c, n_inst, &D.emissive_tri_offset, &W.emissive_tri_offset))) return rc;
    if ((rc = alloc_table(c, n_tris, &D.tri_ng, &W.tri_ng))) return rc;
    if ((rc = alloc_table(c, 8 * std::max<size_t>(1, n_tris), &D.tri_shade, &W.tri_shade))) return rc;   // 8 float4, one 128-byte line, per triangle
    if ((rc = alloc_table(c, n_inst, &D.lights))) return rc;
    if ((rc = alloc_table(c, n_inst, &D.inst_class, &W.inst_class))) return rc;
    if ((rc = upload_environment(c, hs.env, hs.alias, sd.env_width, sd.env_height, hs.env_black))) return rc;
    if ((rc = upload(c, sd.lut_reflection, 64 * 64 * 32, &D.lut_r))) return rc;
    if ((rc = upload(c, sd.lut_refraction_outside, 128 * 128 * 32, &D.lut_o))) return rc;
    if ((rc = upload(c, sd.lut_refraction_inside, 128 * 128 * 32, &D.lut_i))) return rc;
    c->meshes = std::move(hs.meshes); c->instances = std::move(hs.instances); c->materials = std::move(hs.materials);
    c->total_vertices = hs.total_vertices; c->total_indices = hs.total_indices;
    c->texture_count = hs.texture_count; c->tex_1x1 = std::move(hs.tex_1x1);
    c->bvh_input = std::move(hs.tris);
    build_emissive(c);
    return upload_emissive(c);
}

// The persistent grids of the scene's kernels, from the occupancy queries (kernels.hpp).
void size_grids(vpt_ctx* c) {
    const DeviceScene& D = c->dsc;
#if VPT_LAB
    c->trav_blocks = traverse_blocks_per_cu(c->lds_scene, D) * c->cu_count;
    c->shade_blocks = shade_blocks_per_cu() * c->cu_count;
#else
    c->trav_blocks = 0;
    c->shade_blocks = 4 * c->cu_count;   // (the media scatter stage's grid-stride launch)
#endif
    c->join_blocks = join_blocks_per_cu() * c->cu_count;
    c->primary_blocks_general = bounce_blocks_per_cu(c->lds_scene, D, false) * c->cu_count;
    c->primary_blocks_plain = bounce_blocks_per_cu(c->lds_scene, D, true) * c->cu_count;
    c->primary_blocks = std::max(c->primary_blocks_general, c->primary_blocks_plain);   // (sizes the spill regions; update_depth_bounded picks the grid)
    c->whole_blocks = c->lds_scene ? std::max(whole_blocks_per_cu(D, false), whole_blocks_per_cu(D, true)) * c->cu_count : 0;
    c->shade_stream_blocks = shade_stream_blocks_per_cu() * c->cu_count;
    c->finish_blocks = finish_blocks_per_cu(D) * c->cu_count;
    c->shade_media_blocks = shade_media_blocks_per_cu() * c->cu_count;
    c->media_tail_blocks = media_tail_blocks_per_cu() * c->cu_count;
    c->shadow_blocks = trace_shadow_blocks_per_cu() * c->cu_count;
    c->vote_blocks = std::min(trace_blocks_per_cu(VPT_TRACE_VOTE, false), trace_blocks_per_cu(VPT_TRACE_VOTE, true)) * c->cu_count;
    c->max_blocks = std::max(std::max(std::max(std::max(c->trav_blocks, c->shade_blocks), std::max(c->primary_blocks, c->whole_blocks)), c->vote_blocks), std::max(std::max(c->shade_stream_blocks, c->finish_blocks), c->shadow_blocks));
}

// The upload both kinds of grid share: values, the brick table (bricked grids only), the block maxima and the grown list of grids, all allocated and
// filled before the context changes — a failure frees them and leaves the list as it was.  g: dim / cells / brick_count set by the caller.
int install_grid(vpt_ctx* c, DensityGrid g, const float* values, size_t n_values, const std::vector<uint32_t>* table, const grid::Maxima& m) {
    { int rd = quiesce(c); if (rd) return rd; }
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    float *dv = nullptr, *db = nullptr; uint32_t* dt = nullptr; DensityGrid* dl = nullptr;
    std::vector<DensityGrid> list = c->grids;
    bool ok = hipMalloc((void**)&dv, n_values * 4) == hipSuccess && hipMalloc((void**)&db, grid::kBlockTable * 4) == hipSuccess &&
              (!table || hipMalloc((void**)&dt, table->size() * 4) == hipSuccess) && hipMalloc((void**)&dl, (list.size() + 1) * sizeof(DensityGrid)) == hipSuccess;
    g.values = dv; g.block_max = db; g.bricks = dt; g.max_density = m.max_density;
    list.push_back(g);
    ok = ok && hipMemcpy(dv, values, n_values * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(db, m.block_max.data(), grid::kBlockTable * 4, hipMemcpyHostToDevice) == hipSuccess &&
         (!table || hipMemcpy(dt, table->data(), table->size() * 4, hipMemcpyHostToDevice) == hipSuccess) &&
         hipMemcpy(dl, list.data(), list.size() * sizeof(DensityGrid), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        (void)hipFree(dv); (void)hipFree(db); (void)hipFree(dt); (void)hipFree(dl);
        return fail(c, VPT_ERR_OUT_OF_MEMORY, "density grid upload");
    }
    c->state_gen++;
    c->grids.swap(list);
    if (c->d_grids) (void)hipFree(c->d_grids);
    c->d_grids = dl; c->dsc.grids = dl;
    c->tp_history = false;   // (a density-grid call: the temporal history goes, as with every other edit of the media)
    return (int)c->grids.size() - 1;
}

}  // namespace

// ---- helpers the other api_*.hip files call too (declared in api_ctx.hpp)
namespace vpt {
namespace api {

int upload_bytes(vpt_ctx* c, const void* src, size_t bytes, size_t total_bytes, void** out) {
    int rc = alloc_bytes(c, total_bytes, out);
    if (rc) return rc;
    HIPCHK(c, memset_now(c->main.stream, *out, 0, total_bytes));
    if (bytes) HIPCHK(c, hipMemcpy(*out, src, bytes, hipMemcpyHostToDevice));
    return VPT_OK;
}

void free_scene(vpt_ctx* c) {
    for (void* p : c->scene_allocs) (void)hipFree(p);
    c->scene_allocs.clear();
    free_spill(c->main);   // (sized by the scene's grids)
    c->has_scene = false;
    c->dw = vpt_ctx::Writable{};
}

// Everything derived from the materials and the feature flags (FURNACE_TEST_MODE is baked into the resolved-material table): resolve,
// classify the instances, and read the classes back.  Whoever changes a material, the flags or the scene calls this.
int refresh_material_tables(vpt_ctx* c) {
    launch_precompute_materials(c->main.stream, c->dsc, c->params.flags, c->dw.mat_resolved, (uint32_t)c->materials.size());
    launch_classify_instances(c->main.stream, c->dsc, c->dw.inst_class, (uint32_t)c->instances.size());
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return update_class_present(c);
}
void enqueue_first_hit(vpt_ctx* c, const FirstHitArgs& a) {
    c->spill_dirty = true;   // a traversal kernel runs: vpt_get_stats recounts the spill regions
    launch_first_hit(c->main.stream, (uint32_t)c->max_blocks, lane_scene(c, c->main), c->P, a);
}

}  // namespace api
}  // namespace vpt

extern "C" {

int vpt_set_scene(vpt_ctx* c, const vpt_scene_desc* sd) {
    if (!c || !sd) return VPT_ERR_INVALID_ARGUMENT;
    // a rejected description leaves the current scene untouched: everything that can refuse one is in scene::check, and what follows fails only on the device
    const scene::Verdict verdict = scene::check(*sd);
    if (verdict.code) return fail(c, verdict.code, verdict.msg);
    { int rd = quiesce(c); if (rd) return rd; }
    const auto t_scene0 = std::chrono::steady_clock::now();
    // ---- on the host: the tables and the tree
    scene::HostScene hs = scene::prepare(*sd);
    SceneBvh bvh;
    c->sbvh = (c->cfg.build_flags & VPT_BUILD_SBVH) != 0u;   // spatial splits in the builder: a per-context option
    const auto t_bvh0 = std::chrono::steady_clock::now();
    build_bvh(hs.tris, bvh.nodes, bvh.wide, bvh.leaf_tris, &bvh.depth, nullptr, c->sbvh);
    c->bvh_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_bvh0).count();
    // ---- the old scene goes before the new one's tables are allocated: a scene near the memory limit never needs room for both
    free_scene(c);
    reset_accum(c);
    destroy_lanes(c);   // (their spill regions are sized by this scene's grids)
    c->state_gen++;
    int rc;
    if ((rc = upload_scene(c, *sd, hs, bvh))) return rc;
    size_grids(c);
    // two regions: the shadow kernels of bounce k run on the second stream beside the extend kernel of bounce k + 1, and a
    // spill slot is addressed by (block, thread) alone, so concurrent grids must not share one region (round 2 did)
    if ((rc = alloc_spill(c, c->main, 2))) return rc;
    c->spill_dirty = true;
    launch_precompute_tri_ng(c->main.stream, c->dsc, c->dw.tri_ng);
    launch_precompute_tri_shade(c->main.stream, c->dsc, c->dw.tri_shade);
    if ((rc = refresh_material_tables(c))) return rc;
    HIPCHK(c, hipGetLastError());
    c->has_scene = true;
    update_depth_bounded(c);
    // (after a failed vpt_resize there is no image to clear: the scene is installed all the same, rendering needs a successful resize first)
    if (c->buffers_ok) HIPCHK(c, memset_now(c->main.stream, c->image, 0, (size_t)c->P.shard_pixels * 16));
    c->set_scene_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_scene0).count();
    return check_stream_slack(c);
}

int vpt_set_material(vpt_ctx* c, uint32_t index, const vpt_material* m) {
    if (!c || !m) return VPT_ERR_INVALID_ARGUMENT;
    if (!c->has_scene) return fail(c, VPT_ERR_NO_SCENE, "no scene");
    if (index >= c->materials.size()) return fail(c, VPT_ERR_INVALID_ARGUMENT, "material index out of range");
    if (!scene::material_textures_ok(*m, c->texture_count)) return fail(c, VPT_ERR_INVALID_ARGUMENT, "material texture index out of range");
    { int rd = quiesce(c); if (rd) return rd; }   // batches in flight read the tables patched below
    c->state_gen++;
    const vpt_material& old = c->materials[index];
    bool emissive_changed = old.emissive_color[0] != m->emissive_color[0] || old.emissive_color[1] != m->emissive_color[1] || old.emissive_color[2] != m->emissive_color[2];
    c->materials[index] = *m;
    HIPCHK(c, hipMemcpy(c->dw.materials + index, m, sizeof(vpt_material), hipMemcpyHostToDevice));
    if (emissive_changed) { build_emissive(c); int rc = upload_emissive(c); if (rc) return rc; }
    { int rc2 = refresh_material_tables(c); if (rc2) return rc2; }
    update_depth_bounded(c);
    reset_accum(c);
    return VPT_OK;
}
int vpt_set_environment(vpt_ctx* c, const float* env_rgba, uint32_t env_width, uint32_t env_height) {
    if (!c) return VPT_ERR_INVALID_ARGUMENT;
    if (!c->has_scene) return fail(c, VPT_ERR_NO_SCENE, "no scene");
    const scene::Verdict verdict = scene::check_environment(env_rgba, env_width, env_height);
    if (verdict.code) return fail(c, verdict.code, verdict.msg);
    { int rd = quiesce(c); if (rd) return rd; }   // batches in flight read the tables replaced below
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<float> env;
    std::vector<AliasEntry> alias;
    scene::env_tables(env_rgba, env_width, env_height, env, alias);
    // the new tables are on the device before the old ones go: a failure here leaves the previous environment installed
    const void* old_env = c->dsc.env;
    const void* old_alias = c->dsc.alias;
    int rc = upload_environment(c, env, alias, env_width, env_height, scene::env_is_black(env));
    if (rc) return rc;
    release_tables(c, {old_env, old_alias});
    c->state_gen++;            // a captured batch holds the old tables' addresses
    update_depth_bounded(c);   // env_black is one of the conditions of the PLAIN instantiation
    reset_accum(c);
    c->set_environment_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return VPT_OK;
}
int vpt_set_instance_transforms(vpt_ctx* c, uint32_t first, uint32_t count, const float* transforms) {
    if (!c) return VPT_ERR_INVALID_ARGUMENT;
    if (!c->has_scene) return fail(c, VPT_ERR_NO_SCENE, "no scene");
    const scene::Verdict verdict = scene::check_instance_transforms(first, count, transforms, (uint32_t)c->instances.size());
    if (verdict.code) return fail(c, verdict.code, verdict.msg);
    if (count == 0) return VPT_OK;
    { int rd = quiesce(c); if (rd) return rd; }   // batches in flight read the tables replaced below
    const auto t0 = std::chrono::steady_clock::now();
    DeviceScene& D = c->dsc;
    hipStream_t s = c->main.stream;
    // ---- staged: the triangles under the new matrices and the refitted nodes; the installed tables are only read until both are whole
    const size_t held = c->scene_allocs.size();
    const BvhTri* tris = nullptr; const BvhNode* nodes = nullptr; const BvhNodeWide* wide = nullptr;
    BvhTri* w_tris = nullptr; BvhNode* w_nodes = nullptr; BvhNodeWide* w_wide = nullptr;
    char* scratch = nullptr;   // 2 words (sliver flag, extent) | the matrices | 6 floats per node
    const size_t xf_bytes = (size_t)count * 64, scratch_bytes = 256 + xf_bytes + (size_t)D.node_count * 24;
    int rc = alloc_table(c, D.tri_count, &tris, &w_tris);
    if (!rc) rc = alloc_table(c, D.node_count, &nodes, &w_nodes);
    if (!rc && D.nodes_wide) rc = alloc_table(c, D.node_count, &wide, &w_wide);
    uint32_t words[2] = {0u, 0u};
    cull::WorldBox box{};   // of the refitted tree: the root's entry of the refit, padded as put_boxes pads its children (read behind the wait the refit ends with anyway)
    auto staged = [&]() -> int {
        HIPCHK(c, hipMalloc((void**)&scratch, scratch_bytes));
        HIPCHK(c, hipMemsetAsync(scratch, 0, 256, s));
        HIPCHK(c, hipMemcpyAsync(scratch + 256, transforms, xf_bytes, hipMemcpyHostToDevice, s));
        launch_retransform_tris(s, D, c->total_tris, (uint32_t)c->instances.size(), first, count, (const float*)(scratch + 256), w_tris, (uint32_t*)scratch);
        HIPCHK(c, hipMemcpyAsync(words, scratch, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        if (words[0]) return fail(c, VPT_ERR_UNSUPPORTED, "these transforms change which triangles are degenerate, and a refit keeps the tree's leaves: use vpt_set_scene");
        const float pad = refit::pad_of(vptfp::u2f(words[1]));
        for (size_t h = 0; h + 1 < c->refit_level_off.size(); h++)   // lowest first; the kernel boundaries order the heights
            launch_refit_level(s, D, c->refit_order, c->refit_level_off[h], c->refit_level_off[h + 1], w_tris, pad, (float*)(scratch + 256 + xf_bytes), w_nodes, w_wide);
        HIPCHK(c, hipStreamSynchronize(s));
        HIPCHK(c, hipGetLastError());
        if (w_wide) {
            HIPCHK(c, hipMemcpy(box.lo, scratch + 256 + xf_bytes, 24, hipMemcpyDeviceToHost));   // (lo and hi lie back to back, in the struct as in the entry)
            box.valid = box.lo[0] <= box.hi[0];
            for (int a = 0; a < 3; a++) { box.lo[a] -= pad; box.hi[a] += pad; }
        }
        return VPT_OK;
    };
    if (!rc) rc = staged();
    if (scratch) (void)hipFree(scratch);
    if (rc) {   // rejected or failed: the previous transforms stay installed, untouched
        drop_staged(c, held);
        return rc;
    }
    // ---- swapped in
    release_tables(c, {D.tris, D.nodes, D.nodes_wide, D.nodes8, D.nodes4s});
    D.tris = tris; D.nodes = nodes; D.nodes_wide = wide; D.nodes8 = nullptr; D.nodes4s = nullptr;
    D.scene_extent = vptfp::u2f(words[1]);
    c->whole_box = box;
    c->bvh_input = std::vector<BvhTri>(); c->lab_trees_stale = true; c->stats.bvh8_nodes = 0;   // (the trace lab's other trees were built from the old triangles)
    c->state_gen++;   // a captured batch holds the old tables' addresses
    const bool carry = c->tp_options.instance_motion != 0u;   // vpt_set_temporal_options: the history is reprojected through the move
    if (carry && c->tp_valid && c->tp_history) c->tp_snapshot.note_move(first, count, (uint32_t)c->instances.size(), c->instances[0].xform, sizeof(InstanceDesc));
    for (uint32_t i = 0; i < count; i++) {
        InstanceDesc& d = c->instances[first + i];
        memcpy(d.xform, transforms + (size_t)i * 16, 64);
        vptfp::inverse3x3_from_mat4(d.xform, d.inv3);
    }
    HIPCHK(c, hipMemcpy(const_cast<InstanceDesc*>(D.instances) + first, c->instances.data() + first, (size_t)count * sizeof(InstanceDesc), hipMemcpyHostToDevice));
    // ---- everything derived from the instances' matrices: the per-triangle shading tables, the light tables
    launch_precompute_tri_ng(s, D, c->dw.tri_ng);
    launch_precompute_tri_shade(s, D, c->dw.tri_shade);
    build_emissive(c);
    if ((rc = upload_emissive(c))) return rc;
    if ((rc = refresh_material_tables(c))) return rc;
    HIPCHK(c, hipGetLastError());
    reset_accum(c, carry);
    c->set_transforms_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return VPT_OK;
}
int vpt_get_material(const vpt_ctx* c, uint32_t index, vpt_material* out) {
    if (!c || !out || index >= c->materials.size()) return VPT_ERR_INVALID_ARGUMENT;
    *out = c->materials[index];
    return VPT_OK;
}

int vpt_set_volumes(vpt_ctx* c, const vpt_volume* v, uint32_t count) {
    if (!c || (count && !v)) return VPT_ERR_INVALID_ARGUMENT;
    if (count > VPT_MAX_VOLUMES) return fail(c, VPT_ERR_LIMIT, "more than VPT_MAX_VOLUMES volumes");
    if (count && !plan::media_supported(facts_of(c)))
        return fail(c, VPT_ERR_UNSUPPORTED, "volumes run on the fused pipeline or, for a scene whose BVH lives in memory, on the streams (VPT_PIPELINE_AUTO, _FUSED, _STAGED)");
    for (uint32_t i = 0; i < count; i++) {
        if (v[i].density_data_index < -1 || v[i].density_data_index >= (int)c->grids.size())
            return fail(c, VPT_ERR_INVALID_ARGUMENT, "density_data_index must be -1 or an index returned by vpt_add_density_grid");
        if (v[i].has_temperature_data && v[i].density_data_index < 0) return fail(c, VPT_ERR_INVALID_ARGUMENT, "has_temperature_data needs a density grid");
        if (!(v[i].density > 0.0f)) return fail(c, VPT_ERR_INVALID_ARGUMENT, "volume density must be > 0");  // -log(u)/0 (Sampler.slang:427)
    }
    { int rd = quiesce(c); if (rd) return rd; }
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    c->state_gen++;
    if (c->d_volumes) { (void)hipFree(c->d_volumes); c->d_volumes = nullptr; }
    c->volumes.assign(v, v + count);
    if (count) {
        HIPCHK(c, hipMalloc((void**)&c->d_volumes, (size_t)count * sizeof(vpt_volume)));
        HIPCHK(c, hipMemcpy(c->d_volumes, v, (size_t)count * sizeof(vpt_volume), hipMemcpyHostToDevice));
    }
    c->dsc.volumes = c->d_volumes; c->dsc.volume_count = count; c->dsc.phase = c->phase;
    c->dsc.hetero = 0u;
    for (uint32_t i = 0; i < count; i++) if (v[i].density_data_index >= 0) c->dsc.hetero = 1u;
    reset_accum(c);
    return VPT_OK;
}
// AddDensityDataToVolume, PathTracer.cpp:1390-1442, on a dense grid
int vpt_add_density_grid(vpt_ctx* c, uint32_t dx, uint32_t dy, uint32_t dz, const float* d) {
    if (!c || !d || dx == 0 || dy == 0 || dz == 0 || (uint64_t)dx * dy * dz > grid::kMaxDenseVoxels) return VPT_ERR_INVALID_ARGUMENT;
    if (c->grids.size() >= VPT_MAX_DENSITY_GRIDS) return fail(c, VPT_ERR_LIMIT, "more than VPT_MAX_DENSITY_GRIDS density grids");
    grid::Maxima m;
    const grid::Verdict v = grid::dense_maxima(dx, dy, dz, d, m);
    if (v.code) return fail(c, v.code, v.msg);
    DensityGrid g{};
    g.dim[0] = dx; g.dim[1] = dy; g.dim[2] = dz;
    return install_grid(c, g, d, (size_t)dx * dy * dz, nullptr, m);
}
// ... and on the tree's own leaves (grid_prep.hpp): the same grid, never densified
int vpt_add_density_bricks(vpt_ctx* c, uint32_t dx, uint32_t dy, uint32_t dz, uint32_t n, const uint32_t* coords, const float* values) {
    if (!c) return VPT_ERR_INVALID_ARGUMENT;
    grid::Maxima m;
    std::vector<uint32_t> table;
    grid::Verdict v = grid::check_bricks(dx, dy, dz, n, coords, values, c->grids.size());
    if (!v.code) v = grid::brick_table(dx, dy, dz, n, coords, table);
    if (!v.code) v = grid::brick_maxima(dx, dy, dz, n, coords, values, m);
    if (v.code) return fail(c, v.code, v.msg);
    DensityGrid g{};
    g.dim[0] = dx; g.dim[1] = dy; g.dim[2] = dz; g.brick_count = n;
    g.cells[0] = grid::cells_along(dx); g.cells[1] = grid::cells_along(dy); g.cells[2] = grid::cells_along(dz);
    return install_grid(c, g, values, (size_t)n * grid::kBrickVoxels, &table, m);
}
int vpt_get_density_grid_info(const vpt_ctx* c, uint32_t gi, vpt_density_grid_info* out) {
    if (!c || !out || gi >= c->grids.size()) return VPT_ERR_INVALID_ARGUMENT;
    const DensityGrid& g = c->grids[gi];
    *out = vpt_density_grid_info{{g.dim[0], g.dim[1], g.dim[2]}, g.brick_count, grid::device_bytes(g), g.max_density, 0u};
    return VPT_OK;
}
int vpt_read_density_grid(vpt_ctx* c, uint32_t gi, const int32_t* ijk, uint32_t n, float* out) {
    if (!c || gi >= c->grids.size() || (n && (!ijk || !out))) return VPT_ERR_INVALID_ARGUMENT;
    if (n == 0) return VPT_OK;
    { int rd = quiesce(c); if (rd) return rd; }
    int32_t* di = nullptr; float* dout = nullptr;
    HIPCHK(c, hipMalloc((void**)&di, (size_t)n * 12));
    if (hipMalloc((void**)&dout, (size_t)n * 4) != hipSuccess) { (void)hipFree(di); return fail(c, VPT_ERR_OUT_OF_MEMORY, "hipMalloc grid values"); }
    int rc = VPT_OK;
    if (hipMemcpy(di, ijk, (size_t)n * 12, hipMemcpyHostToDevice) != hipSuccess) rc = VPT_ERR_DEVICE;
    if (!rc) {
        launch_read_density_grid(c->main.stream, c->grids[gi], di, n, dout);
        if (hipStreamSynchronize(c->main.stream) != hipSuccess || hipGetLastError() != hipSuccess) rc = VPT_ERR_DEVICE;
    }
    if (!rc && hipMemcpy(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = VPT_ERR_DEVICE;
    (void)hipFree(di); (void)hipFree(dout);
    if (rc) c->err = "vpt_read_density_grid: device error";
    return rc;
}
int vpt_clear_density_grids(vpt_ctx* c) {
    if (!c) return VPT_ERR_INVALID_ARGUMENT;
    for (const vpt_volume& v : c->volumes) if (v.density_data_index >= 0) return fail(c, VPT_ERR_INVALID_ARGUMENT, "a volume still references a density grid");
    { int rd = quiesce(c); if (rd) return rd; }
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    c->state_gen++;
    for (DensityGrid& g : c->grids) { (void)hipFree((void*)g.values); (void)hipFree((void*)g.block_max); (void)hipFree((void*)g.bricks); }
    c->grids.clear();
    if (c->d_grids) { (void)hipFree(c->d_grids); c->d_grids = nullptr; }
    c->dsc.grids = nullptr;
    c->tp_history = false;
    return VPT_OK;
}
void vpt_default_atmosphere(vpt_atmosphere* a) {  // PathTracer.h:222-232
    if (!a) return;
    a->planet_position[0] = 0.0f; a->planet_position[1] = 6360e3f + 1000.0f; a->planet_position[2] = 0.0f;
    a->planet_radius = 6360e3f; a->atmosphere_height = 100e3f;
    a->rayleigh_density_falloff = 8000.0f; a->mie_density_falloff = 1200.0f; a->ozone_density_falloff = 5000.0f; a->ozone_peak = 22000.0f;
    for (int k = 0; k < 3; k++) { a->rayleigh_multiplier[k] = 1.0f; a->mie_multiplier[k] = 1.0f; a->ozone_multiplier[k] = 1.0f; }
    a->sun_color[0] = 1.0f; a->sun_color[1] = 0.956f; a->sun_color[2] = 0.88f;
}
int vpt_set_atmosphere(vpt_ctx* c, const vpt_atmosphere* a) {
    if (!c) return VPT_ERR_INVALID_ARGUMENT;
    if (a && !plan::media_supported(facts_of(c)))
        return fail(c, VPT_ERR_UNSUPPORTED, "the atmosphere runs on the fused pipeline or, for a scene whose BVH lives in memory, on the streams (VPT_PIPELINE_AUTO, _FUSED, _STAGED)");
    if (a && (!(a->planet_radius > 0.0f) || !(a->atmosphere_height > 0.0f) || !(a->rayleigh_density_falloff > 0.0f) || !(a->mie_density_falloff > 0.0f) ||
              !(a->ozone_density_falloff > 0.0f)))
        return fail(c, VPT_ERR_INVALID_ARGUMENT, "planet radius, atmosphere height and the density falloffs must be > 0");
    { int rd = drain(c); if (rd) return rd; }
    c->state_gen++;
    c->dsc.atm_on = a ? 1u : 0u;
    if (a) c->dsc.atm = *a;
    reset_accum(c);
    return VPT_OK;
}
int vpt_set_phase_function(vpt_ctx* c, uint32_t phase) {
    if (!c) return VPT_ERR_INVALID_ARGUMENT;
    if (phase > VPT_PHASE_HENYEY_GREENSTEIN_PLUS_DRAINE) return fail(c, VPT_ERR_INVALID_ARGUMENT, "unknown phase function");
    { int rd = drain(c); if (rd) return rd; }
    c->state_gen++;
    c->phase = phase; c->dsc.phase = phase;
    reset_accum(c);
    return VPT_OK;
}

int vpt_trace_rays(vpt_ctx* c, const vpt_ray* rays, uint32_t n, vpt_hit* hits) {
    if (!c || (n && (!rays || !hits))) return VPT_ERR_INVALID_ARGUMENT;
    if (!c->has_scene) return fail(c, VPT_ERR_NO_SCENE, "no scene");
    if (n == 0) return VPT_OK;
    { int rd = quiesce(c); if (rd) return rd; }
    vpt_ray* dr = nullptr; vpt_hit* dh = nullptr;
    HIPCHK(c, hipMalloc((void**)&dr, (size_t)n * sizeof(vpt_ray)));
    if (hipMalloc((void**)&dh, (size_t)n * sizeof(vpt_hit)) != hipSuccess) { (void)hipFree(dr); return fail(c, VPT_ERR_OUT_OF_MEMORY, "hipMalloc hits"); }
    int rc = VPT_OK;
    if (hipMemcpy(dr, rays, (size_t)n * sizeof(vpt_ray), hipMemcpyHostToDevice) != hipSuccess) rc = VPT_ERR_DEVICE;
    if (!rc) {
        c->spill_dirty = true;   // a traversal kernel runs: vpt_get_stats recounts the spill regions
        launch_trace_rays(c->main.stream, (uint32_t)c->max_blocks, lane_scene(c, c->main), dr, n, dh);
        if (hipStreamSynchronize(c->main.stream) != hipSuccess || hipGetLastError() != hipSuccess) rc = VPT_ERR_DEVICE;
    }
    if (!rc && hipMemcpy(hits, dh, (size_t)n * sizeof(vpt_hit), hipMemcpyDeviceToHost) != hipSuccess) rc = VPT_ERR_DEVICE;
    (void)hipFree(dr); (void)hipFree(dh);
    if (rc) c->err = "vpt_trace_rays: device error";
    return rc;
}

// vpt_render_features and vpt_pick: one launch of k_first_hit over camera rays on the main lane — the whole image, or the one pixel *pixel, whose
// barycentrics and position come back in pick8 (kernels.hpp FirstHitArgs::pick).  Host buffers are filled through ONE staging allocation, freed before
// the return; device buffers are written by the kernel itself.  Nothing of the context changes but spill_dirty.
static int first_hit_camera(vpt_ctx* c, uint32_t mode, uint32_t frame, const vpt_feature_buffers* out, const uint32_t* pixel, float* pick8) {
    if (!c || !out || mode > VPT_FEATURES_SAMPLE || (!out->depth && !out->ids && !out->normal && !out->albedo)) return VPT_ERR_INVALID_ARGUMENT;
    if (!c->has_scene) return fail(c, VPT_ERR_NO_SCENE, "no scene");
    const bool host = out->device == 0u;
    void* const dst[4] = {out->ids, out->normal, out->albedo, out->depth};
    if (!host) for (int k = 0; k < 3; k++) if (((uintptr_t)dst[k] & 15u) != 0u) return fail(c, VPT_ERR_INVALID_ARGUMENT, "device ids / normal / albedo buffers must be 16-byte aligned");
    { int rd = quiesce(c); if (rd) return rd; }
    const uint32_t w = c->P.width, h = c->P.height;
    const size_t npx = pixel ? 1u : (size_t)w * h;
    const size_t bytes[4] = {npx * 16, npx * 16, npx * 16, npx * 4};
    size_t total = pixel ? 32u : 0u;
    if (host) for (int k = 0; k < 4; k++) if (dst[k]) total += bytes[k];
    char* stage = nullptr;
    if (total) HIPCHK(c, hipMalloc((void**)&stage, total));
    void* dev[4]; size_t off = pixel ? 32u : 0u;
    for (int k = 0; k < 4; k++) { dev[k] = dst[k]; if (host && dst[k]) { dev[k] = stage + off; off += bytes[k]; } }
    FirstHitArgs a{};
    a.n = pixel ? 1u : ((w + 7u) / 8u) * ((h + 7u) / 8u) * 64u;   // 8 x 8 pixel tiles, a wave each
    a.mode = mode; a.frame = frame;
    a.ids = (uint4*)dev[0]; a.normal = (float4*)dev[1]; a.albedo = (float4*)dev[2]; a.depth = (float*)dev[3];
    if (pixel) { a.pick = (float4*)stage; a.pixel = *pixel; }
    int rc = VPT_OK;
    enqueue_first_hit(c, a);
    if (hipStreamSynchronize(c->main.stream) != hipSuccess || hipGetLastError() != hipSuccess) rc = VPT_ERR_DEVICE;
    if (!rc && pixel && hipMemcpy(pick8, stage, 32, hipMemcpyDeviceToHost) != hipSuccess) rc = VPT_ERR_DEVICE;
    for (int k = 0; k < 4; k++) if (!rc && host && dst[k] && hipMemcpy(dst[k], dev[k], bytes[k], hipMemcpyDeviceToHost) != hipSuccess) rc = VPT_ERR_DEVICE;
    if (stage) (void)hipFree(stage);
    if (rc) c->err = "vpt_render_features: device error";
    return rc;
}
int vpt_render_features(vpt_ctx* c, uint32_t mode, uint32_t frame, const vpt_feature_buffers* out) {
    return first_hit_camera(c, mode, frame, out, nullptr, nullptr);
}
int vpt_pick(vpt_ctx* c, uint32_t x, uint32_t y, vpt_pick_result* out) {
    if (!c || !out) return VPT_ERR_INVALID_ARGUMENT;
    if (x >= c->P.width || y >= c->P.height) return fail(c, VPT_ERR_INVALID_ARGUMENT, "pixel outside the image");
    uint32_t ids[4]; float t, uvp[8];
    vpt_feature_buffers fb{}; fb.depth = &t; fb.ids = ids;
    const uint32_t pixel = y * c->P.width + x;
    int rc = first_hit_camera(c, VPT_FEATURES_CENTER, 0u, &fb, &pixel, uvp);
    if (rc) return rc;
    *out = vpt_pick_result{ids[0], ids[1], ids[2], ids[3], t, uvp[0], uvp[1], {uvp[4], uvp[5], uvp[6]}};
    return VPT_OK;
}

}  // extern "C"
