// whole_walk_host — the any-hit search of a tree that rides in LDS in two forms, on the host, over the product builder's four-wide
// tree: the stack search (traverse.hpp trace_occluded_pass: hit children in slot order, a stack, return at the first triangle that decides) and
// the DEFINITION a walk without a stack computes (the inner nodes in index order, a bit per entered node under the fixed interval, the OR
// over the entered leaves' triangles).  Same slab.hpp box test and vpt_fp32.h ray_triangle in both.  Also the tree's numbering, which the
// single ascending pass relies on (bvh_build.hpp).  The walk as a kernel, a wave at a time, was measured and not taken
// (profiles/r12_whole_walk_ab.md).  Shared library for tests/test_whole_walk_cpu.py.  Test utility only (built on demand by the test); nothing
// in the product links it.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../vulkan-path-tracer_amd/csrc/bvh_build.hpp"
#include "../../vulkan-path-tracer_amd/csrc/scene_prep.hpp"
#include "../../vulkan-path-tracer_amd/csrc/slab.hpp"
using namespace vpt;

namespace {
struct Tree {
    std::vector<BvhNode> nodes; std::vector<BvhNodeWide> wide; std::vector<BvhTri> leaf; int depth = 0;
};
void build(const void* tris_in, int ntris, int pairwise, Tree& t) {
    std::vector<BvhTri> tris(ntris);
    memcpy(tris.data(), tris_in, sizeof(BvhTri) * (size_t)ntris);
    BvhBuildOptions opt;
    opt.parallel = false; opt.pairwise = pairwise != 0;
    build_bvh_ex(tris, t.nodes, t.wide, t.leaf, &t.depth, opt);
}
struct Query {
    V3 o, d, inv, oi; bool fused; float tmin, tmax, tlimit, t_e; uint32_t expect; bool light;
};
// form: 0 the subtract form of the box test for every ray, 1 the fma form for the rays its guard admits (slab.hpp)
Query make_query(const float* o, const float* d, float tmin, float tmax, bool light, float t_e, uint32_t expect, int form, float reach) {
    Query q;
    q.o = vptfp::v3(o[0], o[1], o[2]); q.d = vptfp::v3(d[0], d[1], d[2]); q.inv = safe_inverse(q.d); q.oi = slab_oi(q.o, q.inv);
    q.fused = form != 0 && slab_fma_ok(q.o, q.oi, reach);
    q.tmin = tmin; q.tmax = tmax; q.light = light; q.t_e = t_e; q.expect = expect; q.tlimit = light ? t_e : tmax;
    return q;
}
bool enters(const Query& q, const BvhNodeWide& n, int k) {
    const float t = q.fused ? box_entry_fma(n.minx[k], n.miny[k], n.minz[k], n.maxx[k], n.maxy[k], n.maxz[k], q.oi, q.inv, q.tmin, q.tlimit)
                            : box_entry(n.minx[k], n.miny[k], n.minz[k], n.maxx[k], n.maxy[k], n.maxz[k], q.o, q.inv, q.tmin, q.tlimit);
    return t < kMissT;
}
bool decides(const Query& q, const BvhTri& tr) {   // the predicate of trace_occluded_pass<.., LIGHT, false>
    float t, u, v;
    if (!vptfp::ray_triangle(q.o, q.d, vptfp::v3(tr.v0[0], tr.v0[1], tr.v0[2]), vptfp::v3(tr.e1[0], tr.e1[1], tr.e1[2]), vptfp::v3(tr.e2[0], tr.e2[1], tr.e2[2]),
                             q.tmin, q.tmax, &t, &u, &v)) return false;
    return !q.light || t < q.t_e || (t == q.t_e && tr.gid < q.expect);
}
bool stack_search(const Tree& t, const Query& q) {
    std::vector<int> stack;
    int cur = 0;
    while (true) {
        if (cur >= 0) {
            const BvhNodeWide& n = t.wide[cur];
            int next = 0x7fffffff;
            for (int k = 3; k >= 0; k--)
                if (enters(q, n, k)) { if (next != 0x7fffffff) stack.push_back(next); next = n.child[k]; }
            if (next != 0x7fffffff) { cur = next; continue; }
        } else {
            const uint32_t enc = (uint32_t)(~cur);
            const int first = (int)(enc >> 3), cnt = (int)(enc & 7u) + 1;
            for (int k = 0; k < cnt; k++) if (decides(q, t.leaf[first + k])) return true;
        }
        if (stack.empty()) break;
        cur = stack.back(); stack.pop_back();
    }
    return false;
}
bool walk(const Tree& t, const Query& q, int* nodes_entered, int* tris_tested) {
    uint32_t entered = 1u;
    bool occluded = false;
    for (uint32_t n = 0; n < (uint32_t)t.wide.size() && n < 32u; n++) {
        if (!((entered >> n) & 1u)) continue;
        (*nodes_entered)++;
        for (int k = 0; k < 4; k++) {
            if (!enters(q, t.wide[n], k)) continue;
            const int c = t.wide[n].child[k];
            if (c >= 0) { if (c < 32) entered |= 1u << c; continue; }
            const uint32_t enc = (uint32_t)(~c);
            const int first = (int)(enc >> 3), cnt = (int)(enc & 7u) + 1;
            for (int j = 0; j < cnt; j++) { (*tris_tested)++; occluded = decides(q, t.leaf[first + j]) || occluded; }   // (no early exit: the definition, not the schedule)
        }
    }
    return occluded;
}
bool used(const BvhNodeWide& n, int k) { return n.minx[k] < 1.0e29f; }   // (an unused slot is an unreachable point box: bvh_build.cpp empty_wide)
}  // namespace

extern "C" {

// out: {four-wide nodes, leaf triangles, rides in LDS (scene_prep.hpp rides_in_lds), inner children whose index is NOT greater than their parent's}
void ww_tree(const void* tris_in, int ntris, int pairwise, int* out) {
    Tree t; build(tris_in, ntris, pairwise, t);
    int bad = 0;
    for (size_t n = 0; n < t.wide.size(); n++)
        for (int k = 0; k < 4; k++)
            if (used(t.wide[n], k) && t.wide[n].child[k] >= 0 && !((size_t)t.wide[n].child[k] > n && (size_t)t.wide[n].child[k] < t.wide.size())) bad++;
    out[0] = (int)t.wide.size(); out[1] = (int)t.leaf.size(); out[2] = scene::rides_in_lds(t.wide.size(), t.leaf.size()) ? 1 : 0; out[3] = bad;
}

// n rays (o, d: n x 3).  light = 0: occluded <=> some triangle is hit in (tmin, tmax).  light = 1: gid[i] is the sampled triangle — tested first by
// its own record over (tmin, tmax) as closest_is does (in_search[i] = 0 and no search when it misses or is in no leaf), then: does anything beat its
// hit at t_e?  by_stack / by_walk: one byte per ray.  totals: {nodes entered, triangles tested} by the walk's definition, over all rays.
void ww_run(const void* tris_in, int ntris, int pairwise, int form, int light, int64_t n, const float* o, const float* d, const uint32_t* gid, float tmin, float tmax,
            uint8_t* in_search, uint8_t* by_stack, uint8_t* by_walk, int64_t* totals) {
    Tree t; build(tris_in, ntris, pairwise, t);
    std::vector<BvhTri> tris(ntris);
    memcpy(tris.data(), tris_in, sizeof(BvhTri) * (size_t)ntris);
    const float reach = kSlabFmaReach * bvh_max_abs_coord(tris);
    uint32_t total = 0;
    for (const BvhTri& tr : t.leaf) total = tr.gid + 1 > total ? tr.gid + 1 : total;
    const std::vector<uint32_t> slot_of = scene::slot_of_gid(t.leaf, total);
    totals[0] = totals[1] = 0;
    for (int64_t i = 0; i < n; i++) {
        in_search[i] = by_stack[i] = by_walk[i] = 0;
        float t_e = 0.0f; uint32_t expect = 0u;
        if (light) {
            expect = gid[i];
            const uint32_t slot = expect < total ? slot_of[expect] : 0xffffffffu;
            if (slot == 0xffffffffu) continue;
            const BvhTri& tr = t.leaf[slot];
            float u, v;
            if (!vptfp::ray_triangle(vptfp::v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), vptfp::v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), vptfp::v3(tr.v0[0], tr.v0[1], tr.v0[2]),
                                     vptfp::v3(tr.e1[0], tr.e1[1], tr.e1[2]), vptfp::v3(tr.e2[0], tr.e2[1], tr.e2[2]), tmin, tmax, &t_e, &u, &v)) continue;
        }
        in_search[i] = 1;
        const Query q = make_query(o + 3 * i, d + 3 * i, tmin, tmax, light != 0, t_e, expect, form, reach);
        int ne = 0, tt = 0;
        by_stack[i] = stack_search(t, q) ? 1 : 0;
        by_walk[i] = walk(t, q, &ne, &tt) ? 1 : 0;
        totals[0] += ne; totals[1] += tt;
    }
}

}  // extern "C"
