// bvh_refit.hpp — the arithmetic of a BVH refit: the tree keeps its topology (children, leaves, slots) and every box is recomputed bottom-up from
// re-transformed triangles.  One source for the builder's quantiser (bvh_build.cpp calls put_boxes), the refit kernels (kernels_aux.hip
// k_retransform_tris / k_refit_level) and the host driver that holds them to each other (tests/tools/refit_driver.cpp, tests/test_refit_cpu.py).
// Plain __host__ __device__ arithmetic on plain values, no HIP call.  Every min / max is std::min / std::max's expression, every quantiser step that
// rounds is in double, and every product there is an integer times a power of two, so host and device agree bit for bit under -ffp-contract=off.
#pragma once
#include <algorithm>
#include <vector>

#include "device_types.hpp"   // (+ vpt.h, vpt_fp32.h)

// The refit kernels run once per edit, one thread per node: their loops stay loops (the library's size is bounded, tests/test_abi.py).
#if defined(__clang__)
#define VPT_REFIT_ROLLED _Pragma("unroll 1")
#else
#define VPT_REFIT_ROLLED
#endif

namespace vpt {
namespace refit {

struct Box {
    float lo[3], hi[3];
};
VPT_HD void box_reset(Box& b) { for (int a = 0; a < 3; a++) { b.lo[a] = 3.0e38f; b.hi[a] = -3.0e38f; } }
VPT_HD void box_grow(Box& b, const float* p) { for (int a = 0; a < 3; a++) { b.lo[a] = vptfp::min_(b.lo[a], p[a]); b.hi[a] = vptfp::max_(b.hi[a], p[a]); } }
VPT_HD void box_grow(Box& b, const Box& o) { for (int a = 0; a < 3; a++) { b.lo[a] = vptfp::min_(b.lo[a], o.lo[a]); b.hi[a] = vptfp::max_(b.hi[a], o.hi[a]); } }

// The world triangle of (instance, primitive), exactly as scene::prepare forms it: mat_point on the three positions, edges from the first.
VPT_HD void world_triangle(const float* xform, const float* p0, const float* p1, const float* p2, BvhTri& t) {
    const V3 a = vptfp::mat_point(xform, vptfp::v3(p0[0], p0[1], p0[2]));
    const V3 b = vptfp::mat_point(xform, vptfp::v3(p1[0], p1[1], p1[2]));
    const V3 c = vptfp::mat_point(xform, vptfp::v3(p2[0], p2[1], p2[2]));
    const V3 e1 = b - a, e2 = c - a;
    t.v0[0] = a.x; t.v0[1] = a.y; t.v0[2] = a.z;
    t.e1[0] = e1.x; t.e1[1] = e1.y; t.e1[2] = e1.z;
    t.e2[0] = e2.x; t.e2[1] = e2.y; t.e2[2] = e2.z;
}
VPT_HD bool degenerate(const BvhTri& t) { return vptfp::triangle_degenerate(vptfp::v3(t.e1[0], t.e1[1], t.e1[2]), vptfp::v3(t.e2[0], t.e2[1], t.e2[2])); }
// A triangle's box as the builder's references hold it (build_bvh_ex, Ref::b): min / max of v0, v0 + e1, v0 + e2.
VPT_HD void grow_triangle(Box& b, const BvhTri& t) {
    float p1[3], p2[3];
    for (int a = 0; a < 3; a++) { p1[a] = t.v0[a] + t.e1[a]; p2[a] = t.v0[a] + t.e2[a]; }
    box_grow(b, t.v0); box_grow(b, p1); box_grow(b, p2);
}
// Largest |coordinate| of those three vertices (bvh_max_abs_coord's term for one triangle).  Never negative, so the unsigned order of its bits
// is its order as a number: a maximum over triangles may be taken on the bits, in any order.
VPT_HD float max_abs_coord(const BvhTri& t) {
    float m = 0.0f;
    for (int a = 0; a < 3; a++) {
        const float p0 = t.v0[a], p1 = t.v0[a] + t.e1[a], p2 = t.v0[a] + t.e2[a];
        m = vptfp::max_(m, vptfp::max_(vptfp::fabs_(p0), vptfp::max_(vptfp::fabs_(p1), vptfp::fabs_(p2))));
    }
    return m;
}
// Conservative padding so a box test can never cull a triangle the shared ray_triangle() accepts; extent = bvh_max_abs_coord.
VPT_HD float pad_of(float extent) { return 2.0e-5f * extent + 1.0e-6f; }

// Which child slots of a node are in use.  The builder fills slots 0 .. nk - 1 and leaves the others as empty_node / empty_wide wrote them: an
// inverted byte box (lower plane 255 above upper plane 0; a used slot always has lower <= upper) and a point box at 1e30.  A refit leaves
// unused slots exactly so.
VPT_HD bool slot_used(const BvhNode& n, int k) { return ((n.lo[0] >> (8 * k)) & 0xffu) <= ((n.hi[0] >> (8 * k)) & 0xffu); }
VPT_HD bool slot_used(const BvhNodeWide& n, int k) { return n.minx[k] != 1.0e30f; }
VPT_HD int used_slots(const BvhNode& n) { int nk = 0; while (nk < 4 && slot_used(n, nk)) nk++; return nk; }

// 2^(e - 127) as a double, e a biased fp32 exponent in [0, 254]: ldexp(1.0, e - 127).
VPT_HD double pow2_biased(int e) { return __builtin_bit_cast(double, (uint64_t)(e - 127 + 1023) << 52); }
// frexp's exponent of a positive normal double (every positive difference of two floats, over 255, is one).
VPT_HD int frexp_exponent(double x) { return (int)((__builtin_bit_cast(uint64_t, x) >> 52) & 0x7ffu) - 1022; }

// Quantise the (padded) child boxes bx[0 .. nk - 1] of one node: origin = their common lower corner, step = the smallest power of two whose 255
// steps span them; lower planes round down, upper planes round up, checked in double (origin + q * step is exact there) so the decoded box
// is a superset of the fp32 one.  The wide node (optional) takes the padded fp32 boxes themselves.  Slots from nk on get the inverted byte box;
// the wide node's are not touched.  B: anything with float lo[3], hi[3].
template <class B>
VPT_HD void put_boxes(BvhNode& n, BvhNodeWide* w, const B* bx, int nk, float pad) {
    if (w)
        for (int k = 0; k < nk; k++) {
            w->minx[k] = bx[k].lo[0] - pad; w->miny[k] = bx[k].lo[1] - pad; w->minz[k] = bx[k].lo[2] - pad;
            w->maxx[k] = bx[k].hi[0] + pad; w->maxy[k] = bx[k].hi[1] + pad; w->maxz[k] = bx[k].hi[2] + pad;
        }
    VPT_REFIT_ROLLED
    for (int a = 0; a < 3; a++) {
        float lo = bx[0].lo[a] - pad, hi = bx[0].hi[a] + pad;
        for (int k = 1; k < nk; k++) { lo = vptfp::min_(lo, bx[k].lo[a] - pad); hi = vptfp::max_(hi, bx[k].hi[a] + pad); }
        const double org = lo, ext = (double)hi - (double)lo;
        int e = 1;  // biased exponent, step = 2^(e-127)
        if (ext > 0.0) { const int ex = frexp_exponent(ext / 255.0); e = ex + 127 < 1 ? 1 : (ex + 127 > 254 ? 254 : ex + 127); }
        while (e < 254 && org + 255.0 * pow2_biased(e) < (double)hi) e++;
        const double step = pow2_biased(e), per_step = pow2_biased(254 - e);   // (dividing by a power of two = multiplying by its inverse, exactly)
        n.origin[a] = lo;
        n.set_step(a, (uint32_t)e);
        uint32_t wl = 0xffffffffu, wh = 0u;
        VPT_REFIT_ROLLED
        for (int k = 0; k < nk; k++) {
            const double cl = (double)(bx[k].lo[a] - pad), ch = (double)(bx[k].hi[a] + pad);
            int ql = (int)__builtin_floor((cl - org) * per_step), qh = (int)__builtin_ceil((ch - org) * per_step);
            ql = ql < 0 ? 0 : (ql > 255 ? 255 : ql); qh = qh < 0 ? 0 : (qh > 255 ? 255 : qh);
            while (ql > 0 && org + ql * step > cl) ql--;
            while (qh < 255 && org + qh * step < ch) qh++;
            wl = (wl & ~(0xffu << (8 * k))) | (uint32_t)ql << (8 * k);
            wh = (wh & ~(0xffu << (8 * k))) | (uint32_t)qh << (8 * k);
        }
        n.lo[a] = wl; n.hi[a] = wh;
    }
}

// One node of a refit.  Per used slot the child's UNPADDED box: a leaf's is the union of its triangles in `tris` (the re-transformed ones; under
// spatial splits a reference gets the bounds of its whole triangle, a superset of the clipped part it was built with), an inner child's is what
// that child left in `boxes` (6 floats per node: lo, hi), so every node of a lower height must have run before.  The node leaves its own union
// there and writes itself to nodes_out (and wide_out, when the scene has wide nodes): children, leaves and unused slots as in nodes_in / wide_in.
// (A child or a leaf range outside the arrays — no tree of the builder's has one — is skipped, never read.)
VPT_HD void refit_node(uint32_t i, const BvhNode* nodes_in, const BvhNodeWide* wide_in, uint32_t node_count, const BvhTri* tris, uint32_t tri_count, float pad, float* boxes,
                       BvhNode* nodes_out, BvhNodeWide* wide_out) {
    BvhNode n = nodes_in[i];
    const int nk = used_slots(n);
    Box bx[4], all;
    box_reset(all);
    VPT_REFIT_ROLLED
    for (int k = 0; k < nk; k++) {
        const int32_t c = n.child[k];
        if (c < 0) {
            const uint32_t code = (uint32_t)~c, first = code >> 3, count = (code & 7u) + 1u;
            box_reset(bx[k]);
            VPT_REFIT_ROLLED
            for (uint32_t t = 0; t < count && first + t < tri_count; t++) grow_triangle(bx[k], tris[first + t]);
        } else if ((uint32_t)c < node_count) {
            for (int a = 0; a < 3; a++) { bx[k].lo[a] = boxes[(size_t)c * 6 + a]; bx[k].hi[a] = boxes[(size_t)c * 6 + 3 + a]; }
        } else {
            box_reset(bx[k]);
        }
        box_grow(all, bx[k]);
    }
    for (int a = 0; a < 3; a++) { boxes[(size_t)i * 6 + a] = all.lo[a]; boxes[(size_t)i * 6 + 3 + a] = all.hi[a]; }
    if (wide_out) wide_out[i] = wide_in[i];
    if (nk > 0) put_boxes(n, wide_out ? wide_out + i : nullptr, bx, nk, pad);   // (nk == 0: the one node of an empty scene stays as it is)
    nodes_out[i] = n;
}

// The order a refit visits the nodes in: by HEIGHT (0: only leaf children; else 1 + the tallest inner child), so that the nodes of one height can run
// in parallel behind those below them.  order = node indices sorted by height (by index within one), level_off[h] .. level_off[h + 1] = height h's.
// (The builder numbers a parent below its children — top_first keeps that — so one backward pass knows every child's height.)
inline void levels(const std::vector<BvhNode>& nodes, std::vector<uint32_t>& order, std::vector<uint32_t>& level_off) {
    const size_t n = nodes.size();
    std::vector<uint32_t> height(n, 0u);
    uint32_t top = 0;
    for (size_t i = n; i-- > 0;) {
        uint32_t h = 0;
        for (int k = 0; k < 4; k++) { const int32_t c = nodes[i].child[k]; if (c >= 0) h = std::max(h, height[c] + 1u); }
        height[i] = h; top = std::max(top, h);
    }
    level_off.assign(n ? top + 2u : 1u, 0u);
    for (size_t i = 0; i < n; i++) level_off[height[i] + 1]++;
    for (size_t h = 1; h < level_off.size(); h++) level_off[h] += level_off[h - 1];
    order.resize(n);
    std::vector<uint32_t> next(level_off.begin(), level_off.end());
    for (size_t i = 0; i < n; i++) order[next[height[i]]++] = (uint32_t)i;
}

}  // namespace refit
}  // namespace vpt
