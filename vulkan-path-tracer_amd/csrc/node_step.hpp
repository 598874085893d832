// node_step.hpp — the node step of a tree staged into LDS (traverse.hpp) as plain functions of floats and child words: the four-wide step every
// search runs, and the TWO-SLOT step the closest-hit search of the whole-path kernel's PLAIN instantiation (k_whole<false, false, true>) takes at a
// node whose slots 2 and 3 are unused.  Compiled for the device and — by tests/tools/narrow_node_host.cpp — for the host with -ffp-contract=off, so that "the two-slot step is visit for visit the four-wide
// one" is tested float for float, order for order and push for push (tests/test_narrow_node_cpu.py).
//
// HALF-EMPTY NODES.  The builder fills a node's slots from 0 up and leaves the others as point boxes at 1e30 (bvh_build.cpp empty_wide,
// bvh_refit.hpp slot_used); the Cornell tree's nodes 1 and 2 use two slots each.  A four-wide step at such a node reads seven 16-byte words and
// runs four box tests and a five-exchange network, half of it on boxes no ray enters.  Whether a node is half-empty is known BEFORE the node is
// read: while the tree is staged, every child word that names such a node gets kNarrowBit (stage_scene<true, true>; memory is not touched, so a
// refitted tree is flagged from its own planes at the next launch), and a search decides from the word it just selected or popped — no LDS read
// stands between it and the branch, which is what made the ballot on a loaded plane slower than no ballot at all (profiles/REJECTED.md, r13).
// Cornell 1080p, same box, alternating: profiles/r22_narrow_node_ab.md.  The any-hit searches run on the flagged words and take no such step: in
// the light query it issued more instructions than it saved and was slower (profiles/REJECTED.md, r22); their node address drops the flag (node_at).
//
// WHY THE TWO-SLOT STEP IS THE FOUR-WIDE ONE, VISIT FOR VISIT.  box_entry_dir sees the same six floats and the same ray constants for slots 0 and
// 1.  Slots 2 and 3 of a flagged node return kMissT (slab.hpp: an unused slot is never entered), so in the closest-hit order cswap(t2, t3),
// cswap(t0, t2), cswap(t1, t3) and cswap(t1, t2) exchange nothing — cswap swaps on `tb < ta` only, and no t is above kMissT — and slots 0 and 1
// leave the network as the one exchange cswap(t0, t1) leaves them, ties included.  The words pushed and descended into are the node's own child
// words, flag included: a flag travels through the stack and its overflow region as any other bit.  A flagged word is >= 0 (leaf words are negative
// and never flagged) and below 0x7fffffff, the any-hit search's "none".
#pragma once
#include "device_types.hpp"
#include "slab.hpp"

namespace vpt {

constexpr int32_t kNarrowBit = 1 << 30;   // in a child word of the LDS copy: the inner node it names uses slots 0 and 1 only
// Node indices of a tree that rides in LDS stay far below the flag: at most 3 KB of 128-byte nodes (scene_prep.hpp fits_lds).
constexpr int32_t kLdsTreeMaxNodes = 3072 / (int32_t)sizeof(BvhNodeWide);
static_assert(kLdsTreeMaxNodes < kNarrowBit, "a node index of an LDS-resident tree would reach the narrow flag");

// The flag rule: `word` names an inner node j whose slots 0 and 1 are used and whose slots 2 and 3 are not (bvh_refit.hpp slot_used's test on the
// planes as they stand in `nodes`).  The root is entered as cur = 0, by no child word, and so is never flagged.
VPT_HD bool narrow_child(const BvhNodeWide* nodes, int32_t word) {
    if (word < 0) return false;   // a leaf
    const BvhNodeWide& n = nodes[word];
    return n.minx[0] != 1.0e30f && n.minx[1] != 1.0e30f && n.minx[2] == 1.0e30f && n.minx[3] == 1.0e30f;
}

VPT_HD void cswap(float& ta, int& ca, float& tb, int& cb) {
    bool sw = tb < ta;
    float tt = sw ? tb : ta; int ct = sw ? cb : ca;
    tb = sw ? ta : tb; cb = sw ? ca : cb;
    ta = tt; ca = ct;
}

// A ray's constants for the box tests of one search (traverse.hpp make_slab fills them): oi = o * inv in the fma form, 0 in the subtract form;
// selx / sely / selz: which float4 of a node (0..2 = min x y z, 3..5 = max x y z) holds this ray's NEAR planes of the axis.
struct RaySlabWide {
    V3 o, inv, oi;
    bool fused;
    int selx, sely, selz;
};
// near* / far*: the planes of the four children this ray meets first / last on each axis; the four child words.
struct NodeDataWide {
    float4 nearx, neary, nearz, farx, fary, farz;
    int c0, c1, c2, c3;
};
// ... and of slots 0 and 1 alone: the .xy halves of the same vectors (64-bit LDS reads).
struct NodeDataNarrow {
    float2 nearx, neary, nearz, farx, fary, farz;
};

// Where node `word` of a tree at `nodes` lies, for a child word that may carry kNarrowBit: the index times the node's eight float4 is formed in
// 32 unsigned bits, where the flag falls out at the top (bit 30 + 3), so nobody has to clear it.  (A tree in LDS is at most 3 KB.)
VPT_HD const float4* node_at(const float4* nodes, uint32_t word) { return nodes + (uint32_t)(word << 3); }

VPT_HD void load_node_wide(const float4* p, const RaySlabWide& r, NodeDataWide& n) {
    n.nearx = p[r.selx]; n.neary = p[r.sely]; n.nearz = p[r.selz]; n.farx = p[3 - r.selx]; n.fary = p[5 - r.sely]; n.farz = p[7 - r.selz];
    float4 c = p[6];
    n.c0 = (int)vptfp::f2u(c.x); n.c1 = (int)vptfp::f2u(c.y); n.c2 = (int)vptfp::f2u(c.z); n.c3 = (int)vptfp::f2u(c.w);
}
#define VPT_XY(V) make_float2((V).x, (V).y)
VPT_HD void load_node_narrow(const float4* p, const RaySlabWide& r, NodeDataNarrow& n) {
    n.nearx = VPT_XY(p[r.selx]); n.neary = VPT_XY(p[r.sely]); n.nearz = VPT_XY(p[r.selz]);
    n.farx = VPT_XY(p[3 - r.selx]); n.fary = VPT_XY(p[5 - r.sely]); n.farz = VPT_XY(p[7 - r.selz]);
}
#undef VPT_XY
// Child words 0 and 1 of the node at p, read behind the box tests (they are not needed before).
VPT_HD void narrow_children(const float4* p, int& c0, int& c1) {
    const float4& c = p[6];
    c0 = (int)vptfp::f2u(c.x); c1 = (int)vptfp::f2u(c.y);
}

// fp32 nodes: the plain slab test (slab.hpp), one fma per plane (24 instead of 48 fp32 operations per node step) when the wave's origins allow it,
// on planes load_node has sorted by the ray's direction (box_entry_dir: the values of box_entry_fma without its six min / max per box).
VPT_HD void node_entries(const NodeDataWide& n, const RaySlabWide& r, float tmin, float tlimit, float& t0, float& t1, float& t2, float& t3) {
    float4 nx = n.nearx, ny = n.neary, nz = n.nearz, fx = n.farx, fy = n.fary, fz = n.farz;
    if (!r.fused) {   // box_entry(): the 24 subtractions here, oi == 0 behind them
        nx.x -= r.o.x; nx.y -= r.o.x; nx.z -= r.o.x; nx.w -= r.o.x; fx.x -= r.o.x; fx.y -= r.o.x; fx.z -= r.o.x; fx.w -= r.o.x;
        ny.x -= r.o.y; ny.y -= r.o.y; ny.z -= r.o.y; ny.w -= r.o.y; fy.x -= r.o.y; fy.y -= r.o.y; fy.z -= r.o.y; fy.w -= r.o.y;
        nz.x -= r.o.z; nz.y -= r.o.z; nz.z -= r.o.z; nz.w -= r.o.z; fz.x -= r.o.z; fz.y -= r.o.z; fz.z -= r.o.z; fz.w -= r.o.z;
    }
#define VPT_BOX(C) box_entry_dir(nx.C, ny.C, nz.C, fx.C, fy.C, fz.C, r.oi, r.inv, tmin, tlimit)
    t0 = VPT_BOX(x); t1 = VPT_BOX(y); t2 = VPT_BOX(z); t3 = VPT_BOX(w);
#undef VPT_BOX
}
// The same for slots 0 and 1: 12 fmas (and the 12 subtractions of the subtract form), two interval tests.
VPT_HD void node_entries(const NodeDataNarrow& n, const RaySlabWide& r, float tmin, float tlimit, float& t0, float& t1) {
    float2 nx = n.nearx, ny = n.neary, nz = n.nearz, fx = n.farx, fy = n.fary, fz = n.farz;
    if (!r.fused) {
        nx.x -= r.o.x; nx.y -= r.o.x; fx.x -= r.o.x; fx.y -= r.o.x;
        ny.x -= r.o.y; ny.y -= r.o.y; fy.x -= r.o.y; fy.y -= r.o.y;
        nz.x -= r.o.z; nz.y -= r.o.z; fz.x -= r.o.z; fz.y -= r.o.z;
    }
#define VPT_BOX(C) box_entry_dir(nx.C, ny.C, nz.C, fx.C, fy.C, fz.C, r.oi, r.inv, tmin, tlimit)
    t0 = VPT_BOX(x); t1 = VPT_BOX(y);
#undef VPT_BOX
}

// The closest-hit order of one node step, as the whole-path kernel's PLAIN instantiation runs it (traverse.hpp trace_closest_pass) and as the host test
// holds the two forms to each other: hit children nearest first — the nearest is returned (kNoChild: none was entered), the others go to `push`
// far -> near.  The entry distances are left in t0.. as ordered.  (Every other search keeps these statements inline, as it has them: they compile
// to the bytes they did.)
constexpr int kNoChild = 0x7fffffff;   // "no child entered" in a search's node step
template <class Push>
VPT_HD int closest_order(float& t0, int c0, float& t1, int c1, float& t2, int c2, float& t3, int c3, Push&& push) {
    cswap(t0, c0, t1, c1); cswap(t2, c2, t3, c3); cswap(t0, c0, t2, c2); cswap(t1, c1, t3, c3); cswap(t1, c1, t2, c2);
    if (!(t0 < kMissT)) return kNoChild;
    if (t3 < kMissT) push(c3);
    if (t2 < kMissT) push(c2);
    if (t1 < kMissT) push(c1);
    return c0;
}
template <class Push>
VPT_HD int closest_order(float& t0, int c0, float& t1, int c1, Push&& push) {
    cswap(t0, c0, t1, c1);
    if (!(t0 < kMissT)) return kNoChild;
    if (t1 < kMissT) push(c1);
    return c0;
}

}  // namespace vpt
