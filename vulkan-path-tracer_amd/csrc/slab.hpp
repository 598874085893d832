// slab.hpp — the slab test of a ray against an fp32 box (the nodes of a tree staged into LDS, traverse.hpp), in two forms, and the guard
// that says when the cheaper one may be used.  Plain functions of floats, compiled for the device and — by tests/tools/box_entry_host.cpp —
// for the host, so the claim below is tested operation for operation (tests/test_box_entry_fma_cpu.py).
//
//   box_entry      plane distance = (b - o) * inv          a subtract and a multiply per plane
//   box_entry_fma  plane distance = fma(b, inv, -oi)       one instruction per plane, with oi = o * inv rounded once per search
//
// A box test only prunes, it never decides a hit, so a form is correct when it never rejects a box the ray touches.  WHY THE FMA FORM IS:
// let u = 2^-24, M = the scene's largest |coordinate| (DeviceScene::scene_extent: the value the builder pads by), and take a ray that is at
// parameter t in [tmin, tlimit], tmin >= 0, inside the UNPADDED box [lo, hi] on every axis.  On one axis with inv > 0 (inv < 0 mirrors it):
//   * the stored lower plane is b = fl(lo - pad) <= lo - pad', pad' = pad - u (M + pad), pad = 2e-5 M + 1e-6 (bvh_build.cpp);
//   * inv = fl(1 / d) = (1 / d)(1 + e0), or the clamp +-1e30 of safe_inverse when |d| <= 1e-30; either way d * inv = th with
//     0 <= th <= 1 + u, so the ray's own point x = o + t d has (x - o) * inv = t th;
//   * oi = o inv (1 + e2) and the fma rounds once: near = (b inv - oi)(1 + e1) = A (1 + e1) with
//         A = (b - o) inv - o inv e2 <= t th - (pad' - u |o|) inv;
//   * near <= t follows when A <= 0, and otherwise when t th (1 + u) - t <= (pad' - u |o|) inv (1 + u); t th = |x - o| inv and
//     |x - o| <= |o| + M, so it is enough that
//         2u (1 + u)(|o| + M) + u |o| <= pad',    which    3u |o| + 3u M <= 2e-5 M (1 - 3u)    implies.
//     With |o| <= k M that is 3 (k + 1) u <= 2e-5, k <= 110; the guard admits k = kSlabFmaReach = 16 (51 u = 3.1e-6, a sixth of the pad).
//   * the far plane the same way gives far >= t, where the clamped case (th < 1) also needs t <= (pad' - u |o|) 1e30, about 1e24:
//     every caller's tlimit is at most 1e6 (the subtract form needs the same);
//   * so max(near..., tmin) <= t <= min(far..., tlimit) and, with t >= 0, the test `tn <= tf * 1.0000005f` accepts.
// A - its sign included - is exact before the fma's single rounding, so an overflowing plane distance becomes the infinity of the right
// sign; what must NOT overflow is oi itself (o = 1e9 against inv = 1e30), which would make both planes of the axis the same infinity: the
// guard requires |oi| to be finite.  Underflow moves a distance by at most 2^-126, against (pad' - u |o|) |inv| >= 8e-7 |inv|.
// An unused slot (the point box at 1e30) gives near = far on every axis and at least 1e30 (1 - |o| / 1e30) > tlimit on one: never entered
// through a distance below tlimit, as before.
// Rays the guard turns away — a camera farther than 16 scene sizes out, an origin whose product with a clamped reciprocal overflows — take
// the subtract form, whose error does not grow with |o|.  Both forms are conservative, so hits do not depend on which one ran.
//
//   box_entry_dir  the same six fmas on planes the CALLER has sorted: near = the min plane of an axis where inv > 0, the max plane where inv < 0
//                  (decided once per search, traverse.hpp make_slab), far = the other one — no min / max per axis
//
// WHY ITS VALUES ARE box_entry_fma's (and, on planes moved to the origin with oi = 0, box_entry's): b -> fl(b * inv - oi) is monotone — rising
// for inv >= 0, falling for inv < 0; the exact value is, and rounding keeps order — and a box has min <= max on every axis (the builder and the refit
// write them so; an unused slot has min = max), so the near plane's distance IS fmin(t0, t1) and the far plane's IS fmax(t0, t1), the very floats;
// moving both planes by the same o keeps min <= max, since rounding a difference keeps order too.  Where t0 = t1 (an unused slot, a flat box,
// inv = +-0) either choice is the same float.  No NaN is there to make min / max differ from a choice: oi is finite in the fma form (the guard) and
// 0 in the subtract form, reciprocals are clamped, planes are finite — inf - inf and 0 * inf cannot arise, in either function alike.  Only the SIGN of a zero
// may differ (fmin(+0, -0) against the plane picked), and tn >= tmin > 0 in every caller, so a zero never is tn and tf = +-0 rejects either way.
// (An INVERTED box, min > max — neither the builder nor the refit writes one into an fp32 node — is the one input on which the two would differ.)
// tests/test_box_entry_dir_cpu.py compares the two float for float.
#pragma once
#include "../../include/vpt_fp32.h"

namespace vpt {

using vptfp::V3;

VPT_HD float fmin_(float a, float b) { return __builtin_fminf(a, b); }
VPT_HD float fmax_(float a, float b) { return __builtin_fmaxf(a, b); }
constexpr float kMissT = 3.0e38f;
constexpr float kSlabFmaReach = 16.0f;   // the fma form serves origins with |o|_inf <= kSlabFmaReach * scene_extent (the derivation allows 110)

VPT_HD V3 safe_inverse(V3 d) {
    // a zero component would give 0*inf = NaN in the slab test: clamp its reciprocal to +-1e30
    V3 inv;
    inv.x = (vptfp::fabs_(d.x) > 1e-30f) ? 1.0f / d.x : (vptfp::f2u(d.x) >> 31 ? -1e30f : 1e30f);
    inv.y = (vptfp::fabs_(d.y) > 1e-30f) ? 1.0f / d.y : (vptfp::f2u(d.y) >> 31 ? -1e30f : 1e30f);
    inv.z = (vptfp::fabs_(d.z) > 1e-30f) ? 1.0f / d.z : (vptfp::f2u(d.z) >> 31 ? -1e30f : 1e30f);
    return inv;
}

// One fma per plane; oi = slab_oi(o, inv).  Entry distance of the ray into the box ([tmin, tlimit] clipped), kMissT for a miss.
// Only for rays slab_fma_ok() admits.
VPT_HD V3 slab_oi(V3 o, V3 inv) { return vptfp::v3(o.x * inv.x, o.y * inv.y, o.z * inv.z); }
VPT_HD float box_entry_fma(float bx0, float by0, float bz0, float bx1, float by1, float bz1, V3 oi, V3 inv, float tmin, float tlimit) {
    float t0x = __builtin_fmaf(bx0, inv.x, -oi.x), t1x = __builtin_fmaf(bx1, inv.x, -oi.x);
    float t0y = __builtin_fmaf(by0, inv.y, -oi.y), t1y = __builtin_fmaf(by1, inv.y, -oi.y);
    float t0z = __builtin_fmaf(bz0, inv.z, -oi.z), t1z = __builtin_fmaf(bz1, inv.z, -oi.z);
    float tn = fmax_(fmax_(fmin_(t0x, t1x), fmin_(t0y, t1y)), fmax_(fmin_(t0z, t1z), tmin));
    float tf = fmin_(fmin_(fmax_(t0x, t1x), fmax_(t0y, t1y)), fmin_(fmax_(t0z, t1z), tlimit));
    return (tn <= tf * 1.0000005f) ? tn : kMissT;
}
// The same on planes sorted by the ray's direction (above): n* = the plane of the axis the ray meets first, f* = the other one.
VPT_HD float box_entry_dir(float nx, float ny, float nz, float fx, float fy, float fz, V3 oi, V3 inv, float tmin, float tlimit) {
    float tnx = __builtin_fmaf(nx, inv.x, -oi.x), tfx = __builtin_fmaf(fx, inv.x, -oi.x);
    float tny = __builtin_fmaf(ny, inv.y, -oi.y), tfy = __builtin_fmaf(fy, inv.y, -oi.y);
    float tnz = __builtin_fmaf(nz, inv.z, -oi.z), tfz = __builtin_fmaf(fz, inv.z, -oi.z);
    float tn = fmax_(fmax_(tnx, tny), fmax_(tnz, tmin));
    float tf = fmin_(fmin_(tfx, tfy), fmin_(tfz, tlimit));
    return (tn <= tf * 1.0000005f) ? tn : kMissT;
}
// The subtract form, for every ray: the planes are moved to the ray's origin first and the shared code runs with oi = 0 — fma(b - o, inv, -0)
// IS fl((b - o) * inv), one rounding, so these are the distances of the plain slab test `(b - o) * inv` (a kernel subtracts under a
// wave-uniform branch and shares the code behind it: traverse.hpp node_entries).
VPT_HD float box_entry(float bx0, float by0, float bz0, float bx1, float by1, float bz1, V3 o, V3 inv, float tmin, float tlimit) {
    return box_entry_fma(bx0 - o.x, by0 - o.y, bz0 - o.z, bx1 - o.x, by1 - o.y, bz1 - o.z, vptfp::v3(0.0f, 0.0f, 0.0f), inv, tmin, tlimit);
}
// The guard of the fma form: the origin within reach = kSlabFmaReach * scene_extent of the world's origin on every axis, and o * inv finite.
// (Two three-way maxima and two compares on the device.  An infinite coordinate fails it; a NaN one is no ray in either form.)
VPT_HD bool slab_fma_ok(V3 o, V3 oi, float reach) {
    return fmax_(fmax_(vptfp::fabs_(o.x), vptfp::fabs_(o.y)), vptfp::fabs_(o.z)) <= reach &&
           fmax_(fmax_(vptfp::fabs_(oi.x), vptfp::fabs_(oi.y)), vptfp::fabs_(oi.z)) <= kMissT;
}

}  // namespace vpt
