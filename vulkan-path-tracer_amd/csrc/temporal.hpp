// temporal.hpp — the arithmetic of vpt_temporal_accumulate, once: the temporal half of SVGF.  The previous result is reprojected through the first-hit
// geometry of the current frame (the VPT_FEATURES_CENTER guides), kept where the same surface is still seen, and the new samples are blended in.  Plain
// functions on plain values built from vptfp:: leaves only (+ - * /, floor_, min_, max_, fabs_, sqrt_, mat_v4, normalize, dot), no context and no HIP
// call: kernels_post.hip k_temporal calls temporal_pixel per pixel, tests/tools/temporal_driver.cpp runs it on the host (tests/test_temporal_cpu.py), and
// because the library is built without contraction and with correctly rounded division and square root the two give the same bits.  The order of every
// sum is fixed HERE: taps (0,0), (1,0), (0,1), (1,1), then channels r, g, b, then the length.
//
// Per pixel p = (x, y) of the current frame, with cur = the accumulation image, (n, t) / albedo / instance = the guides of p, m = frames in cur:
//   miss        t < 0: the image is cur bit for bit, the length 0.  A miss is never a valid tap.
//   world point (o, d) = camera_ray_with(current camera, 0.5, 0.5, (0, 0), x, y), d = normalize(d) — k_first_hit's ray — and X = o + t d.
//   previous    clip = mat_v4(prev.clip, (X, 1)); prev.clip is the previous camera's projection * view (prev_camera_of, below: formed once per call on
//   pixel       the host, in double).  !(clip.w > 0): no history.  fx = ((clip.x / clip.w + 1) 0.5) W - 0.5, fy alike — the inverse of camera_ray's
//               dx = cx / W 2 - 1 with cx = x + 0.5;  x0 = floor_(fx), ax = fx - x0, y alike.
//   depth       te = length(X - o_prev): guide depths are ray distances of unit directions.
//   taps        q = (x0 + i, y0 + j), weight b = bilinear (1 - ax | ax) (1 - ay | ay).  A tap counts when it is inside the image, the previous guide is
//               a hit, |t_q - te| <= depth_tolerance te, dot(n_p, n_q) >= normal_threshold and — MATCH_INSTANCE — the instance ids are equal.
//               sw += b, sc += b hist_q (r, g, b), sl += b len_q.  A tap that does not count is not read into any sum: its colour may be anything.
//   history     exists iff sw > kMinWeight; then hist = sc / sw, n = sl / sw.
//   blend       none:  e = e_cur, len = min_(m, max_history)
//               some:  n' = min_(n + m, max_history), a = min_(m / n', 1), e = hist + (e_cur - hist) a, len = n'; where a is 1 (max_history reached
//               by m alone) e is e_cur itself, not the lerp's rounding of it.
//   DEMODULATE  e_cur = cur.rgb / max_(albedo, 1e-3) (denoise::albedo_scale), the history is kept demodulated, and the image is e * that scale of the
//               CURRENT pixel; otherwise e_cur = cur.rgb.  Alpha is cur's.
// What is kept per pixel for the next call (the record): (e.rgb, len) as one F4, the packed guide (n.xyz, t) as one F4, the instance id as one uint32 —
// a tap is two 16-byte reads and one 4-byte read.
// Non-finite input propagates: a NaN or an infinite colour — of cur, or of a counted tap — reaches the result and the history.  There is no guard.
// Moved instances (vpt_temporal_options.instance_motion, off by default: vpt_set_instance_transforms then drops the history): the PREVIOUS TRANSFORM of an
// instance is the matrix it had when the latest record was made, however many moves lie between (MotionSnapshot, below).  Per instance, on the host in double
// and rounded to float once (instance_motion_of): D = M_prev M_cur^-1 and nt = the inverse transpose of D's upper 3 x 3.  A hit pixel of a moved instance then
// uses Xp = mat_v4(D, (X, 1)).xyz — where its surface point WAS — for X in the clip transform and in te, and normalize(nt n_p) for n_p in the normal test;
// an instance whose two matrices are equal byte for byte keeps X and n_p as they are (today's bits), and one whose M_cur or D is singular or not finite has
// no history.  The instance test, the weights, the blend, the moments and the variance are untouched (temporal_pixel_motion, at the end of this file).
// The motion image is (fx - x, fy - y) wherever fx, fy were computed and (0, 0) elsewhere.  What no reprojection can give: the history of a pixel NEAR a
// moved object still carries the old lighting — its shadow and its reflection lag by up to max_history frames, as in SVGF.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "camera.hpp"
#include "denoise.hpp"

namespace vpt {
namespace temporal {

using denoise::F4;

constexpr float kMinWeight = 0.01f;   // least sum of counted bilinear weights that is a history
constexpr uint32_t kDemodulate = 1u, kMatchInstance = 2u;   // VPT_TEMPORAL_DEMODULATE / VPT_TEMPORAL_MATCH_INSTANCE

// What the previous camera contributes: projection * view as float[16] (column-major, m[col*4+row]) and its position.
struct PrevCamera {
    float clip[16];
    float origin[3];
    uint32_t ok;   // 0: one of the matrices is singular (or not finite) — no history for the whole frame
};
// One frame's launch constants.  The first six fields are what camera_ray_with reads of a camera.
struct Frame {
    float view_inv[16], proj_inv[16];
    uint32_t width, height;
    float focus_distance, dof_strength;
    PrevCamera prev;
    uint32_t have_prev;    // a previous record exists and prev.ok
    float m, max_history, depth_tolerance, normal_threshold;
    uint32_t flags;
};
struct Result {
    F4 image;    // what the caller sees
    F4 record;   // (e.rgb, len): the history of the next call
};

// ---- host only: the previous camera
// General 4 x 4 inverse by cofactors, in double; column-major in and out.  false: singular or not finite.
inline bool inverse4_double(const double* m, double* inv) {
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    const double det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    if (!(det != 0.0) || !(det - det == 0.0)) return false;   // zero, NaN or infinite
    const double r = 1.0 / det;
    for (int i = 0; i < 16; i++) inv[i] = inv[i] * r;
    return true;
}
// projection * view of the camera whose stored matrices are view_inv / proj_inv: both inverted and multiplied in double, rounded to float once.
// The library (api_post.hip) and the host driver call this one function.
inline PrevCamera prev_camera_of(const float* view_inv, const float* proj_inv) {
    PrevCamera pc;
    double vi[16], pi[16], view[16], proj[16];
    for (int i = 0; i < 16; i++) { vi[i] = (double)view_inv[i]; pi[i] = (double)proj_inv[i]; pc.clip[i] = 0.0f; }
    const V4 o4 = mat_v4(view_inv, v4(0.0f, 0.0f, 0.0f, 1.0f));   // camera_ray's origin: the same bits
    pc.origin[0] = o4.x; pc.origin[1] = o4.y; pc.origin[2] = o4.z;
    pc.ok = (inverse4_double(vi, view) && inverse4_double(pi, proj)) ? 1u : 0u;
    if (!pc.ok) return pc;
    for (int col = 0; col < 4; col++)
        for (int row = 0; row < 4; row++) {
            const double s = ((proj[0 * 4 + row] * view[col * 4 + 0] + proj[1 * 4 + row] * view[col * 4 + 1]) + proj[2 * 4 + row] * view[col * 4 + 2]) + proj[3 * 4 + row] * view[col * 4 + 3];
            pc.clip[col * 4 + row] = (float)s;
            if (!(s - s == 0.0)) pc.ok = 0u;
        }
    return pc;
}

// ---- per pixel
// prev.guide(x, y) / prev.hist(x, y) / prev.inst(x, y): the previous record at a pixel INSIDE the image — where they are read from is the caller's business
// and changes no bit; never called when f.have_prev is 0.  cur, guide = (n.xyz, t), albedo, inst: the pixel's own.
template <class Prev>
VPT_HD Result temporal_pixel(const Prev& prev, const Frame& f, int x, int y, const F4& cur, const F4& guide, const F4& albedo, uint32_t inst) {
    Result r;
    if (!denoise::is_hit(guide)) {
        r.image = cur;
        r.record = denoise::f4(cur.x, cur.y, cur.z, 0.0f);
        return r;
    }
    const bool demodulate = (f.flags & kDemodulate) != 0u;
    const F4 scale = denoise::albedo_scale(albedo);
    float er = cur.x, eg = cur.y, eb = cur.z;
    if (demodulate) { er = er / scale.x; eg = eg / scale.y; eb = eb / scale.z; }
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sl = 0.0f;
    if (f.have_prev) {
        V3 o, d;
        V2 rc; rc.x = 0.0f; rc.y = 0.0f;
        camera_ray_with(f, 0.5f, 0.5f, rc, (uint32_t)x, (uint32_t)y, o, d);
        d = normalize(d);
        const V3 X = o + guide.w * d;
        const V4 clip = mat_v4(f.prev.clip, v4(X.x, X.y, X.z, 1.0f));
        if (clip.w > 0.0f) {
            const float fx = ((clip.x / clip.w + 1.0f) * 0.5f) * (float)f.width - 0.5f;
            const float fy = ((clip.y / clip.w + 1.0f) * 0.5f) * (float)f.height - 0.5f;
            const float x0 = floor_(fx), y0 = floor_(fy);
            const float ax = fx - x0, ay = fy - y0;
            const float te = length(X - v3(f.prev.origin[0], f.prev.origin[1], f.prev.origin[2]));
            const float tol = f.depth_tolerance * te;
            const V3 np = v3(guide.x, guide.y, guide.z);
            for (int k = 0; k < 4; k++) {
                const int i = k & 1, j = k >> 1;
                const float qxf = x0 + (float)i, qyf = y0 + (float)j;
                if (!(qxf >= 0.0f && qxf < (float)f.width && qyf >= 0.0f && qyf < (float)f.height)) continue;   // (a NaN is outside)
                const int qx = (int)qxf, qy = (int)qyf;
                const F4 gq = prev.guide(qx, qy);
                const F4 hq = prev.hist(qx, qy);   // (asked for before gq is looked at: the reads of a tap are in flight together)
                const uint32_t iq = prev.inst(qx, qy);
                if (!denoise::is_hit(gq)) continue;
                if (!(fabs_(gq.w - te) <= tol)) continue;
                if (!(dot(np, v3(gq.x, gq.y, gq.z)) >= f.normal_threshold)) continue;
                if ((f.flags & kMatchInstance) != 0u && iq != inst) continue;
                const float b = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                sw = sw + b;
                sr = sr + b * hq.x;
                sg = sg + b * hq.y;
                sb = sb + b * hq.z;
                sl = sl + b * hq.w;
            }
        }
    }
    float len = min_(f.m, f.max_history);
    if (sw > kMinWeight) {
        const float hr = sr / sw, hg = sg / sw, hb = sb / sw, n = sl / sw;
        len = min_(n + f.m, f.max_history);
        const float a = min_(f.m / len, 1.0f);
        if (a < 1.0f) {
            er = hr + (er - hr) * a;
            eg = hg + (eg - hg) * a;
            eb = hb + (eb - hb) * a;
        }
    }
    r.record = denoise::f4(er, eg, eb, len);
    r.image = demodulate ? denoise::f4(er * scale.x, eg * scale.y, eb * scale.z, cur.w) : denoise::f4(er, eg, eb, cur.w);
    return r;
}

// ---- per pixel, with the luminance moments (vpt_svgf_options.variance == 1): SVGF's variance estimate
// temporal_pixel above, statement for statement — image and record have its bits — and beside it a second record per pixel, the first and second moment
// of the luminance l = luminance(e_cur) of the SAME e_cur the colour blend uses (demodulated under DEMODULATE):
//   taps        a counted tap adds b mu1_q and b mu2_q to two more sums, after the length's: the same taps, the same weights.
//   history     sw > kMinWeight: h1 = s1 / sw, h2 = s2 / sw, mu1 = h1 + (l - h1) a, mu2 = h2 + (l l - h2) a with the colour's own a; where a is 1 the new
//               values (l, l l) themselves.  No history: (l, l l).
//   variance    max_(0, mu2 - mu1 mu1) where len' >= min_len (= min_history m, formed by the caller), -1 ("unknown": too few images for the moments to
//               mean anything) otherwise, 0 on a miss.  A miss has moments (0, 0) and is never a tap.
// prev.moments(x, y): the previous moment record, read beside prev.hist.  Non-finite input propagates; there is no guard.
// k_temporal calls THIS function for both settings of the option (one kernel: the library's size bound) and drops the moments when it is off — image and
// record are temporal_pixel's bits either way, which tests/test_svgf_cpu.py holds on the host and tests/test_gpu_temporal.py on the device.
struct alignas(8) M2 { float mu1, mu2; };
struct ResultV {
    Result r;
    M2 moments;
    float variance;
};
constexpr float kUnknownVariance = -1.0f;
// The order of the sum is fixed here: (r + g) + b.
VPT_HD float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

template <class Prev>
VPT_HD ResultV temporal_pixel_variance(const Prev& prev, const Frame& f, float min_len, int x, int y, const F4& cur, const F4& guide, const F4& albedo, uint32_t inst) {
    ResultV rv;
    Result& r = rv.r;
    if (!denoise::is_hit(guide)) {
        r.image = cur;
        r.record = denoise::f4(cur.x, cur.y, cur.z, 0.0f);
        rv.moments.mu1 = 0.0f; rv.moments.mu2 = 0.0f;
        rv.variance = 0.0f;
        return rv;
    }
    const bool demodulate = (f.flags & kDemodulate) != 0u;
    const F4 scale = denoise::albedo_scale(albedo);
    float er = cur.x, eg = cur.y, eb = cur.z;
    if (demodulate) { er = er / scale.x; eg = eg / scale.y; eb = eb / scale.z; }
    const float l = luminance(er, eg, eb);
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sl = 0.0f, s1 = 0.0f, s2 = 0.0f;
    if (f.have_prev) {
        V3 o, d;
        V2 rc; rc.x = 0.0f; rc.y = 0.0f;
        camera_ray_with(f, 0.5f, 0.5f, rc, (uint32_t)x, (uint32_t)y, o, d);
        d = normalize(d);
        const V3 X = o + guide.w * d;
        const V4 clip = mat_v4(f.prev.clip, v4(X.x, X.y, X.z, 1.0f));
        if (clip.w > 0.0f) {
            const float fx = ((clip.x / clip.w + 1.0f) * 0.5f) * (float)f.width - 0.5f;
            const float fy = ((clip.y / clip.w + 1.0f) * 0.5f) * (float)f.height - 0.5f;
            const float x0 = floor_(fx), y0 = floor_(fy);
            const float ax = fx - x0, ay = fy - y0;
            const float te = length(X - v3(f.prev.origin[0], f.prev.origin[1], f.prev.origin[2]));
            const float tol = f.depth_tolerance * te;
            const V3 np = v3(guide.x, guide.y, guide.z);
            for (int k = 0; k < 4; k++) {
                const int i = k & 1, j = k >> 1;
                const float qxf = x0 + (float)i, qyf = y0 + (float)j;
                if (!(qxf >= 0.0f && qxf < (float)f.width && qyf >= 0.0f && qyf < (float)f.height)) continue;   // (a NaN is outside)
                const int qx = (int)qxf, qy = (int)qyf;
                const F4 gq = prev.guide(qx, qy);
                const F4 hq = prev.hist(qx, qy);
                const M2 mq = prev.moments(qx, qy);
                const uint32_t iq = prev.inst(qx, qy);
                if (!denoise::is_hit(gq)) continue;
                if (!(fabs_(gq.w - te) <= tol)) continue;
                if (!(dot(np, v3(gq.x, gq.y, gq.z)) >= f.normal_threshold)) continue;
                if ((f.flags & kMatchInstance) != 0u && iq != inst) continue;
                const float b = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                sw = sw + b;
                sr = sr + b * hq.x;
                sg = sg + b * hq.y;
                sb = sb + b * hq.z;
                sl = sl + b * hq.w;
                s1 = s1 + b * mq.mu1;
                s2 = s2 + b * mq.mu2;
            }
        }
    }
    float len = min_(f.m, f.max_history);
    float mu1 = l, mu2 = l * l;
    if (sw > kMinWeight) {
        const float hr = sr / sw, hg = sg / sw, hb = sb / sw, n = sl / sw;
        len = min_(n + f.m, f.max_history);
        const float a = min_(f.m / len, 1.0f);
        if (a < 1.0f) {
            const float h1 = s1 / sw, h2 = s2 / sw;
            er = hr + (er - hr) * a;
            eg = hg + (eg - hg) * a;
            eb = hb + (eb - hb) * a;
            mu1 = h1 + (mu1 - h1) * a;
            mu2 = h2 + (mu2 - h2) * a;
        }
    }
    r.record = denoise::f4(er, eg, eb, len);
    r.image = demodulate ? denoise::f4(er * scale.x, eg * scale.y, eb * scale.z, cur.w) : denoise::f4(er, eg, eb, cur.w);
    rv.moments.mu1 = mu1; rv.moments.mu2 = mu2;
    rv.variance = len >= min_len ? max_(0.0f, mu2 - mu1 * mu1) : kUnknownVariance;
    return rv;
}

// ---- moved instances (vpt_temporal_options.instance_motion)
// One instance's record, 112 B = seven aligned 16-byte loads: d = D (column-major, d[col*4+row], applied with mat_v4), nt (column-major 3 x 3,
// nt[col*3+row]), the state last.
constexpr uint32_t kMotionStill = 0u, kMotionMoved = 1u, kMotionNoHistory = 2u;
struct alignas(16) InstanceMotion {
    float d[16];
    float nt[9];
    uint32_t pad[2];
    uint32_t state;   // kMotionStill: the two matrices are equal byte for byte (d, nt are not read); kMotionMoved; kMotionNoHistory: M_cur or D's linear part is singular or not finite
};
// Host only, in double, rounded to float once.  The order of every sum: k = 0, 1, 2, 3.
inline InstanceMotion instance_motion_of(const float* prev_xform, const float* cur_xform) {
    InstanceMotion r;
    memset(&r, 0, sizeof r);
    if (memcmp(prev_xform, cur_xform, 64) == 0) return r;
    r.state = kMotionNoHistory;
    double mp[16], mc[16], inv[16], D[16];
    for (int i = 0; i < 16; i++) { mp[i] = (double)prev_xform[i]; mc[i] = (double)cur_xform[i]; }
    if (!inverse4_double(mc, inv)) return r;
    bool ok = true;
    for (int col = 0; col < 4; col++)
        for (int row = 0; row < 4; row++) {
            const double s = ((mp[0 * 4 + row] * inv[col * 4 + 0] + mp[1 * 4 + row] * inv[col * 4 + 1]) + mp[2 * 4 + row] * inv[col * 4 + 2]) + mp[3 * 4 + row] * inv[col * 4 + 3];
            D[col * 4 + row] = s;
            r.d[col * 4 + row] = (float)s;
            if (!(r.d[col * 4 + row] - r.d[col * 4 + row] == 0.0f)) ok = false;   // (NaN, infinite, or beyond float)
        }
    // the inverse transpose of L = D's upper 3 x 3, by cofactors: nt = cof(L) / det L
    const double a = D[0], b = D[4], c = D[8], d = D[1], e = D[5], f = D[9], g = D[2], h = D[6], i = D[10];   // L = [a b c; d e f; g h i]
    const double cof[9] = {e * i - f * h, -(d * i - f * g), d * h - e * g, -(b * i - c * h), a * i - c * g, -(a * h - b * g), b * f - c * e, -(a * f - c * d), a * e - b * d};   // [row*3+col]
    const double det = (a * cof[0] + b * cof[1]) + c * cof[2];
    if (!(det != 0.0) || !(det - det == 0.0)) ok = false;
    for (int row = 0; row < 3 && ok; row++)
        for (int col = 0; col < 3; col++) {
            r.nt[col * 3 + row] = (float)(cof[row * 3 + col] / det);
            if (!(r.nt[col * 3 + row] - r.nt[col * 3 + row] == 0.0f)) ok = false;
        }
    if (ok) r.state = kMotionMoved;
    return r;
}

// Host only: which matrices the instances had when the latest record was made, kept for the instances that were moved since and for those alone.
// note_move BEFORE a range's matrices are overwritten: the first move of an instance after a record keeps its matrix, later ones change nothing — two moves
// compose, and a move there and back compares equal.  table(): the records of a temporal call, or false where no instance's matrix differs byte for byte
// (nothing to upload: the call takes the path without a table).  clear() once a record is made, and wherever the history goes.
struct MotionSnapshot {
    std::vector<uint32_t> ids;     // the instances moved since the record, in the order of their first move
    std::vector<float> xforms;     // their matrices at the record, 16 floats each
    std::vector<uint32_t> slot;    // per instance: 1 + its place in ids, 0 = not moved (sized at the first move)
    // (the current matrices: instance i's 16 floats stand at xform0 + i * stride bytes)
    static const float* at(const void* xform0, size_t stride, uint32_t i) { return (const float*)((const char*)xform0 + (size_t)i * stride); }
    void note_move(uint32_t first, uint32_t count, uint32_t instance_count, const void* xform0, size_t stride) {
        if (slot.size() != instance_count) { clear(); slot.assign(instance_count, 0u); }
        for (uint32_t i = first; i < first + count; i++) {
            if (slot[i]) continue;
            ids.push_back(i);
            const float* m = at(xform0, stride, i);
            xforms.insert(xforms.end(), m, m + 16);
            slot[i] = (uint32_t)ids.size();
        }
    }
    bool table(uint32_t instance_count, const void* xform0, size_t stride, std::vector<InstanceMotion>& out) const {
        if (slot.size() != instance_count) return false;
        bool any = false;
        for (size_t k = 0; k < ids.size() && !any; k++) any = memcmp(&xforms[k * 16], at(xform0, stride, ids[k]), 64) != 0;
        if (!any) return false;
        InstanceMotion still;
        memset(&still, 0, sizeof still);
        out.assign(instance_count, still);
        for (size_t k = 0; k < ids.size(); k++) out[ids[k]] = instance_motion_of(&xforms[k * 16], at(xform0, stride, ids[k]));
        return true;
    }
    void clear() {
        for (uint32_t i : ids) if (i < slot.size()) slot[i] = 0u;
        ids.clear(); xforms.clear();
    }
};

// Per pixel, for every setting: temporal_pixel_variance statement for statement, and where it differs the difference is a branch on `motion`.
//   motion == nullptr, or the pixel's instance is kMotionStill (or beyond motion_count): image, record, moments and variance are temporal_pixel_variance's bits.
//   kMotionMoved: Xp = mat_v4(D, (X, 1)).xyz replaces X in the clip transform and in te; np = normalize(nt n_p), rows summed (x + y) + z, in the normal test.
//   kMotionNoHistory: no tap is read.
// mv: (fx - x, fy - y) where fx, fy were computed — a previous record, clip.w > 0, not kMotionNoHistory — and (0, 0) otherwise, a miss included.
struct ResultM {
    ResultV v;
    V2 mv;
};
template <class Prev>
VPT_HD ResultM temporal_pixel_motion(const Prev& prev, const InstanceMotion* motion, uint32_t motion_count, const Frame& f, float min_len, int x, int y, const F4& cur, const F4& guide,
                                     const F4& albedo, uint32_t inst) {
    ResultM rm;
    ResultV& rv = rm.v;
    Result& r = rv.r;
    rm.mv.x = 0.0f; rm.mv.y = 0.0f;
    if (!denoise::is_hit(guide)) {
        r.image = cur;
        r.record = denoise::f4(cur.x, cur.y, cur.z, 0.0f);
        rv.moments.mu1 = 0.0f; rv.moments.mu2 = 0.0f;
        rv.variance = 0.0f;
        return rm;
    }
    const bool demodulate = (f.flags & kDemodulate) != 0u;
    const F4 scale = denoise::albedo_scale(albedo);
    float er = cur.x, eg = cur.y, eb = cur.z;
    if (demodulate) { er = er / scale.x; eg = eg / scale.y; eb = eb / scale.z; }
    const float l = luminance(er, eg, eb);
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sl = 0.0f, s1 = 0.0f, s2 = 0.0f;
    const uint32_t state = (motion && inst < motion_count) ? motion[inst].state : kMotionStill;
    if (f.have_prev && state != kMotionNoHistory) {
        V3 o, d;
        V2 rc; rc.x = 0.0f; rc.y = 0.0f;
        camera_ray_with(f, 0.5f, 0.5f, rc, (uint32_t)x, (uint32_t)y, o, d);
        d = normalize(d);
        V3 X = o + guide.w * d;
        V3 np = v3(guide.x, guide.y, guide.z);
        if (state == kMotionMoved) {
            const InstanceMotion& im = motion[inst];
            const V4 xp = mat_v4(im.d, v4(X.x, X.y, X.z, 1.0f));
            X = v3(xp.x, xp.y, xp.z);
            np = normalize(v3((im.nt[0] * np.x + im.nt[3] * np.y) + im.nt[6] * np.z, (im.nt[1] * np.x + im.nt[4] * np.y) + im.nt[7] * np.z,
                              (im.nt[2] * np.x + im.nt[5] * np.y) + im.nt[8] * np.z));
        }
        const V4 clip = mat_v4(f.prev.clip, v4(X.x, X.y, X.z, 1.0f));
        if (clip.w > 0.0f) {
            const float fx = ((clip.x / clip.w + 1.0f) * 0.5f) * (float)f.width - 0.5f;
            const float fy = ((clip.y / clip.w + 1.0f) * 0.5f) * (float)f.height - 0.5f;
            rm.mv.x = fx - (float)x; rm.mv.y = fy - (float)y;
            const float x0 = floor_(fx), y0 = floor_(fy);
            const float ax = fx - x0, ay = fy - y0;
            const float te = length(X - v3(f.prev.origin[0], f.prev.origin[1], f.prev.origin[2]));
            const float tol = f.depth_tolerance * te;
            for (int k = 0; k < 4; k++) {
                const int i = k & 1, j = k >> 1;
                const float qxf = x0 + (float)i, qyf = y0 + (float)j;
                if (!(qxf >= 0.0f && qxf < (float)f.width && qyf >= 0.0f && qyf < (float)f.height)) continue;   // (a NaN is outside)
                const int qx = (int)qxf, qy = (int)qyf;
                const F4 gq = prev.guide(qx, qy);
                const F4 hq = prev.hist(qx, qy);
                const M2 mq = prev.moments(qx, qy);
                const uint32_t iq = prev.inst(qx, qy);
                if (!denoise::is_hit(gq)) continue;
                if (!(fabs_(gq.w - te) <= tol)) continue;
                if (!(dot(np, v3(gq.x, gq.y, gq.z)) >= f.normal_threshold)) continue;
                if ((f.flags & kMatchInstance) != 0u && iq != inst) continue;
                const float b = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                sw = sw + b;
                sr = sr + b * hq.x;
                sg = sg + b * hq.y;
                sb = sb + b * hq.z;
                sl = sl + b * hq.w;
                s1 = s1 + b * mq.mu1;
                s2 = s2 + b * mq.mu2;
            }
        }
    }
    float len = min_(f.m, f.max_history);
    float mu1 = l, mu2 = l * l;
    if (sw > kMinWeight) {
        const float hr = sr / sw, hg = sg / sw, hb = sb / sw, n = sl / sw;
        len = min_(n + f.m, f.max_history);
        const float a = min_(f.m / len, 1.0f);
        if (a < 1.0f) {
            const float h1 = s1 / sw, h2 = s2 / sw;
            er = hr + (er - hr) * a;
            eg = hg + (eg - hg) * a;
            eb = hb + (eb - hb) * a;
            mu1 = h1 + (mu1 - h1) * a;
            mu2 = h2 + (mu2 - h2) * a;
        }
    }
    r.record = denoise::f4(er, eg, eb, len);
    r.image = demodulate ? denoise::f4(er * scale.x, eg * scale.y, eb * scale.z, cur.w) : denoise::f4(er, eg, eb, cur.w);
    rv.moments.mu1 = mu1; rv.moments.mu2 = mu2;
    rv.variance = len >= min_len ? max_(0.0f, mu2 - mu1 * mu1) : kUnknownVariance;
    return rm;
}

}  // namespace temporal
}  // namespace vpt
