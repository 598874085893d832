"""SVGF's variance restated in float64 numpy, from the description in include/vpt.h and not from the headers' code: the luminance moments that
vpt_temporal_accumulate carries with vpt_svgf_options.variance == 1, the variance image, and the variance-guided a-trous passes of vpt_denoise.  Vectorised
over pixels, one tap at a time; divisions where the description has divisions.  The reprojection (which taps count, with what weights) is
ref_temporal64's, restated here tap by tap because the moments need the taps themselves; tests/test_svgf_cpu.py holds the host compile to this."""
import numpy as np

import ref_temporal64 as R64

LUM = np.array([0.2126, 0.7152, 0.0722])
KERNEL = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float64)
PREFILTER = np.array([0.25, 0.5, 0.25])      # outer product: corners 1/16, edges 1/8, centre 1/4
DEMODULATE = 1


def moments64(prev, prev_mu, view_inv, proj_inv, m, cur, normal, albedo, depth, inst, max_history, depth_tolerance, normal_threshold, flags, min_history):
    """prev: ref_temporal64.State or None; prev_mu: its moments [h, w, 2] -> moments [h, w, 2], variance [h, w] (-1 unknown, 0 on a miss), new length [h, w],
    close [h, w] bool: the new length is a reprojected mean within 1e-4 of min_history * m, so that "known" may go either way."""
    c = np.asarray(cur, np.float64)
    n = np.asarray(normal, np.float64)[..., :3]
    t = np.asarray(depth, np.float64)
    h, w = t.shape
    hit = t >= 0
    scale = np.maximum(np.asarray(albedo, np.float64)[..., :3], 1e-3) if flags & R64.DEMODULATE else np.ones((h, w, 3))
    lum = (c[..., :3] / scale) @ LUM
    sw = np.zeros((h, w)); sm = np.zeros((h, w, 2)); sl = np.zeros((h, w))
    clip_m = R64.prev_clip(prev.view_inv, prev.proj_inv) if prev is not None else None
    if clip_m is not None:
        o, d = R64.camera_rays(view_inv, proj_inv, w, h)
        X = o + np.where(hit, t, 1.0)[..., None] * d
        clip = np.concatenate([X, np.ones((h, w, 1))], -1) @ clip_m.T
        front = hit & (clip[..., 3] > 0)
        cw = np.where(front, clip[..., 3], 1.0)
        fx = ((clip[..., 0] / cw + 1.0) * 0.5) * w - 0.5
        fy = ((clip[..., 1] / cw + 1.0) * 0.5) * h - 0.5
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0, fy - y0
        te = np.sqrt(((X - np.asarray(prev.view_inv, np.float64)[:3, 3]) ** 2).sum(-1))
        for (i, j) in ((0, 0), (1, 0), (0, 1), (1, 1)):
            qx, qy = x0 + i, y0 + j
            inside = front & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            ix, iy = np.where(inside, qx, 0).astype(int), np.where(inside, qy, 0).astype(int)
            tq = prev.depth[iy, ix]
            ok = inside & (tq >= 0) & (np.abs(tq - te) / te <= depth_tolerance) & ((n * prev.normal[iy, ix]).sum(-1) >= normal_threshold)
            if flags & R64.MATCH_INSTANCE:
                ok &= prev.inst[iy, ix] == inst
            b = (ax if i else 1.0 - ax) * (ay if j else 1.0 - ay)
            sw += np.where(ok, b, 0.0)
            sm += np.where(ok[..., None], b[..., None] * prev_mu[iy, ix], 0.0)
            sl += np.where(ok, b * prev.length[iy, ix], 0.0)
    has = hit & (sw > R64.MIN_WEIGHT)
    swd = np.where(has, sw, 1.0)
    n_new = np.minimum(sl / swd + m, float(max_history))
    a = np.minimum(m / n_new, 1.0)
    new = np.stack([lum, lum * lum], -1)
    hm = sm / swd[..., None]
    mu = np.where(has[..., None], hm + (new - hm) * a[..., None], new)
    mu = np.where(hit[..., None], mu, 0.0)
    length = np.where(hit, np.where(has, n_new, min(float(m), float(max_history))), 0.0)
    known = hit & (length >= min_history * m)
    var = np.where(known, np.maximum(0.0, mu[..., 1] - mu[..., 0] ** 2), np.where(hit, -1.0, 0.0))
    # (a length without history, or one capped, is a small integer in either precision: only a reprojected mean can fall on either side)
    return mu, var, length, has & (n_new < max_history) & (np.abs(length - min_history * m) < 1e-4)


def fixed_pass64(e, n, t, hit, i, sigma_color, sigma_normal, sigma_depth):
    """One pass of the fixed-sigma_color rule (ref_denoise64's loop body) over e [h, w, 3] -> [h, w, 3] on hit pixels."""
    h, w = t.shape
    s = 1 << i
    num = np.zeros((h, w, 3)); den = np.zeros((h, w))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            y0, y1 = max(0, -s * dy), min(h, h - s * dy)
            x0, x1 = max(0, -s * dx), min(w, w - s * dx)
            if y0 >= y1 or x0 >= x1:
                continue
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + s * dy, y1 + s * dy), slice(x0 + s * dx, x1 + s * dx))
            if dx == 0 and dy == 0:
                wt = np.ones((y1 - y0, x1 - x0))
            else:
                dn = np.maximum(0.0, 1.0 - (n[P] * n[Q]).sum(-1)) / sigma_normal
                dz = np.abs(t[P] - t[Q]) / (sigma_depth * s * np.maximum(t[P], 1e-6))
                dc = ((e[P] - e[Q]) ** 2).sum(-1) / (sigma_color * 2.0 ** -i) ** 2
                with np.errstate(under="ignore"):
                    wt = np.exp(-(dn + dz + dc))
            kw = KERNEL[dy + 2] * KERNEL[dx + 2] * wt * hit[Q]
            num[P] += kw[..., None] * np.where(hit[Q][..., None], e[Q], 0.0)
            den[P] += kw
    return num / np.where(hit, den, 1.0)[..., None]


def denoise_variance64(colour, variance, normal, albedo, depth, iterations, sigma_color, sigma_normal, sigma_depth, flags, sigma_luminance, keep_variance=False):
    """colour, normal, albedo [h, w, 4]; variance, depth [h, w] -> float64 [h, w, 4]; with keep_variance the .w of a hit is the filtered variance, not alpha."""
    c = np.asarray(colour, np.float64)
    n = np.asarray(normal, np.float64)[..., :3]
    t = np.asarray(depth, np.float64)
    h, w = t.shape
    if iterations == 0:
        return c.copy()
    hit = t >= 0
    scale = np.maximum(np.asarray(albedo, np.float64)[..., :3], 1e-3) if flags & DEMODULATE else np.ones((h, w, 3))
    e = np.where(hit[..., None], c[..., :3] / scale, c[..., :3])
    v = np.where(hit, np.asarray(variance, np.float64), -1.0)
    for i in range(iterations):
        s = 1 << i
        known = hit & (v >= 0)
        fixed = fixed_pass64(e, n, t, hit, i, sigma_color, sigma_normal, sigma_depth)
        # g: the 3 x 3 Gaussian of v over the known pixels at distance 1
        gs = np.zeros((h, w)); gw = np.zeros((h, w))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                y0, y1 = max(0, -dy), min(h, h - dy)
                x0, x1 = max(0, -dx), min(w, w - dx)
                P = (slice(y0, y1), slice(x0, x1)); Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                k = PREFILTER[dy + 1] * PREFILTER[dx + 1] * known[Q]
                gs[P] += k * np.where(known[Q], v[Q], 0.0)
                gw[P] += k
        g = gs / np.where(known, gw, 1.0)
        lum = e @ LUM
        num = np.zeros((h, w, 3)); den = np.zeros((h, w)); vnum = np.zeros((h, w))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                y0, y1 = max(0, -s * dy), min(h, h - s * dy)
                x0, x1 = max(0, -s * dx), min(w, w - s * dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + s * dy, y1 + s * dy), slice(x0 + s * dx, x1 + s * dx))
                if dx == 0 and dy == 0:
                    wt = np.ones((y1 - y0, x1 - x0))
                else:
                    dn = np.maximum(0.0, 1.0 - (n[P] * n[Q]).sum(-1)) / sigma_normal
                    dz = np.abs(t[P] - t[Q]) / (sigma_depth * s * np.maximum(t[P], 1e-6))
                    dl = np.abs(lum[P] - lum[Q]) / (sigma_luminance * np.sqrt(np.where(known[P], g[P], 0.0)) + 1e-6)
                    with np.errstate(under="ignore", over="ignore"):
                        wt = np.exp(-(dn + dz + dl))
                kw = KERNEL[dy + 2] * KERNEL[dx + 2] * wt * known[Q]
                num[P] += kw[..., None] * np.where(known[Q][..., None], e[Q], 0.0)
                den[P] += kw
                vnum[P] += kw * kw * np.where(known[Q], v[Q], 0.0)
        den = np.where(known, den, 1.0)
        e = np.where(known[..., None], num / den[..., None], np.where(hit[..., None], fixed, e))
        v = np.where(known, vnum / (den * den), -1.0)
    out = c.copy()
    out[..., :3] = np.where(hit[..., None], e * scale, c[..., :3])
    if keep_variance:
        out[..., 3] = np.where(hit, v, c[..., 3])
    return out
