"""vpt_denoise restated in float64 numpy, from the description in include/vpt.h and not from csrc/denoise.hpp: the edge-avoiding a-trous filter
(Dammertz et al. 2010) with optional albedo demodulation.  Vectorised over pixels, one tap at a time; divisions where the description has divisions.
tests/test_denoise_cpu.py holds the host compile of the library's arithmetic to this."""
import numpy as np

KERNEL = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float64)
DEMODULATE = 1


def denoise64(colour, normal, albedo, depth, iterations, sigma_color, sigma_normal, sigma_depth, flags):
    """colour, normal, albedo: [h, w, 4]; depth: [h, w] (t, < 0 on a miss) -> float64 [h, w, 4]."""
    c = np.asarray(colour, np.float64)
    n = np.asarray(normal, np.float64)[..., :3]
    t = np.asarray(depth, np.float64)
    h, w = t.shape
    if iterations == 0:
        return c.copy()
    hit = t >= 0
    scale = np.maximum(np.asarray(albedo, np.float64)[..., :3], 1e-3) if flags & DEMODULATE else np.ones((h, w, 3))
    e = np.where(hit[..., None], c[..., :3] / scale, c[..., :3])
    for i in range(iterations):
        s = 1 << i
        num = np.zeros((h, w, 3))
        den = np.zeros((h, w))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                # the part of the image whose tap (x + s dx, y + s dy) lies inside it
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
                # (a miss tap's colour may be anything, 1e30 included: it is left out, not multiplied by 0)
                num[P] += kw[..., None] * np.where(hit[Q][..., None], e[Q], 0.0)
                den[P] += kw
        den = np.where(hit, den, 1.0)
        e = np.where(hit[..., None], num / den[..., None], e)
    out = c.copy()
    out[..., :3] = np.where(hit[..., None], e * scale, c[..., :3])
    return out
