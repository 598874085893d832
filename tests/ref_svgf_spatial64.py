"""SVGF's spatial variance estimate for young pixels restated in float64 numpy, from the description in include/vpt.h and not from the header's code:
vectorised over pixels, one window offset at a time, divisions where the description has divisions.  tests/test_svgf_spatial_cpu.py holds the host compile
of csrc/svgf_spatial.hpp to this."""
import numpy as np


def spatial_variance64(normal, depth, moments, length, min_len, variance, radius, sigma_normal, sigma_depth, min_weight):
    """normal [h, w, >=3], depth [h, w] (< 0: a miss), moments [h, w, 2], length [h, w]: the record the temporal step wrote; variance [h, w]: its variance image
    -> (variance' [h, w] float64, sw [h, w]: the sum of weights of a young pixel's window, 0 elsewhere, young [h, w] bool, M2 [h, w]: the window's second
    moment where there is an estimate, 0 elsewhere)."""
    n = np.asarray(normal, np.float64)[..., :3]
    t = np.asarray(depth, np.float64)
    mu = np.asarray(moments, np.float64)
    h, w = t.shape
    hit = t >= 0
    young = hit & ~(np.asarray(length, np.float64) >= min_len)
    sw = np.zeros((h, w)); s = np.zeros((h, w, 2))
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            y0, y1 = max(0, -dy), min(h, h - dy)
            x0, x1 = max(0, -dx), min(w, w - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            if dx == 0 and dy == 0:
                wt = np.ones((y1 - y0, x1 - x0))
            else:
                ring = max(abs(dx), abs(dy))
                dn = np.maximum(0.0, 1.0 - (n[P] * n[Q]).sum(-1)) / sigma_normal
                dz = np.abs(t[P] - t[Q]) / (sigma_depth * ring * np.maximum(t[P], 1e-6))
                with np.errstate(under="ignore", over="ignore", invalid="ignore"):
                    wt = np.exp(-(dn + dz))
            counts = hit[Q] & young[P]
            wt = np.where(counts, wt, 0.0)
            sw[P] += wt
            with np.errstate(invalid="ignore", over="ignore"):
                s[P] += np.where(counts[..., None], wt[..., None] * mu[Q], 0.0)
    enough = young & (sw >= min_weight)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = s / np.where(enough, sw, 1.0)[..., None]
        est = np.maximum(0.0, m[..., 1] - m[..., 0] ** 2)
    out = np.where(young, np.where(enough, est, -1.0), np.asarray(variance, np.float64))
    return out, sw, young, np.where(enough, m[..., 1], 0.0)
