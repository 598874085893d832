"""The firefly filter in float64, written from the rule in csrc/firefly.hpp's opening comment and not from its code: per pixel the luminances of the window
are collected into a list and SORTED (the header keeps three running maxima), and the window is cut out of a padded array (the header tests every tap's
coordinates).  tests/test_firefly_cpu.py holds the host compile of the header to it."""
import numpy as np

LUMA = np.array([0.2126, 0.7152, 0.0722])
ALBEDO_FLOOR = 1.0e-3


def luminance(radiance, albedo, depth, demodulate):
    """l(q) per pixel [h, w] in float64; NaN where the pixel is a miss (it has no luminance)."""
    e = np.asarray(radiance, np.float64)[..., :3]
    if demodulate:
        e = e / np.maximum(np.asarray(albedo, np.float64)[..., :3], ALBEDO_FLOOR)
    lum = e @ LUMA
    return np.where(np.asarray(depth) < 0, np.nan, lum)


def firefly(radiance, albedo, depth, radius=1, rank=2, threshold=2.0, floor=1.0, demodulate=True):
    """-> dict: image float64 [h, w, 4], clamped / considered bool [h, w], l_p and limit float64 [h, w] (limit NaN where the pixel was not considered)."""
    radiance = np.asarray(radiance, np.float64)
    h, w = radiance.shape[:2]
    lum = luminance(radiance, albedo, depth, demodulate)
    pad = np.full((h + 2 * radius, w + 2 * radius), np.nan)     # outside the image: no luminance
    pad[radius:radius + h, radius:radius + w] = lum
    out = radiance.copy()
    clamped, considered = np.zeros((h, w), bool), np.zeros((h, w), bool)
    limit = np.full((h, w), np.nan)
    side = 2 * radius + 1
    for y in range(h):
        for x in range(w):
            if np.asarray(depth)[y, x] < 0:
                continue
            win = pad[y:y + side, x:x + side].ravel().tolist()
            del win[side * radius + radius]                      # the centre
            taps = sorted((l for l in win if l >= 0.0), reverse=True)     # (a NaN fails l >= 0)
            if len(taps) < rank:
                continue
            considered[y, x] = True
            limit[y, x] = max(threshold * taps[rank - 1], floor)
            if lum[y, x] > limit[y, x]:
                clamped[y, x] = True
                out[y, x, :3] = radiance[y, x, :3] * (limit[y, x] / lum[y, x])
    return dict(image=out, clamped=clamped, considered=considered, l_p=lum, limit=limit)
