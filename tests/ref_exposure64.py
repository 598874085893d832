"""Auto-exposure restated in float64 numpy, from include/vpt.h's description and not from csrc/exposure.hpp's code: the histogram of log2 luminance,
the trimmed mean over the pixels [lo, hi) in order of luminance, the target and the scale of a first metering.  The luminance itself is formed in float32
(it is the library's input to the logarithm, not part of what is restated); log2, the bin position and everything after it are float64.  What can differ
from the fp32 header: a pixel whose bin position lies within log_'s rounding of a bin edge lands in the neighbouring bin (tests/test_exposure_cpu.py
measures how many do and what that moves)."""
import numpy as np


def luminance32(img):
    img = np.asarray(img, np.float32)
    with np.errstate(all="ignore"):
        return (np.float32(0.2126) * img[..., 0] + np.float32(0.7152) * img[..., 1]) + np.float32(0.0722) * img[..., 2]


def bins64(img, min_log2, max_log2):
    l = luminance32(img).astype(np.float64).ravel()
    b = np.zeros(l.shape, np.int64)
    pos = l > 0                                    # zero, negative, NaN: the black bin
    inf = pos & np.isinf(l)
    fin = pos & ~inf
    with np.errstate(all="ignore"):
        t = (np.log2(l, where=fin, out=np.zeros_like(l)) - float(min_log2)) * (254.0 / (float(max_log2) - float(min_log2)))
    b[fin] = 1 + np.clip(np.floor(t[fin]), 0, 254).astype(np.int64)
    b[inf] = 255
    return b


def meter64(hist, o):
    """hist: 256 counts; o: the options (any object with the fields of vpt_exposure_options) -> None without a target, else (avg_log2, target_log2, scale)."""
    hist = np.asarray(hist, np.int64)
    N = int(hist[1:].sum())
    if N == 0:
        return None
    lo = (N * int(np.rint(np.float32(o.low_percentile) * np.float32(65536)))) >> 16
    hi = min(max((N * int(np.rint(np.float32(o.high_percentile) * np.float32(65536)))) >> 16, lo + 1), N)
    if hi <= lo:
        return None
    c = np.concatenate(([0], np.cumsum(hist[1:])))          # c[b - 1]: pixels in bins 1 .. b - 1
    take = np.maximum(0, np.minimum(c[1:], hi) - np.maximum(c[:-1], lo))
    mean_bin = float((take * np.arange(1, 256)).sum()) / float(take.sum())
    width = (float(o.max_log2) - float(o.min_log2)) / 254.0
    avg = float(o.min_log2) + (mean_bin - 0.5) * width
    target = min(max(np.log2(float(o.key)) - avg + float(o.compensation_log2), float(o.min_exposure_log2)), float(o.max_exposure_log2))
    return avg, target, 2.0 ** target


def first_metering64(img, o):
    return meter64(np.bincount(bins64(img, o.min_log2, o.max_log2), minlength=256), o)
