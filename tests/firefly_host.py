"""What the tests of the firefly filter share: the host compile of csrc/firefly.hpp (tests/tools/firefly_driver.cpp) built and run on one image with its
guides, and the images with planted spikes the CPU tests use."""
import os
import struct
import subprocess

import numpy as np

import temporal_host as TH

ROOT = TH.ROOT
F32 = np.float32
DEFAULTS = dict(radius=1, rank=2, threshold=2.0, floor=1.0, demodulate=1)     # include/vpt.h's defaults, as the temporal call uses them
LUMA = (0.2126, 0.7152, 0.0722)


def compile_driver(exe, extra=()):
    """(the flags of temporal_host.compile_driver)"""
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math", "-march=x86-64-v3"] + list(extra) +
                          ["-I" + TH.CSRC, os.path.join(ROOT, "tests", "tools", "firefly_driver.cpp"), "-o", exe])
    return exe


def run(exe, workdir, radiance, albedo, depth, tag="ff", **params):
    """-> dict: image float32 [h, w, 4], clamped / considered bool [h, w], n_clamped, n_considered: what k_firefly computes, on the host."""
    p = dict(DEFAULTS, **params)
    radiance, albedo, depth = (np.ascontiguousarray(a, F32) for a in (radiance, albedo, depth))
    h, w = depth.shape
    assert radiance.shape == albedo.shape == (h, w, 4)
    src, dst = os.path.join(str(workdir), tag + ".in"), os.path.join(str(workdir), tag + ".out")
    with open(src, "wb") as f:
        f.write(struct.pack("<5I2f", w, h, p["radius"], p["rank"], 1 if p["demodulate"] else 0, p["threshold"], p["floor"]))
        for a in (radiance, albedo, depth):
            f.write(a.tobytes())
    subprocess.check_call([exe, src, dst])
    raw = open(dst, "rb").read()
    n = h * w
    assert len(raw) == 16 * n + 2 * n + 16
    counts = struct.unpack("<2Q", raw[18 * n:])
    return dict(image=np.frombuffer(raw, "<f4", 4 * n).reshape(h, w, 4), clamped=np.frombuffer(raw, np.uint8, n, 16 * n).reshape(h, w).astype(bool),
                considered=np.frombuffer(raw, np.uint8, n, 17 * n).reshape(h, w).astype(bool), n_clamped=counts[0], n_considered=counts[1])


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def luminance32(rgb):
    """denoise.hpp's luminance in float32, in its order."""
    rgb = np.asarray(rgb, F32)
    return (F32(LUMA[0]) * rgb[..., 0] + F32(LUMA[1]) * rgb[..., 1]) + F32(LUMA[2]) * rgb[..., 2]


def flat(w, h, level, albedo=1.0):
    """A flat grey field of hits: radiance (level, level, level, 1) — luminance = level up to rounding —, albedo everywhere `albedo`, depth 1."""
    radiance = np.full((h, w, 4), level, F32); radiance[..., 3] = 1.0
    alb = np.full((h, w, 4), albedo, F32)
    return radiance, alb, np.ones((h, w), F32)


def spiked(w, h, seed, spikes=None, miss_share=0.12):
    """Random guides with planted spikes: the demodulated irradiance is a smooth field (a low-frequency wave, 0.5 .. 4 across the image) times a per-pixel factor
    in [0.9, 1.1]; albedo random in [0.25, 1] per channel; radiance = irradiance * albedo; a share of the pixels, in blobs, are misses (depth -1, environment colours);
    every 11th hit pixel or so carries a spike of 4 .. 40 x its local level in all channels, some of them adjacent pairs.  -> radiance, albedo, depth, spike mask."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    field = 2.25 + 1.75 * np.sin(xx * 0.21 + 0.3) * np.cos(yy * 0.17 - 0.2)
    irr = field[..., None] * rng.uniform(0.9, 1.1, (h, w, 1)) * np.ones((1, 1, 3))
    albedo = np.ones((h, w, 4), F32)
    albedo[..., :3] = rng.uniform(0.25, 1.0, (h, w, 3))
    miss = (np.sin(xx * 0.9 + seed) + np.cos(yy * 1.1 - seed)) > (2.0 - 4.0 * miss_share) if w * h > 1 else np.zeros((h, w), bool)
    n_spikes = max(1, (w * h) // 11) if spikes is None else spikes
    mask = np.zeros((h, w), bool)
    for k in range(n_spikes):
        y, x = int(rng.integers(h)), int(rng.integers(w))
        mask[y, x] = True
        if k % 4 == 0 and x + 1 < w:
            mask[y, x + 1] = True     # an adjacent pair
    mask &= ~miss
    irr = np.where(mask[..., None], irr * rng.uniform(4.0, 40.0, (h, w, 1)), irr)
    radiance = np.ones((h, w, 4), F32)
    radiance[..., :3] = (irr * albedo[..., :3]).astype(F32)
    radiance[miss, :3] = rng.uniform(0.0, 30.0, (int(miss.sum()), 3)).astype(F32)
    albedo[miss] = 0.0
    depth = np.where(miss, -1.0, rng.uniform(1.0, 9.0, (h, w))).astype(F32)
    return radiance, albedo, depth, mask
