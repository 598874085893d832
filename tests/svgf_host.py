"""What the SVGF tests share: the host compile of csrc/temporal.hpp's and csrc/denoise.hpp's variance functions (tests/tools/svgf_driver.cpp) built and run
on a sequence of temporal_host.Frame."""
import os
import struct
import subprocess

import numpy as np

import temporal_host as TH

ROOT = TH.ROOT
F32 = np.float32
KEEP_VARIANCE = 256          # a denoise run's flag, the driver's alone: no pass is the last, the result's .w is the filtered variance
SVGF_DEFAULTS = dict(variance=1, min_history=4, sigma_luminance=4.0)


def compile_driver(exe, extra=()):
    """(the flags of temporal_host.compile_driver)"""
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math", "-march=x86-64-v3"] + list(extra) +
                          ["-I" + TH.CSRC, os.path.join(ROOT, "tests", "tools", "svgf_driver.cpp"), "-o", exe])
    return exe


def denoise_run(iterations, flags=1, sigma_color=1.0, sigma_normal=0.1, sigma_depth=0.05):
    return (int(iterations), int(flags), float(sigma_color), float(sigma_normal), float(sigma_depth))


def run_sequence(exe, workdir, frames, runs=(), tag="s", given_variance=None, **params):
    """given_variance: per frame a float32 [h, w] the denoise runs take in place of the temporal variance (needs variance=1).
    -> per frame a dict: image, record [h, w, 4], moments [h, w, 2], variance [h, w], denoised: one [h, w, 4] per entry of `runs` (denoise_run tuples) —
    what vpt_temporal_accumulate and then vpt_denoise from the temporal source compute, call after call, on the host."""
    p = dict(TH.DEFAULTS, **SVGF_DEFAULTS)
    p.update(params)
    h, w = frames[0].depth.shape
    src, dst = os.path.join(str(workdir), tag + ".in"), os.path.join(str(workdir), tag + ".out")
    with open(src, "wb") as f:
        f.write(struct.pack("<8I5f", w, h, len(frames), p["flags"], p["max_history"], 2 if given_variance is not None else p["variance"], p["min_history"], len(runs),
                            p["depth_tolerance"], p["normal_threshold"], p["focus_distance"], p["dof_strength"], p["sigma_luminance"]))
        for r in runs:
            f.write(struct.pack("<2I3f", *r))
        for k, fr in enumerate(frames):
            assert fr.radiance.shape == fr.normal.shape == fr.albedo.shape == (h, w, 4) and fr.depth.shape == fr.inst.shape == (h, w)
            f.write(fr.view_inv.T.tobytes()); f.write(fr.proj_inv.T.tobytes())      # column-major
            f.write(struct.pack("<fI", fr.m, 1 if fr.drop else 0))
            for a in (fr.radiance, fr.normal, fr.albedo, fr.depth, fr.inst):
                f.write(a.tobytes())
            if given_variance is not None:
                f.write(np.ascontiguousarray(given_variance[k], F32).tobytes())
    subprocess.check_call([exe, src, dst])
    raw = np.fromfile(dst, "<f4")
    n = h * w
    per = n * (4 + 4 + 2 + 1 + 4 * len(runs))
    assert raw.size == per * len(frames)
    out = []
    for k in range(len(frames)):
        a = raw[k * per:(k + 1) * per]
        out.append(dict(image=a[:4 * n].reshape(h, w, 4), record=a[4 * n:8 * n].reshape(h, w, 4), moments=a[8 * n:10 * n].reshape(h, w, 2),
                        variance=a[10 * n:11 * n].reshape(h, w), denoised=[a[(11 + 4 * j) * n:(15 + 4 * j) * n].reshape(h, w, 4) for j in range(len(runs))]))
    return out


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)
