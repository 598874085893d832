"""What the tests of SVGF's spatial variance estimate share: the host compile of csrc/svgf_spatial.hpp inside the viewport loop
(tests/tools/svgf_spatial_driver.cpp) built and run on a sequence of temporal_host.Frame.  The output has svgf_host.run_sequence's shape."""
import os
import struct
import subprocess

import numpy as np

import svgf_host as SH
import temporal_host as TH

ROOT = TH.ROOT
F32 = np.float32
SPATIAL_DEFAULTS = dict(mode=1, radius=3, sigma_normal=0.1, sigma_depth=0.05, min_weight=4.0)     # include/vpt.h's defaults, but on


def compile_driver(exe, extra=()):
    """(the flags of svgf_host.compile_driver)"""
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math", "-march=x86-64-v3"] + list(extra) +
                          ["-I" + TH.CSRC, os.path.join(ROOT, "tests", "tools", "svgf_spatial_driver.cpp"), "-o", exe])
    return exe


def run_sequence(exe, workdir, frames, runs=(), tag="sp", **params):
    """-> per frame a dict: image, record [h, w, 4], moments [h, w, 2], variance [h, w] (after the spatial pass), denoised: one [h, w, 4] per entry of `runs`
    (svgf_host.denoise_run tuples) — what vpt_temporal_accumulate with both options on and then vpt_denoise from the temporal source compute, on the host."""
    p = dict(TH.DEFAULTS, **SH.SVGF_DEFAULTS)
    p.update(SPATIAL_DEFAULTS)
    p.update(params)
    h, w = frames[0].depth.shape
    src, dst = os.path.join(str(workdir), tag + ".in"), os.path.join(str(workdir), tag + ".out")
    with open(src, "wb") as f:
        f.write(struct.pack("<9I8f", w, h, len(frames), p["flags"], p["max_history"], p["min_history"], len(runs), p["mode"], p["radius"],
                            p["depth_tolerance"], p["normal_threshold"], p["focus_distance"], p["dof_strength"], p["sigma_luminance"],
                            p["sigma_normal"], p["sigma_depth"], p["min_weight"]))
        for r in runs:
            f.write(struct.pack("<2I3f", *r))
        for fr in frames:
            assert fr.radiance.shape == fr.normal.shape == fr.albedo.shape == (h, w, 4) and fr.depth.shape == fr.inst.shape == (h, w)
            f.write(fr.view_inv.T.tobytes()); f.write(fr.proj_inv.T.tobytes())      # column-major
            f.write(struct.pack("<fI", fr.m, 1 if fr.drop else 0))
            for a in (fr.radiance, fr.normal, fr.albedo, fr.depth, fr.inst):
                f.write(a.tobytes())
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


bits = SH.bits
