"""Density-grid A/B (not a pytest): the same thresholded cloud (tests/test_oracle_volumes.py cloud_grid at N^3 voxels, N = 256 by default, everything
below a quarter of its maximum set to 0) as a DENSE grid (vpt_add_density_grid) and as 8x8x8 BRICKS (vpt_add_density_bricks), rendered at 1920x1080,
depth 8, in the atrium (a BVH in memory: the media stages on the streams) and in the Cornell box (a tree in LDS: the fused media kernel).  Images
must be bit-identical; prints Msamples/s and vpt_density_grid_info.device_bytes of both.  FRAMES (default 16) frames in flight.

    python tests/tools/density_bricks_ab.py [--n 256] [--library OTHER.so --dense-only] [--parent-json FILE] > density_bricks_ab.json

--library loads another build of the library (the parent commit's, which has no brick entry points: --dense-only) so that its dense figure can
be put beside this build's: run it first, then hand its output to the second run with --parent-json.
"""
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
vpt = importlib.import_module("vulkan-path-tracer_amd")
from test_oracle_volumes import cloud_grid   # noqa: E402


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def load_other(path):
    """Another build of the library behind the package's shim: the prototypes it has are bound, the ones it lacks are left out."""
    lib = C.CDLL(path)
    lib.has_lab = False
    for name, (res, args) in vpt._abi.PROTOTYPES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype = res; fn.argtypes = args
    vpt._LIB = lib


def scenes_and_boxes():
    atrium = vpt.scenes.atrium()
    lo = np.min([np.asarray(xf, np.float64)[:3, 3] for _, _, xf in atrium.instances], 0) - 6.0
    hi = np.max([np.asarray(xf, np.float64)[:3, 3] for _, _, xf in atrium.instances], 0) + 6.0
    cornell = vpt.scenes.Scene.load(os.path.join(ROOT, "tests", "golden", "cornell_box.npz"))
    cornell.env = vpt.scenes.sun_sky_env(64, 32, seed=5, sun_peak=200.0)
    return [("atrium", atrium, tuple(lo), tuple(hi), 0.6), ("cornell_box", cornell, (-4.0, -9.0, -4.0), (4.0, -2.0, 4.0), 1.6)]


def main():
    n = int(arg("--n", "256"))
    F = int(os.environ.get("FRAMES", "16"))
    dense_only = "--dense-only" in sys.argv
    if arg("--library"):
        load_other(arg("--library"))
    parent = json.load(open(arg("--parent-json"))) if arg("--parent-json") else None
    grid = cloud_grid((n, n, n), seed=2)
    grid[grid < grid.max() / np.float32(4.0)] = 0.0
    dims, coords, values = vpt.bricks_of(grid)
    cells = int(np.prod([-(-d // 8) for d in dims]))
    res = {"voxels": int(grid.size), "brick_cells": cells, "bricks": int(len(coords)), "active_voxel_fraction": round(float((grid != 0).mean()), 4),
           "frames_in_flight": F, "library": arg("--library", "this build"), "scenes": []}
    for name, sc, lo, hi, density in scenes_and_boxes():
        row, imgs = {"scene": name}, []
        for kind in ("dense",) if dense_only else ("dense", "bricked"):
            g = vpt.PathTracer(1920, 1080, frames_in_flight=F)
            g.set_scene(sc); g.set_params(vpt.default_params(max_depth=8, max_samples=1 << 30))
            t = time.time()
            gi = g.add_density_grid(grid) if kind == "dense" else g.add_density_bricks(dims, coords, values)
            add_s = time.time() - t
            g.set_volumes([vpt.volume(corner_min=lo, corner_max=hi, color=(0.9, 0.9, 0.92), density=density, anisotropy=0.4, density_data_index=gi)])
            g.render(F); g.reset_stats()
            t = time.time(); g.render(F); dt = time.time() - t
            st = g.stats(); imgs.append(g.radiance())
            row[kind] = {"msamples_per_s": round(st["samples"] / dt / 1e6, 1), "add_seconds": round(add_s, 3),
                         "launches": {k: v for k, v in st["kernel_launches"].items() if v > 0}}
            if not dense_only:
                row[kind]["device_bytes"] = int(g.density_grid_info(gi)["device_bytes"])
            g.close()
            print(json.dumps({name: {kind: row[kind]}}), file=sys.stderr)
        if not dense_only:
            row["identical_images"] = bool(np.array_equal(imgs[0], imgs[1]))
            row["bricked_over_dense"] = round(row["bricked"]["msamples_per_s"] / row["dense"]["msamples_per_s"], 3)
            row["parent_dense_msamples_per_s"] = next((r["dense"]["msamples_per_s"] for r in parent["scenes"] if r["scene"] == name), None) if parent else None
        res["scenes"].append(row)
    print(json.dumps(res, indent=1))
    assert dense_only or all(r["identical_images"] for r in res["scenes"])


if __name__ == "__main__":
    main()
