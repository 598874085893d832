"""The renders of tests/test_gpu_whole_cull.py (not a pytest): every case with the camera cull of the whole-path kernel (camera_cull.hpp) on and off.
The switch, VPT_LAB_WHOLE_CULL, and the count of culled samples, vpt_lab_whole_culled, exist in the laboratory library only — so this runs as a
process of its own with VPT_LAB=1, and the test compares what it leaves in the .npz file named on the command line: images by name, everything else
as one JSON string.  Per case and switch: an uncounted and a counting context (vpt_config.count_traversal)."""
import copy
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
vpt = importlib.import_module("vulkan-path-tracer_amd")
A = vpt._abi
assert vpt.has_lab(), "run with VPT_LAB=1"

KEEP = ("samples", "closest_rays", "shadow_rays", "primary_hits", "connect_paths", "nodes_visited", "tris_tested", "shadow_nodes_visited", "shadow_tris_tested", "kernel_launches")
cornell = vpt.scenes.Scene.load(os.path.join(ROOT, "tests", "golden", "cornell_box.npz"))
hip = C.CDLL("libamdhip64.so")
images, info = {}, {}


def shard_image(g, w, h, rank, count):
    n = g.shard_floats()
    buf, out = C.c_void_p(), np.empty(n, np.float32)
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(n * 4)) == 0
    g.shard_to_device(buf)
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), buf, C.c_size_t(n * 4), 2) == 0   # hipMemcpyDeviceToHost
    hip.hipFree(buf)
    rows = len(range(rank, h, count))
    return out[: rows * w * 4].reshape(rows, w, 4).copy()


def moved_view(z=None, roll_deg=None):
    v = np.array(cornell.view_inverse, np.float32)
    if z is not None:
        v[2, 3] = z
    if roll_deg is not None:
        a = np.radians(roll_deg)
        r = np.eye(4, dtype=np.float32)
        r[0, 0], r[0, 1], r[1, 0], r[1, 1] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
        v = (v @ r).astype(np.float32)   # the camera turned about its own viewing axis
    return v


def with_view(view):
    sc = copy.deepcopy(cornell)
    sc.view_inverse = view
    return sc


def with_env(value):
    sc = copy.deepcopy(cornell)
    sc.env = np.full((4, 8, 4), value, np.float32)
    return sc


def light_instance(sc):
    return next(i for i, (_, m, _) in enumerate(sc.instances) if max(sc.materials[m]["emissive_color"][:3]) > 0.0)


def params(**kw):
    flags = kw.pop("flags", A.FLAGS_DEFAULT)
    p = vpt.default_params(max_depth=6, **kw)
    p.flags = flags
    return p


# name: scene, width, height, parameters, dispatches per batch, context arguments, what happens between the first batch and the second (None: one batch)
CASES = {
    "cornell_192": (cornell, 192, 108, params(), 3, {}, None),                    # 64-sample tiles straddle rows and frames
    "cornell_200": (cornell, 200, 120, params(), 3, {}, None),
    "far_camera": (with_view(moved_view(z=1.1 * 16.0 * 11.558207513143259)), 480, 270, params(), 2, {}, None),   # tests/test_gpu_lds_node_step.py's scene
    # the same camera with focus distance 0: camera_ray's focus point, 0.001 ahead of an origin 203 units out, is rounded to the origin's ulp and
    # the rays are off by pixels — no rectangle (camera_cull.hpp "The roundings")
    "focus_zero": (with_view(moved_view(z=1.1 * 16.0 * 11.558207513143259)), 480, 270, params(focus_distance=0.0), 2, {}, None),
    "inside": (with_view(moved_view(z=-5.0)), 96, 54, params(), 2, {}, None),
    "rolled": (with_view(moved_view(roll_deg=30.0)), 192, 108, params(), 2, {}, None),
    "dof": (cornell, 96, 54, params(dof_strength=0.5, focus_distance=18.0), 2, {}, None),
    "shard": (cornell, 192, 108, params(), 3, dict(shard_rank=1, shard_count=2), None),
    "split": (cornell, 100, 75, params(screen_chunk_count=2), 8, {}, None),         # two passes over the four chunks
    "furnace": (cornell, 96, 54, params(flags=A.FLAGS_DEFAULT | A.FLAG_FURNACE), 2, {}, None),
    "env_hidden": (with_env(0.5), 96, 54, params(flags=A.FLAGS_DEFAULT & ~A.FLAG_SHOW_ENV_DIRECTLY), 2, {}, None),   # the general instantiation
    "env_shown": (with_env(0.5), 96, 54, params(), 2, {}, None),
    "moved_light": (cornell, 192, 108, params(), 2, {}, "move"),
    "set_camera": (cornell, 192, 108, params(), 2, {}, "camera"),
}


def run(name, cull, count):
    sc, w, h, p, frames, kw, then = CASES[name]
    g = vpt.PathTracer(w, h, pipeline=A.PIPELINE_WHOLE, frames_in_flight=frames, count_traversal=count, **kw)
    g.set_scene(sc); g.set_params(p)
    g.lab_set(A.LAB_WHOLE_CULL, cull)
    rec = {"rect": [g.whole_cull()], "culled": []}
    g.render(frames)
    rec["culled"].append(g.lab_whole_culled())
    if then == "move":   # the light goes 11 units to the right, out of the box and into what was background
        i = light_instance(sc)
        m = np.array(sc.instances[i][2], np.float32)
        m[0, 3] += 11.0
        g.set_instance_transforms(i, [m])
    if then == "camera":
        g.set_camera(moved_view(z=40.0), sc.projection_inverse(w / h))
    if then:
        rec["rect"].append(g.whole_cull())
        g.render(frames)
        rec["culled"].append(g.lab_whole_culled())
    key = "%s_%s%s" % (name, "on" if cull else "off", "_counted" if count else "")
    images[key] = shard_image(g, w, h, kw["shard_rank"], kw["shard_count"]) if kw else g.radiance()
    st = g.stats()
    rec.update({k: st[k] for k in KEEP})
    info[key] = rec
    g.close()


for name in CASES:
    for cull in (1, 0):
        for count in (False, True):
            run(name, cull, count)

np.savez(sys.argv[1], info=np.array(json.dumps(info)), **images)
print("ok: %d images" % len(images))
