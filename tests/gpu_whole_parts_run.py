"""The renders of tests/test_gpu_whole_parts.py (not a pytest): whole-path batches forced into parts through VPT_LAB_WHOLE_PARTS, which only the
laboratory library has — so this runs as a process of its own with VPT_LAB=1, and the test compares what it leaves in the .npz file named on
the command line: images by name, the statistics as one JSON string."""
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

SHAPES = {"ragged": (50, 37, {}), "even": (64, 48, {}), "shard": (64, 48, dict(shard_rank=1, shard_count=2))}
PARTS = (1, 2, 3, 7, 8)
FRAMES, DEPTH = 7, 8
KEEP = ("samples", "frames", "closest_rays", "shadow_rays", "primary_hits", "connect_paths", "nodes_visited", "tris_tested", "shadow_nodes_visited", "shadow_tris_tested",
        "kernel_launches", "kernel_ms", "graph_launches")

scene = vpt.scenes.Scene.load(os.path.join(ROOT, "tests", "golden", "cornell_box.npz"))
params = vpt.default_params(max_depth=DEPTH)
hip = C.CDLL("libamdhip64.so")
images, stats = {}, {}


def context(shape, parts, **kw):
    w, h, shard = SHAPES[shape]
    g = vpt.PathTracer(w, h, pipeline=A.PIPELINE_WHOLE, frames_in_flight=FRAMES, **shard, **kw)
    g.set_scene(scene); g.set_params(params)
    g.lab_set(A.LAB_WHOLE_PARTS, parts)
    return g


def image(g, shape):
    """The context's image; of a sharded context its own rows, read through vpt_get_shard_device."""
    w, h, shard = SHAPES[shape]
    if not shard:
        return g.radiance()
    n = g.shard_floats()
    buf, out = C.c_void_p(), np.empty(n, np.float32)
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(n * 4)) == 0
    g.shard_to_device(buf)
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), buf, C.c_size_t(n * 4), 2) == 0   # hipMemcpyDeviceToHost
    hip.hipFree(buf)
    rows = len(range(shard["shard_rank"], h, shard["shard_count"]))
    return out[: rows * w * 4].reshape(rows, w, 4).copy()


def keep(name, g, shape):
    images[name] = image(g, shape)
    st = g.stats()
    stats[name] = {k: st[k] for k in KEEP}


# a batch of 7 frames in 1, 2, 3, 7 and 8 (clamped to 7) parts, then a second one on the same context: frame_base > 0 in every part
for shape in SHAPES:
    for parts in PARTS:
        g = context(shape, parts)
        g.render(FRAMES)
        keep("%s_p%d_first" % (shape, parts), g, shape)
        g.render(FRAMES)
        keep("%s_p%d_second" % (shape, parts), g, shape)
        g.close()

# vpt_render_async: a 7-frame batch in 3 parts behind a post-process, then three 1-frame batches on the lanes; against the blocking unsplit context
g = context("even", 3)
done, _ = g.render_async(FRAMES)
g.postprocess_device()
g.wait()
images["async_out8"] = g.output_to_host()
keep("async_batch", g, "even")
for _ in range(3):
    g.render_async(1)
    g.postprocess_device()
g.wait()
keep("async_lanes", g, "even")
g.close()
g = context("even", 1)
g.render(FRAMES)
images["blocking_out8"] = g.postprocess()
keep("blocking_batch", g, "even")
for _ in range(3):
    g.render(1)
keep("blocking_lanes", g, "even")
g.close()

# kernels timed and visits counted: the same schedule, the same figures
for parts in (1, 3):
    g = context("ragged", parts, profile=True, count_traversal=True)
    g.render(FRAMES)
    keep("counted_p%d" % parts, g, "ragged")
    g.close()

np.savez(sys.argv[1], stats=np.array(json.dumps(stats)), **images)
print("ok: %d images" % len(images))
