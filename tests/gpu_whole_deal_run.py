"""The renders of tests/test_gpu_whole_deal.py (not a pytest): whole-path batches whose launch indices are dealt over the camera's screen rectangle of the
scene's box (csrc/whole_deal.hpp), each beside the same context with the rectangle switched off.  The switches, VPT_LAB_WHOLE_CULL and
VPT_LAB_WHOLE_PARTS, and the count of culled samples, vpt_lab_whole_culled, exist in the laboratory library only — so this runs as a process of its own
with VPT_LAB=1, and the test compares what it leaves in the .npz file named on the command line: images by name, everything else as one JSON string."""
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

W, H, FRAMES, DEPTH = 97, 53, 3, 4
KEEP = ("samples", "closest_rays", "shadow_rays", "primary_hits", "primary_survivors", "connect_paths", "kernel_launches", "graph_launches")
cornell = vpt.scenes.Scene.load(os.path.join(ROOT, "tests", "golden", "cornell_box.npz"))
hip = C.CDLL("libamdhip64.so")
images, info = {}, {}


def view(dx=0.0, dy=0.0, z=None):
    v = np.array(cornell.view_inverse, np.float32)
    v[0, 3] += dx; v[1, 3] += dy
    if z is not None:
        v[2, 3] = z
    return v


# far: the rectangle strictly inside the image; corner: it touches the left and the top edge; inside: the camera stands in the box, no rectangle;
# nearer: what the stale-slot batches move to from `far` — a rectangle that is larger and lies elsewhere
# away: the box lies beside what the camera sees — the rectangle is empty
VIEWS = {"far": view(z=40.0), "corner": view(dx=8.0, dy=6.0), "inside": view(z=-5.0), "nearer": view(dx=3.0, dy=2.0, z=25.0), "away": view(dx=100.0)}
SHARDS = ((0, 1), (0, 3), (1, 3), (2, 3))


def image(g, rank, count):
    """The context's image; of a sharded context its own rows, read through vpt_get_shard_device."""
    if count == 1:
        return g.radiance()
    n = g.shard_floats()
    buf, out = C.c_void_p(), np.empty(n, np.float32)
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(n * 4)) == 0
    g.shard_to_device(buf)
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), buf, C.c_size_t(n * 4), 2) == 0   # hipMemcpyDeviceToHost
    hip.hipFree(buf)
    rows = len(range(rank, H, count))
    return out[: rows * W * 4].reshape(rows, W, 4).copy()


def context(cam, rank, count, cull, parts=0):
    kw = dict(shard_rank=rank, shard_count=count) if count > 1 else {}
    g = vpt.PathTracer(W, H, pipeline=A.PIPELINE_WHOLE, frames_in_flight=FRAMES, **kw)
    g.set_scene(cornell); g.set_params(vpt.default_params(max_depth=DEPTH))
    g.set_camera(VIEWS[cam], cornell.projection_inverse(W / H))
    g.lab_set(A.LAB_WHOLE_CULL, cull)
    if parts:
        g.lab_set(A.LAB_WHOLE_PARTS, parts)
    return g


def keep(key, g, rank, count, rects, culled):
    images[key] = image(g, rank, count)
    st = g.stats()
    rec = {k: st[k] for k in KEEP}
    rec.update(rect=rects, culled=culled)
    info[key] = rec


for cam in ("far", "corner", "inside"):
    for rank, count in SHARDS:
        for cull in (1, 0):
            g = context(cam, rank, count, cull)
            rect = g.whole_cull()
            g.render(FRAMES)
            keep("%s_%d_%d_%s" % (cam, rank, count, "on" if cull else "off"), g, rank, count, [rect], [g.lab_whole_culled()])
            g.close()

# stale slots: a batch from far out, then — the accumulation going on — one from nearer, whose rectangle and zero runs lie elsewhere
for rank, count in ((0, 1), (1, 3)):
    for cull in (1, 0):
        g = context("far", rank, count, cull)
        rects, culled = [g.whole_cull()], []
        g.render(FRAMES); culled.append(g.lab_whole_culled())
        g.set_camera(VIEWS["nearer"], cornell.projection_inverse(W / H))
        rects.append(g.whole_cull())
        g.render(FRAMES); culled.append(g.lab_whole_culled())
        keep("stale_%d_%d_%s" % (rank, count, "on" if cull else "off"), g, rank, count, rects, culled)
        g.close()

# parts: the same batch as one launch and as three, each with its own resolve
for parts in (1, 3):
    g = context("far", 0, 1, 1, parts)
    rect = g.whole_cull()
    g.render(FRAMES)
    keep("parts_%d" % parts, g, 0, 1, [rect], [g.lab_whole_culled()])
    g.close()

# No sample inside the rectangle: an empty rectangle, and a shard whose two rows (10 and 42 of 53) lie above and below the far camera's rectangle.  The
# launch deals nothing; it still counts the samples' rays on the device, and the host fills their zero frame sums.  Once through vpt_render, once
# through five vpt_render_async calls, of which the later ones replay the lane's captured graph.
ASYNC_CALLS = 5
for cam, rank, count in (("away", 0, 1), ("far", 10, 32)):
    for cull in (1, 0):
        for mode in ("render", "async"):
            g = context(cam, rank, count, cull)
            rect, culled = g.whole_cull(), []
            if mode == "render":
                g.render(FRAMES); culled.append(g.lab_whole_culled())
            else:
                for _ in range(ASYNC_CALLS):
                    g.render_async(FRAMES)
                g.wait(); culled.append(g.lab_whole_culled())
            keep("none_%s_%d_%d_%s_%s" % (cam, rank, count, mode, "on" if cull else "off"), g, rank, count, [rect], culled)
            g.close()

np.savez(sys.argv[1], info=np.array(json.dumps(info)), views=np.array(json.dumps({k: v.tolist() for k, v in VIEWS.items()})), **images)
print("ok: %d images" % len(images))
