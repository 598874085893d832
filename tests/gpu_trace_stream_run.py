"""The launches of tests/test_gpu_trace_stream.py (not a pytest): the ray sets of tests/trace_ray_sets.py through the ray-stream traversal kernels of
the stream pipelines — k_trace_vote by vpt_lab_trace (VPT_TRACE_VOTE with the default vote parameter: the product instantiation; with visits the
counting one; under VPT_FLAG_LOCAL_HITS the validating ones) and k_trace_shadow by vpt_lab_trace_shadow.  Those entry points exist in the laboratory
library only, so this runs as a process of its own with VPT_LAB=1 and leaves, in the .npz named on the command line, every result by name and
everything else as one JSON string; the test compares them with the oracle's brute force.  Second argument: the device's compute units, which
size the one launch that goes beyond the static part of the grid.  Nothing here knows a reference: where a launch is compared with another launch
of this process (the same rays in another order, the counting instantiation beside the uncounted one) the file records `same`, bit for bit.  A
launch the library refuses — one that wrote beyond the last ray of its set, say — ends its group of launches, whose error is recorded under its name."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
vpt = importlib.import_module("vulkan-path-tracer_amd")
A = vpt._abi
assert vpt.has_lab(), "run with VPT_LAB=1"
import refit_moves as RM
import trace_ray_sets as T

VOTE, PARAM = 1, 256 + 16   # VPT_TRACE_VOTE, vote.hpp kVoteParamDefault: launch_trace falls through to the product's instantiations
arrays, info = {}, {"errors": {}}


def group(key, fn):
    """One group of launches: an error of the library ends it, is recorded, and the next group runs."""
    try:
        fn()
    except RuntimeError as e:
        info["errors"][key] = str(e)
        print("FAILED", key, e)


def check(g, rc, what):
    if rc != 0:
        raise RuntimeError("%s: %d %s" % (what, rc, g.lib.vpt_last_error(g.ctx).decode()))


def context(sc, **kw):
    g = vpt.PathTracer(8, 8, **kw)
    g.set_scene(sc)
    return g


def set_rays(g, rays):
    rays = np.ascontiguousarray(rays, np.float32)
    check(g, g.lib.vpt_lab_set_rays(g.ctx, rays.ctypes.data, len(rays)), "vpt_lab_set_rays")
    g._n = len(rays)


def set_holes(g, mask):
    check(g, g.lib.vpt_lab_set_holes(g.ctx, mask.ctypes.data if mask is not None else None), "vpt_lab_set_holes")


def set_strict(g, on):
    p = vpt.default_params()
    if on:
        p.flags |= A.FLAG_LOCAL_HITS
    g.set_params(p)


def trace(g, any_hit=False, order=None, visits=False):
    hits = np.zeros(g._n, vpt.HIT_DTYPE)
    ms = C.c_float(0)
    v = (C.c_uint64 * 2)() if visits else None
    check(g, g.lib.vpt_lab_trace(g.ctx, VOTE, int(any_hit), order.ctypes.data if order is not None else None, PARAM, 1, hits.ctypes.data, C.byref(ms), v), "vpt_lab_trace")
    return (hits, [int(v[0]), int(v[1])]) if visits else hits


def shadow(g, light, ray_queries=1, expect=None, media=None, hole=None, visits=False):
    vis = np.zeros(g._n, np.uint8)
    v = (C.c_uint64 * 2)() if visits else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    check(g, g.lib.vpt_lab_trace_shadow(g.ctx, int(light), int(ray_queries), ptr(expect), ptr(media), ptr(hole), vis.ctypes.data, v), "vpt_lab_trace_shadow")
    return (vis, [int(v[0]), int(v[1])]) if visits else vis


def same(a, b):
    return a.tobytes() == b.tobytes()


def four_instantiations(g, key, run):
    """run(visits) under both hit rules: the uncounted results by name, the counting ones as `same`, and their visits."""
    rec = {}
    for rule in ("default", "strict"):
        set_strict(g, rule == "strict")
        plain = run(False)
        counted, visits = run(True)
        arrays["%s_%s" % (key, rule)] = plain
        rec[rule] = {"counting_same": same(plain, counted), "visits": visits}
    set_strict(g, False)
    return rec


# ---- k_trace_vote: every set, four instantiations; the product one again over the hole mask; any-hit on the degenerate and the far sets
def vote_set(name):
    sc, rays = T.load(vpt, name)
    g = context(sc)
    spills_before = g.stats()["stack_spills"]
    set_rays(g, rays)
    rec = four_instantiations(g, "vote_" + name, lambda visits: trace(g, visits=visits))
    rec["stack_spills"] = [spills_before, g.stats()["stack_spills"]]
    info["vote_" + name] = rec
    if name in ("axis_aligned", "far_30", "far_1000"):
        arrays["any_" + name] = trace(g, any_hit=True)["t"]
    set_holes(g, T.hole_mask(len(rays)))
    arrays["vote_%s_holes" % name] = trace(g)
    g.close()


for name in T.SETS:
    group("vote_" + name, lambda: vote_set(name))

# ---- k_trace_vote's scheduler: sizes around a wave and a block and two beyond the grid's static part (the second ends inside a cursor chunk), three visiting orders each
cus = int(sys.argv[2])
BIG = T.beyond_static_sizes(cus)
big_n = BIG[1]
sc_glass, _ = T.load(vpt, "random_glass")
big = T.random_rays(big_n, 5, 8.0)
g = context(sc_glass)


def schedule(n):
    set_rays(g, big[:n])
    rec = {}
    first = None
    for oname, order in T.orders(n).items():
        plain = trace(g, order=order)
        counted, visits = trace(g, order=order, visits=True)
        first = plain if first is None else first
        rec[oname] = {"same_as_identity": same(plain, first), "counting_same": same(counted, first), "visits": visits}
    arrays["sched_%d" % n] = first
    if n >= 4097:   # the hole mask as TraceArgs::valid, and folded into a visiting order
        set_holes(g, T.hole_mask(n))
        holes = trace(g)
        arrays["sched_%d_holes" % n] = holes
        rec["holes_reversed_same"] = same(trace(g, order=T.orders(n)["reversed"]), holes)
    info["sched_%d" % n] = rec


def sky_big(n):   # the sky form of the shadow kernel beyond its static part
    set_holes(g, None)
    set_rays(g, big[:n])
    arrays["sky_n%d" % n] = shadow(g, False)
    arrays["sky_n%d_holes" % n] = shadow(g, False, hole=T.hole_mask(n))


for n in T.SCHEDULE_SIZES + BIG:
    group("sched_%d" % n, lambda: schedule(n))
for n in BIG:
    group("sky_n%d" % n, lambda: sky_big(n))
g.close()

# ---- other trees: spatial splits (leaves share triangles), and boxes loosened by a refit
def sbvh(name):
    sc, rays = T.load(vpt, name)
    g = context(sc, build_flags=1)   # VPT_BUILD_SBVH
    set_rays(g, rays)
    arrays["sbvh_" + name] = trace(g)
    info["sbvh_" + name] = {"build_flags": g.stats()["build_flags"], "bvh_triangles": g.stats()["bvh_triangles"]}
    g.close()


def moved_glass():
    sc, rays = T.load(vpt, "random_glass")
    moved = RM.moved_matrices(sc, RM.GLASS_LAMP_AND_SPHERE)
    g = context(sc)
    g.set_instance_transforms(min(moved), [moved[i] for i in sorted(moved)])
    set_rays(g, rays)
    arrays["moved_glass"] = trace(g)
    g.close()


# ---- k_trace_shadow, sky form: the degenerate, far and scaled sets (the kernel's own window), four instantiations, holes; two of them without ray queries
def sky(name):
    sc, rays = T.load(vpt, name)
    g = context(sc)
    set_rays(g, rays)
    info["sky_" + name] = four_instantiations(g, "sky_" + name, lambda visits: shadow(g, False, visits=visits))
    arrays["sky_%s_holes" % name] = shadow(g, False, hole=T.hole_mask(len(rays)))
    if name in T.SKY_SETS_NO_RAY_QUERIES:
        info["sky_%s_norq" % name] = four_instantiations(g, "sky_%s_norq" % name, lambda visits: shadow(g, False, ray_queries=0, visits=visits))
    g.close()


# ---- k_trace_shadow, light form: aimed at the emissive triangles with the right and a wrong expectation, media-flagged rays past the light
def light(name):
    rays, expect, media = T.light_rays(vpt, name)
    g = context(T.light_scene(vpt, name))
    set_rays(g, rays)
    info["light_" + name] = four_instantiations(g, "light_" + name, lambda visits: shadow(g, True, expect=expect, media=media, visits=visits))
    arrays["light_%s_holes" % name] = shadow(g, True, expect=expect, media=media, hole=T.hole_mask(len(rays)))
    g.close()


def light_size(n):
    rays, expect, media = T.light_rays(vpt, "cornell_box_glass")
    idx = np.arange(n) % len(rays)   # (beyond the set's length: the set over and over)
    g = context(T.light_scene(vpt, "cornell_box_glass"))
    set_rays(g, rays[idx])
    e, m = np.ascontiguousarray(expect[idx]), np.ascontiguousarray(media[idx])
    arrays["light_n%d" % n] = shadow(g, True, expect=e, media=m)
    arrays["light_n%d_holes" % n] = shadow(g, True, expect=e, media=m, hole=T.hole_mask(n))
    g.close()


for name in ("random_glass", "random_viking"):
    group("sbvh_" + name, lambda: sbvh(name))
group("moved_glass", moved_glass)
for name in T.SKY_SETS:
    group("sky_" + name, lambda: sky(name))
for name in T.LIGHT_SCENES:
    group("light_" + name, lambda: light(name))
for n in T.SHADOW_SIZES + BIG:
    group("light_n%d" % n, lambda: light_size(n))

info["compute_units"] = cus
np.savez(sys.argv[1], info=np.array(json.dumps(info)), **arrays)
print("ok: %d results, %d groups refused" % (len(arrays), len(info["errors"])))
