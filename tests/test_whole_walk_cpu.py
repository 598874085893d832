"""An any-hit search of the LDS tree (traverse.hpp trace_occluded_pass) as ONE walk in node-index order, on the host.
Such a search tests every box against a fixed interval, so the nodes and leaves a ray enters do not depend on the order of the visits, and the
answer is the OR over the entered leaves' triangles.  tests/tools/whole_walk_host.cpp holds that definition (inner nodes in index order, one bit
per entered node) next to the stack search, both on slab.hpp's box test and vpt_fp32.h's ray_triangle:
  * numbering: in every tree that rides in LDS every inner child's index is greater than its parent's (the builder's contract, bvh_build.hpp; the
    refit's level order relies on it too) and there are at most 32 nodes — what one ascending pass with a 32-bit mask needs;
  * equivalence: ray by ray the two give the same answer, 0 mismatches in at least 10^5 rays per tree and kind of query, on sets of which at
    least a tenth is occluded and at least a tenth is not.
Trees: the Cornell box, the 16-sheet chain of tests/whole_spill_scene.py, the compact scenes of tests/material_scenes.py; each with the product's
options and collapsed pair-wise.  The whole-path kernel ran its shade step's queries this way, a wave at a time, and was slower for it
(profiles/r12_whole_walk_ab.md: every step runs for the whole wave when one lane needs it); the property and the per-ray node and triangle counts
printed here are what a next attempt starts from."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import material_scenes
import whole_spill_scene as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
TREES = ("cornell_box", "chain", "compact", "compact_environment")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("whole_walk")), "libwhole_walk_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "whole_walk_host.cpp"),
                           os.path.join(ROOT, "vulkan-path-tracer_amd", "csrc", "bvh_build.cpp"), "-o", out])
    L = C.CDLL(out)
    L.ww_tree.restype = None
    L.ww_tree.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.ww_run.restype = None
    L.ww_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def scene_of(vpt, scenes):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = scenes(name) if name == "cornell_box" else W.chain_scene(vpt) if name == "chain" else material_scenes.variant(name)[0]
        return cache[name]
    return get


def tree(L, tris, pairwise):
    out = np.zeros(4, np.int32)
    L.ww_tree(tris.ctypes.data, len(tris), int(pairwise), out.ctypes.data)
    return dict(zip(("nodes", "leaf_tris", "rides_in_lds", "misnumbered"), (int(v) for v in out)))


def run(L, tris, pairwise, form, light, o, d, gid, tmin, tmax):
    o, d, gid = np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32), np.ascontiguousarray(gid, np.uint32)
    n = len(o)
    ins, st, wk, tot = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(2, np.int64)
    L.ww_run(tris.ctypes.data, len(tris), int(pairwise), int(form), int(light), n, o.ctypes.data, d.ctypes.data, gid.ctypes.data, tmin, tmax,
             ins.ctypes.data, st.ctypes.data, wk.ctypes.data, tot.ctypes.data)
    return ins.astype(bool), st.astype(bool), wk.astype(bool), tot


def light_gids(sc):
    """Global ids (instance-major, as tests/whole_spill_scene.py world_triangles numbers them) of the triangles under an emissive material."""
    out, base = [], 0
    for mesh, mat, _ in sc.instances:
        n = len(sc.meshes[mesh][1]) // 3
        if any(sc.materials[mat]["emissive_color"]):
            out += list(range(base, base + n))
        base += n
    return np.array(out, np.uint32)


def points_on(rng, tris, which):
    """A uniform point on each of the triangles tris[which]."""
    a, b = rng.uniform(size=len(which)), rng.uniform(size=len(which))
    flip = a + b > 1
    a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
    return tris[which, 0:3].astype(np.float64) + a[:, None] * tris[which, 3:6] + b[:, None] * tris[which, 6:9]


def scene_box(tris):
    corners = np.concatenate([tris[:, 0:3], tris[:, 0:3] + tris[:, 3:6], tris[:, 0:3] + tris[:, 6:9]]).astype(np.float64)
    return corners.min(axis=0), corners.max(axis=0)


def light_rays(rng, tris, lights, n):
    """Towards a point on a random light triangle: half from a point on a random triangle, moved 1e-2 along the ray (as the shade step's light
    queries start at a surface), half from anywhere within one scene size around the scene's box (a closed room like the Cornell box has nothing
    between its walls and its light: there the occluded rays are the ones that start outside).  Directions are not normalised, as light_visible
    takes them."""
    h = n // 2
    gid = rng.choice(lights, n)
    lo, hi = scene_box(tris)
    p = np.concatenate([points_on(rng, tris, rng.integers(0, len(tris), h)), rng.uniform(lo - (hi - lo).max(), hi + (hi - lo).max(), (n - h, 3))])
    d = points_on(rng, tris, gid) - p     # (gid == index: world_triangles numbers them in order)
    d /= np.maximum(np.linalg.norm(d, axis=1), 1e-9)[:, None]
    return p + 1e-2 * d, d * rng.uniform(0.5, 2.0, n)[:, None], gid


def sky_rays(rng, tris, n):
    """Half from points on the surfaces into random directions (mostly occluded), half from around the scene's box (mostly not)."""
    h = n // 2
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    p = points_on(rng, tris, rng.integers(0, len(tris), h)) + 1e-2 * d[:h]
    lo, hi = scene_box(tris)
    ext = (hi - lo).max()
    return np.concatenate([p, rng.uniform(lo - ext, hi + ext, (n - h, 3))]), d * rng.uniform(0.5, 2.0, n)[:, None]


@pytest.mark.parametrize("pairwise", [False, True])
@pytest.mark.parametrize("name", TREES)
def test_numbering(lib, scene_of, name, pairwise):
    f = tree(lib, W.world_triangles(scene_of(name)), pairwise)
    print(name, "pairwise" if pairwise else "product", f)
    assert f["rides_in_lds"], "every one of these trees is meant to ride in LDS: %r" % (f,)
    assert f["misnumbered"] == 0 and f["nodes"] <= 32, f


def test_the_cornell_box_has_three_nodes(lib, scene_of):
    assert tree(lib, W.world_triangles(scene_of("cornell_box")), False)["nodes"] == 3


@pytest.mark.parametrize("light", [False, True])
@pytest.mark.parametrize("pairwise", [False, True])
@pytest.mark.parametrize("name", TREES)
def test_the_walk_answers_as_the_stack_search(lib, scene_of, name, pairwise, light):
    sc = scene_of(name)
    tris = W.world_triangles(sc)
    rng = np.random.default_rng(12)
    n = 120000
    if light:
        o, d, gid = light_rays(rng, tris, light_gids(sc), n)
        if name == "chain":   # up through the sheets, from the floor (z = -4.5, half width 6) to the light (the scene's last two triangles)
            m = n // 4
            o[:m] = np.stack([rng.uniform(-6, 6, m), rng.uniform(-6, 6, m), np.full(m, -4.5)], axis=1)
            dd = points_on(rng, tris, gid[:m]) - o[:m]
            d[:m] = dd / np.linalg.norm(dd, axis=1)[:, None]
            o[:m] += 1e-2 * d[:m]
        intervals = [(1e-4, 1e6)]                      # light_visible
    else:
        o, d = sky_rays(rng, tris, n)
        gid = np.zeros(n, np.uint32)
        intervals = [(1e-4, 1e6), (1e-5, 1000.0)]      # sky_visible with and without VPT_FLAG_RAY_QUERIES (the latter on normalised directions)
    for tmin, tmax in intervals:
        dd = d / np.linalg.norm(d, axis=1)[:, None] if tmax == 1000.0 else d
        for form in (0, 1):
            ins, st, wk, tot = run(lib, tris, pairwise, form, light, o, dd, gid, tmin, tmax)
            k = int(ins.sum())
            occluded = float(st[ins].mean())
            print("%s %s light=%d form=%d (%g, %g): %d rays in the search, %.1f %% occluded, %.2f nodes and %.2f triangles per ray by the walk"
                  % (name, "pairwise" if pairwise else "product", light, form, tmin, tmax, k, 100 * occluded, tot[0] / k, tot[1] / k))
            assert k >= 100000, "only %d rays reached the search" % k
            assert 0.1 <= occluded <= 0.9, "the set should be at least a tenth occluded and at least a tenth not: %.3f" % occluded
            assert int((st != wk).sum()) == 0, "%d of %d rays differ" % (int((st != wk).sum()), k)
            assert not st[~ins].any() and not wk[~ins].any()


def test_cornell_light_rays_from_the_walls(lib, scene_of):
    """2000 waves of 40 light queries: origins on the walls (every triangle that is no light), 1e-2 along the ray, aimed at the emissive quad."""
    sc = scene_of("cornell_box")
    tris = W.world_triangles(sc)
    lights = light_gids(sc)
    rng = np.random.default_rng(3)
    n = 80000
    walls = np.setdiff1d(np.arange(len(tris)), lights)
    src, gid = rng.choice(walls, n), rng.choice(lights, n)
    p, q = points_on(rng, tris, src), points_on(rng, tris, gid)
    d = q - p
    d /= np.linalg.norm(d, axis=1)[:, None]
    ins, st, wk, tot = run(lib, tris, False, 0, True, p + 1e-2 * d, d, gid, 1e-4, 1e6)
    print("%d of %d in the search, %.1f %% occluded, %.2f nodes and %.2f triangles per ray" % (ins.sum(), n, 100 * st[ins].mean(), tot[0] / ins.sum(), tot[1] / ins.sum()))
    assert ins.sum() > n // 2
    assert int((st != wk).sum()) == 0
