"""Which LDS-resident scenes can overflow the whole-path kernel's six LDS stack rows (traverse.hpp kWholeStackRows), decided on the host.
tests/tools/stack_bound_host.cpp builds the product tree over a scene's triangles and gives (a) a bound on the stack of any search from the
tree's shape alone — a node with k children pushes at most k - 1 and goes down into the other — and (b) the depth given rays reach, by the
closest-hit loop of traverse.hpp on the host.
  * the Cornell box (the headline workload): bound 4, so its searches never touch the overflow region, with 6 rows as with 14;
  * tests/material_scenes.py's compact scenes: bound 9 — the shape allows an overflow, random rays stay within 6;
  * tests/whole_spill_scene.py's chain: under 3 KB, bound above 6, and rays from the floor towards the light do go above 6 with the triangle
    tests pruning as on the device: the scene tests/test_gpu_whole_refill.py needs to see the spill path of the shorter stack run."""
import os
import re

import numpy as np
import pytest

import material_scenes
import whole_spill_scene as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_SCENE_BYTES = 3072      # scene_prep.hpp fits_lds


def constant(name):
    src = open(os.path.join(ROOT, "vulkan-path-tracer_amd", "csrc", "traverse.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return W.stack_bound_lib(tmp_path_factory.mktemp("stack_bound"))


def random_rays(rng, tris, n):
    lo, hi = tris[:, 0:3].min(axis=0) - 1.0, tris[:, 0:3].max(axis=0) + 1.0
    o = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    return o, d / np.linalg.norm(d, axis=1)[:, None]


def floor_to_light_rays(rng, n):
    """From the chain scene's floor (z = -4.5, half width 6) towards its light (z = 4, half width 3)."""
    o = np.stack([rng.uniform(-6, 6, n), rng.uniform(-6, 6, n), np.full(n, -4.5)], axis=1)
    t = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), np.full(n, 4.0)], axis=1)
    d = t - o
    return o, d / np.linalg.norm(d, axis=1)[:, None]


def test_constants():
    assert constant("kWholeStackRows") == 6 and constant("kStackDepth") == 14 and constant("kStackOverflow") == 82


def test_the_cornell_box_never_overflows_six_rows(lib, scenes, vpt):
    f = W.tree_facts(lib, W.world_triangles(scenes("cornell_box")))
    assert f["nodes"] == 3 and f["lds_bytes"] <= LDS_SCENE_BYTES
    assert f["stack_bound"] == 4 and f["stack_bound"] <= constant("kWholeStackRows")


@pytest.mark.parametrize("variant", ["compact", "compact_environment"])
def test_the_compact_scenes(lib, variant):
    sc, _ = material_scenes.variant(variant)
    tris = W.world_triangles(sc)
    f = W.tree_facts(lib, tris)
    assert f["lds_bytes"] <= LDS_SCENE_BYTES
    assert f["stack_bound"] == 9        # above 6: nothing in the tree's shape keeps a search out of the overflow region
    o, d = random_rays(np.random.default_rng(5), tris, 100000)
    for prune in (0, 1):
        assert W.ray_depths(lib, tris, o, d, prune).max() <= f["stack_bound"]


def test_the_chain_overflows_six_rows(lib, vpt):
    tris = W.world_triangles(W.chain_scene(vpt))
    f = W.tree_facts(lib, tris)
    rows = constant("kWholeStackRows")
    assert f["lds_bytes"] <= LDS_SCENE_BYTES, f
    assert rows < f["stack_bound"] <= constant("kStackDepth") + constant("kStackOverflow")
    rng = np.random.default_rng(6)
    o, d = floor_to_light_rays(rng, 20000)
    sp = W.ray_depths(lib, tris, o, d, 1)
    assert sp.max() > rows and (sp > rows).mean() > 0.01, "rays through the stack should need more than %d entries: max %d" % (rows, sp.max())
    assert sp.max() <= constant("kStackDepth"), "... and stay within the 14 rows of the other kernels, so only the whole-path kernel spills here"
    o2, d2 = random_rays(rng, tris, 50000)
    for oo, dd in ((o, d), (o2, d2)):
        for prune in (0, 1):
            assert W.ray_depths(lib, tris, oo, dd, prune).max() <= f["stack_bound"]
