"""The node step of a tree in LDS (vulkan-path-tracer_amd/csrc/traverse.hpp load_node / node_entries) reads each axis' near and far planes by the sign
of the ray's direction and sorts nothing per box (slab.hpp box_entry_dir: no min / max per axis).  That may not change a value a box test returns,
so on every case here
  * the image is the oracle's bit for bit, on the whole-path kernel and on the per-bounce pipeline, whose ray statistics agree;
  * samples, closest_rays, shadow_rays, connect_paths of a whole-path context and, from a counting context, nodes_visited, tris_tested,
    shadow_nodes_visited and shadow_tris_tested equal EXPECT.
EXPECT was measured on the PARENT commit's library (the node step before this change: min / max per axis) with measure() below on the same inputs,
on the same MI355X and in the same session as the first run of this test, and written down here; nothing in it comes from the build under test.
Host side of the same claim, float for float: tests/test_box_entry_dir_cpu.py.
Cases: the Cornell box (three nodes, two of them with two unused slots: the PLAIN instantiation); the 16-sheet chain of tests/whole_spill_scene.py
(four nodes, searches that spill the stack); tests/material_scenes.py's compact scene with an environment (seven nodes, the general instantiation and
its sky any-hit searches) and tests/material_sweep.py's three-lobe walls under its lit environment (the same on the Cornell tree); the Cornell box
from beyond kSlabFmaReach scene sizes (camera rays take the subtract form); VPT_FLAG_LOCAL_HITS (the validating instantiations: subtract form
throughout, searches repeated without a triangle)."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RAY_KEYS = ("samples", "closest_rays", "shadow_rays", "connect_paths")
VISIT_KEYS = ("nodes_visited", "tris_tested", "shadow_nodes_visited", "shadow_tris_tested")
PIPELINES_AGREE_ON = ("closest_rays", "shadow_rays", "primary_hits", "primary_survivors", "primary_shadow_rays", "samples", "frames")
EXTENT, REACH = 11.558207513143259, 16.0   # the Cornell box's largest |coordinate|, slab.hpp kSlabFmaReach (tests/test_gpu_far_camera.py)

CASES = ("cornell", "chain", "compact_environment", "sweep_walls_lit", "far_camera", "local_hits")

# measured on the parent commit's library (see above): RAY_KEYS from a whole-path context, VISIT_KEYS from a counting whole-path context
EXPECT = {
    "cornell": dict(samples=9216, closest_rays=15005, shadow_rays=8545, connect_paths=4510, nodes_visited=27978, tris_tested=21680, shadow_nodes_visited=25635, shadow_tris_tested=32473),
    "chain": dict(samples=9216, closest_rays=15923, shadow_rays=9375, connect_paths=1080, nodes_visited=17677, tris_tested=36576, shadow_nodes_visited=24442, shadow_tris_tested=25571),
    "compact_environment": dict(samples=6912, closest_rays=10930, shadow_rays=8761, connect_paths=3104, nodes_visited=26202, tris_tested=16801, shadow_nodes_visited=27874, shadow_tris_tested=27969),
    "sweep_walls_lit": dict(samples=6912, closest_rays=11449, shadow_rays=9014, connect_paths=2416, nodes_visited=19880, tris_tested=14282, shadow_nodes_visited=23527, shadow_tris_tested=28127),
    "far_camera": dict(samples=259200, closest_rays=260131, shadow_rays=1393, connect_paths=747, nodes_visited=261996, tris_tested=3388, shadow_nodes_visited=4179, shadow_tris_tested=5015),
    "local_hits": dict(samples=9216, closest_rays=15005, shadow_rays=8545, connect_paths=4510, nodes_visited=27978, tris_tested=21680, shadow_nodes_visited=25635, shadow_tris_tested=32473),
}


def case_inputs(vpt, scenes, name):
    """(scene, width, height, params, frames)"""
    A = vpt._abi
    if name == "cornell":
        return scenes("cornell_box"), 64, 36, vpt.default_params(max_depth=8), 4
    if name == "chain":
        import whole_spill_scene
        return whole_spill_scene.chain_scene(vpt), 64, 36, vpt.default_params(max_depth=4), 4
    if name == "compact_environment":
        import material_scenes
        sc, info = material_scenes.variant("compact_environment")
        material_scenes.check_preconditions(sc, info)
        assert np.asarray(sc.env).max() > 0.0, "the environment must not be black: the sky searches would not run"
        return sc, 64, 36, vpt.default_params(max_depth=7, sky_azimuth=35.0, sky_altitude=-20.0, sky_intensity=1.5), 3
    if name == "sweep_walls_lit":
        import material_sweep
        sc = material_sweep.walls("three_lobes", "lit")
        assert np.asarray(sc.env).max() > 0.0
        return sc, 64, 36, material_sweep.params(vpt, "lit", depth=8), 3
    if name == "far_camera":
        sc = copy.deepcopy(scenes("cornell_box"))
        sc.view_inverse = np.array(sc.view_inverse, np.float32)
        sc.view_inverse[2, 3] = 1.1 * REACH * EXTENT   # straight back along the viewing axis: the box is ~22 of 270 rows from there
        assert abs(float(sc.view_inverse[2, 3])) > REACH * EXTENT
        return sc, 480, 270, vpt.default_params(max_depth=8), 2
    assert name == "local_hits"
    p = vpt.default_params(max_depth=8)
    p.flags = A.FLAGS_DEFAULT | A.FLAG_LOCAL_HITS
    return scenes("cornell_box"), 64, 36, p, 4


def render(vpt, sc, w, h, p, frames, **kw):
    g = vpt.PathTracer(w, h, frames_in_flight=frames, **kw)
    g.set_scene(sc); g.set_params(p)
    g.render(frames)
    img, st = g.radiance(), g.stats()
    g.close()
    return img, st


def measure(vpt, scenes, name):
    """What EXPECT holds for a case, on the library that is loaded, and the images it came with."""
    sc, w, h, p, frames = case_inputs(vpt, scenes, name)
    A = vpt._abi
    img, st = render(vpt, sc, w, h, p, frames, pipeline=A.PIPELINE_WHOLE)
    cimg, cst = render(vpt, sc, w, h, p, frames, pipeline=A.PIPELINE_WHOLE, count_traversal=True)
    assert st["bvh_node_bytes"] == 128, "the scene should ride in LDS"
    assert st["kernel_launches"]["primary"] == 1 and st["kernel_launches"]["bounce"] == 0
    got = {k: int(st[k]) for k in RAY_KEYS}
    got.update({k: int(cst[k]) for k in VISIT_KEYS})
    return got, img, cimg, st, cst


@pytest.fixture(scope="module")
def oracle_images(vpt, oracle, scenes):
    cache = {}

    def get(name):
        if name not in cache:
            sc, w, h, p, frames = case_inputs(vpt, scenes, name)
            o = oracle.Oracle(sc, w, h)
            o.set_params(p)
            o.render(frames)
            cache[name] = (o.radiance(), o.counters())
            o.close()
        return cache[name]
    return get


@pytest.mark.parametrize("name", CASES)
def test_node_step_keeps_images_and_visit_counts(vpt, scenes, oracle_images, name):
    ref, ctr = oracle_images(name)
    got, img, cimg, st, cst = measure(vpt, scenes, name)
    print(name, got)
    if name == "far_camera":
        lit = int((ref[..., :3].max(axis=2) > 0).sum())
        assert lit >= 200, "the box is hardly in the picture: %d lit pixels" % lit
    assert np.array_equal(img, ref), "%d px differ from the oracle" % int((np.abs(img - ref).max(axis=2) > 0).sum())
    assert np.array_equal(cimg, ref), "the counting context's image differs"
    assert st["closest_rays"] == ctr["closest"]
    for k in RAY_KEYS:
        assert int(cst[k]) == got[k], (k, int(cst[k]), got[k])
    assert got == EXPECT[name], {k: (got[k], EXPECT[name][k]) for k in got if got[k] != EXPECT[name][k]}
    # the per-bounce pipeline: same image, same ray statistics (as tests/test_gpu_whole.py holds them to each other)
    sc, w, h, p, frames = case_inputs(vpt, scenes, name)
    fused, sf = render(vpt, sc, w, h, p, frames, pipeline=vpt._abi.PIPELINE_FUSED)
    assert np.array_equal(fused, img)
    assert sf["kernel_launches"]["bounce"] > 0
    for k in PIPELINES_AGREE_ON:
        assert st[k] == sf[k], (k, st[k], sf[k])
