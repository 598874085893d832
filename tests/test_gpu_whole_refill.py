"""The whole-path kernel (kernels_whole.hip k_whole) generates its camera rays a full tile at a time into a wave-private buffer and hands
them to free lanes from there (vulkan-path-tracer_amd/csrc/whole_refill.hpp; the host side: tests/test_whole_refill_cpu.py).  Which lane
runs which sample cannot matter — seeds come from (pixel, frame), results go to the sample's own slot — so images and ray counts must be the
oracle's, bit for bit, at every shape of batch the tile cursor and the buffer see: ragged rows, less than a tile, row shards, split screens,
depth of field, one bounce and eight, replayed 1-frame graphs, every instantiation, a tree that is deeper than the Cornell box's
three nodes, and one whose searches overflow the kernel's shorter LDS stack into the per-thread region in memory."""
import copy
import ctypes as C

import numpy as np
import pytest

import material_scenes

pytestmark = pytest.mark.gpu


def oracle_image(oracle, sc, w, h, params, frames):
    o = oracle.Oracle(sc, w, h)
    o.set_params(params)
    o.render(frames)
    ref, ctr = o.radiance(), o.counters()
    o.close()
    return ref, ctr


RAY_STATS = ("samples", "frames", "closest_rays", "shadow_rays", "primary_hits", "primary_survivors", "primary_shadow_rays")


def gpu_image(vpt, sc, w, h, params, batches, pipeline=None, **kw):
    g = vpt.PathTracer(w, h, pipeline=vpt._abi.PIPELINE_WHOLE if pipeline is None else pipeline, **kw)
    g.set_scene(sc); g.set_params(params)
    for n in batches:
        g.render(n)
    img, st = g.radiance(), g.stats()
    g.close()
    return img, st


def check(vpt, oracle, sc, w, h, params, batches, **kw):
    frames = sum(batches)
    ref, ctr = oracle_image(oracle, sc, w, h, params, frames)
    img, st = gpu_image(vpt, sc, w, h, params, batches, **kw)
    assert np.array_equal(img, ref), "%d px differ" % int((np.abs(img - ref).max(axis=2) > 0).sum())
    assert st["closest_rays"] == ctr["closest"], (st["closest_rays"], ctr["closest"])
    assert st["kernel_launches"]["primary"] == len(batches) and st["kernel_launches"]["bounce"] == 0
    fused, sf = gpu_image(vpt, sc, w, h, params, batches, pipeline=vpt._abi.PIPELINE_FUSED, **kw)   # the per-bounce kernels: the same image, the same ray counts
    assert np.array_equal(img, fused)
    for k in RAY_STATS:
        assert st[k] == sf[k], (k, st[k], sf[k])
    return st


def glass(vpt, scenes):
    """The Cornell box's 12 triangles with a glass wall, a rough glass floor holding a medium, and a sky: the general (non-PLAIN) instantiation."""
    sc = copy.deepcopy(scenes("cornell_box"))
    sc.materials[0].update(transmission=1.0, roughness=0.05, ior=1.5, base_color=(1, 1, 1))
    sc.materials[2].update(transmission=1.0, roughness=0.3, ior=1.33, medium_density=0.6, medium_anisotropy=0.3, medium_color=(0.9, 0.5, 0.4))
    sc.env = vpt.scenes.sun_sky_env(64, 32, seed=9, sun_peak=100.0)
    return sc


@pytest.mark.parametrize("depth", [1, 8])
@pytest.mark.parametrize("w,h", [(100, 37), (65, 3), (7, 5), (64, 2)])
def test_ragged_rows_and_images_below_one_tile(vpt, oracle, scenes, w, h, depth):
    """100 and 65 are no multiples of 64 (the last tile of every batch is ragged); 7 x 5 is less than one tile per frame, so a
    multi-frame batch's tiles straddle frames and most waves of the grid never get one; 64 x 2 is whole tiles only."""
    check(vpt, oracle, scenes("cornell_box"), w, h, vpt.default_params(max_depth=depth), [3, 2], frames_in_flight=3)


def test_row_shards(vpt, scenes):
    """shard_count 8: a shard's launch indices cover every eighth row; assembled, the shards are the unsharded image."""
    sc, w, h, frames, G = scenes("cornell_box"), 100, 37, 3, 8      # 37 rows over 8 shards: ragged
    p = vpt.default_params(max_depth=8)
    whole, st_whole = gpu_image(vpt, sc, w, h, p, [frames])
    parts = []
    for r in range(G):
        g = vpt.PathTracer(w, h, shard_rank=r, shard_count=G, pipeline=vpt._abi.PIPELINE_WHOLE)
        g.set_scene(sc); g.set_params(p); g.render(frames)
        parts.append(g)
    stats = [g.stats() for g in parts]
    for k in ("samples", "closest_rays", "shadow_rays", "primary_hits", "primary_survivors", "primary_shadow_rays"):
        assert sum(s[k] for s in stats) == st_whole[k], k
    hip = C.CDLL("libamdhip64.so")
    n = parts[0].shard_floats()
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), n * 4 * G) == 0
    for r, g in enumerate(parts):
        g.shard_to_device(C.c_void_p(buf.value + r * n * 4))
    parts[0].assemble_shards(buf, G)
    assert np.array_equal(parts[0].radiance(), whole)
    hip.hipFree(buf)
    for g in parts:
        g.close()


@pytest.mark.parametrize("split", [2, 3])
def test_split_screens(vpt, oracle, scenes, split):
    """ScreenSplitCount > 1: a dispatch covers one chunk of the pixels, and a batch's launch indices run through its dispatches' chunks."""
    p = vpt.default_params(max_depth=8, screen_chunk_count=split)
    check(vpt, oracle, scenes("cornell_box"), 100, 37, p, [split * split, split * split + 1], frames_in_flight=split * split + 1)


def test_depth_of_field(vpt, oracle, scenes):
    p = vpt.default_params(max_depth=8, dof_strength=0.8, focus_distance=20.0)
    check(vpt, oracle, scenes("cornell_box"), 100, 37, p, [4])


@pytest.mark.parametrize("flags", ["default", "local_hits"])
@pytest.mark.parametrize("count", [False, True])
def test_general_and_validating_instantiations(vpt, oracle, scenes, flags, count):
    """The glass variant runs the general instantiation, VPT_FLAG_LOCAL_HITS the validating (STRICT) ones, count_traversal the counting ones."""
    A = vpt._abi
    p = vpt.default_params(max_depth=8)
    p.flags = A.FLAGS_DEFAULT | (A.FLAG_LOCAL_HITS if flags == "local_hits" else 0)
    check(vpt, oracle, glass(vpt, scenes), 100, 37, p, [3, 1], frames_in_flight=3, count_traversal=count)
    check(vpt, oracle, scenes("cornell_box"), 65, 9, p, [2], count_traversal=count)


@pytest.mark.parametrize("w,h", [(100, 37), (7, 5)])
def test_one_frame_async_batches_replayed_from_graphs(vpt, oracle, scenes, w, h):
    """vpt_render_async(1): the launch is captured once and replayed with the batch's first dispatch index in device memory (dispatch_base_dev)."""
    sc, frames = scenes("cornell_box"), 10
    p = vpt.default_params(max_depth=8)
    ref, ctr = oracle_image(oracle, sc, w, h, p, frames)
    g = vpt.PathTracer(w, h, frames_in_flight=1)
    g.set_scene(sc); g.set_params(p)
    prev = 0
    for _ in range(frames):
        g.render_async(1)
        cur = g.postprocess_device()
        if prev:
            g.wait(prev)
        prev = cur
    g.wait()
    st = g.stats()
    assert np.array_equal(g.radiance(), ref)
    assert st["closest_rays"] == ctr["closest"] and st["samples"] == w * h * frames
    assert st["kernel_launches"]["primary"] == frames and st["kernel_launches"]["bounce"] == 0
    assert st["graph_launches"] >= frames - 3
    g.close()


@pytest.mark.parametrize("variant", ["compact", "compact_environment"])
def test_a_deeper_tree_under_the_shorter_stack(vpt, oracle, scenes, variant):
    """tests/material_scenes.py's compact scenes ride in LDS with seven nodes where the Cornell box has three (normal maps, emissive textures, affine
    instances, an environment: the general instantiation on a deeper tree).  Their shape allows 9 stack entries, but rays stay within the 6 that k_whole
    keeps in LDS (tests/test_stack_bound_cpu.py), so this is no test of the spill path: test_the_spill_path_of_the_shorter_stack is."""
    sc, info = material_scenes.variant(variant)
    material_scenes.check_preconditions(sc, info)
    p = vpt.default_params(max_depth=7, sky_azimuth=35.0, sky_altitude=-20.0, sky_intensity=1.5)
    g = vpt.PathTracer(8, 8); g.set_scene(scenes("cornell_box")); cornell_nodes = g.stats()["bvh_nodes"]; g.close()
    st = check(vpt, oracle, sc, 100, 37, p, [3])
    print("bvh_nodes %d (Cornell box %d), stack_spills %r" % (st["bvh_nodes"], cornell_nodes, st["stack_spills"]))
    assert st["bvh_node_bytes"] == 128 and st["bvh_nodes"] > cornell_nodes


@pytest.mark.parametrize("flags", ["default", "local_hits"])
def test_the_spill_path_of_the_shorter_stack(vpt, oracle, flags):
    """tests/whole_spill_scene.py: a chain-shaped tree under 3 KB whose searches from the floor up through the sheets hold up to 11 entries
    (tests/test_stack_bound_cpu.py) — more than the 6 rows k_whole keeps in LDS (traverse.hpp kWholeStackRows), fewer than the 14 of the per-bounce
    kernels.  So the whole-path kernel, and only it, writes the per-thread overflow region (TravStackT<6>::push / pop beyond row 6, stride kOverflow = 90),
    and the image and ray counts are still the oracle's and the per-bounce kernels'.  vpt_stats.stack_spills counts the words written."""
    import whole_spill_scene
    A = vpt._abi
    sc = whole_spill_scene.chain_scene(vpt)
    p = vpt.default_params(max_depth=4)
    p.flags = A.FLAGS_DEFAULT | (A.FLAG_LOCAL_HITS if flags == "local_hits" else 0)
    st = check(vpt, oracle, sc, 100, 37, p, [3, 1], frames_in_flight=3)
    print("bvh_nodes %d, stack_spills %r" % (st["bvh_nodes"], st["stack_spills"]))
    assert st["bvh_node_bytes"] == 128, "the scene should ride in LDS"
    assert st["stack_spills"][0] > 0, "no spills: %r" % (st["stack_spills"],)
    g = vpt.PathTracer(100, 37, pipeline=A.PIPELINE_FUSED, frames_in_flight=3)
    g.set_scene(sc); g.set_params(p); g.render(3)
    assert g.stats()["stack_spills"] == [0, 0], "the per-bounce kernels keep 14 rows: 11 entries fit"
    g.close()
