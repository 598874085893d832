"""The whole-path kernel (kernels_whole.hip k_whole) reads the camera from a per-block copy in LDS when it generates a tile of camera rays, and
knows its frames to be one-sample frames at compile time.  Neither changes a value: images and ray counters must be the oracle's, bit for bit,
wherever a tile of 64 launch indices can lie on the image — astride rows and frames, exactly inside a row, on the rows of a shard — with and
without depth of field (every field of the copied block is read), in the PLAIN and the general instantiation."""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RAY_STATS = ("samples", "closest_rays", "shadow_rays", "primary_hits", "primary_survivors", "primary_shadow_rays")


@pytest.fixture(scope="module")
def reference(oracle, scenes, vpt):
    """Oracle images and counters, computed once per (scene, shape, parameters)."""
    cache = {}

    def get(kind, w, h, frames, **params):
        key = (kind, w, h, frames, tuple(sorted(params.items())))
        if key not in cache:
            o = oracle.Oracle(scene_of(vpt, scenes, kind), w, h)
            o.set_params(vpt.default_params(max_depth=8, **params))
            o.render(frames)
            cache[key] = (o.radiance(), o.counters())
            o.close()
        return cache[key]
    return get


def scene_of(vpt, scenes, kind):
    sc = scenes("cornell_box")
    if kind == "glass":     # a glass wall and a sky: the general instantiation
        sc = copy.deepcopy(sc)
        sc.materials[0].update(transmission=1.0, roughness=0.05, ior=1.5, base_color=(1, 1, 1))
        sc.env = vpt.scenes.sun_sky_env(64, 32, seed=9, sun_peak=100.0)
    return sc


def render(vpt, sc, w, h, batches, pipeline, **params):
    g = vpt.PathTracer(w, h, pipeline=pipeline, frames_in_flight=max(batches))
    g.set_scene(sc); g.set_params(vpt.default_params(max_depth=8, **params))
    for n in batches:
        g.render(n)
    img, st = g.radiance(), g.stats()
    g.close()
    return img, st


# 100 x 37, three frames in one batch: tiles straddle rows and frames; 128 x 8: two whole tiles per row; 64 x 5: a row is a tile
@pytest.mark.parametrize("kind", ["cornell", "glass"])
@pytest.mark.parametrize("w,h,batches", [(100, 37, [3]), (128, 8, [2, 1]), (64, 5, [3])])
def test_tiles_astride_and_inside_rows(vpt, scenes, reference, kind, w, h, batches):
    A = vpt._abi
    ref, ctr = reference(kind, w, h, sum(batches))
    img, st = render(vpt, scene_of(vpt, scenes, kind), w, h, batches, A.PIPELINE_WHOLE)
    assert np.array_equal(img, ref), "%d px differ" % int((np.abs(img - ref).max(axis=2) > 0).sum())
    assert st["closest_rays"] == ctr["closest"], (st["closest_rays"], ctr)
    assert st["kernel_launches"]["primary"] == len(batches) and st["kernel_launches"]["bounce"] == 0
    # the per-bounce kernels: the same ray statistics (shadow rays are compared between the kernels, as tests/test_gpu_whole_refill.py does: the oracle's own
    # shadow counter follows another definition)
    _, sf = render(vpt, scene_of(vpt, scenes, kind), w, h, batches, A.PIPELINE_FUSED)
    for k in RAY_STATS:
        assert st[k] == sf[k], (k, st[k], sf[k])


def test_depth_of_field_reads_the_whole_camera_block(vpt, scenes, reference):
    kw = dict(dof_strength=0.8, focus_distance=20.0)
    ref, ctr = reference("cornell", 128, 8, 2, **kw)
    img, st = render(vpt, scenes("cornell_box"), 128, 8, [2], vpt._abi.PIPELINE_WHOLE, **kw)
    assert np.array_equal(img, ref)
    assert st["closest_rays"] == ctr["closest"]
    _, sf = render(vpt, scenes("cornell_box"), 128, 8, [2], vpt._abi.PIPELINE_FUSED, **kw)
    for k in RAY_STATS:
        assert st[k] == sf[k], (k, st[k], sf[k])


def test_every_rank_of_three_row_shards(vpt, scenes, reference):
    """96 x 12 over three shards: a shard's launch indices cover every third row, four rows of one and a half tiles each.  Assembled, the
    shards are the oracle's image; their ray counters add up to the oracle's closest-hit rays and to the unsharded per-bounce kernels' statistics."""
    sc, w, h, frames, G = scenes("cornell_box"), 96, 12, 2, 3
    ref, ctr = reference("cornell", w, h, frames)
    parts = []
    for r in range(G):
        g = vpt.PathTracer(w, h, shard_rank=r, shard_count=G, pipeline=vpt._abi.PIPELINE_WHOLE)
        g.set_scene(sc); g.set_params(vpt.default_params(max_depth=8)); g.render(frames)
        parts.append(g)
    stats = [g.stats() for g in parts]
    assert all(s["kernel_launches"]["primary"] == 1 and s["kernel_launches"]["bounce"] == 0 for s in stats)
    assert sum(s["closest_rays"] for s in stats) == ctr["closest"]
    _, sf = render(vpt, sc, w, h, [frames], vpt._abi.PIPELINE_FUSED)
    for k in RAY_STATS:
        assert sum(s[k] for s in stats) == sf[k], (k, [s[k] for s in stats], sf[k])
    assert sf["samples"] == w * h * frames
    hip = C.CDLL("libamdhip64.so")
    n = parts[0].shard_floats()
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), n * 4 * G) == 0
    for r, g in enumerate(parts):
        g.shard_to_device(C.c_void_p(buf.value + r * n * 4))
    parts[0].assemble_shards(buf, G)
    assert np.array_equal(parts[0].radiance(), ref)
    hip.hipFree(buf)
    for g in parts:
        g.close()
