"""The device's texture-slot and instance-transform code paths, which no shipped scene reaches (tests/material_scenes.py):
per-hit normal maps (shading.hpp surface_frame), a 1x1 non-default normal texel (k_precompute_materials kMatNormal), textured light
samples (sample_emissive with LightSampler.uniform == 0), a 1x1 coloured and a 1x1 black emissive texel, the per-class shade kernels of
VPT_PIPELINE_STAGED_SORTED (k_classify_instances), and world-space tables under non-uniform scale, shear and mirroring
(k_precompute_tri_ng / _tri_shade / _emissive).

Three kinds of check: bit-exact parity with the oracle on every pipeline; 1x1 textures (values resolved once per material, the PLAIN
kernel instantiations, a uniform light sampler) against 2x2 and 3x1 textures of the same texel (fetched per hit), bit-identical without
the oracle; closest hits on the affine scene against the oracle's brute force.  vpt_stats has no per-class counters, so every test asserts
from the scene itself that the path it is about is in play."""
import copy

import numpy as np
import pytest

import material_scenes
from test_gpu_parity import assert_parity
from trace_ray_sets import affine_rays

pytestmark = pytest.mark.gpu

# name: (PathTracer keywords, samples_per_frame, size)
CONFIGS = {
    "auto": (dict(pipeline=0), 1, (96, 54)),
    "auto_ragged": (dict(pipeline=0), 1, (63, 37)),
    "fused": (dict(pipeline=1), 1, (96, 54)),
    "staged": (dict(pipeline=2), 1, (96, 54)),
    "staged_streams_only": (dict(pipeline=2, build_flags=4), 1, (96, 54)),    # VPT_BUILD_STREAMS_ONLY
    "staged_sorted": (dict(pipeline=4), 1, (96, 54)),
    "general_kernels": (dict(pipeline=0, build_flags=2), 1, (96, 54)),        # VPT_BUILD_GENERAL_KERNELS
    "auto_2spf": (dict(pipeline=0), 2, (96, 54)),                             # not a whole-path batch
}
VARIANTS = ("normal_map", "emissive_texture", "affine_instances", "combined", "compact", "compact_environment")
_ORACLE = {}


def params(vpt, spf=1, depth=7):
    return vpt.default_params(max_depth=depth, samples_per_frame=spf, sky_azimuth=35.0, sky_altitude=-20.0, sky_intensity=1.5)


def oracle_image(oracle, key, sc, w, h, P, frames):
    if key not in _ORACLE:
        o = oracle.Oracle(sc, w, h); o.set_params(P); o.render(frames)
        _ORACLE[key] = o.radiance(); o.close()
    return _ORACLE[key]


def render(vpt, sc, w, h, P, frames, **kw):
    g = vpt.PathTracer(w, h, **kw)
    g.set_scene(sc); g.set_params(P); g.render(frames)
    img = g.radiance(); st = g.stats(); g.close()
    return img, st


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("variant", VARIANTS)
def test_parity_with_the_oracle(vpt, oracle, variant, config):
    sc, info = material_scenes.variant(variant)
    material_scenes.check_preconditions(sc, info)
    kw, spf, (w, h) = CONFIGS[config]
    P = params(vpt, spf)
    frames = 3
    ref = oracle_image(oracle, (variant, w, h, spf), sc, w, h, P, frames)
    assert (ref[..., :3].sum(axis=2) > 0).mean() > 0.3
    img, st = render(vpt, sc, w, h, P, frames, **kw)
    assert_parity(img, ref)
    if config == "auto":
        # the compact scenes ride in LDS: one whole-path launch per batch; the others run on the streams
        compact = variant.startswith("compact")
        assert st["bvh_node_bytes"] == (128 if compact else 64)
        if compact:
            assert st["kernel_launches"]["primary"] > 0 and st["kernel_launches"]["bounce"] == 0 and st["kernel_launches"]["extend"] == 0
        else:
            assert st["kernel_launches"]["extend"] > 0


# one slot of one material, the 1x1 texel and the same texel as 2x2 and 3x1 (bilinear filtering of equal texels returns the texel)
SLOTS = {
    "normal": ("normal_texture", 2, (200, 90, 180, 255)),
    "base_color": ("base_color_texture", 2, (180, 140, 90, 255)),
    "roughness": ("roughness_texture", 2, (140,)),
    "metallic": ("metallic_texture", 2, (100,)),
    "emissive": ("emissive_texture", 3, (255, 200, 120, 255)),
}


def slot_scene(vpt, scenes, slot, shape):
    sc = copy.deepcopy(scenes("cornell_box"))
    key, mat, texel = SLOTS[slot]
    sc.materials[mat]["metallic"] = 0.8 if slot == "metallic" else sc.materials[mat]["metallic"]
    if slot in ("roughness", "normal"):
        sc.materials[mat].update(metallic=0.6, roughness=0.9, anisotropy=0.4, anisotropy_rotation=25.0)
    sc.materials[mat][key] = sc.add_texture(np.tile(np.array(texel, np.uint8), shape + (1,)))
    return sc


@pytest.mark.parametrize("pipeline", [0, 1, 2, 4])
@pytest.mark.parametrize("slot", list(SLOTS))
def test_one_texel_textures_equal_their_per_hit_fetch(vpt, oracle, scenes, slot, pipeline):
    """A 1x1 texture (resolved once: MatResolved, kShadePlain / k_whole<PLAIN> / k_bounce<PLAIN>, a uniform LightSampler) against a
    2x2 and a 3x1 texture of the same texel (fetched per hit by the general code): the images must be bit-identical, here and on the oracle."""
    w, h, frames = 96, 54, 3
    P = vpt.default_params(max_depth=6)
    imgs, refs = [], []
    for shape in ((1, 1), (2, 2), (1, 3)):
        sc = slot_scene(vpt, scenes, slot, shape)
        key, mat, _ = SLOTS[slot]
        t = sc.textures[sc.materials[mat][key]]
        assert t.shape[:2] == shape
        # the 1x1 scene is a PLAIN one (every texture 1x1, black environment), the others are not
        assert all(x.shape[:2] == (1, 1) for x in sc.textures) == (shape == (1, 1)) and not sc.env.any()
        refs.append(oracle_image(oracle, ("slot", slot, shape), sc, w, h, P, frames))
        img, _ = render(vpt, sc, w, h, P, frames, pipeline=pipeline, build_flags=4 if pipeline == 2 else 0)
        imgs.append(img)
    assert refs[0][..., :3].max() > 0
    assert np.array_equal(refs[0], refs[1]) and np.array_equal(refs[0], refs[2]), "oracle: per-hit fetch differs from the 1x1 texel"
    assert np.array_equal(imgs[0], imgs[1]), "device: the 2x2 texture differs from the 1x1 texel"
    assert np.array_equal(imgs[0], imgs[2]), "device: the 3x1 texture differs from the 1x1 texel"
    assert_parity(imgs[0], refs[0])


def test_closest_hits_on_affine_instances(vpt, oracle):
    """trace_rays against the oracle's brute force on the affine scene: random rays, and rays aimed into the mirrored, sheared and
    non-uniformly scaled instances (t, u, v, primitive, instance all equal)."""
    sc, info = material_scenes.variant("affine_instances")
    material_scenes.check_preconditions(sc, info)
    rays = affine_rays(sc, info)
    o = oracle.Oracle(sc, 8, 8); o.set_brute_force(True); ref = o.trace_rays(rays); o.close()
    g = vpt.PathTracer(8, 8); g.set_scene(sc); got = g.trace_rays(rays); g.close()
    for k in ("t", "u", "v", "primitive", "instance"):
        assert np.array_equal(got[k], ref[k]), k
    hit_inst = ref["instance"][ref["t"] >= 0]
    for inst in info["mirrored"] + info["sheared"]:
        assert (hit_inst == inst).sum() > 1000, inst
