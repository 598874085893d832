"""The oracle's per-sample values against tests/ref_integrator64.py on scenes with the inputs the shipped fixtures never use
(tests/material_scenes.py): per-hit and 1x1 non-default normal maps, emissive textures on the lights (a 16 x 9 RGBA8 panel, a 1 x 7 R8
strip, a 1x1 coloured texel, a 1x1 black texel under a non-zero emissive colour), and affine instances (non-uniform scale, shear,
mirroring — the sphere and a box —, a tilted and stretched lamp, a box whose z faces keep an exact +-z world normal).

These inputs reach code the oracle shares with the device (include/vpt_fp32.h rowvec_mat3 / inverse3x3_from_mat4 / texel_coords, the
normal-map decode, the light sample's uv, the light pdf's world area): only the float64 restatement, written from the Slang sources, can
tell a shared mistake there.  Same rule as tests/test_oracle_integrator_fp64.py: 2e-3 relative per sample, at most 1 % of the samples
differing outright, more than half of them lit."""
import numpy as np
import pytest

import material_scenes

CASES = {   # name: (variant, depth, pixels, frames, flags: None = the defaults)
    "normal_map": ("normal_map", 6, 80, 2, None),
    "emissive_texture": ("emissive_texture", 6, 80, 2, None),
    "emissive_texture_no_mis": ("emissive_texture_environment", 6, 80, 2, "no_mis"),   # (lit: by the environment, as flags_no_mis_no_compensation)
    "affine_instances": ("affine_instances", 8, 80, 2, None),
    "combined": ("combined", 6, 90, 3, None),
    "combined_no_mis": ("combined", 6, 80, 2, "no_mis"),
    "compact_environment": ("compact_environment", 6, 80, 2, None),   # the scene the whole-path kernels serve on the device
}


@pytest.mark.parametrize("which", list(CASES))
def test_per_sample_values_match_the_float64_integrator(vpt, oracle, which):
    import ref_integrator64 as R
    name, depth, npix, frames, flags = CASES[which]
    sc, info = material_scenes.variant(name)
    material_scenes.check_preconditions(sc, info)
    a = vpt._abi
    fl = a.FLAGS_DEFAULT if flags is None else a.FLAGS_DEFAULT & ~(a.FLAG_SKY_MIS | a.FLAG_MESH_MIS | a.FLAG_ENERGY_COMPENSATION)
    P = vpt.default_params(max_depth=depth, sky_azimuth=35.0, sky_altitude=-20.0, sky_intensity=1.5, flags=fl)
    W, H = 64, 36
    S = R.Scene64(sc, W, H)
    luts = vpt.scenes.load_luts()
    o = oracle.Oracle(sc, W, H)
    o.set_params(P)
    rng = np.random.default_rng(7)
    lo_x, hi_x = (0, 64) if sc.env.size > 4 else (14, 50)   # with the environment, also the pixels beside the box
    xs = rng.integers(lo_x, hi_x, npix).astype(np.uint32); ys = rng.integers(4, 32, npix).astype(np.uint32)
    got = o.pixel_samples(xs, ys, 0, frames).astype(np.float64)
    o.close()
    bad, total, lit = 0, 0, 0
    for i, (x, y) in enumerate(zip(xs, ys)):
        for f in range(frames):
            ref = R.sample_value(S, luts, int(x), int(y), f, P)
            total += 1
            lit += bool(ref.max() > 0)
            if not np.allclose(got[i, f], ref, rtol=2e-3, atol=1e-6):
                bad += 1
    assert lit > 0.5 * total
    assert bad <= 0.01 * total, (bad, total)
