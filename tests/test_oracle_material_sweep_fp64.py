"""The oracle's per-sample values (orc_pixel_samples) against tests/ref_integrator64.py on the material sets of tests/material_sweep.py:
the float64 restatement, written from the Slang sources, says whether the oracle is right at the edges of the material parameter space
before tests/test_gpu_material_sweep.py holds the device to the oracle there bit for bit.

Every set on the Cornell walls under the lit and the black environment, and on the walls with set members 0, 2 and 4 on the sphere
under the lit one: 64 x 36, depth 10, 200 pixels x 2 frames per case.  Same rule as tests/test_oracle_integrator_fp64.py: 2e-3 relative
(1e-6 absolute) per sample, at most 1 % of the samples differing outright, more than half of them lit.  Under the black environment the
pixels are those that look into the box (x in [12, 52), y in [4, 32)).  colour_edges does not reach 50 % lit there (186 of 400: two of
its walls are black and a third reflects nothing diffusely), so its walls case runs under the lit environment only.

Measured (15,600 samples): no sample differs in any case, none is non-finite.  Worst relative deviation of a sample per set, over its cases:
three_lobes 5.5e-05, smooth 1.0e-04, ior_edges 3.4e-05, aniso_edges 3.1e-04, colour_edges 3.9e-05, emitters 1.0e-04, medium_edges 3.0e-05,
three_lobes_textured 5.5e-05."""
import numpy as np
import pytest

import material_sweep as M

NPIX, FRAMES = 200, 2
SCENES = ("walls_lit", "walls_black", "sphere0_lit", "sphere2_lit", "sphere4_lit")


def build(name, which):
    place, env = which.split("_")
    return (M.walls(name, env) if place == "walls" else M.sphere(name, int(place[-1]), env)), env


CASES = [(name, which) for name in M.SETS for which in SCENES if (name, which) != ("colour_edges", "walls_black")]


@pytest.mark.parametrize("name,which", CASES)
def test_per_sample_values_match_the_float64_integrator(vpt, oracle, name, which):
    sc, env = build(name, which)
    if name in M.TEXTURED:
        M.check_texture(sc, name)
    xs, ys = M.window(env, NPIX, 4)
    o = oracle.Oracle(sc, M.W64, M.H64)
    o.set_params(M.params(vpt, env))
    got = o.pixel_samples(xs, ys, 0, FRAMES)
    o.close()
    assert np.isfinite(got).all()
    ref = M.ref64_samples(vpt, (name, which), sc, env, xs, ys, FRAMES)
    bad, total, lit, worst = M.compare64(got, ref)
    print("%s %s: %d of %d samples differ, %d lit, worst relative deviation %.2e" % (name, which, bad, total, lit, worst))
    assert total >= 400
    assert lit > 0.5 * total
    assert bad <= 0.01 * total, (bad, total)
