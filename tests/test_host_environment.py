"""The C++ facade's SetEnvMapFilepath AFTER SetScene (vpt_render --env-late: the Editor's order of calls) goes through
vpt_set_environment: radiance and PNG are byte-identical to the run that sets the map before SetScene, and equal the oracle with the
decoded .hdr.  Reads the outputs tests/test_host_cpp.py test_hdr_env_and_png_export_through_the_cli reads."""
import os
import subprocess

import numpy as np
import pytest

from test_host_cpp import GOLDEN, LUTS, cli  # noqa: F401  (the fixture that builds vpt_render)

pytestmark = pytest.mark.gpu


def test_env_late_equals_env_first_and_the_oracle(cli, vpt, oracle, tmp_path):  # noqa: F811
    gltf = os.path.join(GOLDEN, "cornell_box.gltf")
    hdr = str(tmp_path / "sky.hdr")
    vpt.imagefiles.save_hdr(hdr, vpt.scenes.sun_sky_env(64, 32, seed=2, sun_peak=500.0)[..., :3])
    w, h, spp, depth = 96, 54, 3, 5
    out = {}
    for tag, extra in (("first", []), ("late", ["--env-late"])):
        rad, cam, png = (str(tmp_path / (tag + n)) for n in ("_r.f32", "_c.f32", "_o.png"))
        subprocess.check_output([cli, "--scene", gltf, "--luts", LUTS, "--size", "%dx%d" % (w, h), "--spp", str(spp), "--depth", str(depth), "--radiance", rad,
                                 "--camera", cam, "--env-hdr", hdr, "--png", png] + extra)
        out[tag] = (open(rad, "rb").read(), open(cam, "rb").read(), open(png, "rb").read())
    assert out["late"][0] == out["first"][0], "radiance differs between --env-late and the map set before SetScene"
    assert out["late"][1] == out["first"][1], "the swap moved the camera"
    assert out["late"][2] == out["first"][2], "PNG differs between --env-late and the map set before SetScene"
    img = np.frombuffer(out["late"][0], "<f4").reshape(h, w, 4)
    m = np.frombuffer(out["late"][1], "<f4").reshape(2, 4, 4)
    sc = vpt.scenes.load_gltf(gltf)
    own = sc.env
    sc.env = vpt.imagefiles.load_hdr(hdr)
    P = vpt.default_params(max_depth=depth, base_seed=1, max_samples=spp)
    o = oracle.Oracle(sc, w, h)
    o.set_camera(m[0].T, m[1].T); o.set_params(P); o.render(spp)
    ref = o.radiance(); o.close()
    sc.env = own                                             # the map the scene would have kept had the late call done nothing
    o = oracle.Oracle(sc, w, h)
    o.set_camera(m[0].T, m[1].T); o.set_params(P); o.render(spp)
    assert not np.array_equal(o.radiance(), ref), "the sky reaches no pixel of this scene: the comparison would show nothing"
    o.close()
    assert np.array_equal(img, ref)
    ref8, _ = oracle.postprocess(ref, vpt.default_post_params())
    assert np.array_equal(vpt.imagefiles.load_png(str(tmp_path / "late_o.png")), ref8)
