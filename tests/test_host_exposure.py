"""The C++ facade's auto-exposure members (extensions: no upstream members) through a small program of its own, tests/tools/facade_exposure.cpp:
PostProcessor::SetAutoExposureData / GetExposureState give the states and the RGBA8 images the Python shim's calls give, bit for bit; and vpt_render
--auto-exposure writes the image of one instant metering."""
import os
import subprocess

import numpy as np
import pytest

import exposure_host as EH
from test_host_cpp import GOLDEN, HOST, LUTS, ROOT, cli  # noqa: F401  (the fixture that builds the facade library)

pytestmark = pytest.mark.gpu


def test_facade_auto_exposure_equals_the_shim(cli, vpt, tmp_path):  # noqa: F811
    exe = str(tmp_path / "facade_exposure")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-I" + HOST, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "facade_exposure.cpp"),
                           os.path.join(HOST, "libvpt_host.a"), "-o", exe, "-L" + os.path.dirname(HOST), "-lvpt_hip", "-lz", "-Wl,-rpath," + os.path.dirname(HOST), "-Wl,-rpath,/opt/rocm/lib"])
    gltf = os.path.join(GOLDEN, "cornell_box.gltf")
    w, h, spp, depth, exposure2 = 45, 37, 2, 4, 0.5
    out = [str(tmp_path / n) for n in ("a.rgba8", "b.rgba8", "states.bin", "radiance.f32")]
    subprocess.check_call([exe, gltf, LUTS, str(w), str(h), str(spp), str(depth), repr(exposure2)] + out)
    a8, b8 = (np.fromfile(p, np.uint8).reshape(h, w, 4) for p in out[:2])
    states = np.fromfile(out[2], EH.STATE_DTYPE)
    assert len(states) == 3 and (states[0]["scale"], states[0]["valid"], states[0]["meterings"]) == (1.0, 0, 0)
    g = vpt.PathTracer(w, h)
    try:
        g.set_radiance(np.fromfile(out[3], "<f4").reshape(h, w, 4), spp)     # the image the facade rendered and metered
        g.set_exposure_options(mode=1)
        want_a, sa = g.postprocess(), g.exposure_state()
        want_b, sb = g.postprocess(vpt.default_post_params(exposure=exposure2)), g.exposure_state()
    finally:
        g.close()
    assert EH.state_tuple(states[1]) == EH.state_tuple(sa) and EH.state_tuple(states[2]) == EH.state_tuple(sb)
    assert sa.valid == 1 and sb.meterings == 2 and sa.scale != 1.0
    assert np.array_equal(a8, want_a) and np.array_equal(b8, want_b) and not np.array_equal(a8, b8)


def test_vpt_render_auto_exposure(cli, vpt, tmp_path):  # noqa: F811
    gltf = os.path.join(GOLDEN, "cornell_box.gltf")
    w, h, spp, depth = 40, 30, 2, 4
    ppm, rad = str(tmp_path / "auto.ppm"), str(tmp_path / "auto.f32")
    text = subprocess.check_output([cli, "--scene", gltf, "--luts", LUTS, "--size", "%dx%d" % (w, h), "--spp", str(spp), "--depth", str(depth), "--auto-exposure",
                                    "--ppm", ppm, "--radiance", rad], text=True)
    assert "auto-exposure: scale" in text
    got = np.frombuffer(open(ppm, "rb").read().split(b"\n255\n", 1)[1], np.uint8).reshape(h, w, 3)
    g = vpt.PathTracer(w, h)
    try:
        g.set_radiance(np.fromfile(rad, "<f4").reshape(h, w, 4), spp)     # the image vpt_render metered
        plain = g.postprocess()
        g.set_exposure_options(mode=1, rate_up=1.0, rate_down=1.0)
        want = g.postprocess()
    finally:
        g.close()
    assert np.array_equal(got, want[..., :3]) and not np.array_equal(got, plain[..., :3])
