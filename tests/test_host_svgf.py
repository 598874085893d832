"""The C++ facade's SVGF members (extensions: no upstream members) through a small program of its own, tests/tools/facade_svgf.cpp: TemporalAccumulate after
SetBaseSeed and a camera move, with the variance on, and Denoise from the temporal source, equal the Python shim's results of the same calls bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from test_host_cpp import GOLDEN, HOST, LUTS, ROOT, cli  # noqa: F401  (the fixture that builds the facade library)

pytestmark = pytest.mark.gpu


def test_facade_temporal_accumulate_after_set_base_seed_equals_the_shim(cli, vpt, tmp_path):  # noqa: F811
    exe = str(tmp_path / "facade_svgf")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-I" + HOST, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "facade_svgf.cpp"),
                           os.path.join(HOST, "libvpt_host.a"), "-o", exe, "-L" + os.path.dirname(HOST), "-lvpt_hip", "-lz", "-Wl,-rpath," + os.path.dirname(HOST), "-Wl,-rpath,/opt/rocm/lib"])
    gltf = os.path.join(GOLDEN, "cornell_box.gltf")
    sc = vpt.scenes.load_gltf(gltf)
    w, h, spp, depth, seed = 45, 37, 2, 4, 9
    move = np.eye(4); move[:3, 3] = (0.5, 0.15, 0.0)
    second = (np.asarray(sc.view_inverse, np.float64) @ move).astype(np.float32)
    out = [str(tmp_path / n) for n in ("temporal.f32", "denoised.f32", "camera.f32")]
    subprocess.check_call([exe, gltf, LUTS, str(w), str(h), str(spp), str(depth), str(seed)] + ["%r" % float(v) for v in second.T.reshape(-1)] + out)
    temporal, denoised = (np.fromfile(p, "<f4").reshape(h, w, 4) for p in out[:2])
    cam = np.fromfile(out[2], "<f4").reshape(3, 4, 4)
    assert np.array_equal(cam[2].T, second)
    g = vpt.PathTracer(w, h)
    try:
        g.set_scene(sc)
        g.set_params(vpt.default_params(max_depth=depth, max_samples=spp))
        g.set_svgf_options(variance=1, min_history=2)
        g.set_denoise_source(vpt.DENOISE_SOURCE_TEMPORAL)
        g.set_camera(cam[0].T, cam[1].T); g.render(spp)
        first = g.temporal_accumulate()
        g.set_camera(second, cam[1].T); g.set_base_seed(seed); g.render(spp)
        want_t, want_d = g.temporal_accumulate(), g.denoise()
        assert (g.temporal_history() > spp).sum() > 50 and (g.temporal_variance() > 0).sum() > 50
    finally:
        g.close()
    assert not np.array_equal(first, want_t)
    assert np.array_equal(temporal.view(np.uint32), want_t.view(np.uint32))
    assert np.array_equal(denoised.view(np.uint32), want_d.view(np.uint32))
