"""The C++ facade's SetInstanceTransforms (an extension: no upstream member) through a small program of its own, tests/tools/facade_move.cpp:
called after SetScene it goes through vpt_set_instance_transforms (a refit), called before it the matrix waits for the scene; both renders are
byte-identical and equal the oracle's of the moved description."""
import os
import subprocess

import numpy as np
import pytest

import refit_moves as RM
from test_host_cpp import GOLDEN, HOST, LUTS, ROOT, cli  # noqa: F401  (the fixture that builds the facade library)

pytestmark = pytest.mark.gpu
FLAG_LOCAL_HITS = 256


def test_facade_move_after_and_before_set_scene(cli, vpt, oracle, tmp_path):  # noqa: F811
    exe = str(tmp_path / "facade_move")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-I" + HOST, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "facade_move.cpp"),
                           os.path.join(HOST, "libvpt_host.a"), "-o", exe, "-L" + os.path.dirname(HOST), "-lvpt_hip", "-lz", "-Wl,-rpath," + os.path.dirname(HOST), "-Wl,-rpath,/opt/rocm/lib"])
    gltf = os.path.join(GOLDEN, "cornell_box.gltf")
    sc = vpt.scenes.load_gltf(gltf)
    w, h, spp, depth = 96, 54, 3, 5
    matrix = RM.moved_matrices(sc, RM.CORNELL_LAMP)[RM.LAMP]
    args = ["%r" % float(v) for v in matrix.T.reshape(-1)]
    out = {}
    for when in ("after", "before"):
        rad, cam = str(tmp_path / (when + "_r.f32")), str(tmp_path / (when + "_c.f32"))
        subprocess.check_call([exe, gltf, LUTS, str(w), str(h), str(spp), str(depth), when, str(RM.LAMP)] + args + [rad, cam])
        out[when] = (open(rad, "rb").read(), open(cam, "rb").read())
    assert out["after"] == out["before"]
    img = np.frombuffer(out["after"][0], "<f4").reshape(h, w, 4)
    m = np.frombuffer(out["after"][1], "<f4").reshape(2, 4, 4)
    P = vpt.default_params(max_depth=depth, base_seed=1, max_samples=spp)
    refs = []
    for scene in (RM.with_matrices(sc, {RM.LAMP: matrix}), sc):
        o = oracle.Oracle(scene, w, h)
        o.set_camera(m[0].T, m[1].T); o.set_params(P); o.render(spp)
        refs.append(o.radiance()); o.close()
    assert not np.array_equal(refs[0], refs[1]), "the move changes no pixel: the comparison would show nothing"
    assert np.array_equal(img, refs[0])
