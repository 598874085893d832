"""vpt_denoise / vpt_denoise_device / vpt_set_post_source on the device: the edge-avoiding a-trous filter over the accumulation image and the first-hit
guide images.  The kernels call the per-pixel functions of csrc/denoise.hpp, so the device image is held BIT FOR BIT to a host compile of that header
(tests/tools/denoise_driver.cpp) fed the context's own radiance and guide images; the arithmetic itself is held to float64 by tests/test_denoise_cpu.py.
Then: the post source, that a call disturbs nothing, the device / asynchronous / sharded forms, that it follows edits, that it lowers the error of a
4-spp image, every error code, and the command-line tool."""
import copy
import ctypes as C
import os
import subprocess
from importlib import import_module

import numpy as np
import pytest
import torch   # before the first context exists (see tests/test_gpu_features.py)

import denoise_host as DH
import refit_moves as RM
from test_gpu_features import scene as feature_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LUTS = os.path.join(ROOT, "vulkan-path-tracer_amd", "assets", "lookup_tables.bin")
NO_SCENE, INVALID = "VPT_ERR_NO_SCENE", "VPT_ERR_INVALID_ARGUMENT"
FLAG_LOCAL_HITS = 256
_CACHE = {}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("denoise_gpu")
    return DH.compile_driver(str(d / "denoise_driver")), d


def context(vpt, sc, w, h, frames=2, flags=0, **cfg):
    g = vpt.PathTracer(w, h, **cfg)
    g.set_scene(sc)
    P = vpt.default_params(max_depth=4)
    P.flags |= flags
    g.set_params(P)
    if frames:
        g.render(frames)
    return g


# ---- 1. device == host compile, bit for bit
@pytest.mark.parametrize("w,h", [(45, 37), (150, 9)], ids=["45x37", "150x9"])
@pytest.mark.parametrize("name", ["cornell_gltf", "textured_boxes"])
def test_device_equals_the_host_compile_bit_for_bit(vpt, driver, name, w, h):
    """45 x 37: partial tiles on both edges, steps 8 and 16 reach past the image.  150 x 9: three tiles across with a partial last one, fewer rows than a
    halo.  1 and 2 iterations run the LDS-tiled kernel only; 3 and 5 the one that reads its taps from memory as well."""
    g = context(vpt, feature_scene(vpt, name), w, h)
    try:
        f = g.render_features(0, 0, which=("depth", "normal", "albedo"))
        rad = g.radiance()
        hit = f["depth"] >= 0
        assert hit.any() and (~hit).any(), "the view must hold hits and misses"
        for it in (1, 2, 3, 5):
            for flags in (0, vpt.DENOISE_DEMODULATE):
                dp = vpt.default_denoise_params(iterations=it, flags=flags)
                want = DH.run_driver(driver[0], driver[1], rad, f["normal"], f["albedo"], f["depth"], it, dp.sigma_color, dp.sigma_normal, dp.sigma_depth, flags, tag="bits")
                got = g.denoise(dp)
                diff = DH.bits(got) != DH.bits(want)
                assert not diff.any(), "%d iterations, flags %d: %d words differ, first at %r" % (it, flags, diff.sum(), tuple(np.argwhere(diff)[0]))
                assert np.array_equal(DH.bits(got)[~hit], DH.bits(rad)[~hit])
                assert np.abs(got[hit][:, :3] - rad[hit][:, :3]).max() > 0
        assert np.array_equal(DH.bits(g.denoise(vpt.default_denoise_params(iterations=0))), DH.bits(rad))
        assert np.array_equal(g.radiance(), rad)
    finally:
        g.close()


# ---- 2. the post source
def test_post_source(vpt, scenes):
    sc = scenes("cornell_box")
    w, h = 45, 37
    g = context(vpt, sc, w, h)
    other = context(vpt, sc, w, h, frames=0)
    try:
        parent = g.postprocess()
        g.set_post_source(vpt.POST_SOURCE_DENOISED)
        with pytest.raises(vpt.VptError, match=INVALID):
            g.postprocess()                                   # never denoised
        with pytest.raises(vpt.VptError, match=INVALID):
            g.postprocess_device()
        den = g.denoise()
        got = g.postprocess()
        other.set_radiance(den, 2)
        assert np.array_equal(got, other.postprocess())
        assert not np.array_equal(got, parent)
        g.postprocess_device(); g.wait()
        assert np.array_equal(g.output_to_host(), got)
        g.set_post_source(vpt.POST_SOURCE_RADIANCE)
        assert np.array_equal(g.postprocess(), parent)      # the default source after a denoise: the parent's bytes
        g.set_post_source(vpt.POST_SOURCE_DENOISED)
        g.resize(w + 3, h)
        g.render(1)
        with pytest.raises(vpt.VptError, match=INVALID):
            g.postprocess()                                   # resized since
        g.denoise()
        assert g.postprocess().shape == (h, w + 3, 4)
    finally:
        g.close(); other.close()


# ---- 3. it disturbs nothing
@pytest.mark.parametrize("use_async", [False, True], ids=["render", "render_async"])
def test_a_call_between_batches_changes_no_image_and_no_counter(vpt, oracle, scenes, use_async):
    sc = scenes("cornell_box")
    w, h = 32, 24
    P = vpt.default_params(max_depth=4)
    key = ("oracle6", w, h)
    if key not in _CACHE:
        o = oracle.Oracle(sc, w, h); o.set_params(P); o.render(6); _CACHE[key] = o.radiance(); o.close()

    def run(interrupt):
        g = vpt.PathTracer(w, h); g.set_scene(sc); g.set_params(P)
        try:
            render = (lambda n: g.render_async(n)) if use_async else g.render
            render(3)
            if interrupt:
                a = g.denoise()
                dev = torch.zeros((h, w, 4), device="cuda:0")
                g.denoise_device(None, dev.data_ptr())
                g.wait()
                assert np.array_equal(dev.cpu().numpy(), a) and (a[..., :3] > 0).any()
            render(3)
            g.wait()
            st = g.stats()
            return g.radiance(), [st[k] for k in ("samples", "frames", "dispatches", "closest_rays")]
        finally:
            g.close()
    img, st = run(True)
    img0, st0 = run(False)
    assert np.array_equal(img, img0) and np.array_equal(img, _CACHE[key])
    assert st == st0 and st[1] == 6


# ---- 4. device pointer, asynchronous form, shards
def test_device_pointer_ticket_and_shards(vpt):
    sc = feature_scene(vpt, "textured_boxes")
    w, h = 45, 37
    g = context(vpt, sc, w, h)
    try:
        want = g.denoise()
        dev = torch.full((h, w, 4), 7.0, device="cuda:0")
        t = g.denoise_device(None, dev.data_ptr())
        assert t > 0
        g.wait(t)
        assert np.array_equal(DH.bits(dev.cpu().numpy()), DH.bits(want))
        t2 = g.denoise_device(vpt.default_denoise_params(iterations=2), None)     # no copy asked for: the image stays in the context
        assert t2 > t
        g.wait()
    finally:
        g.close()
    parts = [context(vpt, sc, w, h, shard_rank=r, shard_count=2) for r in range(2)]
    hip = C.CDLL("libamdhip64.so")
    buf = C.c_void_p()
    try:
        for f in (parts[0].denoise, lambda: parts[0].denoise_device(None, None)):
            with pytest.raises(vpt.VptError, match=INVALID):
                f()                                            # a sharded context before vpt_assemble_shards
        n = parts[0].shard_floats()
        assert hip.hipMalloc(C.byref(buf), n * 4 * 2) == 0
        for r, s in enumerate(parts):
            s.shard_to_device(C.c_void_p(buf.value + r * n * 4))
        parts[0].assemble_shards(buf, 2)
        assert np.array_equal(DH.bits(parts[0].denoise()), DH.bits(want))
    finally:
        if buf.value:
            hip.hipFree(buf)
        for s in parts:
            s.close()


# ---- 5. it follows edits
def test_the_result_follows_camera_instances_and_materials(vpt, scenes):
    """Every call traces its guides anew: after each edit the next denoise() equals a fresh context's that was built in the edited state."""
    w, h = 45, 37
    sc = copy.deepcopy(scenes("cornell_box_glass"))
    moved = RM.moved_matrices(sc, RM.GLASS_LAMP_AND_SPHERE)
    dp = vpt.default_denoise_params()

    def fresh(scene):
        f = context(vpt, scene, w, h, flags=FLAG_LOCAL_HITS)
        try:
            return f.denoise(dp)
        finally:
            f.close()
    g = context(vpt, sc, w, h, flags=FLAG_LOCAL_HITS)   # (as tests/test_gpu_features.py compares a refitted tree with a rebuilt one)
    try:
        results = [g.denoise(dp)]
        # the camera
        sc1 = copy.deepcopy(sc)
        sc1.view_inverse = np.linalg.inv(vpt.scenes.look_at((1.5, 0.5, 9.0), (0.0, 0.0, -5.0), (0.0, 1.0, 0.0))).astype(np.float32)
        g.set_camera(sc1.view_inverse, sc1.projection_inverse(w / h))
        g.render(2)
        results.append(g.denoise(dp))
        assert np.array_equal(DH.bits(results[-1]), DH.bits(fresh(sc1)))
        # instance transforms
        for i, m in moved.items():
            g.set_instance_transforms(i, [m])
        g.render(2)
        results.append(g.denoise(dp))
        sc2 = RM.with_matrices(sc1, moved)
        sc2.view_inverse = sc1.view_inverse
        assert np.array_equal(DH.bits(results[-1]), DH.bits(fresh(sc2)))
        # a material
        m = g.get_material(1)
        m.base_color[:] = (0.1, 0.9, 0.3)
        g.set_material(1, m)
        g.render(2)
        results.append(g.denoise(dp))
        sc3 = copy.deepcopy(sc2)
        sc3.materials = copy.deepcopy(sc2.materials)
        sc3.materials[1]["base_color"] = (0.1, 0.9, 0.3)
        assert np.array_equal(DH.bits(results[-1]), DH.bits(fresh(sc3)))
        for a, b in zip(results, results[1:]):
            assert not np.array_equal(a, b), "every edit was meant to be visible"
    finally:
        g.close()


# ---- 6. quality
def test_the_defaults_lower_the_error_of_a_4_spp_image(vpt, scenes):
    """Cornell box, 64 x 48, depth 4: relative L2 error against 1024 spp of the same renderer (which other tests hold to the oracle), before and after.
    Measured with the defaults: 4 spp 0.2182, denoised 0.2174, ratio 0.996 — the whole-image figure is governed by the few pixels on the lamp's edge
    (radiance 50 against a median of 0.04), which the filter rightly leaves alone; without the 1 % of pixels with the largest error the ratio is 0.60
    (DESIGN.md §9)."""
    sc = scenes("cornell_box")
    w, h = 64, 48
    g = context(vpt, sc, w, h, frames=1024)
    try:
        ref = g.radiance()[..., :3].astype(np.float64)
        g.reset()
        g.render(4)
        noisy = g.radiance()[..., :3].astype(np.float64)
        den = g.denoise()[..., :3].astype(np.float64)
        assert g.stats()["frames"] == 4
    finally:
        g.close()
    err = lambda a: float(np.sqrt(((a - ref) ** 2).sum() / (ref ** 2).sum()))
    print("relative L2 error against 1024 spp: 4 spp %.4f, denoised %.4f, ratio %.3f" % (err(noisy), err(den), err(den) / err(noisy)))
    assert np.isfinite(den).all()
    assert err(den) < err(noisy)


# ---- 7. errors
def test_errors_leave_the_context_usable(vpt, oracle, scenes):
    sc = scenes("cornell_box")
    w, h = 32, 24
    P = vpt.default_params(max_depth=4)
    o = oracle.Oracle(sc, w, h); o.set_params(P); o.render(2); ref = o.radiance(); o.close()
    lib = vpt.load_library()
    g = vpt.PathTracer(w, h)
    try:
        ok = vpt.default_denoise_params()
        with pytest.raises(vpt.VptError, match=NO_SCENE):
            g.denoise()
        with pytest.raises(vpt.VptError, match=NO_SCENE):
            g.denoise_device()
        g.set_scene(sc); g.set_params(P)
        g.render(2)
        first = g.denoise()
        assert lib.vpt_denoise(g.ctx, None, None) == -1 and lib.vpt_denoise(None, C.byref(ok), None) == -1
        assert lib.vpt_denoise_device(g.ctx, None, None, None) == -1 and lib.vpt_denoise_device(None, C.byref(ok), None, None) == -1
        bad = [dict(iterations=vpt.DENOISE_MAX_ITERATIONS + 1), dict(sigma_color=0.0), dict(sigma_normal=-1.0), dict(sigma_depth=float("nan")), dict(flags=2), dict(flags=0x80000001)]
        for kw in bad:
            for call in (g.denoise, g.denoise_device):
                with pytest.raises(vpt.VptError, match=INVALID):
                    call(vpt.default_denoise_params(**kw))
        dev = torch.zeros(w * h * 4 + 4, device="cuda:0")
        with pytest.raises(vpt.VptError, match=INVALID):
            g.denoise_device(ok, dev.data_ptr() + 4)          # not 16-byte aligned
        with pytest.raises(vpt.VptError, match=INVALID):
            g.set_post_source(2)
        assert lib.vpt_set_post_source(None, 0) == -1
        # the previous denoised image is still valid, and the context renders bit-exact
        g.set_post_source(vpt.POST_SOURCE_DENOISED)
        other = vpt.PathTracer(w, h); other.set_scene(sc); other.set_params(P); other.set_radiance(first, 2)
        try:
            assert np.array_equal(g.postprocess(), other.postprocess())
        finally:
            other.close()
        g.denoise(vpt.default_denoise_params(iterations=vpt.DENOISE_MAX_ITERATIONS))   # the largest count is accepted
        g.reset()
        g.render(2)
        assert np.array_equal(g.radiance(), ref)
    finally:
        g.close()


# ---- 8. the command-line tool
def test_cli_denoise_writes_the_denoised_image_through_the_post_chain(vpt, tmp_path):
    from test_host_cpp import CLI, HOST
    import fcntl
    vpt.load_library()
    with open(os.path.join(HOST, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-C", HOST, "vpt_render"], stdout=subprocess.DEVNULL)
    gltf = os.path.join(GOLDEN, "cornell_box.gltf")
    w, h = 32, 24
    png, plain, cam = str(tmp_path / "d.png"), str(tmp_path / "p.png"), str(tmp_path / "c.f32")
    base = [CLI, "--scene", gltf, "--luts", LUTS, "--size", "%dx%d" % (w, h), "--spp", "2", "--depth", "3", "--camera", cam]
    subprocess.check_output(base + ["--png", png, "--denoise"])
    subprocess.check_output(base + ["--png", plain])
    m = np.fromfile(cam, "<f4").reshape(2, 4, 4)
    g = vpt.PathTracer(w, h)
    try:
        g.set_scene(vpt.scenes.load_gltf(gltf))
        g.set_camera(m[0].T, m[1].T)   # column-major dumps -> math matrices
        g.set_params(vpt.default_params(max_depth=3, base_seed=1, max_samples=2))
        g.render(2)
        g.denoise()
        g.set_post_source(vpt.POST_SOURCE_DENOISED)
        want = g.postprocess()
    finally:
        g.close()
    load = import_module("vulkan-path-tracer_amd.imagecodec").load_image
    got = np.asarray(load(png))
    assert got.shape == (h, w, 4) and np.array_equal(got, want)
    assert not np.array_equal(got, np.asarray(load(plain)))
