"""vpt_temporal_accumulate / _device / vpt_temporal_reset / vpt_get_temporal_history / vpt_set_denoise_source on the device: the previous result reprojected
through the first-hit guides and blended with the new samples.  The kernel calls csrc/temporal.hpp's temporal_pixel, so image and history length are held BIT FOR
BIT to a host compile of that header (tests/tools/temporal_driver.cpp) fed the context's own radiance and guide images of every step; the arithmetic itself is
held to float64 by tests/test_temporal_cpu.py.  Then: that a call disturbs nothing, when the history survives and when it is dropped, the denoise source, the
device / asynchronous / sharded forms, that it lowers the error of a moving 1-spp viewport, and every error code."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch   # before the first context exists (see tests/test_gpu_features.py)

import denoise_host as DH
import temporal_host as TH
from test_gpu_features import scene as feature_scene

pytestmark = pytest.mark.gpu
NO_SCENE, INVALID = "VPT_ERR_NO_SCENE", "VPT_ERR_INVALID_ARGUMENT"
_CACHE = {}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("temporal_gpu")
    return TH.compile_driver(str(d / "temporal_driver")), d


def context(vpt, sc, w, h, frames=2, **cfg):
    g = vpt.PathTracer(w, h, **cfg)
    g.set_scene(sc)
    g.set_params(vpt.default_params(max_depth=4))
    if frames:
        g.render(frames)
    return g


def rot_y(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    m = np.eye(4); m[0, 0], m[0, 2], m[2, 0], m[2, 2] = c, s, -s, c
    return m


def rot_x(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    m = np.eye(4); m[1, 1], m[1, 2], m[2, 1], m[2, 2] = c, -s, s, c
    return m


def shift(x, y, z):
    m = np.eye(4); m[:3, 3] = (x, y, z)
    return m


def camera_path(sc):
    """Four inverse view matrices: the scene's own camera, then — as motions in camera space — a sideways translation, a pan on top of it that pushes part of the
    view out of the image, and a large move."""
    v0 = np.asarray(sc.view_inverse, np.float64)
    t1 = shift(0.5, 0.15, 0.0)
    return [m.astype(np.float32) for m in (v0, v0 @ t1, v0 @ t1 @ rot_y(6.0) @ rot_x(1.0), v0 @ shift(-1.5, 0.6, -2.0) @ rot_y(-8.0))]


def hits_of(g):
    return g.render_features(0, 0, which=("depth",))["depth"] >= 0


# ---- 1. device == host compile, bit for bit, image and length
@pytest.mark.parametrize("w,h", [(45, 37), (150, 9)], ids=["45x37", "150x9"])
@pytest.mark.parametrize("name", ["cornell_gltf", "textured_boxes"])
def test_device_equals_the_host_compile_bit_for_bit(vpt, driver, name, w, h):
    """45 x 37: partial tiles on both edges.  150 x 9: three tiles across with a partial last one.  Four cameras, 2 frames after each vpt_set_camera, every flag
    set; the driver is fed what the context itself reports of each step (radiance, CENTER guides)."""
    sc = feature_scene(vpt, name)
    g = context(vpt, sc, w, h, frames=0)
    focus = vpt.default_params().focus_distance
    try:
        proj_inv = sc.projection_inverse(w / h)
        for flags in (0, vpt.TEMPORAL_DEMODULATE, vpt.TEMPORAL_MATCH_INSTANCE, vpt.TEMPORAL_DEMODULATE | vpt.TEMPORAL_MATCH_INSTANCE):
            tp = vpt.default_temporal_params(flags=flags)
            g.temporal_reset()
            frames, got = [], []
            for view_inv in camera_path(sc):
                g.set_camera(view_inv, proj_inv)
                g.render(2)
                f = g.render_features(0, 0)
                frames.append(TH.Frame(view_inv, proj_inv, 2, g.radiance(), f["normal"], f["albedo"], f["depth"], f["ids"][..., 0]))
                image = g.temporal_accumulate(tp)
                got.append((image, g.temporal_history()))
            want = TH.run_sequence(driver[0], driver[1], frames, tag="bits", flags=flags, max_history=tp.max_history, depth_tolerance=tp.depth_tolerance,
                                   normal_threshold=tp.normal_threshold, focus_distance=focus, dof_strength=0.0)
            with_history = without = misses = 0
            for k, ((image, length), (w_image, w_record)) in enumerate(zip(got, want)):
                diff = DH.bits(image) != DH.bits(w_image)
                assert not diff.any(), "flags %d, step %d: %d image words differ, first at %r" % (flags, k, diff.sum(), tuple(np.argwhere(diff)[0]))
                diff = DH.bits(length) != DH.bits(w_record[..., 3])
                assert not diff.any(), "flags %d, step %d: %d lengths differ, first at %r" % (flags, k, diff.sum(), tuple(np.argwhere(diff)[0]))
                hit = frames[k].depth >= 0
                assert np.array_equal(DH.bits(image)[~hit], DH.bits(frames[k].radiance)[~hit]) and (w_record[..., 3][~hit] == 0).all()
                if k:
                    with_history += int((w_record[..., 3][hit] > 2).sum()); without += int((w_record[..., 3][hit] == 2).sum()); misses += int((~hit).sum())
                else:
                    assert (w_record[..., 3][hit] == 2).all()
            assert with_history > 50 and without > 20 and misses > 20, (with_history, without, misses)
            assert np.abs(got[1][0][..., :3] - frames[1].radiance[..., :3]).max() > 0      # ... and it blended
    finally:
        g.close()


# ---- 2. it disturbs nothing
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
                a = g.temporal_accumulate()
                dev = torch.zeros((h, w, 4), device="cuda:0")
                g.temporal_reset()                       # (the second call is to see what the first saw: no history)
                g.temporal_accumulate_device(None, dev.data_ptr())
                g.wait()
                assert np.array_equal(dev.cpu().numpy(), a) and (a[..., :3] > 0).any()
                assert g.temporal_history().max() == 3
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


# ---- 3. the history survives and is dropped as specified
def test_history_survives_the_camera_and_is_dropped_by_edits(vpt):
    sc = copy.deepcopy(feature_scene(vpt, "cornell_gltf"))
    w, h = 45, 37
    m = 2
    g = context(vpt, sc, w, h, frames=m)
    views = camera_path(sc)

    def accumulate():
        g.temporal_accumulate()
        return g.temporal_history(), hits_of(g)

    def assert_fresh(what):
        length, hit = accumulate()
        assert hit.any() and (length[hit] == m).all() and (length[~hit] == 0).all(), what

    def assert_carried(what):
        length, hit = accumulate()
        assert (length[hit] > m).sum() > 50 and length.max() <= 32, what
    try:
        assert_fresh("the first call")
        g.set_camera(views[1], sc.projection_inverse(w / h)); g.render(m)
        assert_carried("vpt_set_camera")
        g.reset(); g.render(m)
        assert_carried("vpt_reset")
        g.denoise(); g.render_features(0, 0); g.pick(3, 3); g.postprocess()
        g.reset(); g.render(m)
        assert_carried("vpt_denoise, vpt_render_features, vpt_pick, vpt_postprocess")
        mat = g.get_material(1)
        edits = [("vpt_set_material", lambda: g.set_material(1, mat)),
                 ("vpt_set_instance_transforms", lambda: g.set_instance_transforms(0, [sc.instances[0][2]])),
                 ("vpt_set_environment", lambda: g.set_environment(vpt.scenes.constant_env((0.5, 0.5, 0.5)))),
                 ("vpt_set_params", lambda: g.set_params(vpt.default_params(max_depth=3))),
                 ("vpt_temporal_reset", lambda: (g.temporal_reset(), g.reset()))]
        for what, edit in edits:
            edit(); g.render(m)
            assert_fresh(what)
            g.reset(); g.render(m)
            assert_carried("the call after " + what)
        g.set_radiance(g.radiance(), m)
        assert_fresh("vpt_set_radiance")
        g.reset(); g.render(m)
        assert_carried("the call after vpt_set_radiance")
        g.resize(w + 3, h)
        g.set_camera(views[1], sc.projection_inverse((w + 3) / h)); g.render(m)
        length, hit = accumulate()
        assert length.shape == (h, w + 3) and (length[hit] == m).all(), "vpt_resize"
        tp = vpt.default_temporal_params(max_history=1)        # min(m, max_history)
        g.temporal_reset(); g.temporal_accumulate(tp)
        assert (g.temporal_history()[hit] == 1).all()
    finally:
        g.close()


# ---- 4. the denoise source
def test_denoise_source(vpt, driver, tmp_path_factory):
    sc = feature_scene(vpt, "cornell_gltf")
    w, h = 45, 37
    g = context(vpt, sc, w, h)
    never = context(vpt, sc, w, h)
    other = context(vpt, sc, w, h, frames=0)
    d = tmp_path_factory.mktemp("temporal_denoise")
    dn_exe = DH.compile_driver(str(d / "denoise_driver"))
    try:
        plain = never.denoise()
        g.set_denoise_source(vpt.DENOISE_SOURCE_TEMPORAL)
        for call in (g.denoise, g.denoise_device):
            with pytest.raises(vpt.VptError, match=INVALID):
                call()                                           # no temporal image yet
        g.temporal_accumulate()
        g.set_camera(camera_path(sc)[1], sc.projection_inverse(w / h)); g.render(2)
        timg = g.temporal_accumulate()
        assert not np.array_equal(timg, g.radiance())
        assert np.array_equal(DH.bits(g.denoise(vpt.default_denoise_params(iterations=0))), DH.bits(timg))
        f = g.render_features(0, 0, which=("depth", "normal", "albedo"))
        dp = vpt.default_denoise_params(iterations=3)
        want = DH.run_driver(dn_exe, d, timg, f["normal"], f["albedo"], f["depth"], 3, dp.sigma_color, dp.sigma_normal, dp.sigma_depth, dp.flags, tag="t")
        assert np.array_equal(DH.bits(g.denoise(dp)), DH.bits(want))
        # the post chain reaches the temporal image through a zero-iteration denoise
        g.denoise(vpt.default_denoise_params(iterations=0))
        g.set_post_source(vpt.POST_SOURCE_DENOISED)
        other.set_radiance(timg, 2)
        assert np.array_equal(g.postprocess(), other.postprocess())
        g.set_post_source(vpt.POST_SOURCE_RADIANCE)
        # the default source, after temporal calls: what a context that never made one returns
        g.set_denoise_source(vpt.DENOISE_SOURCE_RADIANCE)
        g.set_camera(sc.view_inverse, sc.projection_inverse(w / h)); g.render(2)
        assert np.array_equal(DH.bits(g.denoise()), DH.bits(plain))
        g.set_denoise_source(vpt.DENOISE_SOURCE_TEMPORAL)
        g.resize(w + 3, h); g.render(1)
        with pytest.raises(vpt.VptError, match=INVALID):
            g.denoise()                                          # resized since
        g.temporal_accumulate()
        assert g.denoise().shape == (h, w + 3, 4)
    finally:
        g.close(); never.close(); other.close()


# ---- 5. device pointer, ticket, shards
def test_device_pointer_ticket_and_shards(vpt):
    sc = feature_scene(vpt, "textured_boxes")
    w, h = 45, 37
    g = context(vpt, sc, w, h)
    try:
        want = g.temporal_accumulate()
        g.temporal_reset()
        dev = torch.full((h, w, 4), 7.0, device="cuda:0")
        t = g.temporal_accumulate_device(None, dev.data_ptr())
        assert t > 0
        g.wait(t)
        assert np.array_equal(DH.bits(dev.cpu().numpy()), DH.bits(want))
        t2 = g.temporal_accumulate_device(vpt.default_temporal_params(max_history=4), None)     # no copy asked for: the image stays in the context
        assert t2 > t
        g.wait()
        assert g.temporal_history().max() == 4
    finally:
        g.close()
    parts = [context(vpt, sc, w, h, shard_rank=r, shard_count=2) for r in range(2)]
    hip = C.CDLL("libamdhip64.so")
    buf = C.c_void_p()
    try:
        for f in (parts[0].temporal_accumulate, lambda: parts[0].temporal_accumulate_device(None, None)):
            with pytest.raises(vpt.VptError, match=INVALID):
                f()                                            # a sharded context before vpt_assemble_shards
        n = parts[0].shard_floats()
        assert hip.hipMalloc(C.byref(buf), n * 4 * 2) == 0
        for r, s in enumerate(parts):
            s.shard_to_device(C.c_void_p(buf.value + r * n * 4))
        parts[0].assemble_shards(buf, 2)
        assert np.array_equal(DH.bits(parts[0].temporal_accumulate()), DH.bits(want))
    finally:
        if buf.value:
            hip.hipFree(buf)
        for s in parts:
            s.close()


# ---- 6. quality
def test_history_lowers_the_error_of_a_moving_1_spp_viewport(vpt, scenes):
    """Cornell box, 64 x 48, depth 4; eight camera positions on a short arc about the centre of the scene's bounding box (an orbit: 1 degree per step, 7 in
    all, ending at the scene's own camera), render(1) and one temporal call after each move; the reference is 1024 spp at the last camera.  Relative L2 over
    the pixels whose first hit is not emissive (the lamp's own pixels are noise-free and 1000 x brighter: they would govern a whole-image figure).
    Measured on an MI355X with the defaults:
      first hit not emissive (1864 pixels)            1 spp 0.6328, temporal 0.6032, ratio 0.953     <- the condition
      ... and 2 pixels or more from an emissive hit   1 spp 0.5129, temporal 0.4743, ratio 0.925     (1808 pixels; asserted as well)
      whole image                                     1 spp 0.4943, temporal 0.4068, ratio 0.823     mean history length 7.55
    Why the gain is this small: every vpt_set_camera restarts the accumulation at dispatch 0, so every frame of a moving viewport draws the same random numbers
    per pixel; the noise is locked to the screen, an orbit moves the surfaces under it by less than half a pixel per step, and what the history averages
    is nearly the same noise eight times.
    What the condition is sensitive to: a path that sweeps the lamp's edge over the pixel grid.  With the same 1 degree per step about a point only 10 units
    ahead — in front of the box, so the whole box pans by a pixel per step — the first figure is 0.7161 against 0.6328 (the second 0.3180 against 0.5129, the
    whole image 0.1665 against 0.4943): 78 % of that error sits in ten pixels along the lamp's edge, whose CENTER ray hits the ceiling (same instance, same
    plane: every tap test passes) while their jittered samples cover the lamp by a few per cent of radiance 50, by how much changing from frame to frame;
    the blend as specified has no colour clamp that could reject such a tap.  DESIGN.md section 9 has both sets of figures."""
    sc = scenes("cornell_box")
    w, h = 64, 48
    g = context(vpt, sc, w, h, frames=1024)
    try:
        ref = g.radiance()[..., :3].astype(np.float64)
        f = g.render_features(0, 0, which=("ids", "depth"))
        emissive = np.array([max(m["emissive_color"]) > 0 for m in sc.materials])
        hit = f["depth"] >= 0
        mask = hit & ~emissive[np.where(hit, f["ids"][..., 2], 0)]
        assert mask.sum() > 0.5 * w * h and (hit & ~mask).sum() > 5      # most of the image, and the lamp is in view
        v0 = np.asarray(sc.view_inverse, np.float64)
        # the arc's centre: the centre of the scene's bounding box, as far ahead of the camera as it lies along the view direction (20.85 units)
        corners = np.array([f(np.asarray(sc.meshes[mesh][0]["position"], np.float64) @ np.asarray(xf, np.float64)[:3, :3].T + np.asarray(xf, np.float64)[:3, 3], axis=0)
                            for mesh, _, xf in sc.instances for f in (np.min, np.max)])
        centre = (corners.min(0) + corners.max(0)) / 2
        ahead = float(-(np.linalg.inv(v0) @ np.append(centre, 1.0))[2])
        assert 15.0 < ahead < 25.0
        for k in range(8):
            g.set_camera((v0 @ shift(0, 0, -ahead) @ rot_y(k - 7.0) @ shift(0, 0, ahead)).astype(np.float32), sc.projection_inverse(w / h))
            g.render(1)
            temporal = g.temporal_accumulate()[..., :3].astype(np.float64)
        noisy = g.radiance()[..., :3].astype(np.float64)
        length = g.temporal_history()
        assert g.stats()["frames"] == 1
    finally:
        g.close()
    # 2 pixels or more (in x and in y) from every pixel whose first hit is emissive: half a pixel of jitter and one pixel of bilinear footprint, rounded up
    near = np.zeros((h, w), bool)
    lamp = hit & ~mask
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            near[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] |= lamp[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
    away = mask & ~near
    err = lambda a, m: float(np.sqrt(((a - ref)[m] ** 2).sum() / (ref[m] ** 2).sum()))
    everything = np.ones((h, w), bool)
    for what, m in (("first hit not emissive", mask), ("... and 2 pixels or more from an emissive hit", away), ("whole image", everything)):
        print("relative L2 error against 1024 spp, %s (%d pixels): 1 spp %.4f, temporal %.4f, ratio %.3f" % (what, m.sum(), err(noisy, m), err(temporal, m), err(temporal, m) / err(noisy, m)))
    print("mean history length %.2f" % float(length[hit].mean()))
    assert np.isfinite(temporal).all()
    assert err(temporal, away) < err(noisy, away)
    assert err(temporal, mask) < err(noisy, mask)


# ---- 7. errors
def test_errors_leave_the_context_usable(vpt, oracle, scenes):
    sc = scenes("cornell_box")
    w, h = 32, 24
    P = vpt.default_params(max_depth=4)
    o = oracle.Oracle(sc, w, h); o.set_params(P); o.render(2); ref = o.radiance(); o.close()
    lib = vpt.load_library()
    g = vpt.PathTracer(w, h)
    try:
        ok = vpt.default_temporal_params()
        with pytest.raises(vpt.VptError, match=NO_SCENE):
            g.temporal_accumulate()
        with pytest.raises(vpt.VptError, match=NO_SCENE):
            g.temporal_accumulate_device()
        g.set_scene(sc); g.set_params(P)
        for call in (g.temporal_accumulate, g.temporal_accumulate_device):
            with pytest.raises(vpt.VptError, match=INVALID):
                call()                                          # nothing rendered since the last reset
        with pytest.raises(vpt.VptError, match=INVALID):
            g.temporal_history()                                # no result yet
        g.render(2)
        first = g.temporal_accumulate()
        length = g.temporal_history()
        assert lib.vpt_temporal_accumulate(g.ctx, None, None) == -1 and lib.vpt_temporal_accumulate(None, C.byref(ok), None) == -1
        assert lib.vpt_temporal_accumulate_device(g.ctx, None, None, None) == -1 and lib.vpt_temporal_accumulate_device(None, C.byref(ok), None, None) == -1
        assert lib.vpt_temporal_reset(None) == -1 and lib.vpt_get_temporal_history(None, None) == -1 and lib.vpt_get_temporal_history(g.ctx, None) == -1
        bad = [dict(max_history=0), dict(depth_tolerance=0.0), dict(depth_tolerance=float("nan")), dict(normal_threshold=1.5), dict(normal_threshold=-1.01),
               dict(normal_threshold=float("nan")), dict(flags=4), dict(flags=0x80000001), dict(reserved=(1, 0)), dict(reserved=(0, 7))]
        for kw in bad:
            for call in (g.temporal_accumulate, g.temporal_accumulate_device):
                with pytest.raises(vpt.VptError, match=INVALID):
                    call(vpt.default_temporal_params(**kw))
        dev = torch.zeros(w * h * 4 + 4, device="cuda:0")
        with pytest.raises(vpt.VptError, match=INVALID):
            g.temporal_accumulate_device(ok, dev.data_ptr() + 4)          # not 16-byte aligned
        with pytest.raises(vpt.VptError, match=INVALID):
            g.set_denoise_source(2)
        assert lib.vpt_set_denoise_source(None, 0) == -1
        # the previous result and history are still valid ...
        assert np.array_equal(g.temporal_history(), length)
        g.set_denoise_source(vpt.DENOISE_SOURCE_TEMPORAL)
        assert np.array_equal(DH.bits(g.denoise(vpt.default_denoise_params(iterations=0))), DH.bits(first))
        g.set_denoise_source(vpt.DENOISE_SOURCE_RADIANCE)
        g.reset(); g.render(2)
        g.temporal_accumulate(vpt.default_temporal_params(normal_threshold=-1.0, depth_tolerance=1e9))   # the widest settings are accepted
        assert g.temporal_history().max() == 4
        # ... and the context renders bit-exact
        g.reset()
        g.render(2)
        assert np.array_equal(g.radiance(), ref)
    finally:
        g.close()
