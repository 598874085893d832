"""vpt_set_temporal_options / vpt_get_temporal_options / vpt_get_temporal_motion on the device: the temporal history carried across instance moves.  The kernel
calls csrc/temporal.hpp's temporal_pixel_motion, so image, history length, motion, moments and variance are held BIT FOR BIT to a host compile of that header
(tests/tools/motion_driver.cpp) fed the context's own radiance and guide images of every step and the matrices the instances were given; the arithmetic itself
is held to float64 by tests/test_motion_cpu.py.  Then: the device form, a move that moves nothing, the option off, when the history survives and when it is
dropped, every error code, that carrying the history lowers the error on a moving object, and the C++ facade.

Quality, measured on an MI355X (Cornell box with a box on its floor, 64 x 48, depth 4, the box moved by 0.35 — a pixel is 0.36 there — per step over 8 steps, 1 spp per step,
against 1024 spp at the last pose, relative L2 over the box's pixels): option off 0.9890 (every move drops the history: the raw 1-spp error, mean history length 1),
option on 0.3352 (mean history length 8.92 of 9): ratio 0.3389."""
import copy
import os
import subprocess

import numpy as np
import pytest
import torch   # before the first context exists (see tests/test_gpu_features.py)

import denoise_host as DH
import motion_host as MH
import refit_moves as RM
from test_gpu_features import scene as feature_scene
from test_host_cpp import GOLDEN, HOST, LUTS, ROOT, cli  # noqa: F401  (the fixture that builds the facade library)

pytestmark = pytest.mark.gpu
INVALID = "VPT_ERR_INVALID_ARGUMENT"
FLAG_LOCAL_HITS = 256
M = 2            # frames per step
QUALITY_RATIO = 0.3389    # on / off, measured (the module's docstring); asserted: on <= off (1 + ratio) / 2, halfway between the measured ratio and no gain


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("motion_gpu")
    return MH.compile_driver(str(d / "motion_driver")), d


def context(vpt, sc, w, h, frames=M, motion=1, **cfg):
    g = vpt.PathTracer(w, h, **cfg)
    g.set_scene(sc)
    P = vpt.default_params(max_depth=4)
    P.flags |= FLAG_LOCAL_HITS
    g.set_params(P)
    if motion is not None:
        g.set_temporal_options(instance_motion=motion)
    if frames:
        g.render(frames)
    return g


def start_of(sc):
    return np.stack([np.asarray(x, np.float32) for _, _, x in sc.instances])


def world(sc, i, W):
    """The instance's own matrix under the world transform W, float32."""
    return (np.asarray(W, np.float64) @ np.asarray(sc.instances[i][2], np.float64)).astype(np.float32)


def camera_moved(sc):
    """A sideways translation and a pan of 10 degrees that pushes part of the view out of the image (what comes in has no history)."""
    m = np.eye(4); m[:3, 3] = (0.5, 0.15, 0.0)
    c, sn = np.cos(np.radians(10.0)), np.sin(np.radians(10.0))
    r = np.eye(4); r[0, 0], r[0, 2], r[2, 0], r[2, 2] = c, sn, -sn, c
    return (np.asarray(sc.view_inverse, np.float64) @ m @ r).astype(np.float32)


MOVER = 2        # the back wall: many pixels from either camera


def mover_a(sc):
    return world(sc, MOVER, RM.translate(0.9, 0.5, 0.0))


def steps_of(sc):
    """(inverse view matrix, [vpt_set_instance_transforms calls]) per step, instance 5 being the lamp and 2 the back wall (refit_moves): nothing; the lamp moved
    under a still camera; the camera moved and two instances with it, the lamp by a non-uniform scale; two calls before one temporal call, the second of which
    moves the wall back where it started; no move."""
    v0, v1 = np.asarray(sc.view_inverse, np.float32), camera_moved(sc)
    lamp_a = world(sc, RM.LAMP, RM.translate(0.9, 0.5, -0.6))
    lamp_b = world(sc, RM.LAMP, RM.CORNELL_LAMP[RM.LAMP])
    wall_b = world(sc, 2, RM.CORNELL_WALL[2])
    lamp_c = world(sc, RM.LAMP, RM.about((0.0, -5.65, -5.84), RM.rotate((0.0, 1.0, 0.0), 20.0)))
    return [(v0, []), (v0, [(RM.LAMP, [lamp_a])]), (v1, [(2, [wall_b]), (RM.LAMP, [lamp_b])]), (v1, [(RM.LAMP, [lamp_a]), (2, [np.asarray(sc.instances[2][2], np.float32), ]), (RM.LAMP, [lamp_c])]),
            (v1, [])]


def walk(g, sc, w, h, tp, steps, device=False):
    """Every step on the context -> (frames for the driver, what the context answered per step)."""
    proj_inv = sc.projection_inverse(w / h)
    frames, got = [], []
    for view_inv, moves in steps:
        for first, mats in moves:
            g.set_instance_transforms(first, mats)
        g.set_camera(view_inv, proj_inv)
        g.render(M)
        f = g.render_features(0, 0)
        frames.append(MH.Frame(view_inv, proj_inv, M, g.radiance(), f["normal"], f["albedo"], f["depth"], f["ids"][..., 0], moves=moves))
        if device:
            dev = torch.zeros((h, w, 4), device="cuda:0")
            g.temporal_accumulate_device(tp, dev.data_ptr())
            g.wait()
            image = dev.cpu().numpy()
        else:
            image = g.temporal_accumulate(tp)
        got.append(dict(image=image, length=g.temporal_history(), motion=g.temporal_motion()))
    return frames, got


# ---- 1. device == host compile, bit for bit
@pytest.mark.parametrize("variance", [0, 1], ids=["variance_off", "variance_on"])
@pytest.mark.parametrize("w,h", [(45, 37), (150, 9)], ids=["45x37", "150x9"])
def test_device_equals_the_host_compile_bit_for_bit(vpt, driver, w, h, variance):
    """45 x 37: partial tiles on both edges.  150 x 9: three tiles across with a partial last one.  The Cornell box seen from outside (walls, lamp and misses), six
    instances, VPT_FLAG_LOCAL_HITS, 2 frames per step, the steps of steps_of, every flag set; the driver is fed what the context itself reports of each step."""
    sc = copy.deepcopy(feature_scene(vpt, "cornell_gltf"))
    assert len(sc.instances) >= 3
    g = context(vpt, sc, w, h, frames=0)
    focus = vpt.default_params().focus_distance
    start = start_of(sc)
    try:
        g.set_svgf_options(variance=variance)
        for flags in (0, vpt.TEMPORAL_DEMODULATE, vpt.TEMPORAL_MATCH_INSTANCE, vpt.TEMPORAL_DEMODULATE | vpt.TEMPORAL_MATCH_INSTANCE):
            tp = vpt.default_temporal_params(flags=flags)
            g.set_instance_transforms(0, list(start))
            g.temporal_reset()
            frames, got = [], []
            proj_inv = sc.projection_inverse(w / h)
            for view_inv, moves in steps_of(sc):
                for first, mats in moves:
                    g.set_instance_transforms(first, mats)
                g.set_camera(view_inv, proj_inv)
                g.render(M)
                f = g.render_features(0, 0)
                frames.append(MH.Frame(view_inv, proj_inv, M, g.radiance(), f["normal"], f["albedo"], f["depth"], f["ids"][..., 0], moves=moves))
                r = dict(image=g.temporal_accumulate(tp), length=g.temporal_history(), motion=g.temporal_motion())
                if variance:
                    r.update(moments=g.temporal_moments(), variance=g.temporal_variance())
                got.append(r)
            want = MH.run_sequence(driver[0], driver[1], frames, start, tag="bits", flags=flags, max_history=tp.max_history, depth_tolerance=tp.depth_tolerance,
                                   normal_threshold=tp.normal_threshold, focus_distance=focus, dof_strength=0.0, variance=variance, min_history=g.svgf_options().min_history)
            assert [r["table"] for r in want] == [False, True, True, True, False]
            assert list(want[1]["state"]) == [0, 0, 0, 0, 0, 1] and list(want[2]["state"]) == [0, 0, 1, 0, 0, 1] and list(want[3]["state"]) == [0, 0, 1, 0, 0, 1]
            carried = fresh = misses = 0
            for k, (r, wr) in enumerate(zip(got, want)):
                for what in r:
                    a, b = DH.bits(r[what]), DH.bits(wr["record"][..., 3] if what == "length" else wr[what])
                    diff = a != b
                    assert not diff.any(), "flags %d, step %d, %s: %d words differ, first at %r" % (flags, k, what, diff.sum(), tuple(np.argwhere(diff)[0]))
                hit = frames[k].depth >= 0
                moved = np.isin(frames[k].inst, np.nonzero(wr["state"] == 1)[0]) & hit
                carried += int((r["length"][moved] > M).sum()); fresh += int((r["length"][hit] == M).sum()) if k else 0; misses += int((~hit).sum())
                if k in (1, 2, 3) and moved.any():
                    assert np.abs(r["motion"][moved]).max() > 0.1
            print("flags", flags, "moved and carried", carried, "fresh", fresh, "misses", misses)
            # (at 150 x 9 the box is 9 pixels tall: some 50 hit pixels per step)
            assert carried > (50 if h > 9 else 10) and fresh > (20 if h > 9 else 10) and misses > 20, (carried, fresh, misses)
    finally:
        g.close()


# ---- 2. the device form
def test_the_device_form_gives_the_blocking_forms_bits(vpt):
    """The same steps with vpt_temporal_accumulate_device, and then a second call enqueued right behind the first — it finds the first's record, whose table is
    the one it must not overwrite, and counts the same frames again: the bits of two blocking calls."""
    sc = copy.deepcopy(feature_scene(vpt, "cornell_gltf"))
    w, h = 45, 37
    tp = vpt.default_temporal_params()
    results = {}
    for device in (False, True):
        g = context(vpt, sc, w, h, frames=0)
        try:
            _, got = walk(g, sc, w, h, tp, steps_of(sc)[:3], device=device)
            g.set_instance_transforms(RM.LAMP, [np.asarray(sc.instances[RM.LAMP][2], np.float32)])
            g.render(M)
            if device:
                a, b = torch.zeros((h, w, 4), device="cuda:0"), torch.zeros((h, w, 4), device="cuda:0")
                g.temporal_accumulate_device(tp, a.data_ptr())
                g.temporal_accumulate_device(tp, b.data_ptr())
                g.wait()
                pair = (a.cpu().numpy(), b.cpu().numpy())
            else:
                pair = (g.temporal_accumulate(tp), g.temporal_accumulate(tp))
            results[device] = (got, pair, g.temporal_history(), g.temporal_motion())
        finally:
            g.close()
    (got0, pair0, len0, mv0), (got1, pair1, len1, mv1) = results[False], results[True]
    for a, b in zip(got0, got1):
        for what in a:
            assert np.array_equal(DH.bits(a[what]), DH.bits(b[what])), what
    assert np.array_equal(DH.bits(pair0[0]), DH.bits(pair1[0])) and np.array_equal(DH.bits(pair0[1]), DH.bits(pair1[1]))
    assert np.array_equal(DH.bits(len0), DH.bits(len1)) and np.array_equal(DH.bits(mv0), DH.bits(mv1))
    assert not np.array_equal(pair0[0], pair0[1]) and len0.max() > 3 * M


# ---- 3. a move that moves nothing
def test_the_matrices_the_instances_already_have_carry_the_history(vpt):
    """Option on, vpt_set_instance_transforms with the installed matrices: the history is carried, and the temporal image is, bit for bit, that of a twin context
    that called vpt_reset instead (VPT_FLAG_LOCAL_HITS: the refitted tree reports the hits of the built one)."""
    sc = copy.deepcopy(feature_scene(vpt, "cornell_gltf"))
    w, h = 45, 37
    out = []
    for move in (True, False):
        g = context(vpt, sc, w, h)
        try:
            g.temporal_accumulate()
            if move:
                g.set_instance_transforms(0, list(start_of(sc)))
            else:
                g.reset()
            g.render(M)
            image = g.temporal_accumulate()
            out.append((image, g.temporal_history(), g.temporal_motion()))
            hit = g.render_features(0, 0, which=("depth",))["depth"] >= 0
            assert (out[-1][1][hit] == 2 * M).all() and hit.sum() > 50
        finally:
            g.close()
    for a, b in zip(*out):
        assert np.array_equal(DH.bits(a), DH.bits(b))


# ---- 4. the option off
def test_with_the_option_off_a_move_drops_the_history_and_the_motion_is_refused(vpt):
    sc = copy.deepcopy(feature_scene(vpt, "cornell_gltf"))
    w, h = 45, 37
    g = context(vpt, sc, w, h, motion=0)
    try:
        g.temporal_accumulate()
        with pytest.raises(RuntimeError, match=INVALID):
            g.temporal_motion()
        g.reset(); g.render(M); g.temporal_accumulate()
        hit = g.render_features(0, 0, which=("depth",))["depth"] >= 0
        assert (g.temporal_history()[hit] == 2 * M).all()
        g.set_instance_transforms(MOVER, [mover_a(sc)])
        g.render(M); g.temporal_accumulate()
        hit = g.render_features(0, 0, which=("depth",))["depth"] >= 0
        assert hit.sum() > 50 and (g.temporal_history()[hit] == M).all()
        with pytest.raises(RuntimeError, match=INVALID):
            g.temporal_motion()
    finally:
        g.close()


# ---- 5. bookkeeping with the option on
def test_what_keeps_and_what_drops_the_history_with_the_option_on(vpt):
    sc = copy.deepcopy(feature_scene(vpt, "cornell_gltf"))
    w, h = 45, 37
    g = context(vpt, sc, w, h)
    proj_inv = sc.projection_inverse(w / h)
    moved_a = mover_a(sc)
    moved_0 = np.asarray(sc.instances[MOVER][2], np.float32)

    def accumulate():
        g.temporal_accumulate()
        return g.temporal_history(), g.render_features(0, 0, which=("depth",))["depth"] >= 0, g.temporal_motion()

    def assert_fresh(what):
        length, hit, motion = accumulate()
        assert hit.any() and (length[hit] == M).all() and (length[~hit] == 0).all() and not motion.any(), what

    def assert_carried(what):
        length, hit, _ = accumulate()
        assert (length[hit] > M).sum() > 50 and length.max() <= 32, what
    try:
        assert_fresh("the first call")
        for what, keep in (("vpt_set_camera", lambda: g.set_camera(camera_moved(sc), proj_inv)), ("vpt_reset", g.reset), ("vpt_set_base_seed", lambda: g.set_base_seed(7)),
                           ("a move", lambda: g.set_instance_transforms(MOVER, [moved_a])), ("a move back", lambda: g.set_instance_transforms(MOVER, [moved_0]))):
            keep(); g.render(M)
            assert_carried(what)
        # a rejected move — its range runs past the instance count — changes nothing: the accumulation is not even restarted
        before = g.stats()["frames"]
        with pytest.raises(RuntimeError, match=INVALID):
            g.set_instance_transforms(len(sc.instances) - 1, [moved_a, moved_a])
        assert g.stats()["frames"] == before
        g.reset(); g.render(M)
        assert_carried("a rejected move")
        mat = g.get_material(1)
        P3 = vpt.default_params(max_depth=3); P3.flags |= FLAG_LOCAL_HITS
        drops = [("vpt_set_material", lambda: g.set_material(1, mat)), ("vpt_set_environment", lambda: g.set_environment(vpt.scenes.constant_env((0.5, 0.5, 0.5)))),
                 ("vpt_set_params", lambda: g.set_params(P3)), ("vpt_temporal_reset", lambda: (g.temporal_reset(), g.reset())),
                 ("the option off", lambda: g.set_temporal_options(instance_motion=0)), ("the option on", lambda: g.set_temporal_options(instance_motion=1))]
        for what, drop in drops:
            g.set_instance_transforms(MOVER, [moved_a])      # a snapshot the drop must forget: the instance is back before the next record
            drop()
            g.set_instance_transforms(MOVER, [moved_0]); g.render(M)
            if what == "the option off":
                g.temporal_accumulate()
                with pytest.raises(RuntimeError, match=INVALID):
                    g.temporal_motion()
                continue
            assert_fresh(what)
            g.reset(); g.render(M)
            assert_carried("the call after " + what)
        # the same value again changes nothing
        g.set_temporal_options(instance_motion=1); g.reset(); g.render(M)
        assert_carried("the option set to the value it has")
        # vpt_set_scene: no stale snapshot — an instance of the OLD scene was moved, the new scene's instances are where it puts them
        g.set_instance_transforms(MOVER, [moved_a])
        g.set_scene(sc); g.render(M)
        assert_fresh("vpt_set_scene")
        g.set_instance_transforms(MOVER, [moved_a]); g.render(M)
        length, hit, motion = accumulate()
        ids = g.render_features(0, 0, which=("ids",))["ids"][..., 0]
        assert (length[hit & (ids == MOVER)] > M).sum() > 20 and np.abs(motion[ids == MOVER]).max() > 0.5
        assert np.abs(motion[hit & (ids != MOVER)]).max() < 1e-2      # (a still camera: what did not move is where it was, to rounding)
        g.resize(w + 3, h)
        g.set_camera(np.asarray(sc.view_inverse, np.float32), sc.projection_inverse((w + 3) / h)); g.render(M)
        length, hit, motion = accumulate()
        assert length.shape == (h, w + 3) and motion.shape == (h, w + 3, 2) and (length[hit] == M).all(), "vpt_resize"
    finally:
        g.close()


# ---- 6. errors and defaults
def test_errors_and_defaults(vpt):
    import ctypes as C
    sc = feature_scene(vpt, "cornell_gltf")
    g = vpt.PathTracer(16, 12)
    try:
        o = g.temporal_options()
        assert (o.instance_motion, list(o.reserved)) == (0, [0, 0, 0])          # off by default, before a scene too
        g.set_temporal_options(instance_motion=1)                               # context state: needs no scene
        assert g.temporal_options().instance_motion == 1
        with pytest.raises(RuntimeError, match=INVALID):
            g.set_temporal_options(instance_motion=2)
        bad = vpt.default_temporal_options(instance_motion=0); bad.reserved[2] = 1
        assert g.lib.vpt_set_temporal_options(g.ctx, C.byref(bad)) == -1
        assert g.temporal_options().instance_motion == 1                        # a refused call changes nothing
        assert g.lib.vpt_set_temporal_options(g.ctx, None) == -1 and g.lib.vpt_get_temporal_options(g.ctx, None) == -1
        assert g.lib.vpt_get_temporal_motion(g.ctx, None) == -1
        with pytest.raises(RuntimeError, match=INVALID):
            g.temporal_motion()                                                 # no temporal result yet
        g.set_scene(sc); g.set_params(vpt.default_params(max_depth=2)); g.render(1)
        g.temporal_accumulate()
        assert g.temporal_motion().shape == (12, 16, 2) and not g.temporal_motion().any()
        g.resize(20, 12)
        with pytest.raises(RuntimeError, match=INVALID):
            g.temporal_motion()                                                 # no result of the current size
    finally:
        g.close()


# ---- 7. quality: a moving object keeps its history
def box_scene(vpt, scenes):
    """The Cornell box (y points down: the floor is y = 5.55) with a box of side 3 standing on its floor, left of the middle — instance 6."""
    S = vpt.scenes
    sc = copy.deepcopy(scenes("cornell_box"))
    faces = [((1, 0, 0), (0, 1, 0), (0, 0, 1)), ((-1, 0, 0), (0, 0, 1), (0, 1, 0)), ((0, 1, 0), (0, 0, 1), (1, 0, 0)), ((0, -1, 0), (1, 0, 0), (0, 0, 1)), ((0, 0, 1), (1, 0, 0), (0, 1, 0)),
             ((0, 0, -1), (0, 1, 0), (1, 0, 0))]
    pos, nrm, idx = [], [], []
    for n, u, v in faces:
        n, u, v = (np.asarray(a, np.float32) for a in (n, u, v))
        base = len(pos)
        for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
            pos.append(1.5 * (n + su * u + sv * v)); nrm.append(n)
        idx += [base, base + 1, base + 2, base, base + 2, base + 3]
    sc.materials.append(S.material(base_color=(0.8, 0.7, 0.3)))
    mesh = sc.add_mesh(np.array(pos, np.float32), np.array(nrm, np.float32), np.zeros((len(pos), 2), np.float32), np.array(idx, np.uint32))
    sc.add_instance(mesh, len(sc.materials) - 1, RM.translate(-2.4, 4.05, -6.0) @ RM.rotate((0.0, 1.0, 0.0), 20.0))
    return sc


def test_a_moving_box_keeps_its_history_and_loses_error(vpt, scenes):
    sc = box_scene(vpt, scenes)
    box = len(sc.instances) - 1
    w, h, steps = 64, 48, 8
    poses = [world(sc, box, RM.translate(0.35 * k, 0.0, 0.0)) for k in range(steps + 1)]
    last = RM.with_matrices(sc, {box: poses[-1]})
    g = vpt.PathTracer(w, h)
    try:
        g.set_scene(last); g.set_params(vpt.default_params(max_depth=4)); g.render(1024)
        ref = g.radiance()[..., :3].astype(np.float64)
        mask = g.render_features(0, 0, which=("ids",))["ids"][..., 0] == box
    finally:
        g.close()
    assert mask.sum() > 100
    err, length = {}, {}
    for on in (1, 0):
        g = vpt.PathTracer(w, h)
        try:
            g.set_scene(sc); g.set_params(vpt.default_params(max_depth=4)); g.set_temporal_options(instance_motion=on)
            for k in range(steps + 1):
                if k:
                    g.set_instance_transforms(box, [poses[k]])
                g.set_base_seed(k); g.render(1)
                image = g.temporal_accumulate()[..., :3].astype(np.float64)
            err[on] = float(np.sqrt(((image - ref)[mask] ** 2).sum() / (ref[mask] ** 2).sum()))
            length[on] = float(g.temporal_history()[mask].mean())
        finally:
            g.close()
    print("relative L2 over the box: option on %.4f, off %.4f, ratio %.4f; mean history length on %.2f, off %.2f" % (err[1], err[0], err[1] / err[0], length[1], length[0]))
    assert length[0] == 1.0                        # with the option off every move drops the history: the raw 1-spp error
    assert length[1] > 2.0
    assert err[1] <= err[0] * (1.0 + QUALITY_RATIO) / 2.0


# ---- 8. the C++ facade
def test_facade_carries_the_history_across_a_move(cli, vpt, tmp_path):  # noqa: F811
    exe = str(tmp_path / "facade_motion")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-I" + HOST, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "facade_motion.cpp"),
                           os.path.join(HOST, "libvpt_host.a"), "-o", exe, "-L" + os.path.dirname(HOST), "-lvpt_hip", "-lz", "-Wl,-rpath," + os.path.dirname(HOST), "-Wl,-rpath,/opt/rocm/lib"])
    gltf = os.path.join(GOLDEN, "cornell_box.gltf")
    sc = vpt.scenes.load_gltf(gltf)
    w, h, spp, depth, seed = 45, 37, 2, 4, 9
    moved = mover_a(sc)
    out = [str(tmp_path / n) for n in ("temporal.f32", "motion.f32", "camera.f32")]
    subprocess.check_call([exe, gltf, LUTS, str(w), str(h), str(spp), str(depth), str(seed), str(MOVER)] + ["%r" % float(v) for v in moved.T.reshape(-1)] + out)
    temporal = np.fromfile(out[0], "<f4").reshape(h, w, 4)
    motion = np.fromfile(out[1], "<f4").reshape(h, w, 2)
    cam = np.fromfile(out[2], "<f4").reshape(2, 4, 4)
    g = vpt.PathTracer(w, h)
    try:
        g.set_scene(sc)
        g.set_params(vpt.default_params(max_depth=depth, max_samples=spp))
        g.set_temporal_options(instance_motion=1)
        g.set_camera(cam[0].T, cam[1].T); g.render(spp)
        g.temporal_accumulate()
        g.set_instance_transforms(MOVER, [moved]); g.set_base_seed(seed); g.render(spp)
        want = g.temporal_accumulate()
        ids = g.render_features(0, 0, which=("ids",))["ids"][..., 0]
        assert (g.temporal_history()[ids == MOVER] > spp).sum() > 50         # the history is carried on the moved instance
        assert np.array_equal(DH.bits(g.temporal_motion()), DH.bits(motion))
    finally:
        g.close()
    assert np.array_equal(DH.bits(temporal), DH.bits(want))
    assert (ids == MOVER).sum() > 50 and np.sqrt((motion[ids == MOVER] ** 2).sum(-1)).min() > 0.5
    assert np.abs(motion[ids != MOVER]).max() < 1e-2      # (a still camera: what did not move is where it was, to rounding)
