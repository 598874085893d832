"""The firefly filter on the device: vpt_set_firefly_options and k_firefly ahead of k_temporal and k_denoise_prepare.  The kernel calls csrc/firefly.hpp's
firefly_pixel, so the filtered image and the two counters are held BIT FOR BIT to a host compile of the header (tests/tools/firefly_driver.cpp) fed the
context's own radiance and guide images, with outliers planted through vpt_set_radiance where the tile geometry could go wrong; the arithmetic itself is held
to float64 by tests/test_firefly_cpu.py.  Then: that the two filters really read the filtered image (their own host drivers fed it), that off is off, that the
history and the accumulation image survive, the device / sharded forms, every error code, and which way the error of a 1-spp image goes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch   # before the first context exists (see tests/test_gpu_features.py)

import denoise_host as DH
import firefly_host as FH
import svgf_host as SH
import temporal_host as TH
from test_firefly_abi_cpu import option_cases
from test_gpu_features import scene as feature_scene
from test_gpu_temporal import camera_path, context

pytestmark = pytest.mark.gpu
INVALID = "VPT_ERR_INVALID_ARGUMENT"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUSY = dict(mode=1, radius=1, rank=2, threshold=1.0, floor=0.0)      # every hit pixel above its second-largest neighbour is clamped: a third of a 1-spp image


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("firefly_gpu")
    return dict(dir=d, firefly=FH.compile_driver(str(d / "firefly_driver")), temporal=TH.compile_driver(str(d / "temporal_driver")),
                svgf=SH.compile_driver(str(d / "svgf_driver")), denoise=DH.compile_driver(str(d / "denoise_driver")))


def assert_bits(got, want, what):
    diff = FH.bits(got) != FH.bits(want)
    assert not diff.any(), "%s: %d words differ, first at %r" % (what, diff.sum(), tuple(np.argwhere(diff)[0]))


def host_filter(drivers, rad, f, demodulate, o, tag="ff"):
    return FH.run(drivers["firefly"], drivers["dir"], rad, f["albedo"], f["depth"], tag=tag, radius=o["radius"], rank=o["rank"], threshold=o["threshold"],
                  floor=o["floor"], demodulate=1 if demodulate else 0)


def plant(rad, level=300.0):
    """Spikes where k_firefly's 64 x 4 tiles meet and where the image ends: x = 63 | 64 (and 127 | 128), y = 3 | 4, as 2 x 2 clusters across the tile corner and as
    single pixels along both seams; the four corners; a few pixels of the last row and the last column.  -> the image, the planted mask."""
    h, w = rad.shape[:2]
    out = rad.copy()
    mask = np.zeros((h, w), bool)
    xs = [x for x in (63, 64, 127, 128) if x < w]
    ys = [y for y in (3, 4) if y < h]
    for x in xs:
        for y in ys:
            mask[y, x] = True                              # the cluster across the tile corner
        for y in range(0, h, 5):
            mask[y, x] = True                              # along the vertical seam
    for y in ys:
        for x in range(1, w, 7):
            mask[y, x] = True                              # along the horizontal seam
    for y in (0, h - 1):
        for x in (0, w - 1):
            mask[y, x] = True
    mask[h - 1, ::9] = True
    mask[::3, w - 1] = True
    k = np.arange(h * w, dtype=np.float64).reshape(h, w)
    out[mask, :3] = (level * (1.0 + 0.37 * np.sin(k[mask]))[:, None] * np.array([1.0, 0.8, 0.6])).astype(np.float32)     # (no two planted values equal)
    return out, mask


# ---- 1. device == host compile, bit for bit
@pytest.mark.parametrize("w,h", [(45, 37), (150, 9), (130, 6), (7, 5), (1, 1)], ids=["45x37", "150x9", "130x6", "7x5", "1x1"])
def test_device_equals_the_host_compile_bit_for_bit(vpt, drivers, w, h):
    """45 x 37: partial tiles on both edges.  150 x 9: three tiles across, a height of two tiles and a row.  130 x 6: a last tile two pixels wide — its halo is
    most of what it stages.  7 x 5: an image smaller than a tile plus halo.  1 x 1: no neighbour at all.  A rendered 1-spp image of the textured boxes with
    planted spikes; both radii, every rank, both demodulations; through the temporal call (its flag) and through the denoise call (its own)."""
    sc = feature_scene(vpt, "textured_boxes")
    g = context(vpt, sc, w, h, frames=1)
    try:
        f = g.render_features(0, 0)
        rad, planted = plant(g.radiance())
        g.set_radiance(rad, 1)
        hit = f["depth"] >= 0
        clamped_planted = clamped_total = considered_total = 0
        for radius in (1, 2):
            for rank in (1, 2, 3):
                o = dict(radius=radius, rank=rank, threshold=2.0, floor=1.0)
                g.set_firefly_options(mode=1, **o)
                for demodulate in (True, False):
                    want = host_filter(drivers, rad, f, demodulate, o)
                    for call in ("temporal", "denoise"):
                        if call == "temporal":
                            g.temporal_accumulate(vpt.default_temporal_params(flags=(vpt.TEMPORAL_DEMODULATE if demodulate else 0) | vpt.TEMPORAL_MATCH_INSTANCE))
                        else:
                            g.denoise(vpt.default_denoise_params(iterations=1, flags=vpt.DENOISE_DEMODULATE if demodulate else 0))
                        what = "%s, radius %d, rank %d, demodulate %d" % (call, radius, rank, demodulate)
                        assert_bits(g.firefly_image(), want["image"], what)
                        s = g.firefly_state()
                        assert (s.clamped, s.considered) == (want["n_clamped"], want["n_considered"]), what
                    assert not want["considered"][~hit].any() and np.array_equal(FH.bits(want["image"])[~want["clamped"]], FH.bits(rad)[~want["clamped"]])
                    clamped_planted += int((want["clamped"] & planted).sum()); clamped_total += want["n_clamped"]; considered_total += want["n_considered"]
        assert_bits(g.radiance(), rad, "the accumulation image")
        print("%d x %d: %d hits, %d planted; over 12 settings %d pixels clamped (%d of them planted), %d considered" %
              (w, h, hit.sum(), planted.sum(), clamped_total, clamped_planted, considered_total))
        if (w, h) == (1, 1):
            assert considered_total == 0 and clamped_total == 0
        else:      # (a planted pixel on a miss, or in a cluster at a low rank, stays: at least one per setting must not)
            assert clamped_planted >= (12 if w * h > 100 else 1) and considered_total > clamped_total
    finally:
        g.close()


# ---- 2. the filters read the filtered image
def run_chain(vpt, g, sc, drivers, w, h, views, tp, o):
    """One step per view: 1 frame with a seed of its own, the temporal call -> (frames for the temporal drivers, whose radiance is the HOST-filtered image, what the
    context returned).  The filtered image the context reports is held to the host's in passing."""
    proj_inv = sc.projection_inverse(w / h)
    frames, got = [], []
    for k, view_inv in enumerate(views):
        g.set_camera(view_inv, proj_inv)
        g.set_base_seed(40 + k)
        g.render(1)
        f = g.render_features(0, 0)
        rad = g.radiance()
        image = g.temporal_accumulate(tp)
        ff = host_filter(drivers, rad, f, tp.flags & vpt.TEMPORAL_DEMODULATE, o, tag="chain")
        assert_bits(g.firefly_image(), ff["image"], "step %d: the filtered image" % k)
        assert ff["n_clamped"] > 0.05 * ff["n_considered"]
        frames.append(TH.Frame(view_inv, proj_inv, 1, ff["image"], f["normal"], f["albedo"], f["depth"], f["ids"][..., 0]))
        got.append(dict(image=image, length=g.temporal_history(), moments=g.temporal_moments(), variance=g.temporal_variance()))
    return frames, got


@pytest.mark.parametrize("moving", [False, True], ids=["still", "moving"])
def test_the_temporal_call_reads_the_filtered_image(vpt, drivers, moving):
    """Three steps of 1 frame, a still and a moving camera, SVGF's variance on, the filter busy (threshold 1, floor 0).  The existing drivers — temporal_driver for
    image and history length, svgf_driver for the moments and the variance too — fed the host-filtered image as their radiance give the context's bits: k_temporal
    read ff_out, and nothing else about it changed."""
    sc = feature_scene(vpt, "cornell_gltf")
    w, h = 45, 37
    g = context(vpt, sc, w, h, frames=0)
    try:
        g.set_svgf_options(variance=1, min_history=2)
        g.set_firefly_options(**BUSY)
        tp = vpt.default_temporal_params()
        views = camera_path(sc)[:3] if moving else [camera_path(sc)[0]] * 3
        frames, got = run_chain(vpt, g, sc, drivers, w, h, views, tp, BUSY)
        kw = dict(flags=tp.flags, max_history=tp.max_history, depth_tolerance=tp.depth_tolerance, normal_threshold=tp.normal_threshold,
                  focus_distance=vpt.default_params().focus_distance, dof_strength=0.0)
        plain = TH.run_sequence(drivers["temporal"], drivers["dir"], frames, tag="chain_t", **kw)
        full = SH.run_sequence(drivers["svgf"], drivers["dir"], frames, tag="chain_s", min_history=2, **kw)
        for k in range(3):
            assert_bits(got[k]["image"], plain[k][0], "step %d: image (temporal_driver)" % k)
            assert_bits(got[k]["length"], plain[k][1][..., 3], "step %d: history length (temporal_driver)" % k)
            for name in ("image", "moments", "variance"):
                assert_bits(got[k][name], full[k][name], "step %d: %s (svgf_driver)" % (k, name))
            assert_bits(got[k]["length"], full[k]["record"][..., 3], "step %d: history length (svgf_driver)" % k)
        assert (got[2]["length"] > 1).sum() > 50 and (got[2]["variance"] >= 0).sum() > 50      # a history was blended in, and long enough for a variance
    finally:
        g.close()


@pytest.mark.parametrize("iterations", [1, 3])
def test_the_denoise_call_reads_the_filtered_image(vpt, drivers, iterations):
    """vpt_denoise from the radiance source against denoise_driver fed the host-filtered image, with and without demodulation (the filter's own demodulation
    follows the call's flag).  From the temporal source, and with 0 iterations, the filter does not run: the filtered image and the call count stay."""
    sc = feature_scene(vpt, "textured_boxes")
    w, h = 45, 37
    g = context(vpt, sc, w, h, frames=1)
    try:
        f = g.render_features(0, 0)
        rad = g.radiance()
        g.set_firefly_options(**BUSY)
        for flags in (vpt.DENOISE_DEMODULATE, 0):
            dp = vpt.default_denoise_params(iterations=iterations, flags=flags)
            ff = host_filter(drivers, rad, f, flags & vpt.DENOISE_DEMODULATE, BUSY, tag="dn")
            want = DH.run_driver(drivers["denoise"], drivers["dir"], ff["image"], f["normal"], f["albedo"], f["depth"], iterations, dp.sigma_color, dp.sigma_normal, dp.sigma_depth, flags, tag="dn")
            raw = DH.run_driver(drivers["denoise"], drivers["dir"], rad, f["normal"], f["albedo"], f["depth"], iterations, dp.sigma_color, dp.sigma_normal, dp.sigma_depth, flags, tag="dn_raw")
            got = g.denoise(dp)
            assert_bits(got, want, "%d iterations, flags %d" % (iterations, flags))
            assert_bits(g.firefly_image(), ff["image"], "the filtered image")
            assert (FH.bits(want) != FH.bits(raw)).any() and ff["n_clamped"] > 50
        calls = g.firefly_state().calls
        assert calls == 2
        kept = g.firefly_image()
        assert_bits(g.denoise(vpt.default_denoise_params(iterations=0)), rad, "0 iterations: a copy of the unfiltered source")
        assert g.firefly_state().calls == calls
        temporal = g.temporal_accumulate()                                   # filtered call 3 (demodulated: the temporal default)
        kept = g.firefly_image()
        g.set_denoise_source(vpt.DENOISE_SOURCE_TEMPORAL)
        dp = vpt.default_denoise_params(iterations=iterations)
        want = DH.run_driver(drivers["denoise"], drivers["dir"], temporal, f["normal"], f["albedo"], f["depth"], iterations, dp.sigma_color, dp.sigma_normal, dp.sigma_depth, dp.flags, tag="dn_tp")
        assert_bits(g.denoise(dp), want, "the temporal source is not filtered again")
        assert g.firefly_state().calls == calls + 1
        assert_bits(g.firefly_image(), kept, "the filtered image of the temporal call")
        assert_bits(g.radiance(), rad, "the accumulation image")
    finally:
        g.close()


# ---- 3. off is off
def test_off_is_off(vpt, drivers):
    """Mode 0 with every other field changed: the temporal and the denoise result are what the host drivers of the existing tests make of the UNfiltered image,
    vpt_get_firefly_image refuses, the state is zeros — and the device's free memory does not move across the calls, where the first filtered call of this
    1024 x 1024 context takes 16 MB (both through hipMemGetInfo, 8 MB of slack for whatever else lives on the device)."""
    sc = feature_scene(vpt, "cornell_gltf")
    w, h = 45, 37
    g = context(vpt, sc, w, h, frames=0)
    try:
        g.set_firefly_options(mode=0, radius=2, rank=3, threshold=1.0, floor=0.0)
        tp = vpt.default_temporal_params()
        proj_inv = sc.projection_inverse(w / h)
        frames, got = [], []
        for k, view_inv in enumerate(camera_path(sc)[:2]):
            g.set_camera(view_inv, proj_inv); g.render(2)
            f = g.render_features(0, 0)
            rad = g.radiance()
            frames.append(TH.Frame(view_inv, proj_inv, 2, rad, f["normal"], f["albedo"], f["depth"], f["ids"][..., 0]))
            got.append((g.temporal_accumulate(tp), g.temporal_history()))
            dp = vpt.default_denoise_params(iterations=3)
            want = DH.run_driver(drivers["denoise"], drivers["dir"], rad, f["normal"], f["albedo"], f["depth"], 3, dp.sigma_color, dp.sigma_normal, dp.sigma_depth, dp.flags, tag="off")
            assert_bits(g.denoise(dp), want, "step %d: denoise" % k)
        want = TH.run_sequence(drivers["temporal"], drivers["dir"], frames, tag="off_t", flags=tp.flags, max_history=tp.max_history, depth_tolerance=tp.depth_tolerance,
                               normal_threshold=tp.normal_threshold, focus_distance=vpt.default_params().focus_distance, dof_strength=0.0)
        for k in range(2):
            assert_bits(got[k][0], want[k][0], "step %d: temporal image" % k)
            assert_bits(got[k][1], want[k][1][..., 3], "step %d: history length" % k)
        with pytest.raises(vpt.VptError, match=INVALID):
            g.firefly_image()
        s = g.firefly_state()
        assert (s.clamped, s.considered, s.calls) == (0, 0, 0)
    finally:
        g.close()
    big = context(vpt, feature_scene(vpt, "cornell_gltf"), 1024, 1024, frames=1)
    try:
        free = lambda: torch.cuda.mem_get_info(0)[0]
        big.temporal_accumulate(); big.denoise(vpt.default_denoise_params(iterations=1))      # the calls' own buffers are there now
        big.set_firefly_options(mode=0, radius=2, rank=3)
        before = free()
        big.temporal_accumulate(); big.denoise(vpt.default_denoise_params(iterations=1))
        off = before - free()
        big.set_firefly_options(mode=1)
        big.temporal_accumulate()
        on = before - free()
        print("free device memory across the calls: off %+d B, first filtered call %+d B" % (-off, -on))
        assert abs(off) < 8 << 20 and on >= (16 << 20) - (8 << 20)
        assert big.firefly_state().calls == 1
    finally:
        big.close()


# ---- 4. state and forms
def test_toggling_keeps_the_history_and_the_accumulation_image(vpt):
    """The history length does not depend on colours: a context that switches the filter on and off between its steps has, step for step, the lengths of one that
    never made the call — the call dropped nothing.  And vpt_get_radiance after a filtered call returns the bits it returned before it."""
    sc = feature_scene(vpt, "cornell_gltf")
    w, h = 45, 37
    never, toggled = context(vpt, sc, w, h, frames=0), context(vpt, sc, w, h, frames=0)
    try:
        proj_inv = sc.projection_inverse(w / h)
        for k, view_inv in enumerate(camera_path(sc)[:3]):
            toggled.set_firefly_options(mode=(1, 0, 1)[k], threshold=1.0, floor=0.0)
            lengths = []
            for g in (never, toggled):
                g.set_camera(view_inv, proj_inv); g.render(2)
                rad = g.radiance()
                g.temporal_accumulate()
                assert_bits(g.radiance(), rad, "step %d: the accumulation image" % k)
                lengths.append(g.temporal_history())
            assert_bits(lengths[1], lengths[0], "step %d: history length" % k)
        assert (lengths[1] > 4).sum() > 50      # it grew across both toggles
        assert toggled.firefly_state().calls == 1 and toggled.firefly_state().clamped > 0      # (counted from the latest switch to mode 1)
    finally:
        never.close(); toggled.close()


def test_device_forms_and_shards(vpt):
    """The _device forms, with tickets, give the blocking forms' bits, and the read-backs wait for them.  A sharded context follows vpt_denoise's rule: refused
    before vpt_assemble_shards, the whole image's bits after it."""
    sc = feature_scene(vpt, "textured_boxes")
    w, h = 45, 37
    g = context(vpt, sc, w, h)
    try:
        g.set_firefly_options(**BUSY)
        want_tp = g.temporal_accumulate()
        want_ff_tp, want_state = g.firefly_image(), g.firefly_state()
        want_dn = g.denoise(vpt.default_denoise_params(iterations=2))
        want_ff_dn = g.firefly_image()
        g.temporal_reset()
        dev = torch.full((h, w, 4), 7.0, device="cuda:0")
        t = g.temporal_accumulate_device(None, dev.data_ptr())
        assert t > 0
        assert_bits(g.firefly_image(), want_ff_tp, "the read-back waits for the queued call")
        s = g.firefly_state()
        assert (s.clamped, s.considered) == (want_state.clamped, want_state.considered) and s.calls == want_state.calls + 2
        g.wait(t)
        assert_bits(dev.cpu().numpy(), want_tp, "temporal_accumulate_device")
        t2 = g.denoise_device(vpt.default_denoise_params(iterations=2), dev.data_ptr())
        g.wait(t2)
        assert t2 > t
        assert_bits(dev.cpu().numpy(), want_dn, "denoise_device")
        assert_bits(g.firefly_image(), want_ff_dn, "the filtered image of denoise_device")
    finally:
        g.close()
    parts = [context(vpt, sc, w, h, shard_rank=r, shard_count=2) for r in range(2)]
    hip = C.CDLL("libamdhip64.so")
    buf = C.c_void_p()
    try:
        parts[0].set_firefly_options(**BUSY)
        with pytest.raises(vpt.VptError, match=INVALID):
            parts[0].temporal_accumulate()
        with pytest.raises(vpt.VptError, match=INVALID):
            parts[0].firefly_image()
        n = parts[0].shard_floats()
        assert hip.hipMalloc(C.byref(buf), n * 4 * 2) == 0
        for r, s in enumerate(parts):
            s.shard_to_device(C.c_void_p(buf.value + r * n * 4))
        parts[0].assemble_shards(buf, 2)
        assert_bits(parts[0].temporal_accumulate(), want_tp, "sharded: temporal")
        assert_bits(parts[0].firefly_image(), want_ff_tp, "sharded: the filtered image")
        assert_bits(parts[0].denoise(vpt.default_denoise_params(iterations=2)), want_dn, "sharded: denoise")
    finally:
        if buf.value:
            hip.hipFree(buf)
        for s in parts:
            s.close()


def test_every_error_code(vpt, scenes):
    sc = scenes("cornell_box")
    lib = vpt.load_library()
    g = vpt.PathTracer(32, 24)
    fields = lambda o: (o.mode, o.radius, o.rank, o.threshold, o.floor, tuple(o.reserved))
    try:
        g.set_scene(sc)
        assert fields(g.firefly_options()) == fields(vpt.default_firefly_options()) == (0, 1, 2, 2.0, 1.0, (0, 0, 0))
        g.set_firefly_options(mode=1, radius=2, rank=3, threshold=1.5, floor=0.25)
        kept = fields(g.firefly_options())
        assert kept == (1, 2, 3, 1.5, 0.25, (0, 0, 0))      # the round trip
        refused = 0
        for o, accepted in option_cases():
            if accepted:
                continue
            with pytest.raises(vpt.VptError, match=INVALID):
                g.set_firefly_options(**o)
            assert fields(g.firefly_options()) == kept, o      # a refused call changes nothing
            refused += 1
        assert refused >= 19
        for o, accepted in option_cases():
            if accepted:
                g.set_firefly_options(**o)
                assert fields(g.firefly_options()) == (o["mode"], o["radius"], o["rank"], np.float32(o["threshold"]), np.float32(o["floor"]), (0, 0, 0))
        ok = vpt.default_firefly_options()
        st = vpt.FireflyState()
        assert lib.vpt_set_firefly_options(g.ctx, None) == -1 and lib.vpt_set_firefly_options(None, C.byref(ok)) == -1
        assert lib.vpt_get_firefly_options(g.ctx, None) == -1 and lib.vpt_get_firefly_options(None, C.byref(ok)) == -1
        assert lib.vpt_get_firefly_state(g.ctx, None) == -1 and lib.vpt_get_firefly_state(None, C.byref(st)) == -1
        assert lib.vpt_get_firefly_image(g.ctx, None) == -1 and lib.vpt_get_firefly_image(None, C.byref(st)) == -1
        # before the first filtered call: the image refuses, the state is zeros
        g.set_firefly_options(mode=1, radius=1, rank=2, threshold=2.0, floor=1.0)
        with pytest.raises(vpt.VptError, match=INVALID):
            g.firefly_image()
        s = g.firefly_state()
        assert (s.clamped, s.considered, s.calls, s.reserved) == (0, 0, 0, 0)
        # a filtered call needs what its call needs
        with pytest.raises(vpt.VptError, match=INVALID):
            g.temporal_accumulate()                      # nothing rendered yet
        g.set_params(vpt.default_params(max_depth=4))
        g.render(1)
        g.temporal_accumulate()
        s = g.firefly_state()
        assert g.firefly_image().shape == (24, 32, 4) and s.calls == 1 and 0 < s.considered <= 32 * 24 and s.clamped <= s.considered
        # ... and after vpt_resize there is no filtered image of the current size again
        g.resize(40, 20)
        with pytest.raises(vpt.VptError, match=INVALID):
            g.firefly_image()
        s = g.firefly_state()
        assert (s.clamped, s.considered, s.calls) == (0, 0, 0)
        g.render(1)
        g.denoise(vpt.default_denoise_params(iterations=1))
        assert g.firefly_image().shape == (20, 40, 4) and g.firefly_state().calls == 2
    finally:
        g.close()


def test_vpt_stats_is_untouched(vpt, scenes):
    """As for vpt_denoise: a filtered call adds no launch and no time to vpt_stats."""
    g = vpt.PathTracer(32, 24, profile=True)
    try:
        g.set_scene(scenes("cornell_box"))
        g.set_params(vpt.default_params(max_depth=4))
        g.render(1)
        g.set_firefly_options(**BUSY)
        before = g.stats()
        g.temporal_accumulate(); g.denoise(vpt.default_denoise_params(iterations=1))
        after = g.stats()
        assert g.firefly_state().calls == 2
        assert before["kernel_launches"] == after["kernel_launches"] and before["samples"] == after["samples"]
    finally:
        g.close()


# ---- 5. quality: direction only
# Relative L2 over the rgb of every pixel — sqrt(sum (d - ref)^2 / sum ref^2), tests/test_gpu_denoise.py's figure — of ONE 1-spp image (seed 0,
# tests/test_gpu_svgf_spatial.py's) through the default SVGF chain (variance on, the temporal source, 5 a-trous passes) against 1024 spp of the same view, 64 x 48,
# depth 4, with the filter off and on at its defaults.  "on <= off" is asserted for the Cornell box of the project's other quality tests (cornell_box.npz, its
# own camera, inside the box).  Measured on an MI355X (profiles/firefly_quality.md): off 0.5637, on 0.5633; 2.34 % of the
# pixels clamped; the mean luminance of the filter's input 0.93 % lower (the bias), of the denoised image 0.3877 -> 0.3840 (1024 spp: 0.3757).  The gain is
# small because this figure hangs on the lamp's edge pixels (radiance 50 against a median of 0.04), which the filter rightly leaves alone.
# The second view is REPORTED ONLY, and it goes the other way: cornell_gltf seen from outside past its right edge (tests/test_gpu_features.py's camera), where the
# lamp is a sliver ONE pixel tall — the thin emitter of the header's second limit.  A 1-spp pixel on it is either 50 or the ceiling's 0.5, its neighbours
# are the ceiling, and the filter takes the lamp down to twice the ceiling: off 0.7498, on 0.8770, the input's mean luminance 31.9 % lower with 1.76 % of the
# pixels clamped.  floor = 64 (above the lamp's radiance) leaves the lamp alone: on 0.7114, 1.50 % lower, 0.68 % clamped.
QUALITY_SEED = 0


def quality(vpt, sc, seed=QUALITY_SEED, w=64, h=48, spp=1024, **options):
    g = context(vpt, sc, w, h, frames=spp)
    try:
        ref = g.radiance()[..., :3].astype(np.float64)
        g.set_svgf_options(variance=1)
        g.set_denoise_source(vpt.DENOISE_SOURCE_TEMPORAL)
        lum = lambda img: float(FH.luminance32(np.asarray(img[..., :3], np.float32)).astype(np.float64).mean())
        out = {"ref_mean": lum(ref)}
        for mode in (0, 1):
            g.set_firefly_options(mode=mode, **options)
            g.temporal_reset()
            g.set_base_seed(seed)
            g.render(1)
            rad = g.radiance()
            g.temporal_accumulate()
            d = g.denoise(vpt.default_denoise_params(iterations=5))[..., :3].astype(np.float64)
            out[mode] = float(np.sqrt(((d - ref) ** 2).sum() / (ref ** 2).sum()))
            out["mean_%d" % mode] = lum(d)
            if mode:
                s = g.firefly_state()
                out["clamped_share"] = s.clamped / float(w * h)
                out["considered_share"] = s.considered / float(w * h)
                out["input_loss"] = 1.0 - lum(g.firefly_image()) / lum(rad)
        return out
    finally:
        g.close()


def report(name, e, what=""):
    print("%s 64 x 48 seed %d%s: relative L2 against 1024 spp off %.4f, on %.4f; %.2f %% of the pixels clamped (%.1f %% considered); mean luminance of the "
          "filter's input %.2f %% lower, of the denoised image %.4f -> %.4f (1024 spp: %.4f)" %
          (name, QUALITY_SEED, what, e[0], e[1], 100 * e["clamped_share"], 100 * e["considered_share"], 100 * e["input_loss"], e["mean_0"], e["mean_1"], e["ref_mean"]))


def test_quality_direction_only(vpt, scenes):
    e = quality(vpt, scenes("cornell_box"))
    report("cornell_box", e)
    sliver = quality(vpt, feature_scene(vpt, "cornell_gltf"))
    report("cornell_gltf from outside (reported only)", sliver)
    report("cornell_gltf from outside (reported only)", quality(vpt, feature_scene(vpt, "cornell_gltf"), floor=64.0), ", floor 64")
    assert np.isfinite(e[0]) and np.isfinite(e[1]) and e["clamped_share"] > 0
    assert e[1] <= e[0], e
