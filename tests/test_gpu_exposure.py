"""Auto-exposure on the device (vpt_set_exposure_options; kernels_post.hip k_luminance_histogram and k_exposure_adapt) against the host compile of
csrc/exposure.hpp (tests/tools/exposure_driver.cpp): histogram and state bit for bit — the sums are of integers, the rest is a handful of fp32 operations
in one lane —, the RGBA8 output byte for byte against the oracle run with exposure * scale, and what the options promise: off is off, the asynchronous
form, what the state survives, the errors.  Images are injected with vpt_set_radiance; only the cases that say so render a scene."""
import ctypes as C

import numpy as np
import pytest

import exposure_host as EH

pytestmark = pytest.mark.gpu

# kernels.hpp: at most kHistMaxBlocks blocks of kHistThreads threads, two pixels per thread and trip — one pixel more than 2 * 256 * 1024 makes block 0
# take a second grid-stride trip (1025 x 512 = 524 800 pixels, 8.4 MB)
HIST_MAX_BLOCKS, HIST_THREADS = 256, 1024
SECOND_TRIP = (1025, 512)
assert SECOND_TRIP[0] * SECOND_TRIP[1] > 2 * HIST_MAX_BLOCKS * HIST_THREADS >= (SECOND_TRIP[0] - 1) * SECOND_TRIP[1]
SHAPES = [(16, 16), (67, 35), (256, 4), SECOND_TRIP]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return EH.compile_driver(str(tmp_path_factory.mktemp("exposure") / "exposure_driver"))


def rgba(rgb):
    img = np.ones(rgb.shape[:2] + (4,), np.float32)
    img[..., :3] = rgb
    return img


def flat_image(w, h, value=0.25):
    return rgba(np.full((h, w, 3), value, np.float32))


def wild_image(w, h, seed):
    """Log-uniform luminance from 2^-16 to 2^12 — well beyond both ends of the default range 2^-10 .. 2^6 — with black, negative, NaN and infinite pixels."""
    rng = np.random.RandomState(seed)
    rgb = (2.0 ** rng.uniform(-16.0, 12.0, (h, w, 1)) * rng.uniform(0.5, 1.5, (h, w, 3))).astype(np.float32)
    kind = rng.randint(0, 40, (h, w))
    rgb[kind == 0] = 0.0
    rgb[kind == 1] = -1.0
    rgb[kind == 2] = np.nan
    rgb[kind == 3] = np.inf
    return rgba(rgb)


def tame_image(w, h, seed, level):
    """A finite image around `level`, with highlights above the bloom threshold: what the oracle's post chain takes."""
    rng = np.random.RandomState(seed)
    rgb = (level * rng.gamma(0.6, 2.0, (h, w, 3))).astype(np.float32)
    rgb[rng.rand(h, w) < 0.02] *= 50.0
    return rgba(rgb)


def assert_state(got, want, what):
    assert EH.state_tuple(got) == EH.state_tuple(want["state"]), "%s: device %r, host %r" % (what, EH.state_tuple(got), EH.state_tuple(want["state"]))


@pytest.mark.parametrize("w,h", SHAPES)
def test_histogram_equals_the_host_compile(vpt, driver, tmp_path, w, h):
    """Every pixel in one bin (all 64 lanes of every wave on one LDS word: the count must be exactly w * h), all black (N = 0: nothing counted, no target),
    and the wild image."""
    opts = vpt.default_exposure_options(mode=1)
    images = [flat_image(w, h), rgba(np.zeros((h, w, 3), np.float32)), wild_image(w, h, w * 7 + h)]
    want = EH.run(driver, tmp_path, opts, [("image", im, EH.RESET_ALL if k == 0 else EH.RESET_NONE) for k, im in enumerate(images)])
    g = vpt.PathTracer(w, h)
    try:
        g.set_exposure_options(mode=1)
        for k, im in enumerate(images):
            g.set_radiance(im, 1)
            g.postprocess()
            hist = g.exposure_histogram()
            assert hist.sum() == w * h
            diff = np.flatnonzero(hist != want[k]["hist"])
            assert diff.size == 0, "image %d: %d bins differ, first %d: device %d, host %d" % (k, diff.size, diff[0], hist[diff[0]], want[k]["hist"][diff[0]])
            assert_state(g.exposure_state(), want[k], "image %d" % k)
        flat_bin = int(np.flatnonzero(want[0]["hist"])[0])
        assert want[0]["hist"][flat_bin] == w * h and 1 <= flat_bin <= 254
        assert want[1]["hist"][0] == w * h and want[1]["state"]["counted"] == 0 and want[1]["has_target"] == 0
        assert (want[2]["hist"][[0, 1, 255]] > 0).all()       # the wild image reaches the black bin and both ends of the range
    finally:
        g.close()


def test_state_follows_the_host_compile_through_bright_dark_bright(vpt, driver, tmp_path):
    """Default rates; bright, dark, all black (the state is kept), dark again, bright: all seven fields after every call."""
    w, h = 67, 35
    images = [tame_image(w, h, 1, 8.0), tame_image(w, h, 2, 0.01), rgba(np.zeros((h, w, 3), np.float32)), tame_image(w, h, 3, 0.01), tame_image(w, h, 4, 8.0)]
    opts = vpt.default_exposure_options(mode=1)
    want = EH.run(driver, tmp_path, opts, [("image", im, EH.RESET_ALL if k == 0 else EH.RESET_NONE) for k, im in enumerate(images)])
    g = vpt.PathTracer(w, h)
    try:
        g.set_exposure_options(mode=1)
        seen = []
        for k, im in enumerate(images):
            g.set_radiance(im, 1)
            g.postprocess()
            s = g.exposure_state()
            assert_state(s, want[k], "call %d" % k)
            seen.append((s.cur_log2, s.target_log2, s.valid, s.meterings, s.counted))
        assert seen[0][0] == seen[0][1] and seen[0][2] == 1                      # the first metering jumps
        assert seen[0][0] < seen[1][0] < seen[1][1]                              # darker image: the exposure rises, by rate_up, not at once
        assert seen[2][:2] == seen[1][:2] and seen[2][4] == 0 and seen[2][3] == 3  # all black: kept, but counted as a metering
        assert seen[4][1] < seen[4][0] < seen[3][0]                              # brighter image: it falls, by rate_down
    finally:
        g.close()


@pytest.mark.parametrize("schedule", [0, 1])
@pytest.mark.parametrize("linear_tap", [True, False])
def test_output_equals_the_oracle_with_exposure_times_scale(vpt, oracle, schedule, linear_tap):
    """Odd width; two calls, so that the second's scale is a blend and not a jump."""
    w, h = 97, 33
    flags = vpt._abi.FLAGS_DEFAULT if linear_tap else vpt._abi.FLAGS_DEFAULT & ~vpt._abi.FLAG_TONEMAP_LINEAR_BLOOM_TAP
    g = vpt.PathTracer(w, h)
    try:
        g.set_params(vpt.default_params(flags=flags))
        g.set_exposure_options(mode=1)
        for k, level in enumerate((6.0, 0.05)):
            img = tame_image(w, h, 10 + k, level)
            pp = vpt.default_post_params(schedule=schedule, exposure=1.25)
            g.set_radiance(img, 1)
            out8 = g.postprocess(pp)
            s = g.exposure_state()
            assert s.valid == 1 and s.scale != 1.0
            ref_pp = vpt.default_post_params(schedule=schedule, exposure=float(np.float32(pp.exposure) * np.float32(s.scale)))
            ref8, _ = oracle.postprocess(img, ref_pp, flags)
            assert np.array_equal(out8, ref8), "call %d: %d bytes differ" % (k, (out8 != ref8).sum())
    finally:
        g.close()


def test_output_of_a_denoised_cornell_render(vpt, oracle, scenes):
    """The metered image is the post SOURCE: a Cornell render through vpt_denoise with iterations = 0 and VPT_POST_SOURCE_DENOISED."""
    w, h = 48, 32
    g = vpt.PathTracer(w, h)
    try:
        g.set_scene(scenes("cornell_box"))
        g.set_params(vpt.default_params(max_depth=4))
        g.render(2)
        den = g.denoise(vpt.default_denoise_params(iterations=0))
        g.set_post_source(vpt.POST_SOURCE_DENOISED)
        g.set_exposure_options(mode=1)
        out8 = g.postprocess()
        s = g.exposure_state()
        assert s.valid == 1 and s.counted > 0
        ref8, _ = oracle.postprocess(den, vpt.default_post_params(exposure=float(np.float32(1.0) * np.float32(s.scale))))
        assert np.array_equal(out8, ref8)
    finally:
        g.close()


def test_off_is_off(vpt):
    w, h = 67, 35
    img = tame_image(w, h, 5, 4.0)
    fresh = vpt.PathTracer(w, h)
    fresh.set_radiance(img, 1)
    want = fresh.postprocess()
    s0 = fresh.exposure_state()
    fresh.close()
    assert (s0.valid, s0.scale, s0.meterings) == (0, 1.0, 0)
    g = vpt.PathTracer(w, h)
    try:
        g.set_radiance(img, 1)
        g.set_exposure_options(mode=1)
        on = g.postprocess()
        assert g.exposure_state().valid == 1 and not np.array_equal(on, want)
        g.set_exposure_options(mode=0)
        assert np.array_equal(g.postprocess(), want)
        s = g.exposure_state()
        assert (s.valid, s.scale, s.meterings, s.counted) == (0, 1.0, 0, 0)
        with pytest.raises(vpt.VptError):
            g.exposure_histogram()
    finally:
        g.close()


def test_asynchronous_form_equals_the_blocking_one(vpt, scenes):
    """Cornell box 64 x 64: three rounds of set_base_seed, render_async(1), postprocess_device with nothing waited for, then one wait."""
    sc, w, h = scenes("cornell_box"), 64, 64

    def run(use_async):
        g = vpt.PathTracer(w, h)
        try:
            g.set_scene(sc)
            g.set_params(vpt.default_params(max_depth=4))
            g.set_exposure_options(mode=1)
            for k in range(3):
                g.set_base_seed(100 + k)
                if use_async:
                    g.render_async(1)
                    g.postprocess_device()
                else:
                    g.render(1)
                    g.postprocess()
            if use_async:
                g.wait()
            return EH.state_tuple(g.exposure_state()), g.output_to_host()
        finally:
            g.close()
    (sa, oa), (sb, ob) = run(True), run(False)
    assert sa == sb and sa[4:6] == (1, 3)
    assert np.array_equal(oa, ob)


def test_what_the_state_survives(vpt, driver, tmp_path):
    """vpt_resize keeps cur_log2; a change of rates alone does not make the next metering jump; vpt_exposure_reset does."""
    opts = vpt.default_exposure_options(mode=1)
    slow = vpt.default_exposure_options(mode=1, rate_up=0.5, rate_down=0.5)
    a, b = tame_image(40, 24, 6, 5.0), tame_image(52, 20, 7, 0.02)
    g = vpt.PathTracer(40, 24)
    try:
        g.set_exposure_options(mode=1)
        g.set_radiance(a, 1)
        g.postprocess()
        first = g.exposure_state()
        g.resize(52, 20)
        kept = g.exposure_state()
        assert EH.state_tuple(kept) == EH.state_tuple(first)
        g.set_exposure_options(rate_up=0.5, rate_down=0.5)
        g.set_radiance(b, 1)
        g.postprocess()
        blended = g.exposure_state()
        assert blended.valid == 1 and first.cur_log2 < blended.cur_log2 < blended.target_log2
        half = np.float32(first.cur_log2) + (np.float32(blended.target_log2) - np.float32(first.cur_log2)) * np.float32(0.5)
        assert np.float32(blended.cur_log2) == half
        g.exposure_reset()
        g.postprocess()
        jumped = g.exposure_state()
        assert jumped.cur_log2 == jumped.target_log2 == blended.target_log2 and jumped.meterings == 3
        # the same sequence on the host: the options of each metering, the reset of the third
        want = EH.run(driver, tmp_path, opts, [("image", a, EH.RESET_ALL)])[0]
        assert_state(first, want, "first")
        seq = EH.run(driver, tmp_path, slow, [("hist", want["hist"], EH.RESET_ALL), ("image", b, EH.RESET_NONE), ("image", b, EH.RESET_JUMP)])
        assert_state(blended, seq[1], "after the change of rates")
        assert_state(jumped, seq[2], "after vpt_exposure_reset")
    finally:
        g.close()


def test_errors_leave_the_context_usable(vpt):
    lib = vpt.load_library()
    w, h = 16, 16
    g = vpt.PathTracer(w, h)
    try:
        bad = [dict(mode=2), dict(min_log2=6.0), dict(max_log2=-10.0), dict(min_log2=float("nan")), dict(max_log2=float("inf")),
               dict(low_percentile=-0.1), dict(low_percentile=0.95), dict(high_percentile=1.5), dict(high_percentile=0.5), dict(low_percentile=float("nan")),
               dict(key=0.0), dict(key=-1.0), dict(key=float("inf")), dict(compensation_log2=float("nan")),
               dict(min_exposure_log2=9.0), dict(max_exposure_log2=float("inf")),
               dict(rate_up=0.0), dict(rate_up=1.5), dict(rate_down=0.0), dict(rate_down=-0.25), dict(rate_down=float("nan")), dict(reserved=1)]
        before = bytes(g.exposure_options())
        for kw in bad:
            o = vpt.default_exposure_options(**dict(dict(mode=1), **kw))
            assert lib.vpt_set_exposure_options(g.ctx, C.byref(o)) == -1, kw
            assert bytes(g.exposure_options()) == before, kw
        o = vpt.default_exposure_options()
        st = vpt.ExposureState()
        hist = (C.c_uint32 * 256)()
        assert lib.vpt_set_exposure_options(g.ctx, None) == -1 and lib.vpt_get_exposure_options(g.ctx, None) == -1
        assert lib.vpt_get_exposure_state(g.ctx, None) == -1 and lib.vpt_get_exposure_histogram(g.ctx, None) == -1
        assert lib.vpt_set_exposure_options(None, C.byref(o)) == -1 and lib.vpt_exposure_reset(None) == -1
        # edge values that ARE allowed
        g.set_exposure_options(mode=1, low_percentile=0.0, high_percentile=1.0, rate_up=1.0, rate_down=1.0, min_exposure_log2=2.0, max_exposure_log2=2.0)
        assert lib.vpt_get_exposure_histogram(g.ctx, hist) == -1            # before the first metering
        assert lib.vpt_get_exposure_state(g.ctx, C.byref(st)) == 0 and (st.valid, st.scale) == (0, 1.0)
        g.set_radiance(flat_image(w, h), 1)
        g.postprocess()
        s = g.exposure_state()
        assert (s.valid, s.cur_log2, s.counted) == (1, 2.0, w * h) and abs(s.scale - 4.0) <= 4.0 * 2.0 ** -22   # both clamps at 2: 2^2 whatever the image (exp_: within 2 ulp)
        assert g.exposure_histogram().sum() == w * h
    finally:
        g.close()
