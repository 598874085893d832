"""csrc/exposure.hpp on the host (tests/tools/exposure_driver.cpp): bin_of at its edges, meter on histograms whose integers are worked out by hand, adapt's
rules, an analytic anchor with a derived bound, a float64 restatement (tests/ref_exposure64.py), and one run of the driver under the address and
undefined-behaviour sanitizers (bin_of's float-to-int conversion is where undefined behaviour would hide).  The device is held to these bits by
tests/test_gpu_exposure.py."""
import subprocess

import numpy as np
import pytest

import exposure_host as EH
import ref_exposure64 as R


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return EH.compile_driver(str(tmp_path_factory.mktemp("exposure") / "exposure_driver"))


def f32(x):
    return np.float32(x)


def below(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def hist_of(**bins):
    h = np.zeros(256, np.uint32)
    for k, v in bins.items():
        h[int(k[1:])] = v
    return h


def test_bin_of_at_the_edges(vpt, driver, tmp_path):
    """The edges of the range are placed on the luminance itself: a green-only pixel is searched whose fp32 luminance 0.7152 g is exactly the edge."""
    o = vpt.default_exposure_options(mode=1)          # range 2^-10 .. 2^6
    w = [f32(0.2126), f32(0.7152), f32(0.0722)]

    def lum(p):
        return (w[0] * f32(p[0]) + w[1] * f32(p[1])) + w[2] * f32(p[2])

    def pixel_with(l, exact=True):
        """A green-only pixel whose fp32 luminance is exactly l (the green value is found by stepping around l / 0.7152) — or, not exact, next to l."""
        g = f32(l) / w[1]
        for _ in range(8 if exact else 0):
            got = lum((0, g, 0))
            if got == f32(l):
                break
            g = np.nextafter(g, f32(np.inf) if got < f32(l) else f32(-np.inf))
        assert not exact or lum((0, g, 0)) == f32(l), "no green value gives luminance %r exactly" % l
        return (0.0, float(g), 0.0)

    cases = [((0.0, 0.0, 0.0), 0), ((-1.0, -1.0, -1.0), 0), ((np.nan, 0.0, 0.0), 0), ((np.inf, 0.0, 0.0), 255),
             ((1e-42, 1e-42, 1e-42), 1),                                 # a denormal: far below the range, positive
             (pixel_with(2.0 ** -10), 1),                                # exactly 2^min_log2: t = 0
             (pixel_with(below(2.0 ** 6)), 255),                         # the largest float below 2^max_log2: its logarithm differs from log 64 by 6e-8, a
                                                                         # quarter ulp of the fp32 result, so t is 254 as for 2^6 itself — the edge is
                                                                         # as sharp as fp32's log, and the header's t is the definition
             (pixel_with(2.0 ** 6), 255),                                # 2^max_log2: t = 254
             ((-np.inf, 0.0, 0.0), 0), ((np.inf, -np.inf, 0.0), 0),      # -inf and inf - inf = NaN: black
             (pixel_with(64.0 * (1.0 - 2.0 ** -12), False), 254),        # 0.006 bins below 2^max_log2: the last bin inside the range
             (pixel_with(2.0 ** -10 * (1.0 + 2.0 ** -12), False), 1), (pixel_with(2.0 ** -10 * 1.05, False), 2)]   # 0.006 and 1.1 bins above 2^min_log2
    img = np.zeros((1, len(cases), 4), np.float32)
    for k, (p, _) in enumerate(cases):
        img[0, k, :3] = p
    with np.errstate(all="ignore"):
        assert lum(cases[5][0]) == f32(2.0 ** -10) and lum(cases[6][0]) == below(2.0 ** 6) and lum(cases[7][0]) == f32(64.0)
    got = EH.run(driver, tmp_path, o, [("bins", img, 0)])[0]
    assert got[0].tolist() == [b for _, b in cases]


def test_meter_on_hand_made_histograms(vpt, driver, tmp_path):
    """Default percentiles: lo_q16 = 32768, hi_q16 = rint(0.95 * 65536) = 62259."""
    o = vpt.default_exposure_options(mode=1)
    full = vpt.default_exposure_options(mode=1, low_percentile=0.0, high_percentile=1.0)
    steps = [("hist", hist_of(b100=1000), EH.RESET_ALL),                   # one bin: lo = 500, hi = (1000 * 62259) >> 16 = 949, S = 449 * 100
             ("hist", hist_of(b50=600, b200=400), EH.RESET_ALL),           # split: bin 50 gives [500, 600), bin 200 gives [600, 949)
             ("hist", hist_of(b7=1), EH.RESET_ALL),                        # N = 1: lo = 0, hi = max(0, lo + 1) = 1
             ("hist", hist_of(b0=77), EH.RESET_NONE)]                      # everything black: no target, the state stays
    r = EH.run(driver, tmp_path, o, steps)
    assert [(int(x["lo"]), int(x["hi"]), int(x["S"]), int(x["W"]), int(x["has_target"])) for x in r] == \
        [(500, 949, 44900, 449, 1), (500, 949, 100 * 50 + 349 * 200, 449, 1), (0, 1, 7, 1, 1), (0, 0, 0, 0, 0)]
    width = f32(1.0) / (f32(254.0) / f32(16.0))

    def avg(mean_bin):
        return f32(-10.0) + (f32(mean_bin) - f32(0.5)) / (f32(254.0) / f32(16.0))
    assert f32(r[0]["state"]["avg_log2"]) == avg(100.0) and abs(float(r[0]["state"]["avg_log2"]) - (-10.0 + 99.5 * float(width))) < 1e-5
    assert f32(r[1]["state"]["avg_log2"]) == avg(np.float32(74800.0 / 449.0))
    assert f32(r[2]["state"]["avg_log2"]) == avg(7.0)
    # all black: every field of the state but the count of meterings and N stays
    for k in ("scale", "cur_log2", "target_log2", "avg_log2", "valid"):
        assert r[3]["state"][k] == r[2]["state"][k], k
    assert (r[3]["state"]["meterings"], r[3]["state"]["counted"], r[2]["state"]["counted"]) == (2, 0, 1)
    # low = 0 with high = 1: every pixel counts
    x = EH.run(driver, tmp_path, full, [("hist", hist_of(b10=3, b20=5), EH.RESET_ALL)])[0]
    assert (int(x["lo"]), int(x["hi"]), int(x["S"]), int(x["W"])) == (0, 8, 3 * 10 + 5 * 20, 8)
    # all black before anything else: cur = 0, scale = 1, not valid — and the next metering with a target jumps
    y = EH.run(driver, tmp_path, o, [("hist", hist_of(b0=5), EH.RESET_ALL), ("hist", hist_of(b100=10), EH.RESET_NONE)])
    assert (y[0]["state"]["valid"], y[0]["state"]["cur_log2"], y[0]["state"]["scale"], y[0]["state"]["meterings"]) == (0, 0.0, 1.0, 1)
    assert y[1]["state"]["valid"] == 1 and y[1]["state"]["cur_log2"] == y[1]["state"]["target_log2"] != 0.0


def test_adapt(vpt, driver, tmp_path):
    bright, dark = hist_of(b200=100), hist_of(b40=100)          # a bright image wants a LOW exposure
    o = vpt.default_exposure_options(mode=1, rate_up=0.5, rate_down=0.125)
    r = EH.run(driver, tmp_path, o, [("hist", bright, EH.RESET_ALL), ("hist", dark, 0), ("hist", bright, 0), ("hist", dark, EH.RESET_JUMP)])
    s = [x["state"] for x in r]
    t_bright, t_dark = f32(s[0]["target_log2"]), f32(s[1]["target_log2"])
    assert t_bright < t_dark and s[0]["cur_log2"] == t_bright and s[0]["valid"] == 1          # the first metering jumps
    up = t_bright + (t_dark - t_bright) * f32(0.5)
    assert f32(s[1]["cur_log2"]) == up                                                        # towards a brighter exposure: rate_up
    assert f32(s[2]["cur_log2"]) == up + (t_bright - up) * f32(0.125)                         # towards a darker one: rate_down
    assert s[3]["cur_log2"] == t_dark and s[3]["meterings"] == 4                              # after a reset: a jump
    for x in s:
        assert abs(float(x["scale"]) - 2.0 ** float(x["cur_log2"])) <= 2.0 ** float(x["cur_log2"]) * 2.0 ** -21
    # rate 1 returns the target's bits — cur + (target - cur) * 1 would not for these two
    one = vpt.default_exposure_options(mode=1, rate_up=1.0, rate_down=1.0, key=0.18)
    a, b = hist_of(b3=1, b200=2), hist_of(b41=7, b43=9)
    q = [x["state"] for x in EH.run(driver, tmp_path, one, [("hist", a, EH.RESET_ALL), ("hist", b, 0), ("hist", a, 0)])]
    assert q[1]["cur_log2"] == q[1]["target_log2"] and q[2]["cur_log2"] == q[2]["target_log2"] == q[0]["target_log2"]
    # both clamps
    lo = vpt.default_exposure_options(mode=1, min_exposure_log2=-1.0, max_exposure_log2=1.5)
    c = [x["state"] for x in EH.run(driver, tmp_path, lo, [("hist", bright, EH.RESET_ALL), ("hist", dark, EH.RESET_JUMP)])]
    assert (c[0]["target_log2"], c[1]["target_log2"]) == (-1.0, 1.5) and t_bright < -1.0 and t_dark > 1.5


@pytest.mark.parametrize("L", [2.0 ** -9.7, 0.0123, 0.18, 1.0, 3.3, 60.0])
def test_one_luminance_lands_on_the_key(vpt, driver, tmp_path, L):
    """An image of one luminance L inside the range: avg_log2 is the centre of L's bin, so |avg_log2 - log2 L| <= half a bin = (max_log2 - min_log2) / 508,
    plus the rounding of log_ and of the three fp32 operations behind it (2^-16 is generous: log_ is good to a few ulp of a value below 16); and
    scale * L is then within a factor 2^(that + 2^-16) of the key (the second 2^-16: log_(key) and exp_) — with the clamp of the result out of the way:
    the default one, 2^-8, is reached by L = 60 (0.18 / 60 = 2^-8.4)."""
    o = vpt.default_exposure_options(mode=1, min_exposure_log2=-20.0, max_exposure_log2=20.0)
    img = np.zeros((3, 5, 4), np.float32)
    img[..., :3] = np.float32(L)
    l32 = float(R.luminance32(img)[0, 0])
    s = EH.run(driver, tmp_path, o, [("image", img, EH.RESET_ALL)])[0]["state"]
    bound = (o.max_log2 - o.min_log2) / 508.0 + 2.0 ** -16
    assert s["valid"] == 1 and s["counted"] == 15
    assert abs(float(s["avg_log2"]) - np.log2(l32)) <= bound
    assert abs(np.log2(float(s["scale"]) * l32) - np.log2(0.18)) <= bound + 2.0 ** -16


def wild_image(w, h, seed):
    rng = np.random.RandomState(seed)
    rgb = (2.0 ** rng.uniform(-16.0, 12.0, (h, w, 1)) * rng.uniform(0.5, 1.5, (h, w, 3))).astype(np.float32)
    kind = rng.randint(0, 40, (h, w))
    rgb[kind == 0] = 0.0
    rgb[kind == 1] = -1.0
    rgb[kind == 2] = np.nan
    rgb[kind == 3] = np.inf
    img = np.ones((h, w, 4), np.float32)
    img[..., :3] = rgb
    return img


MEASURED_AVG_LOG2 = 5.6e-6       # the worst of the six images below, against tests/ref_exposure64.py (recorded in DESIGN.md §5 too)
MEASURED_SCALE_REL = 4.2e-6


def test_against_the_float64_restatement(vpt, driver, tmp_path, capsys):
    """Six wild images of 192 x 160 — log-uniform from 2^-16 to 2^12, well beyond both ends of the range, with black, negative, NaN and infinite pixels.
    The black bin agrees exactly.  What differs is a pixel whose bin position lies within log_'s rounding of a bin edge: ONE pixel of the 184 320 lands in
    the neighbouring bin, which moves S by 1 and avg_log2 by a bin's width over W.  Measured: |avg_log2 - ref| <= 5.51e-6 (log2 units), |scale / ref - 1| <=
    4.11e-6; the bound asserted is four times the measured value, the project's rule for its float64 restatements."""
    o = vpt.default_exposure_options(mode=1)
    worst_avg, worst_scale, flips = 0.0, 0.0, 0
    for seed in range(6):
        img = wild_image(192, 160, seed)
        got = EH.run(driver, tmp_path, o, [("image", img, EH.RESET_ALL)])[0]
        ref_hist = np.bincount(R.bins64(img, o.min_log2, o.max_log2), minlength=256)
        assert ref_hist[0] > 0 and ref_hist[1] > 0 and ref_hist[255] > 0 and ref_hist.sum() == got["hist"].sum() == 192 * 160
        assert got["hist"][0] == ref_hist[0]                         # black is black on both sides
        flips += int(np.abs(got["hist"].astype(np.int64) - ref_hist).sum()) // 2
        avg, _, scale = R.first_metering64(img, o)
        worst_avg = max(worst_avg, abs(float(got["state"]["avg_log2"]) - avg))
        worst_scale = max(worst_scale, abs(float(got["state"]["scale"]) / scale - 1.0))
    with capsys.disabled():
        print("\nexposure vs float64: |avg_log2| %.3e, scale rel %.3e, %d pixels in another bin" % (worst_avg, worst_scale, flips))
    assert worst_avg <= 4.0 * MEASURED_AVG_LOG2 and worst_scale <= 4.0 * MEASURED_SCALE_REL


def test_driver_is_clean_under_the_sanitizers(vpt, tmp_path):
    """The stand-alone driver, built with -fsanitize=address,undefined and made to stop at the first report, over the edge pixels, a wild image and hand-made
    histograms (the largest counts a uint32 bin can hold included: the 64-bit products must not overflow)."""
    exe = EH.compile_driver(str(tmp_path / "exposure_driver_san"), extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    o = vpt.default_exposure_options(mode=1, low_percentile=0.0, high_percentile=1.0)
    edge = np.zeros((1, 8, 4), np.float32)
    edge[0, :, 0] = [0.0, -1.0, np.nan, np.inf, 1e-42, 3.4e38, -np.inf, 1e-30]
    huge = np.zeros(256, np.uint32)
    huge[1:] = 0xffffffff
    r = EH.run(exe, tmp_path, o, [("bins", edge, 0), ("image", wild_image(67, 35, 9), EH.RESET_ALL), ("hist", huge, 0), ("hist", hist_of(b0=9), EH.RESET_JUMP)])
    assert r[0][0].tolist() == [0, 0, 0, 255, 1, 255, 0, 1]
    assert int(r[2]["state"]["counted"]) == 255 * 0xffffffff and int(r[2]["W"]) == 255 * 0xffffffff and int(r[2]["S"]) == 0xffffffff * sum(range(1, 256))
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 2 and "usage" in out.stderr
