"""SVGF's spatial variance estimate for young pixels without a device: csrc/svgf_spatial.hpp's spatial_variance_pixel compiled for the host inside the viewport
loop (tests/tools/svgf_spatial_driver.cpp, driven as api_post.hip drives the kernels), held to
  * a float64 restatement written from the description (tests/ref_svgf_spatial64.py), on the analytic frames of tests/temporal_host.py;
  * the constructed properties, exactly: the value of a checkerboard, what a hard edge weighs, what is left at -1, what the option must leave alone;
  * AddressSanitizer / UBSan: the same driver built with -fsanitize=address,undefined, as a stand-alone program.
The same function on the device, against this host compile bit for bit: tests/test_gpu_svgf_spatial.py."""
import numpy as np
import pytest

import ref_svgf_spatial64 as P64
import svgf_host as SH
import svgf_spatial_host as PH
import temporal_host as TH
from test_svgf_cpu import FLAG_SETS, MIN_HISTORIES, MS, SIZES, uniform_frame

F32 = np.float32
RADII = [1, 3]
RUNS = [SH.denoise_run(1, 1), SH.denoise_run(5, 1)]
SP = PH.SPATIAL_DEFAULTS
# Host compile against float64, measured on these inputs (x86-64-v3, g++ -O2) over every size, flag set, min_history, radius and step, per young pixel both
# sides estimate and that is not left out: |host - float64| in units of the pixel's M2 (the window's second moment — the variance is a cancelling difference
# of M2 and M1 M1).  The rule is tests/test_svgf_cpu.py's: the suite's 1e-4 where the measured worst is at most a quarter of it, otherwise 4 x the figure.
#   measured worst: 1.19e-06 (150 x 9, no demodulation, min_history 4, radius 3; radius 1: 4.34e-07)    -> 1e-4
# Left out: a pixel whose float64 sw lies within 1e-3 relative of min_weight (the two sides may fall on either side of "enough"); at most 5 % of a step's
# young pixels, asserted.  "Young" itself cannot differ: both sides compare the host compile's float32 length with min_history * m, exact in either precision.
# min_weight is the default 4: with it the float64 side leaves out at most 0.33 % of a step's young pixels (150 x 9, radius 1: 8 of the sequence's 3565 — a
# 2 x 2 corner window on one plane sums to 4 but for rounding); radius 3 leaves out 1 pixel in all.  With min_history 1 no pixel is young (a length is m at the least).
TOL_VARIANCE = 1e-4
LEFT_OUT_CAP = 0.05
MIN_WEIGHT = 4.0


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("svgf_spatial")
    return PH.compile_driver(str(d / "svgf_spatial_driver")), d


@pytest.fixture(scope="module")
def sequences():
    return {(w, h): TH.analytic_sequence(w, h, ms=MS) for (w, h) in SIZES}


@pytest.fixture(scope="module")
def plain_results(sequences, tmp_path_factory):
    """tests/tools/svgf_driver.cpp with the variance on: what the spatial estimate must leave alone."""
    d = tmp_path_factory.mktemp("svgf_plain")
    exe = SH.compile_driver(str(d / "svgf_driver"))
    return {(key, fl, mh): SH.run_sequence(exe, d, frames, RUNS, tag="plain_%d_%d_%d_%d" % (key + (fl, mh)), flags=fl, min_history=mh)
            for key, frames in sequences.items() for fl in FLAG_SETS for mh in MIN_HISTORIES}


@pytest.fixture(scope="module")
def host_results(driver, sequences):
    exe, d = driver
    return {(key, fl, mh, R): PH.run_sequence(exe, d, frames, RUNS, tag="seq_%d_%d_%d_%d_%d" % (key + (fl, mh, R)), flags=fl, min_history=mh, radius=R, min_weight=MIN_WEIGHT)
            for key, frames in sequences.items() for fl in FLAG_SETS for mh in MIN_HISTORIES for R in RADII}


def run(driver, frames, runs=(), tag="p", **kw):
    return PH.run_sequence(driver[0], driver[1], frames, runs, tag=tag, **kw)


def young_of(fr, got, mh):
    return (fr.depth >= 0) & ~(got["record"][..., 3] >= F32(mh) * F32(fr.m))


@pytest.mark.parametrize("R", RADII)
@pytest.mark.parametrize("mh", MIN_HISTORIES)
@pytest.mark.parametrize("flags", FLAG_SETS)
@pytest.mark.parametrize("key", SIZES, ids=lambda k: "%dx%d" % k)
def test_host_compile_against_float64(sequences, host_results, plain_results, key, flags, mh, R):
    """Every step on its own: the float64 side is given the record the host compile's temporal step wrote and estimates from it."""
    frames, results, plain = sequences[key], host_results[(key, flags, mh, R)], plain_results[(key, flags, mh)]
    worst, worst_share, young_total, left_total, estimated_total, unknown_total = 0.0, 0.0, 0, 0, 0, 0
    for k, fr in enumerate(frames):
        got = results[k]
        want, sw, young, m2 = P64.spatial_variance64(fr.normal, fr.depth, got["moments"], got["record"][..., 3], float(mh) * fr.m, plain[k]["variance"], R,
                                                     SP["sigma_normal"], SP["sigma_depth"], MIN_WEIGHT)
        assert np.array_equal(young, young_of(fr, got, mh)) and np.array_equal(young, (fr.depth >= 0) & (plain[k]["variance"] == -1))   # young: where the temporal step wrote -1
        left_out = young & (np.abs(sw - MIN_WEIGHT) <= 1e-3 * MIN_WEIGHT)
        assert left_out.sum() <= LEFT_OUT_CAP * max(int(young.sum()), 1), (key, k, left_out.sum(), young.sum())
        worst_share = max(worst_share, left_out.sum() / max(int(young.sum()), 1))
        keep = young & ~left_out
        gv = got["variance"].astype(np.float64)
        assert np.array_equal(gv[keep] < 0, want[keep] < 0), (key, k)
        assert ((gv[keep] >= 0) | (gv[keep] == -1)).all()
        est = keep & (want >= 0)
        if est.any():
            worst = max(worst, float((np.abs(gv - want)[est] / np.maximum(m2[est], 1e-30)).max()))
        young_total += int(young.sum()); left_total += int(left_out.sum()); estimated_total += int(est.sum()); unknown_total += int((keep & (want < 0)).sum())
    print("%s flags %d min_history %d radius %d: worst |host - float64| / M2 %.3g; %d young, %d estimated, %d left at -1, %d left out (%.2f %% of a step's young at the most)" %
          (key, flags, mh, R, worst, young_total, estimated_total, unknown_total, left_total, 100 * worst_share))
    assert worst <= TOL_VARIANCE
    if mh == 4:
        assert estimated_total > (50 if key != (7, 5) else 5)      # (with min_history 1 no hit pixel is ever young: its length is m at the least)
    else:
        assert young_total == 0


def test_records_and_the_pixels_that_are_not_estimated_keep_their_bits(sequences, host_results, plain_results, driver):
    """Image, record (the length in it), moments: svgf_driver's bits in every step, whatever the radius.  The variance: svgf_driver's at every miss and every
    pixel with len >= min_len.  With mode 0 the variance image — and so every filtered image — is svgf_driver's too."""
    untouched = 0
    for (key, fl, mh, R), results in host_results.items():
        plain = plain_results[(key, fl, mh)]
        for fr, got, want in zip(sequences[key], results, plain):
            for name in ("image", "record", "moments"):
                assert np.array_equal(PH.bits(got[name]), PH.bits(want[name])), (key, fl, mh, R, name)
            young = young_of(fr, got, mh)
            assert np.array_equal(PH.bits(got["variance"])[~young], PH.bits(want["variance"])[~young])
            untouched += int(((fr.depth >= 0) & ~young).sum())
    assert untouched > 1000
    for key in SIZES:
        for fl in FLAG_SETS:
            off = run(driver, sequences[key], RUNS, tag="off", flags=fl, min_history=4, mode=0)
            for got, want in zip(off, plain_results[(key, fl, 4)]):
                for name in ("image", "record", "moments", "variance"):
                    assert np.array_equal(PH.bits(got[name]), PH.bits(want[name])), (key, fl, name)
                for x, y in zip(got["denoised"], want["denoised"]):
                    assert np.array_equal(PH.bits(x), PH.bits(y))


def test_the_estimate_reaches_the_variance_guided_passes(sequences, host_results, plain_results):
    """A young pixel with an estimate is filtered by the variance-guided rule, not by the fixed-sigma one: its filtered bits differ from svgf_driver's."""
    key, fl, mh = (45, 37), TH.DEMODULATE | TH.MATCH_INSTANCE, 4
    got, want = host_results[(key, fl, mh, 3)][0], plain_results[(key, fl, mh)][0]
    est = (sequences[key][0].depth >= 0) & (got["variance"] >= 0)
    assert est.sum() > 500 and (want["variance"][est] == -1).all()
    assert (PH.bits(got["denoised"][1])[est] != PH.bits(want["denoised"][1])[est]).any(-1).mean() > 0.9


def grey_of_luminance(l):
    """A float32 grey g whose fp32 luminance (0.2126 g + 0.7152 g) + 0.0722 g — temporal.hpp's sum — is exactly l, found by stepping around l."""
    lum = lambda g: (F32(0.2126) * g + F32(0.7152) * g) + F32(0.0722) * g
    g = F32(l)
    for _ in range(64):
        if lum(g) == F32(l):
            return g
        g = np.nextafter(g, F32(0.0) if lum(g) > F32(l) else F32(np.inf))
    raise AssertionError("no grey gives luminance %r exactly" % l)


def checkerboard(w, h, a, b):
    colour = np.ones((h, w, 4), F32)
    yy, xx = np.mgrid[:h, :w]
    colour[..., :3] = np.where((xx + yy) % 2 == 0, grey_of_luminance(a), grey_of_luminance(b))[..., None]
    return colour


@pytest.mark.parametrize("R", RADII)
def test_a_checkerboard_of_two_dyadic_luminances_has_the_exact_variance(driver, R):
    """Uniform guides (every weight is exp_(-0) = 1), one image with min_history 2 (everything young, moments (l, l l)), luminances a = 1/2 and b = 1/4 in a
    checkerboard.  The corner pixel's window inside the image is 4 x 4 (R = 3) or 2 x 2 (R = 1) taps, half of each value: sw = 16 or 4, M1 = (a + b) / 2,
    M2 = (a a + b b) / 2 — every sum and quotient a dyadic rational float32 holds — and the variance is ((a - b) / 2)^2 = 2^-6 EXACTLY.  So it is wherever the
    window holds as many of one as of the other: every pixel whose window has an even number of rows or of columns inside the image."""
    w, h = 19, 11
    a, b = 0.5, 0.25
    got = run(driver, [uniform_frame(w, h, checkerboard(w, h, a, b))], tag="checker%d" % R, flags=0, min_history=2, radius=R)[0]
    mu = got["moments"]
    assert set(np.unique(mu[..., 0])) == {F32(a), F32(b)} and np.array_equal(mu[..., 1], mu[..., 0] * mu[..., 0])      # the luminances ARE dyadic
    exact = F32(((a - b) / 2) ** 2)
    v = got["variance"]
    for (x, y) in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)):
        assert v[y, x] == exact, (x, y, v[y, x])
    yy, xx = np.mgrid[:h, :w]
    rows = np.minimum(yy + R, h - 1) - np.maximum(yy - R, 0) + 1
    cols = np.minimum(xx + R, w - 1) - np.maximum(xx - R, 0) + 1
    balanced = (rows % 2 == 0) | (cols % 2 == 0)
    assert balanced.sum() > 20 and (v[balanced] == exact).all()
    assert (v[~balanced] >= 0).all() and np.abs(v[~balanced] / exact - 1).max() < 0.1      # (one tap more of one value than of the other: a little off 2^-6)


def edge_frame(w, h, colour, far=500.0):
    """uniform_frame with the right half 100 times as far away: from a near pixel, dz of a far tap is 495 / (0.05 r 5) >= 660 — exp_ returns exactly 0 below -103.9."""
    f = uniform_frame(w, h, colour)
    depth = f.depth.copy()
    depth[:, w // 2:] = far
    return TH.Frame(f.view_inv, f.proj_inv, f.m, f.radiance, f.normal, f.albedo, depth, f.inst)


def test_a_hard_depth_edge_weighs_exactly_0(driver):
    """The far side's moments made huge (a colour of 1e15: its square is finite) change no bit of the near side's variance."""
    w, h = 24, 10
    rng = np.random.default_rng(5)
    colour = np.ones((h, w, 4), F32)
    colour[..., :3] = rng.uniform(0.1, 1.0, (h, w, 3)).astype(F32)
    loud = colour.copy()
    loud[:, w // 2:, :3] = 1e15
    for R in RADII:
        a = run(driver, [edge_frame(w, h, colour)], tag="edge", flags=0, min_history=2, radius=R)[0]
        b = run(driver, [edge_frame(w, h, loud)], tag="edge_loud", flags=0, min_history=2, radius=R)[0]
        assert (a["variance"] > 0).all() and (b["variance"][:, : w // 2] > 0).all()
        assert np.array_equal(PH.bits(a["variance"])[:, : w // 2], PH.bits(b["variance"])[:, : w // 2])
        assert not np.array_equal(PH.bits(a["variance"])[:, w // 2:], PH.bits(b["variance"])[:, w // 2:])
        # ... and the near side's estimate is the one it has without a far side at all (the far half turned into misses)
        f = edge_frame(w, h, colour)
        depth = f.depth.copy(); depth[:, w // 2:] = -1.0
        c = run(driver, [TH.Frame(f.view_inv, f.proj_inv, f.m, f.radiance, f.normal, f.albedo, depth, f.inst)], tag="edge_miss", flags=0, min_history=2, radius=R)[0]
        assert np.array_equal(PH.bits(a["variance"])[:, : w // 2], PH.bits(c["variance"])[:, : w // 2])
        assert (c["variance"][:, w // 2:] == 0).all()      # a miss keeps the temporal step's 0


def test_an_isolated_young_pixel_stays_unknown(driver):
    """sw = 1 < min_weight: a young hit pixel whose every neighbour is a miss, one that is near with every neighbour far beyond a hard edge, and — with
    min_weight 4 — one of a pair of hit pixels with only each other for a neighbour, stay at -1."""
    w, h = 24, 12
    rng = np.random.default_rng(6)
    colour = np.ones((h, w, 4), F32)
    colour[..., :3] = rng.uniform(0.1, 1.0, (h, w, 3)).astype(F32)
    f = uniform_frame(w, h, colour)
    depth = np.full((h, w), 500.0, F32)
    depth[:, : w // 2] = -1.0                    # left half: misses ...
    lonely = [(3, 4), (8, 8), (0, 0)]            # ... but for these (x, y)
    for (x, y) in lonely:
        depth[y, x] = 5.0
    near = [(17, 5), (23, 11)]                   # right half: far, but for these near ones
    for (x, y) in near:
        depth[y, x] = 5.0
    fr = TH.Frame(f.view_inv, f.proj_inv, f.m, f.radiance, f.normal, f.albedo, depth, f.inst)
    for R in RADII:
        got = run(driver, [fr], tag="lonely", flags=0, min_history=2, radius=R)[0]
        v = got["variance"]
        for (x, y) in lonely + near:
            assert v[y, x] == -1, (R, x, y, v[y, x])
        assert (v[depth < 0] == 0).all()
        far = depth == 500.0
        estimated = far & (v >= 0)
        assert estimated.sum() > 100 and ((v[far] >= 0) | (v[far] == -1)).all()
    # a corner pair: two hit pixels alone, each other's only neighbour: sw = 2
    depth = np.full((h, w), -1.0, F32); depth[0, 0] = depth[0, 1] = 5.0
    fr = TH.Frame(f.view_inv, f.proj_inv, f.m, f.radiance, f.normal, f.albedo, depth, f.inst)
    v = run(driver, [fr], tag="pair", flags=0, min_history=2)[0]["variance"]
    assert v[0, 0] == -1 and v[0, 1] == -1
    v = run(driver, [fr], tag="pair2", flags=0, min_history=2, min_weight=2.0)[0]["variance"]
    assert v[0, 0] >= 0 and v[0, 1] >= 0 and v[0, 0] == v[0, 1]


def test_a_nan_moment_reaches_exactly_the_young_pixels_that_weigh_it(driver):
    """Uniform guides: every tap of a window weighs 1, every pixel outside it nothing.  A NaN colour in one pixel makes that pixel's moments NaN, and s1 and s2 of
    exactly the young pixels whose window holds it: max_(0, NaN) is 0 there (temporal_pixel_variance's answer to NaN moments too); every other pixel keeps its
    bits.  There is no guard: where a weight underflowed to exactly 0 the product 0 NaN is still NaN, as in denoise.hpp's sums — a hard edge stops huge
    moments (the test above), not NaNs."""
    w, h = 24, 12
    rng = np.random.default_rng(7)
    colour = np.ones((h, w, 4), F32)
    colour[..., :3] = rng.uniform(0.1, 1.0, (h, w, 3)).astype(F32)
    bad = colour.copy()
    px, py = 9, 5
    bad[py, px, 1] = np.nan
    yy, xx = np.mgrid[:h, :w]
    for R in RADII:
        a = run(driver, [uniform_frame(w, h, colour)], tag="clean", flags=0, min_history=2, radius=R)[0]
        b = run(driver, [uniform_frame(w, h, bad)], tag="nan", flags=0, min_history=2, radius=R)[0]
        assert np.isnan(b["moments"][py, px]).all() and np.isnan(b["moments"]).sum() == 2
        reached = np.maximum(np.abs(xx - px), np.abs(yy - py)) <= R
        assert (a["variance"] > 0).all()
        assert (b["variance"][reached] == 0).all() and reached.sum() == (2 * R + 1) ** 2
        assert np.array_equal(PH.bits(a["variance"])[~reached], PH.bits(b["variance"])[~reached])


def test_the_driver_is_clean_under_address_and_undefined_behaviour_sanitizers(driver, sequences, host_results, tmp_path):
    """Host code in a stand-alone program, on the inputs of the float64 comparison; the bits are the plain build's."""
    exe = PH.compile_driver(str(tmp_path / "svgf_spatial_driver_san"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    for (key, fl, mh, R), want in host_results.items():
        got = PH.run_sequence(exe, tmp_path, sequences[key], RUNS, tag="san", flags=fl, min_history=mh, radius=R, min_weight=MIN_WEIGHT)
        for g, w_ in zip(got, want):
            for name in ("image", "record", "moments", "variance"):
                assert np.array_equal(PH.bits(g[name]), PH.bits(w_[name])), (key, fl, mh, R, name)
            for x, y in zip(g["denoised"], w_["denoised"]):
                assert np.array_equal(PH.bits(x), PH.bits(y))
    off = PH.run_sequence(exe, tmp_path, sequences[(7, 5)], RUNS[:1], tag="san_off", flags=3, mode=0)
    assert (off[0]["variance"][sequences[(7, 5)][0].depth >= 0] == -1).all()
