"""SVGF's variance without a device: the new functions of csrc/temporal.hpp (temporal_pixel_variance) and csrc/denoise.hpp (prepare_pixel_variance,
atrous_pixel_variance) compiled for the host (tests/tools/svgf_driver.cpp, driven as api_post.hip drives the kernels), held to
  * a float64 restatement written from the description (tests/ref_svgf64.py), on the analytic frames of tests/temporal_host.py;
  * the constructed properties, exactly: what the option must leave alone, what is unknown, what has no influence;
  * AddressSanitizer / UBSan: the same driver built with -fsanitize=address,undefined, as a stand-alone program.
The same functions on the device, against this host compile bit for bit: tests/test_gpu_svgf.py."""
import numpy as np
import pytest

import denoise_host as DH
import ref_svgf64 as S64
import ref_temporal64 as R64
import svgf_host as SH
import temporal_host as TH

F32 = np.float32
SIZES = [(45, 37), (150, 9), (7, 5)]
FLAG_SETS = [0, TH.DEMODULATE | TH.MATCH_INSTANCE]
MIN_HISTORIES = [1, 4]
# Frames per step.  With temporal_host's own (2, 1, 3, 2) a pixel of full history reaches 6 + 2 = 8 = min_history m in the last step, and whether the mean of four
# sixes is 6 or an ulp less decides "known": with these no attainable length lies on a threshold (3 and 1 under 4; 7 and 4 under 16; 8, 5 and what lies between over 4).
MS = (2, 1, 4, 1)
RUNS = [SH.denoise_run(1, 1), SH.denoise_run(3, 0), SH.denoise_run(5, 1), SH.denoise_run(3, 1 | SH.KEEP_VARIANCE)]
P = TH.DEFAULTS
# Host compile against float64, measured on these inputs (x86-64-v3, g++ -O2) over every size, flag set, min_history and step, per hit pixel that neither
# restatement calls marginal (at most 5 % per step, asserted).  The rule: the suite's 1e-4 where the measured figure is at most a quarter of it, otherwise 4 x the figure.
#   moments, relative (|host - float64| / |float64|, the larger of mu1's and mu2's):       3.94e-04 (45 x 37, no demodulation)       -> 1.6e-3
#   variance, absolute in units of the pixel's mu2 (a cancelling difference):              3.93e-04 (the same pixel)                 -> 1.6e-3
#   variance-guided image, relative per pixel (max |diff| over r, g, b / largest channel): 8.01e-05 (45 x 37, demodulated, 5 passes)  -> 3.3e-4
#   filtered variance of the KEEP_VARIANCE run, absolute in units of the image's largest:  6.79e-07                                  -> 1e-4
# The moments' ABSOLUTE error is the colour's of tests/test_temporal_cpu.py — at most 2.3e-5 here, the reprojected position's 1e-5 of a pixel times the difference
# between neighbouring history pixels — and the relative figure is that over the moments of the black-albedo band, whose undemodulated colours are 1e-3 of the
# others (mu1 = 6.9e-4 at the worst pixel); with demodulation it is 1.1e-4.
TOL_MOMENTS = 1.6e-3
TOL_VARIANCE = 1.6e-3
TOL_IMAGE = 3.3e-4
TOL_FILTERED = 1e-4
LEFT_OUT_CAP = 0.05


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("svgf")
    return SH.compile_driver(str(d / "svgf_driver")), d


@pytest.fixture(scope="module")
def sequences():
    return {(w, h): TH.analytic_sequence(w, h, ms=MS) for (w, h) in SIZES}


@pytest.fixture(scope="module")
def host_results(driver, sequences):
    exe, d = driver
    return {(key, fl, mh): SH.run_sequence(exe, d, frames, RUNS, tag="seq_%d_%d_%d_%d" % (key + (fl, mh)), flags=fl, min_history=mh)
            for key, frames in sequences.items() for fl in FLAG_SETS for mh in MIN_HISTORIES}


def run(driver, frames, runs=(), tag="p", **kw):
    return SH.run_sequence(driver[0], driver[1], frames, runs, tag=tag, **kw)


def state_of(frame, record):
    return R64.State(record[..., :3].astype(np.float64), record[..., 3].astype(np.float64), frame.normal[..., :3].astype(np.float64), frame.depth.astype(np.float64),
                     frame.inst, frame.view_inv, frame.proj_inv)


@pytest.mark.parametrize("mh", MIN_HISTORIES)
@pytest.mark.parametrize("flags", FLAG_SETS)
@pytest.mark.parametrize("key", SIZES, ids=lambda k: "%dx%d" % k)
def test_host_compile_against_float64(sequences, host_results, key, flags, mh):
    """Every step on its own: its history is what the host compile left behind the step before."""
    frames, results = sequences[key], host_results[(key, flags, mh)]
    worst = dict(moments=0.0, variance=0.0, image=0.0, filtered=0.0)
    known_total = 0
    for k, fr in enumerate(frames):
        prev = state_of(frames[k - 1], results[k - 1]["record"]) if k else None
        prev_mu = results[k - 1]["moments"].astype(np.float64) if k else None
        args = (fr.view_inv, fr.proj_inv, fr.m, fr.radiance, fr.normal, fr.albedo, fr.depth, fr.inst, P["max_history"], P["depth_tolerance"], P["normal_threshold"], flags)
        info = R64.temporal64(prev, *args)[3]
        mu, var, length, close = S64.moments64(prev, prev_mu, *args, mh)
        hit = fr.depth >= 0
        left_out = info["marginal"] | close
        assert left_out.sum() <= LEFT_OUT_CAP * hit.sum(), (key, k, left_out.sum(), hit.sum())
        keep = hit & ~left_out
        got = results[k]
        err_mu = (np.abs(got["moments"] - mu) / np.maximum(np.abs(mu), 1e-30))[keep].max()
        gv = got["variance"].astype(np.float64)
        assert np.array_equal(gv[keep] < 0, var[keep] < 0)
        known = keep & (var >= 0)
        known_total += int(known.sum())
        err_var = (np.abs(gv - var) / np.maximum(mu[..., 1], 1e-30))[known].max() if known.any() else 0.0
        worst["moments"] = max(worst["moments"], err_mu); worst["variance"] = max(worst["variance"], err_var)
        # the filter, fed what the host compile's temporal step gave it
        for r, out in zip(RUNS, got["denoised"]):
            keepv = bool(r[1] & SH.KEEP_VARIANCE)
            ref = S64.denoise_variance64(got["image"], got["variance"], fr.normal, fr.albedo, fr.depth, r[0], r[2], r[3], r[4], r[1] & 1, SH.SVGF_DEFAULTS["sigma_luminance"], keepv)
            rel = np.abs(out[..., :3] - ref[..., :3]).max(-1) / np.maximum(np.abs(ref[..., :3]).max(-1), 1e-30)
            worst["image"] = max(worst["image"], rel[hit].max())
            assert np.array_equal(SH.bits(out)[~hit], SH.bits(got["image"])[~hit])
            if keepv:
                kn = hit & (ref[..., 3] >= 0)
                assert np.array_equal(out[..., 3][hit] < 0, ref[..., 3][hit] < 0)
                if kn.any():
                    worst["filtered"] = max(worst["filtered"], np.abs(out[..., 3] - ref[..., 3])[kn].max() / ref[..., 3][kn].max())
            else:
                assert np.array_equal(SH.bits(out)[..., 3], SH.bits(got["image"])[..., 3])     # alpha is the source's
    print("%s flags %d min_history %d: max moments rel %.3g, variance / mu2 %.3g, image rel %.3g, filtered variance / max %.3g; %d known" %
          (key, flags, mh, worst["moments"], worst["variance"], worst["image"], worst["filtered"], known_total))
    assert worst["moments"] <= TOL_MOMENTS and worst["variance"] <= TOL_VARIANCE and worst["image"] <= TOL_IMAGE and worst["filtered"] <= TOL_FILTERED
    if key != (7, 5):
        assert known_total > 50


def test_the_option_off_gives_the_bits_of_temporal_pixel_and_atrous_pixel(driver, sequences, host_results, tmp_path):
    """variance = 0 in the driver calls temporal_pixel / atrous_pixel: it equals the existing drivers, and with the option on image and record keep those bits."""
    t_exe = TH.compile_driver(str(tmp_path / "temporal_driver"))
    d_exe = DH.compile_driver(str(tmp_path / "denoise_driver"))
    for key in SIZES:
        frames = sequences[key]
        for fl in FLAG_SETS:
            plain = TH.run_sequence(t_exe, tmp_path, frames, tag="plain", flags=fl)
            off = run(driver, frames, RUNS[:3], tag="off", flags=fl, variance=0)
            on = host_results[(key, fl, 4)]
            for k, fr in enumerate(frames):
                for other in (off[k], on[k]):
                    assert np.array_equal(SH.bits(other["image"]), SH.bits(plain[k][0])) and np.array_equal(SH.bits(other["record"]), SH.bits(plain[k][1])), (key, fl, k)
                assert not off[k]["variance"].any() and not off[k]["moments"].any()
                for r, out in zip(RUNS[:3], off[k]["denoised"]):
                    want = DH.run_driver(d_exe, tmp_path, plain[k][0], fr.normal, fr.albedo, fr.depth, r[0], r[2], r[3], r[4], r[1], tag="dn")
                    assert np.array_equal(SH.bits(out), SH.bits(want)), (key, fl, k, r)


def test_a_pixel_of_unknown_variance_gets_the_fixed_sigma_result_bit_for_bit(driver, sequences, tmp_path):
    """min_history so large that every variance is -1: every pass of every pixel is the fixed-sigma_color rule, alpha included.  And in a field that mixes
    known and unknown pixels, the unknown ones have the fixed rule's bits after ONE pass (their taps are every hit tap, whatever its variance)."""
    d_exe = DH.compile_driver(str(tmp_path / "denoise_driver"))
    frames = sequences[(45, 37)]
    for fl in FLAG_SETS:
        never = run(driver, frames, RUNS[:3], tag="never", flags=fl, min_history=1000)
        mixed = run(driver, frames, RUNS[:1], tag="mixed", flags=fl, min_history=3)
        unknown_in_mixed = 0
        for k, fr in enumerate(frames):
            hit = fr.depth >= 0
            assert (never[k]["variance"][hit] == -1).all() and (never[k]["variance"][~hit] == 0).all()
            for r, out in zip(RUNS[:3], never[k]["denoised"]):
                want = DH.run_driver(d_exe, tmp_path, never[k]["image"], fr.normal, fr.albedo, fr.depth, r[0], r[2], r[3], r[4], r[1], tag="dn")
                assert np.array_equal(SH.bits(out), SH.bits(want)), (fl, k, r)
            r = RUNS[0]
            want = DH.run_driver(d_exe, tmp_path, mixed[k]["image"], fr.normal, fr.albedo, fr.depth, r[0], r[2], r[3], r[4], r[1], tag="dn1")
            unknown = hit & (mixed[k]["variance"] < 0)
            if k == 3:
                assert unknown.sum() > 20 and (hit & ~unknown).sum() > 20
                unknown_in_mixed += int(unknown.sum())
                assert not np.array_equal(SH.bits(mixed[k]["denoised"][0])[hit & ~unknown], SH.bits(want)[hit & ~unknown])      # ... and the known ones do not
            assert np.array_equal(SH.bits(mixed[k]["denoised"][0])[unknown], SH.bits(want)[unknown]), (fl, k)
        assert unknown_in_mixed > 20


def test_the_variance_is_unknown_below_min_history_images_and_zero_on_a_miss(sequences, host_results):
    for (key, fl, mh), results in host_results.items():
        for fr, got in zip(sequences[key], results):
            hit = fr.depth >= 0
            length, var = got["record"][..., 3], got["variance"]
            short = hit & (length < F32(mh) * F32(fr.m))
            assert (var[short] == -1).all() and (var[hit & ~short] >= 0).all(), (key, fl, mh)
            assert (var[~hit] == 0).all() and not got["moments"][~hit].any()
            assert np.array_equal(SH.bits(got["image"])[~hit], SH.bits(fr.radiance)[~hit])


def test_a_miss_is_no_tap(driver, sequences, host_results):
    """A huge colour in every miss pixel of every frame: the hit pixels keep their bits — image, record, moments, variance and every filtered image."""
    frames = sequences[(45, 37)]
    fl = TH.DEMODULATE | TH.MATCH_INSTANCE
    loud_frames = []
    for fr in frames:
        rad = fr.radiance.copy()
        rad[fr.depth < 0, :3] = 1e30
        loud_frames.append(TH.Frame(fr.view_inv, fr.proj_inv, fr.m, rad, fr.normal, fr.albedo, fr.depth, fr.inst))
    loud = run(driver, loud_frames, RUNS, tag="loud", flags=fl, min_history=1)
    for fr, a, b in zip(frames, host_results[((45, 37), fl, 1)], loud):
        hit = fr.depth >= 0
        assert (~hit).sum() > 20
        for name in ("image", "record", "moments", "variance"):
            assert np.array_equal(SH.bits(a[name])[hit], SH.bits(b[name])[hit]), name
        for x, y in zip(a["denoised"], b["denoised"]):
            assert np.array_equal(SH.bits(x)[hit], SH.bits(y)[hit])
            assert (y[~hit][:, :3] == F32(1e30)).all()


def uniform_frame(w, h, colour):
    """One plane seen head-on: every pixel a hit of the same normal and depth, albedo 1."""
    f0 = TH.analytic_frame(w, h, TH.CAMERAS[0], 1, seed=1)
    normal = np.zeros((h, w, 4), F32); normal[..., 2] = 1.0
    return TH.Frame(f0.view_inv, f0.proj_inv, 1, colour, normal, np.ones((h, w, 4), F32), np.full((h, w), 5.0, F32), np.zeros((h, w), np.uint32))


def test_a_constant_luminance_history_has_variance_0_and_other_luminances_weigh_exactly_0(driver):
    """A history of one image (min_history 1): mu2 = l l and mu1 mu1 = l l are one product, so the variance is 0 on every hit pixel, g = 0, the divisor of dl is
    1e-6, and a tap whose luminance differs by 0.3 has dl = 3e5: exp_ returns exactly 0 below -103.9.  The right half made huge changes no bit of the left."""
    w, h = 24, 10
    colour = np.ones((h, w, 4), F32)
    colour[:, : w // 2, :3] = (0.5, 0.5, 0.5)
    colour[:, w // 2:, :3] = (0.8, 0.8, 0.8)
    runs = [SH.denoise_run(4, 0), SH.denoise_run(4, SH.KEEP_VARIANCE)]
    a = run(driver, [uniform_frame(w, h, colour)], runs, tag="halves", flags=0, min_history=1)[0]
    assert (a["variance"] == 0).all()
    loud = colour.copy()
    loud[:, w // 2:, :3] = 1e15           # (its square is finite: the right half's own variance is 0 too)
    b = run(driver, [uniform_frame(w, h, loud)], runs, tag="halves_loud", flags=0, min_history=1)[0]
    assert (b["variance"] == 0).all()
    for x, y in zip(a["denoised"], b["denoised"]):
        assert np.array_equal(SH.bits(x)[:, : w // 2], SH.bits(y)[:, : w // 2])
    assert np.abs(a["denoised"][0][:, : w // 2, :3] - 0.5).max() <= 1e-6 and (a["denoised"][1][..., 3] == 0).all()


def test_equal_weights_filter_a_constant_variance_by_the_squared_kernel(driver):
    """Uniform guides and one colour: every weight is 1.  A variance image of one value v = 2^-3 comes out of a pass as v sum (k)^2 / (sum k)^2 over the taps
    inside the image: where all 25 are, sum k = 1 and sum k^2 = (35/128)^2 are sums of dyadic rationals, and the result is v (35/128)^2 EXACTLY."""
    w, h = 19, 11
    colour = np.broadcast_to(np.array([0.7, 1.9, 3.3, 1.0], F32), (h, w, 4)).copy()
    v = F32(0.125)
    got = run(driver, [uniform_frame(w, h, colour)], [SH.denoise_run(1, SH.KEEP_VARIANCE), SH.denoise_run(1, 0)], tag="constv", flags=0,
              given_variance=[np.full((h, w), v, F32)])[0]
    k = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
    want = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            ky = k[[d + 2 for d in range(-2, 3) if 0 <= y + d < h]]; kx = k[[d + 2 for d in range(-2, 3) if 0 <= x + d < w]]
            want[y, x] = float(v) * (ky ** 2).sum() * (kx ** 2).sum() / ((ky.sum() * kx.sum()) ** 2)
    out = got["denoised"][0][..., 3]
    assert np.array_equal(out[2:-2, 2:-2], np.full((h - 4, w - 4), F32(float(v) * (35 / 128) ** 2)))
    assert np.abs(out / want - 1).max() <= 1e-6
    assert np.abs(got["denoised"][0][..., :3] / colour[..., :3] - 1).max() <= 1e-6
    assert (got["denoised"][1][..., 3] == 1).all()          # the last pass returns alpha


def test_the_driver_is_clean_under_address_and_undefined_behaviour_sanitizers(driver, sequences, host_results, tmp_path):
    """Host code in a stand-alone program, on the inputs of the float64 comparison; the bits are the plain build's."""
    exe = SH.compile_driver(str(tmp_path / "svgf_driver_san"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    for (key, fl, mh), want in host_results.items():
        got = SH.run_sequence(exe, tmp_path, sequences[key], RUNS, tag="san", flags=fl, min_history=mh)
        for g, w_ in zip(got, want):
            for name in ("image", "record", "moments", "variance"):
                assert np.array_equal(SH.bits(g[name]), SH.bits(w_[name])), (key, fl, mh, name)
            for x, y in zip(g["denoised"], w_["denoised"]):
                assert np.array_equal(SH.bits(x), SH.bits(y))
    off = SH.run_sequence(exe, tmp_path, sequences[(7, 5)], RUNS[:1], tag="san_off", flags=3, variance=0)
    assert not off[-1]["variance"].any()
