"""csrc/firefly.hpp on the host (tests/tools/firefly_driver.cpp): the closed forms of the rule in its opening comment, the n < rank borders, what non-finite
pixels give, a float64 restatement (tests/ref_firefly64.py), and one run of the driver under the address and undefined-behaviour sanitizers.  The device is
held to these bits by tests/test_gpu_firefly.py."""
import subprocess

import numpy as np
import pytest

import firefly_host as FH
import ref_firefly64 as R

F32 = np.float32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return FH.compile_driver(str(tmp_path_factory.mktemp("firefly") / "firefly_driver"))


def scaled(rgb, limit, l_p):
    """firefly_pixel's clamp of one pixel in float32, in its order: s = limit / l_p, then the three products."""
    s = F32(limit) / F32(l_p)
    return np.asarray(rgb, F32) * s


def test_one_spike_in_a_flat_field_lands_on_threshold_times_the_field(driver, tmp_path):
    """A flat field of luminance a with threshold a >= floor, one spike of 8 a (coloured: 12 a, 8 a, 4 a): the limit is exactly threshold x the field's fp32
    luminance, the spike's three channels are multiplied by ONE factor limit / l_p — its channel ratios are kept — and nothing else changes a bit."""
    a = 1.5
    rad, alb, depth = FH.flat(9, 7, a)
    spike = np.array([12.0 * a, 8.0 * a, 4.0 * a], F32)
    rad[3, 4, :3] = spike
    for demodulate, albedo in ((0, 1.0), (1, 0.5)):
        alb[...] = albedo
        out = FH.run(driver, tmp_path, rad, alb, depth, demodulate=demodulate, threshold=2.0, floor=1.0)
        scale = F32(1.0) if not demodulate else F32(albedo)
        L = FH.luminance32(np.full(3, a, F32) / scale)                 # the field, as the filter sees it
        l_p = FH.luminance32(spike / scale)
        limit = F32(2.0) * L
        assert limit >= 1.0 and l_p > limit
        assert out["clamped"].sum() == 1 and out["clamped"][3, 4] and out["n_clamped"] == 1
        assert out["considered"].all() and out["n_considered"] == 63
        assert np.array_equal(FH.bits(out["image"][3, 4, :3]), FH.bits(scaled(spike, limit, l_p))) and out["image"][3, 4, 3] == 1.0
        got = FH.luminance32(out["image"][3, 4, :3] / scale)
        assert abs(float(got) - float(limit)) <= 4 * float(np.spacing(limit))          # threshold x a in luminance, to the rounding of three products and a sum
        assert np.allclose(out["image"][3, 4, :3] / out["image"][3, 4, 1], spike / spike[1], rtol=3e-7, atol=0)
        keep = np.ones((7, 9), bool); keep[3, 4] = False
        assert np.array_equal(FH.bits(out["image"])[keep], FH.bits(rad)[keep])


def test_two_adjacent_spikes_need_a_third_neighbour_at_rank_two(driver, tmp_path):
    """Rank 2, R = 1.  Inside a field two adjacent spikes see each other as the LARGEST tap, the second largest is the field: both are clamped (rank 1 would
    keep both).  The n < rank borders: a 1 x 1 image (n = 0) and a 2 x 1 image (n = 1) are untouched whatever they hold; in a 3 x 1 image with spikes at x = 0, 1
    the end pixel still has one tap only and stays, the middle one has two and is clamped to threshold x the third pixel.  A corner of an image of two rows or
    more has three taps, which serves every rank 1..3; in a single row rank 3 is considered nowhere at R = 1 (n <= 2) and only in the interior at R = 2 (n = 3, 4)."""
    a, big = 2.0, 50.0
    rad, alb, depth = FH.flat(8, 6, a)
    rad[2, 3, :3] = big; rad[2, 4, :3] = big
    out = FH.run(driver, tmp_path, rad, alb, depth, demodulate=0, rank=2)
    assert out["clamped"].sum() == 2 and out["clamped"][2, 3] and out["clamped"][2, 4]
    limit = F32(2.0) * FH.luminance32(np.full(3, a, F32))
    assert np.array_equal(FH.bits(out["image"][2, 3, :3]), FH.bits(scaled(rad[2, 3, :3], limit, FH.luminance32(rad[2, 3, :3]))))
    assert FH.run(driver, tmp_path, rad, alb, depth, demodulate=0, rank=1)["n_clamped"] == 0      # each is the other's largest neighbour
    # 1 x 1 and 2 x 1
    for w in (1, 2):
        r1, a1, d1 = FH.flat(w, 1, a)
        r1[0, :, :3] = big
        o = FH.run(driver, tmp_path, r1, a1, d1, demodulate=0, rank=2, floor=0.0)
        assert o["n_considered"] == 0 and o["n_clamped"] == 0 and np.array_equal(FH.bits(o["image"]), FH.bits(r1))
    o = FH.run(driver, tmp_path, r1, a1, d1, demodulate=0, rank=1, threshold=1.0, floor=0.0)           # 2 x 1 at rank 1: considered, equal: not above the limit
    assert o["n_considered"] == 2 and o["n_clamped"] == 0
    # 3 x 1: spikes at 0 and 1, the field at 2
    r3, a3, d3 = FH.flat(3, 1, a)
    r3[0, :2, :3] = big
    o = FH.run(driver, tmp_path, r3, a3, d3, demodulate=0, rank=2)
    assert o["considered"].tolist() == [[False, True, False]] and o["clamped"].tolist() == [[False, True, False]]
    assert np.array_equal(FH.bits(o["image"][0, 1, :3]), FH.bits(scaled(r3[0, 1, :3], limit, FH.luminance32(r3[0, 1, :3]))))
    # corners and single rows, rank 3
    r4, a4, d4 = FH.flat(2, 2, a)
    assert FH.run(driver, tmp_path, r4, a4, d4, demodulate=0, rank=3)["considered"].all()
    r5, a5, d5 = FH.flat(7, 1, a)
    assert FH.run(driver, tmp_path, r5, a5, d5, demodulate=0, rank=3, radius=1)["n_considered"] == 0
    assert FH.run(driver, tmp_path, r5, a5, d5, demodulate=0, rank=3, radius=2)["considered"].tolist() == [[False, True, True, True, True, True, False]]


def test_misses_keep_their_bits_and_are_never_taps(driver, tmp_path):
    """A spike whose window holds no other hit is untouched (n = 0), however bright the misses around it; a miss keeps its bits whatever it holds; and a miss
    beside a spike in a field does not enter the order statistic: the limit is the field's."""
    rad, alb, depth = FH.flat(5, 5, 1.0)
    depth[...] = -1.0
    rad[..., :3] = 1000.0
    depth[2, 2] = 3.0
    rad[2, 2, :3] = 77.0
    for radius in (1, 2):
        o = FH.run(driver, tmp_path, rad, alb, depth, demodulate=0, rank=1, radius=radius, floor=0.0)
        assert o["n_considered"] == 0 and o["n_clamped"] == 0 and np.array_equal(FH.bits(o["image"]), FH.bits(rad))
    a = 2.0
    rad, alb, depth = FH.flat(7, 7, a)
    rad[3, 3, :3] = 64.0
    for q in ((2, 3), (3, 4), (4, 4)):
        depth[q] = -1.0
        rad[q[0], q[1], :3] = (1e6, np.nan, -5.0)
    o = FH.run(driver, tmp_path, rad, alb, depth, demodulate=0, rank=1)
    limit = F32(2.0) * FH.luminance32(np.full(3, a, F32))
    assert o["n_clamped"] == 1 and np.array_equal(FH.bits(o["image"][3, 3, :3]), FH.bits(scaled(rad[3, 3, :3], limit, FH.luminance32(rad[3, 3, :3]))))
    miss = depth < 0
    assert np.array_equal(FH.bits(o["image"])[miss], FH.bits(rad)[miss]) and not o["considered"][miss].any()


def test_floor_holds_when_the_neighbours_are_black(driver, tmp_path):
    rad, alb, depth = FH.flat(5, 4, 0.0)
    rad[1, 1, :3] = (8.0, 4.0, 2.0)
    rad[2, 3, :3] = 0.75                  # below the floor: never touched, whatever surrounds it
    o = FH.run(driver, tmp_path, rad, alb, depth, demodulate=0, floor=1.0)
    assert o["clamped"].sum() == 1 and o["clamped"][1, 1]
    assert np.array_equal(FH.bits(o["image"][1, 1, :3]), FH.bits(scaled(rad[1, 1, :3], 1.0, FH.luminance32(rad[1, 1, :3]))))
    assert abs(float(FH.luminance32(o["image"][1, 1, :3])) - 1.0) <= 4 * float(np.spacing(F32(1.0)))
    assert np.array_equal(FH.bits(o["image"][2, 3]), FH.bits(rad[2, 3]))


def test_non_finite_pixels(driver, tmp_path):
    """A NaN neighbour is skipped — the limit is what the other taps give; a NaN centre keeps its bits (NaN > limit is false) though it is considered; a +inf
    neighbour IS a tap.  What a +inf centre gives is pinned, not prescribed: over a finite limit s = limit / inf = 0, so its finite channels become 0 and its
    infinite ones 0 inf = NaN, and it counts as clamped; over an infinite limit (a +inf neighbour at the rank) inf > inf is false and it keeps its bits."""
    a = 2.0
    limit = F32(2.0) * FH.luminance32(np.full(3, a, F32))
    rad, alb, depth = FH.flat(6, 6, a)
    rad[2, 2, :3] = 40.0
    rad[2, 3, :3] = (np.nan, 1.0, 1.0)               # a NaN neighbour of the spike, itself a NaN centre
    with np.errstate(all="ignore"):
        o = FH.run(driver, tmp_path, rad, alb, depth, demodulate=0, rank=1)
        assert o["clamped"].sum() == 1 and np.array_equal(FH.bits(o["image"][2, 2, :3]), FH.bits(scaled(rad[2, 2, :3], limit, FH.luminance32(rad[2, 2, :3]))))
        assert o["considered"][2, 3] and not o["clamped"][2, 3] and np.array_equal(FH.bits(o["image"][2, 3]), FH.bits(rad[2, 3]))
        # +inf centre over a finite limit
        rad, alb, depth = FH.flat(6, 6, a)
        rad[3, 3, :3] = (np.inf, 5.0, 7.0)
        o = FH.run(driver, tmp_path, rad, alb, depth, demodulate=0, rank=2)
        px = o["image"][3, 3]
        assert o["clamped"][3, 3] and np.isnan(px[0]) and px[1] == 0.0 and px[2] == 0.0 and px[3] == 1.0
        # a +inf neighbour is a tap: at rank 1 it is every neighbour's limit, nothing around it is clamped; and the +inf centre beside ANOTHER +inf stays
        rad[3, 4, :3] = (np.inf, 5.0, 7.0)
        o = FH.run(driver, tmp_path, rad, alb, depth, demodulate=0, rank=1)
        assert o["n_clamped"] == 0 and np.array_equal(FH.bits(o["image"]), FH.bits(rad))


# max over the clamped pixels' channels of |host - float64| / |float64|, measured over every case below: 2.48e-7 at 45 x 37, 1.65e-7 at 7 x 5, 2.52e-7 at
# 150 x 9 (a handful of fp32 roundings of 6e-8 each: the demodulating quotients, the luminance sums of centre and neighbour, threshold L, limit / l_p, the product)
MEASURED_COLOUR_REL = 2.52e-7
MARGIN, MARGINAL_CAP = 1e-5, 0.01


@pytest.mark.parametrize("size", [(45, 37), (7, 5), (150, 9)])
def test_against_the_float64_restatement(driver, tmp_path, size, capsys):
    """Random guides with planted spikes (>= 4 x the local level over a field varying +- 10 %), every radius, rank and both demodulations.  The decision
    l_p > limit is discontinuous: a pixel whose float64 l_p lies within a relative 1e-5 of its float64 limit is marginal and left out — at most 1 % of the hit
    pixels, which the restatement alone is first held to.  On the others the clamped / untouched decision agrees everywhere, `considered` agrees on all pixels,
    untouched pixels keep their bits and the colour of the clamped ones is within 4 x the measured 2.52e-7 (relative, per channel)."""
    w, h = size
    rad, alb, depth, spikes = FH.spiked(w, h, seed=7 * w + h)
    hits = int((depth >= 0).sum())
    assert hits > 0.7 * w * h and spikes.sum() >= 3
    worst, seen = 0.0, 0
    for radius in (1, 2):
        for rank in (1, 2, 3):
            for demodulate in (1, 0):
                ref = R.firefly(rad, alb, depth, radius=radius, rank=rank, threshold=2.0, floor=1.0, demodulate=bool(demodulate))
                with np.errstate(invalid="ignore"):
                    marginal = ref["considered"] & (np.abs(ref["l_p"] - ref["limit"]) <= MARGIN * ref["limit"])
                assert marginal.sum() <= MARGINAL_CAP * hits, (radius, rank, demodulate, int(marginal.sum()))
                got = FH.run(driver, tmp_path, rad, alb, depth, radius=radius, rank=rank, threshold=2.0, floor=1.0, demodulate=demodulate)
                assert np.array_equal(got["considered"], ref["considered"])
                ok = ~marginal
                assert np.array_equal(got["clamped"][ok], ref["clamped"][ok]), (radius, rank, demodulate)
                assert got["n_clamped"] == got["clamped"].sum() and got["n_considered"] == got["considered"].sum()
                assert np.array_equal(FH.bits(got["image"])[~got["clamped"]], FH.bits(rad)[~got["clamped"]])
                both = ok & got["clamped"]
                seen += int(both.sum())
                if not both.any():      # (7 x 5 at rank 1: its spikes stand in pairs)
                    continue
                a, b = got["image"][both][:, :3].astype(np.float64), ref["image"][both][:, :3]
                worst = max(worst, float((np.abs(a - b) / np.abs(b)).max()))
                assert np.array_equal(got["image"][both][:, 3], rad[both][:, 3])
    with capsys.disabled():
        print("\nfirefly vs float64 at %d x %d: colour rel %.3e over %d clamped pixels" % (w, h, worst, seen))
    assert seen >= 12 and worst <= 4.0 * MEASURED_COLOUR_REL


def test_driver_is_clean_under_the_sanitizers(driver, tmp_path):
    """The stand-alone driver, built with -fsanitize=address,undefined and made to stop at the first report, on the inputs above (image edges at both radii,
    misses, non-finite pixels): it ends clean and writes the bytes the plain build writes."""
    exe = FH.compile_driver(str(tmp_path / "firefly_driver_san"), extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    for k, (w, h) in enumerate([(45, 37), (7, 5), (150, 9), (1, 1)]):
        rad, alb, depth, _ = FH.spiked(w, h, seed=7 * w + h)
        if w > 4:
            rad[1, 2, :3] = (np.nan, np.inf, -1.0); rad[h - 1, w - 1, :3] = np.inf; rad[0, 0, :3] = 3.0e38
        for radius, rank, demodulate in ((1, 2, 1), (2, 3, 0)):
            a = FH.run(exe, tmp_path, rad, alb, depth, tag="san", radius=radius, rank=rank, demodulate=demodulate)
            b = FH.run(driver, tmp_path, rad, alb, depth, tag="plain", radius=radius, rank=rank, demodulate=demodulate)
            assert np.array_equal(FH.bits(a["image"]), FH.bits(b["image"])) and (a["n_clamped"], a["n_considered"]) == (b["n_clamped"], b["n_considered"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 2 and "usage" in out.stderr
