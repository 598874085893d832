"""A context whose size the library chose (vpt_config.frames_in_flight = 0) renders one long batch, then changes to a schedule that keeps every
sample resident, at 1280x720 — where the 8192-frame bound does not bind, so the long batch really is 4 x F frames.  The path buffers must be
re-planned for the new schedule within the memory F was chosen from (csrc/path_plan.hpp; the arithmetic itself: tests/test_path_plan_cpu.py)
instead of failing with VPT_ERR_OUT_OF_MEMORY, and the image must be the oracle's on 64 pixels.  Holds 65-150 GB while it runs."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W, H = 1280, 720
SAMPLE_BYTES, RESIDENT_BYTES = 36, 286   # path_plan.hpp kSampleBytes / kResidentBytes


def crop_pixels():
    rng = np.random.default_rng(11)
    return rng.integers(0, W, 64).astype(np.uint32), rng.integers(0, H, 64).astype(np.uint32)


def running_mean(smp):
    """The running mean of the frames in order, as RayGen.slang:130-159 forms it: frame 0, then lerp(old, new, 1 / (k + 1)) in fp32."""
    c = smp[:, 0, :].astype(np.float32)
    for k in range(1, smp.shape[1]):
        c = (c + (smp[:, k, :] - c) * (np.float32(1.0) / np.float32(k + 1))).astype(np.float32)
    return c


def check_crops(oracle, sc, img, params, frames, volumes=()):
    xs, ys = crop_pixels()
    o = oracle.Oracle(sc, W, H); o.set_params(params)
    if volumes:
        o.set_volumes(list(volumes))
    smp = o.pixel_samples(xs, ys, 0, frames); o.close()
    assert np.array_equal(img[ys, xs, :3], running_mean(smp))


def check_plan(st, F, batch):
    """(a) of tests/test_path_plan_cpu.py: no more than the all-resident batch of F frames; (c) the batch is resident."""
    fa, rf = st["frames_allocated"], st["resident_frames"]
    assert fa * SAMPLE_BYTES + rf * RESIDENT_BYTES <= F * (SAMPLE_BYTES + RESIDENT_BYTES), (fa, rf, F)
    assert fa >= batch and rf >= batch, (fa, rf, batch)


def test_long_whole_batch_then_two_samples_per_frame(vpt, oracle, scenes):
    sc = scenes("cornell_box")
    P = vpt.default_params(max_depth=8)
    g = vpt.PathTracer(W, H)
    F = g.stats()["frames_in_flight"]                # no scene yet: the all-resident cap the library chose
    g.set_scene(sc); g.set_params(P)
    long = g.stats()["frames_in_flight"]
    assert long == 4 * F and long < 8192
    g.render(long)                                   # one call, one whole-path batch of 4 F frames: 36 B per sample
    st = g.stats()
    assert (st["frames_allocated"], st["resident_frames"]) == (long, 1)
    check_crops(oracle, sc, g.radiance(), P, long)
    P2 = vpt.default_params(max_depth=8, samples_per_frame=2)
    g.set_params(P2)                                 # leaves the whole-path launch; an LDS scene does not regenerate
    g.render(2)
    st = g.stats()
    check_plan(st, F, 2)
    assert st["frames_in_flight"] == F
    check_crops(oracle, sc, g.radiance(), P2, 2)
    g.close()


def test_long_regenerating_batch_then_a_volume(vpt, oracle, scenes):
    sc = scenes("cornell_box_glass")
    P = vpt.default_params(max_depth=8)
    g = vpt.PathTracer(W, H)
    F = g.stats()["frames_in_flight"]
    g.set_scene(sc); g.set_params(P)
    long = g.stats()["frames_in_flight"]
    assert long == 4 * F and long < 8192
    g.render(long)                                   # regenerating: 4 F frames, F / 2 of them resident
    st = g.stats()
    assert (st["frames_allocated"], st["resident_frames"]) == (long, F // 2)
    check_crops(oracle, sc, g.radiance(), P, long)
    fog = [vpt.volume(corner_min=(-5.0, -10.5, -5.0), corner_max=(5.0, -0.5, 5.0), color=(0.9, 0.85, 0.8), density=0.12, anisotropy=0.3)]
    g.set_volumes(fog)                               # media keep every sample resident: more frames than the F / 2 resident ones
    n = F // 2 + 1
    g.render(n)
    st = g.stats()
    check_plan(st, F, n)
    check_crops(oracle, sc, g.radiance(), P, n, fog)
    g.close()
