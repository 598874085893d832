"""tests/trace_ray_sets.py without a GPU: the sets are seeded, keep the ray counts the vpt_trace_rays tests have always used and one tmin / tmax each,
and the shadow tests' sets are what tests/test_gpu_trace_stream.py needs them to be — judged by the oracle's brute force alone."""
import json

import numpy as np

import trace_ray_sets as T

COUNTS = {"random_glass": 200000, "random_viking": 60000, "axis_aligned": 7500, "window": 50000, "scaled_0.001": 60000, "scaled_1000": 60000,
          "scaled_37000": 60000, "far_30": 40000, "far_1000": 40000, "affine": 220000, "chain": 6000}


def test_sets_are_seeded_and_keep_their_sizes(vpt):
    assert sorted(COUNTS) == sorted(T.SETS)
    for name in T.SETS:
        _, rays = T.load(vpt, name)
        assert rays.dtype == np.float32 and rays.shape == (COUNTS[name], 8), name
        assert len(np.unique(rays[:, 3])) == 1 and len(np.unique(rays[:, 7])) == 1, name
    assert T.axis_aligned_rays().tobytes() == T.load(vpt, "axis_aligned")[1].tobytes()
    assert T.scaled_rays(1e3).tobytes() == T.load(vpt, "scaled_1000")[1].tobytes() and T.far_rays(30.0).tobytes() == T.load(vpt, "far_30")[1].tobytes()
    assert [float(n[len("scaled_"):]) for n in T.SETS if n.startswith("scaled_")] == list(T.SCALES)
    assert [float(n[len("far_"):]) for n in T.SETS if n.startswith("far_")] == list(T.FAR)
    # the degenerate set: every direction has two zero components, and half the origins lie on the wall plane exactly
    _, rays = T.load(vpt, "axis_aligned")
    assert ((rays[:, 4:7] == 0).sum(axis=1) == 2).all() and (rays[:, 0] == np.float32(T.WALL)).sum() >= len(rays) // 2
    assert tuple(T.load(vpt, "window")[1][0, [3, 7]]) == T.WINDOW


def test_light_rays_come_in_triples(vpt):
    for name in T.LIGHT_SCENES:
        rays, expect, media = T.light_rays(vpt, name)
        again = T.light_rays(vpt, name)
        assert rays.tobytes() == again[0].tobytes() and expect.tobytes() == again[1].tobytes()
        assert np.array_equal(rays[0::3], rays[1::3]) and np.array_equal(rays[0::3, 0:3], rays[2::3, 0:3])
        assert (expect[0::3] != expect[1::3]).all() and np.array_equal(expect[0::3], expect[2::3])
        assert not media[0::3].any() and not media[1::3].any() and media[2::3].all()
    assert T.hole_mask(70).sum() == 10 and T.hole_mask(3).sum() == 0
    assert T.beyond_static_sizes(256) == (786432, 786432 + 77)


def test_the_shadow_sets_meet_their_conditions(vpt, oracle):
    print(json.dumps(T.check_conditions(vpt, oracle)))
