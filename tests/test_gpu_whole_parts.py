"""A whole-path batch in PARTS (path_plan.hpp Schedule::parts, api_render.hip batch_begin / batch_resolve): one launch of k_whole and one
resolve per part, the resolve of part i on the lane's second stream beside the launch of part i + 1.  The rule splits only batches of the
headline's size, so the tests force the part count through VPT_LAB_WHOLE_PARTS — a laboratory entry point: tests/gpu_whole_parts_run.py
renders everything once in a process that loads the laboratory library, and the tests compare what it left.  Seeds come from (pixel,
dispatch index) and the resolves run in part order, so every image is the unsplit one bit for bit, and the oracle's.
50 x 37 = 1850 pixels is no multiple of 64: every part ends in a ragged tile and tiles straddle rows."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"ragged": (50, 37), "even": (64, 48), "shard": (64, 48)}
PARTS = (1, 2, 3, 7, 8)
FRAMES, DEPTH = 7, 8
RAY_STATS = ("samples", "closest_rays", "shadow_rays", "primary_hits", "connect_paths")


@pytest.fixture(scope="module")
def runs(vpt, tmp_path_factory):
    vpt.build(lab=True)
    out = str(tmp_path_factory.mktemp("whole_parts") / "runs.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_whole_parts_run.py"), out], env=dict(os.environ, VPT_LAB="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    z = np.load(out)
    return {k: z[k] for k in z.files if k != "stats"}, json.loads(str(z["stats"]))


@pytest.fixture(scope="module")
def refs(vpt, oracle, scenes):
    """The oracle's image after 7 and after 14 frames, per image size."""
    out = {}
    for w, h in sorted(set(SHAPES.values())):
        o = oracle.Oracle(scenes("cornell_box"), w, h)
        o.set_params(vpt.default_params(max_depth=DEPTH))
        o.render(FRAMES)
        first = o.radiance()
        o.render(FRAMES)
        out[(w, h)] = (first, o.radiance())
        o.close()
    return out


def rows_of(shape, img):
    return img[1::2] if shape == "shard" else img   # (shard_count 2, rank 1: rows y % 2 == 1)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_a_batch_in_parts_is_the_unsplit_batch(runs, refs, shape):
    images, stats = runs
    first, second = (rows_of(shape, r) for r in refs[SHAPES[shape]])
    for batch, ref in (("first", first), ("second", second)):   # second: frame_base > 0 in every part
        one = images["%s_p1_%s" % (shape, batch)]
        assert np.array_equal(one, ref), "%d px differ from the oracle" % int((np.abs(one - ref).max(axis=2) > 0).sum())
        for parts in PARTS:
            name = "%s_p%d_%s" % (shape, parts, batch)
            assert images[name].tobytes() == one.tobytes(), name
            assert np.array_equal(images[name], ref), name
            for k in RAY_STATS:
                assert stats[name][k] == stats["%s_p1_%s" % (shape, batch)][k] and stats[name][k] > 0, (name, k)
            launches, n = stats[name]["kernel_launches"], min(parts, FRAMES) * (2 if batch == "second" else 1)
            assert launches["primary"] == n and launches["resolve"] == n and launches["bounce"] == 0, (name, launches)


def test_async_batch_in_parts_and_frames_on_the_lanes_behind_it(runs, refs):
    """vpt_render_async: 7 frames in 3 parts, vpt_postprocess_device, vpt_wait — then three 1-frame batches, which go to the lanes as one part each."""
    images, stats = runs
    assert images["async_batch"].tobytes() == images["blocking_batch"].tobytes()
    assert np.array_equal(images["async_batch"], refs[SHAPES["even"]][0])
    assert np.array_equal(images["async_out8"], images["blocking_out8"])
    assert images["async_lanes"].tobytes() == images["blocking_lanes"].tobytes()
    assert stats["async_batch"]["kernel_launches"]["primary"] == 3 and stats["async_batch"]["kernel_launches"]["resolve"] == 3
    assert stats["async_lanes"]["kernel_launches"]["primary"] == 6 and stats["async_lanes"]["kernel_launches"]["resolve"] == 6
    assert stats["blocking_lanes"]["kernel_launches"]["primary"] == 4
    for k in RAY_STATS:
        assert stats["async_lanes"][k] == stats["blocking_lanes"][k], k


def test_timed_and_counted_batches_split_alike(runs, refs):
    """vpt_config.profile and .count_traversal do not change the schedule: same image, every launch timed on its own stream, the same visits."""
    images, stats = runs
    assert images["counted_p3"].tobytes() == images["counted_p1"].tobytes()
    assert np.array_equal(images["counted_p3"], refs[SHAPES["ragged"]][0])
    split, whole = stats["counted_p3"], stats["counted_p1"]
    assert split["kernel_launches"]["primary"] == 3 and split["kernel_launches"]["resolve"] == 3 and whole["kernel_launches"]["primary"] == 1
    assert split["kernel_ms"]["primary"] > 0 and split["kernel_ms"]["resolve"] > 0
    for k in RAY_STATS + ("nodes_visited", "tris_tested", "shadow_nodes_visited", "shadow_tris_tested"):
        assert split[k] == whole[k] and split[k] > 0, k
