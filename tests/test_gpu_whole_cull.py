"""The whole-path kernel starts no path for a sample whose pixel lies outside the screen bound of the scene's box (csrc/camera_cull.hpp, api_render.hip
batch_begin, kernels_whole.hip's refill step): such a sample's frame sum is exactly zero, and it is counted as the one closest-hit ray its path would
have been (a counting context, vpt_config.count_traversal, culls nothing: its visit counters are the searches' own).  So nothing a caller can see
may depend on the cull.  tests/gpu_whole_cull_run.py renders every case with the cull on and off (VPT_LAB_WHOLE_CULL, a laboratory entry point: a process of its own with VPT_LAB=1), uncounted and counting, and the tests compare
what it left: the same radiance bit for bit, the same ray statistics and visit counters, and a culled count (vpt_lab_whole_culled) that is the number
of the batch's samples outside the rectangle vpt_get_whole_cull reported — 0 wherever the rectangle must be the whole image.  The CPU side:
tests/test_camera_cull_cpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAY_STATS = ("samples", "closest_rays", "shadow_rays", "primary_hits", "connect_paths")
VISITS = ("nodes_visited", "tris_tested", "shadow_nodes_visited", "shadow_tris_tested")
# name: (width, height, dispatches per batch, rows of the context (first, step), pixels per dispatch as a fraction 1 / n, batches, must the cull be idle)
CASES = {
    "cornell_192": (192, 108, 3, (0, 1), 1, 1, False),
    "cornell_200": (200, 120, 3, (0, 1), 1, 1, False),
    "far_camera": (480, 270, 2, (0, 1), 1, 1, False),
    "focus_zero": (480, 270, 2, (0, 1), 1, 1, True),
    "inside": (96, 54, 2, (0, 1), 1, 1, True),
    "rolled": (192, 108, 2, (0, 1), 1, 1, False),
    "dof": (96, 54, 2, (0, 1), 1, 1, True),
    "shard": (192, 108, 3, (1, 2), 1, 1, False),
    "split": (100, 75, 8, (0, 1), 4, 1, False),
    "furnace": (96, 54, 2, (0, 1), 1, 1, True),
    "env_hidden": (96, 54, 2, (0, 1), 1, 1, False),
    "env_shown": (96, 54, 2, (0, 1), 1, 1, True),
    "moved_light": (192, 108, 2, (0, 1), 1, 2, False),
    "set_camera": (192, 108, 2, (0, 1), 1, 2, False),
}


@pytest.fixture(scope="module")
def runs(vpt, tmp_path_factory):
    vpt.build(lab=True)
    out = str(tmp_path_factory.mktemp("whole_cull") / "runs.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_whole_cull_run.py"), out], env=dict(os.environ, VPT_LAB="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    z = np.load(out)
    return {k: z[k] for k in z.files if k != "info"}, json.loads(str(z["info"]))


def outside_pixels(rect, w, h, rows):
    """Pixels of the context's rows outside the inclusive rectangle (x0, y0, x1, y1)."""
    x0, y0, x1, y1 = rect
    ys = range(rows[0], h, rows[1])
    if x0 > x1:
        return w * len(ys)
    return sum(w - (x1 - x0 + 1) if y0 <= y <= y1 else w for y in ys)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_cull_changes_nothing_a_caller_sees(runs, name):
    images, info = runs
    w, h, frames, rows, chunks, batches, idle = CASES[name]
    on, off = info[name + "_on"], info[name + "_off"]
    print(name, "rect", on["rect"], "culled", on["culled"], {k: on[k] for k in RAY_STATS})
    assert np.array_equal(images[name + "_on"], images[name + "_off"]), "%d px differ" % int((np.abs(images[name + "_on"] - images[name + "_off"]).max(axis=2) > 0).sum())
    assert images[name + "_on"].tobytes() == images[name + "_off"].tobytes()
    assert float(images[name + "_on"][..., :3].max()) > 0.0
    for k in RAY_STATS:
        assert on[k] == off[k] and on[k] > 0, (k, on[k], off[k])
    assert on["kernel_launches"]["primary"] == batches and on["kernel_launches"]["bounce"] == 0     # whole-path batches, one launch each
    # the counting contexts: the same image, the same rays, the same visits
    con, coff = info[name + "_on_counted"], info[name + "_off_counted"]
    assert images[name + "_on_counted"].tobytes() == images[name + "_on"].tobytes() and images[name + "_off_counted"].tobytes() == images[name + "_on"].tobytes()
    for k in RAY_STATS:
        assert con[k] == on[k] and coff[k] == on[k], k
    for k in VISITS:
        assert con[k] == coff[k] and (con[k] > 0 or k.startswith("shadow")), (k, con[k], coff[k])
    # the culled count is the batch's samples outside the reported rectangle; the switch leaves none, and a counting context has none either way
    # (the test is compiled out of k_whole's counting instantiations, for the library's size bound: the host reports the whole image there)
    assert len(on["rect"]) == len(on["culled"]) == batches
    for rect, culled in zip(on["rect"], on["culled"]):
        assert culled == outside_pixels(rect, w, h, rows) * frames // chunks, (rect, culled)
    for rec in (off, con, coff):
        assert all(r == [0, 0, w - 1, h - 1] for r in rec["rect"]) and all(c == 0 for c in rec["culled"])
    if idle:
        assert on["rect"] == [[0, 0, w - 1, h - 1]] and on["culled"] == [0]
    else:
        assert all(c > 0 for c in on["culled"]), on["culled"]


def test_the_rectangles_are_the_ones_the_cases_are_about(runs):
    images, info = runs
    # Cornell at 1/10 of 1080p: the projection of the scene's box (470..1454 x 47..1020 there) in these pixels, within the margin's rounding
    x0, y0, x1, y1 = info["cornell_192_on"]["rect"][0]
    assert 44 <= x0 <= 47 and 145 <= x1 <= 148 and 2 <= y0 <= 5 and 101 <= y1 <= 104, (x0, y0, x1, y1)
    # (at this size the two-pixel margin weighs ten times what it does at 1080p: the largest rectangle the line above admits, 105 x 103, leaves 47.8 % outside)
    assert info["cornell_192_on"]["culled"][0] * 100 > 47 * 192 * 108 * 3
    # the rolled camera's rectangle is the bounding box of a turned square: larger than the upright one
    rx0, ry0, rx1, ry1 = info["rolled_on"]["rect"][0]
    assert (rx1 - rx0) > (x1 - x0) and info["rolled_on"]["culled"][0] > 0
    # the far camera sees the box in a few dozen pixels
    fx0, fy0, fx1, fy1 = info["far_camera_on"]["rect"][0]
    assert fx1 - fx0 < 40 and fy1 - fy0 < 40
    # the moved light: the refitted root's box reaches into what was background, the rectangle follows it, and the light shows there
    first, second = info["moved_light_on"]["rect"]
    assert first == [x0, y0, x1, y1] and second[2] > first[2] + 10 and second[0] == first[0]
    img = images["moved_light_on"]
    assert float(img[:, first[2] + 1:, :3].max()) > 0.0, "nothing to see right of the old rectangle"
    # vpt_set_camera between two batches: the second batch uses the new camera's rectangle
    first, second = info["set_camera_on"]["rect"]
    assert first == [x0, y0, x1, y1] and second[0] > first[0] and second[2] < first[2]
    assert info["set_camera_on"]["culled"][1] > info["set_camera_on"]["culled"][0]
    # the sharded context reports the whole image's rectangle; its samples are its own rows'
    assert info["shard_on"]["rect"][0] == [x0, y0, x1, y1]
    assert info["shard_on"]["samples"] == 192 * 54 * 3
