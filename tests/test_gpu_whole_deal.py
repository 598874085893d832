"""A whole-path batch whose camera sees the scene's box inside a rectangle of the image deals its launch indices over the samples inside that
rectangle alone (csrc/whole_deal.hpp, kernels_whole.hip's refill step): a sample outside takes no lane, its zero frame sum is written in the runs
between the rectangle's rows by the wave that deals a row's end, and its one ray is a constant the launch adds to the count.  Nothing a caller can
see may depend on it.  tests/gpu_whole_deal_run.py renders the Cornell box at 97 x 53, depth 4, 3 frames, with the rectangle on and off (VPT_LAB_WHOLE_CULL, a
laboratory entry point: a process of its own with VPT_LAB=1) from three cameras — far out (the rectangle strictly inside the image), beside the box
(it touches the left and the top edge), inside the box (no rectangle) — whole and as each of 3 shards, and the tests compare what it left: the
radiance bit for bit with the switched-off context's and the oracle's, the same ray statistics, and a culled count that is frames x (shard pixels -
rectangle pixels).  Then two batches with the camera moved in between (the two rectangles differ, and so do the runs of zeros around them), and one batch
as one launch and as three parts; and contexts with no sample inside the rectangle at all (an empty rectangle; a shard whose rows lie outside it), through
vpt_render and through vpt_render_async batches replayed from a captured graph.  The CPU side: tests/test_whole_deal_cpu.py."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FRAMES, DEPTH = 97, 53, 3, 4
RAY_STATS = ("samples", "closest_rays", "shadow_rays", "primary_hits", "primary_survivors", "connect_paths")
SHARDS = ((0, 1), (0, 3), (1, 3), (2, 3))


@pytest.fixture(scope="module")
def runs(vpt, tmp_path_factory):
    vpt.build(lab=True)
    out = str(tmp_path_factory.mktemp("whole_deal") / "runs.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_whole_deal_run.py"), out], env=dict(os.environ, VPT_LAB="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    z = np.load(out)
    return {k: z[k] for k in z.files if k not in ("info", "views")}, json.loads(str(z["info"])), json.loads(str(z["views"]))


@pytest.fixture(scope="module")
def references(vpt, oracle, scenes, runs):
    """The oracle's image per camera, computed once."""
    out = {}
    for cam in ("far", "corner", "inside"):
        sc = copy.deepcopy(scenes("cornell_box"))
        sc.view_inverse = np.array(runs[2][cam], np.float32)
        o = oracle.Oracle(sc, W, H)
        o.set_params(vpt.default_params(max_depth=DEPTH))
        o.render(FRAMES)
        out[cam] = o.radiance()
        o.close()
    return out


def inside_pixels(rect, rank, count):
    """Pixels of the context's rows inside the inclusive rectangle (x0, y0, x1, y1)."""
    x0, y0, x1, y1 = rect
    return sum(x1 - x0 + 1 for y in range(rank, H, count) if y0 <= y <= y1) if x0 <= x1 else 0


@pytest.mark.parametrize("rank,count", SHARDS)
@pytest.mark.parametrize("cam", ["far", "corner", "inside"])
def test_dealing_over_the_rectangle_changes_nothing_a_caller_sees(runs, references, cam, rank, count):
    images, info, _ = runs
    key = "%s_%d_%d_" % (cam, rank, count)
    on, off = info[key + "on"], info[key + "off"]
    rect, shard_pixels = on["rect"][0], len(range(rank, H, count)) * W
    print(key, "rect", rect, "culled", on["culled"], {k: on[k] for k in RAY_STATS})
    # the cameras are the ones the cases are about
    if cam == "far":
        assert 0 < rect[0] <= rect[2] < W - 1 and 0 < rect[1] <= rect[3] < H - 1, rect
    if cam == "corner":
        assert rect[0] == 0 and rect[1] == 0 and rect[2] < W - 1 and rect[3] < H - 1, rect
    if cam == "inside":
        assert rect == [0, 0, W - 1, H - 1] and on["culled"] == [0]
    assert off["rect"] == [[0, 0, W - 1, H - 1]] and off["culled"] == [0]
    assert images[key + "on"].tobytes() == images[key + "off"].tobytes(), "%d px differ" % int((np.abs(images[key + "on"] - images[key + "off"]).max(axis=2) > 0).sum())
    assert images[key + "on"].tobytes() == np.ascontiguousarray(references[cam][rank::count]).tobytes(), "differs from the oracle"
    assert float(images[key + "on"][..., :3].max()) > 0.0
    for k in RAY_STATS:
        assert on[k] == off[k] and on[k] > 0, (k, on[k], off[k])
    assert on["samples"] == FRAMES * shard_pixels
    assert on["kernel_launches"]["primary"] == 1 and on["kernel_launches"]["bounce"] == 0
    if cam != "inside":
        assert on["culled"] == [FRAMES * (shard_pixels - inside_pixels(rect, rank, count))] and on["culled"][0] > 0


@pytest.mark.parametrize("rank,count", [(0, 1), (1, 3)])
def test_a_grown_rectangle_leaves_no_slot_of_the_batch_before_behind(runs, rank, count):
    """Far out, then nearer with the accumulation going on: the second batch's rectangle is larger and lies elsewhere, so slots that held the first
    batch's paths must now hold zeros and the other way round, and the first batch's rectangle pixels outside the second's decay as they must."""
    images, info, _ = runs
    key = "stale_%d_%d_" % (rank, count)
    on, off = info[key + "on"], info[key + "off"]
    first, second = on["rect"]
    assert second[0] < first[0] and second[1] < first[1] and (second[2] - second[0]) > (first[2] - first[0]) and second[2] < first[2], (first, second)
    assert images[key + "on"].tobytes() == images[key + "off"].tobytes(), "%d px differ" % int((np.abs(images[key + "on"] - images[key + "off"]).max(axis=2) > 0).sum())
    shard_pixels = len(range(rank, H, count)) * W
    assert on["culled"] == [FRAMES * (shard_pixels - inside_pixels(r, rank, count)) for r in (first, second)] and off["culled"] == [0, 0]
    for k in RAY_STATS:
        assert on[k] == off[k] and on[k] > 0, (k, on[k], off[k])
    assert on["kernel_launches"]["primary"] == 2


def test_parts_of_a_dealt_batch_add_up_to_the_batch(runs):
    images, info, _ = runs
    one, three = info["parts_1"], info["parts_3"]
    assert one["kernel_launches"]["primary"] == 1 and three["kernel_launches"]["primary"] == 3 and three["kernel_launches"]["resolve"] == 3
    assert images["parts_1"].tobytes() == images["parts_3"].tobytes() == images["far_0_1_on"].tobytes()
    for k in RAY_STATS + ("rect", "culled"):
        assert one[k] == three[k] == info["far_0_1_on"][k], k


@pytest.mark.parametrize("mode", ["render", "async"])
@pytest.mark.parametrize("cam,rank,count", [("away", 0, 1), ("far", 10, 32)])
def test_a_context_with_no_sample_inside_the_rectangle_still_counts_and_clears(runs, cam, rank, count, mode):
    """An empty rectangle, and a shard whose rows all lie outside the far camera's rectangle: the launch has no index to deal, yet every sample is one
    closest-hit ray — counted on the device, so that a replayed graph counts it in every replay — and its frame sum is zero.  Through vpt_render (one
    batch) and through five vpt_render_async calls (the later ones replayed from the captured graph): image, ray statistics and launches equal to the
    switched-off context's, and the culled count every sample of the batch."""
    images, info, _ = runs
    key = "none_%s_%d_%d_%s_" % (cam, rank, count, mode)
    on, off = info[key + "on"], info[key + "off"]
    shard_pixels, batches = len(range(rank, H, count)) * W, 1 if mode == "render" else 5
    print(key, "rect", on["rect"], "culled", on["culled"], {k: on[k] for k in RAY_STATS}, "graph launches", on["graph_launches"], off["graph_launches"])
    assert inside_pixels(on["rect"][0], rank, count) == 0 and shard_pixels > 0
    assert images[key + "on"].tobytes() == images[key + "off"].tobytes()
    assert not images[key + "on"][..., :3].any()                      # nothing to see: every camera ray misses
    for k in RAY_STATS:
        assert on[k] == off[k], (k, on[k], off[k])
    assert on["samples"] == on["closest_rays"] == batches * FRAMES * shard_pixels and on["shadow_rays"] == 0 and on["primary_hits"] == 0
    assert on["culled"] == [FRAMES * shard_pixels] and off["culled"] == [0]     # (the latest batch's)
    assert on["kernel_launches"]["primary"] == off["kernel_launches"]["primary"] == batches
    if mode == "async":
        assert on["graph_launches"] >= 2 and on["graph_launches"] == off["graph_launches"]   # the replays are what this case is about
