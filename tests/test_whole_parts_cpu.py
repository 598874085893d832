"""The parts of a whole-path batch (vulkan-path-tracer_amd/csrc/path_plan.hpp: Parts, split_parts, Schedule::parts — what api_render.hip's
batch_begin / batch_resolve turn into one launch and one resolve per part) on the host: tests/tools/whole_parts_driver.cpp runs decide()
over frames x shard pixels x kind x split x capturing x on-lane x forced part count x PLAIN scene or not, and this test checks the shape of every answer and
where the rule splits.  The same driver runs stand-alone under -fsanitize=address,undefined.  The GPU side: tests/test_gpu_whole_parts.py."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vulkan-path-tracer_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "tools", "whole_parts_driver.cpp")

AUTO, FUSED, STAGED, WHOLE = 0, 1, 2, 5   # include/vpt.h
K_WHOLE = 0                               # path_plan.hpp Kind::Whole
MAX_PARTS = 8
IN = ["pipeline", "split", "capturing", "on_lane", "forced", "frames", "shard_pixels", "n_slots", "plain"]

FRAMES = list(range(1, 41)) + [904, 6912, 8192]
PIXELS = [1, 63, 64, 65, 1850, 2073600, 259200]   # 1080p, and its 1/8 shard
HEADLINE = (904, 2073600)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("whole_parts") / "libwhole_parts.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I" + CSRC, DRIVER, "-o", out])
    L = C.CDLL(out)
    L.wp_run.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p]
    L.wp_run.restype = None
    L.wp_constant.argtypes = [C.c_uint32]
    L.wp_constant.restype = C.c_uint32
    assert (L.wp_in_columns(), L.wp_out_columns()) == (len(IN), 3 + MAX_PARTS + 1)
    assert L.wp_constant(0) == MAX_PARTS
    return L


def run(lib, rows):
    tin = np.ascontiguousarray(np.array(rows, dtype=np.uint32).reshape(-1, len(IN)))
    tout = np.zeros((len(tin), 3 + MAX_PARTS + 1), dtype=np.uint32)
    lib.wp_run(len(tin), tin.ctypes.data, tout.ctypes.data)
    c = {k: tin[:, i].astype(np.int64) for i, k in enumerate(IN)}
    return c, tout[:, 0].astype(np.int32), tout[:, 1].astype(np.int64), tout[:, 2].astype(np.int64), tout[:, 3:].astype(np.int64)


@pytest.fixture(scope="module")
def sweep(lib):
    rows = []
    for frames, px in itertools.product(FRAMES, PIXELS):
        if frames * px >= 1 << 31:   # (path_plan.hpp batch_cap: the slots of a batch fit 31 bits)
            continue
        for pipeline, split, capturing, on_lane, forced, plain in itertools.product((AUTO, FUSED, STAGED, WHOLE), (1, 2), (0, 1), (0, 1), range(MAX_PARTS + 1), (0, 1)):
            rows.append((pipeline, split, capturing, on_lane, forced, frames, px, frames * px if split == 1 else frames * px // 4, plain))
    return run(lib, rows)


def test_parts_cover_the_batch(sweep):
    """Contiguous, ascending, none empty, at most 8, covering [0, frames)."""
    c, err, kind, n, first = sweep
    assert len(n) > 160000 and (err == 0).all()
    assert ((n >= 1) & (n <= MAX_PARTS)).all()
    assert (first[:, 0] == 0).all()
    assert (first[np.arange(len(n)), n] == c["frames"]).all()
    for i in range(MAX_PARTS):
        used = n > i
        assert (first[used, i + 1] > first[used, i]).all(), i
        assert (first[~used, i + 1] == 0).all(), i   # nothing behind the last boundary


def test_one_part_where_a_batch_may_not_be_split(sweep):
    """Not a whole-path batch, split-screen dispatch, a captured batch, a batch on an extra lane: one part, whatever is forced."""
    c, err, kind, n, first = sweep
    assert set(np.unique(kind)) > {K_WHOLE}
    barred = (kind != K_WHOLE) | (c["split"] != 1) | (c["capturing"] == 1) | (c["on_lane"] == 1)
    assert barred.any() and (n[barred] == 1).all()
    assert (n[~barred] > 1).any()


def test_forced_parts_are_equal(sweep):
    """Forced n: min(n, frames) parts whose sizes differ by at most 1, the longer ones first."""
    c, err, kind, n, first = sweep
    free = (kind == K_WHOLE) & (c["split"] == 1) & (c["capturing"] == 0) & (c["on_lane"] == 0) & (c["forced"] != 0)
    assert free.any()
    assert (n[free] == np.minimum(c["forced"], c["frames"])[free]).all()
    size = np.diff(first, axis=1)
    for i in range(MAX_PARTS):
        rows = free & (n > i)
        base = c["frames"][rows] // n[rows]
        assert ((size[rows, i] == base) | (size[rows, i] == base + 1)).all(), i
        if i:
            assert (size[rows, i] <= size[rows, i - 1]).all(), i


def test_default_rule(lib, sweep):
    """The rule (nothing forced) leaves every batch below the threshold whole — among them every batch of the GPU tests' sizes, all below 2^24
    samples — and splits the headline's 904 frames of 1080p; what it splits, it splits into kPartsCount parts that shrink."""
    c, err, kind, n, first = sweep
    threshold = lib.wp_constant(3) | (lib.wp_constant(4) << 32)
    count, ratio = lib.wp_constant(1), lib.wp_constant(2)
    assert threshold >= 1 << 26, "the threshold is far above anything the GPU tests render"
    free = (kind == K_WHOLE) & (c["split"] == 1) & (c["capturing"] == 0) & (c["on_lane"] == 0) & (c["forced"] == 0)
    small = free & (c["n_slots"] < 1 << 24)
    assert small.any() and (n[small] == 1).all()
    assert (n[free & (c["n_slots"] < threshold)] == 1).all()
    assert (n[free & (c["plain"] == 0)] == 1).all()   # the general instantiation leaves the resolve no registers: nothing to overlap
    big = free & (c["n_slots"] >= threshold) & (c["plain"] == 1)
    assert (n[big] == np.minimum(count, c["frames"])[big]).all()
    head = free & (c["frames"] == HEADLINE[0]) & (c["shard_pixels"] == HEADLINE[1]) & (c["plain"] == 1)   # (the Cornell box is a PLAIN scene)
    assert head.sum() == 2 and (n[head] > 1).all()   # (AUTO and VPT_PIPELINE_WHOLE)
    size = np.diff(first[head][0][: n[head][0] + 1])
    assert size.sum() == HEADLINE[0] and (np.diff(size) <= 0).all()
    if ratio > 1:
        assert size[-1] * ratio <= size[-2] + ratio   # each part about 1 / ratio of the one before


def test_driver_runs_clean_under_sanitizers(tmp_path):
    """The stand-alone program: the same axes and every (count, ratio) split_parts accepts, under AddressSanitizer and UBSan."""
    exe = str(tmp_path / "whole_parts_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC, DRIVER, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "cases" in r.stdout
