"""How the waves of the whole-path kernel (kernels_whole.hip k_whole) come by their fresh samples, on the host: the tile cursor and the wave's buffer
of generated camera rays are vulkan-path-tracer_amd/csrc/whole_refill.hpp, and tests/tools/whole_refill_driver.cpp plays a grid of waves against it —
seeded survivor masks between refills, a seeded order in which the waves meet the shared tile counter.  For every case:
  (a) every launch index in [0, n) is handed to a lane exactly once;
  (b) no index >= n is handed out;
  (c) a wave never stops with entries left in its buffer;
  (d) camera rays are generated a full tile at a time: the only passes on fewer than 64 lanes are those over the ragged end of [0, n).
The GPU side: tests/test_gpu_whole_refill.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vulkan-path-tracer_amd", "csrc")
GUIDED = 0x100


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("whole_refill") / "libwhole_refill.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "tools", "whole_refill_driver.cpp"), "-o", out])
    L = C.CDLL(out)
    L.wr_run.restype = None
    L.wr_run.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
    return L


def run(L, n, n_waves, static_rounds, chunk_tiles, survive, seed):
    handed = np.zeros(max(n, 1), np.uint32)
    out = np.zeros(6, np.uint64)
    L.wr_run(n, n_waves, static_rounds, chunk_tiles, survive, seed, handed.ctypes.data, out.ctypes.data)
    return handed[:n], dict(zip(("out_of_range", "leftover", "gen_passes", "gen_lanes", "partial_gens", "counter_adds"), (int(v) for v in out)))


def check(L, n, n_waves, static_rounds, chunk_tiles, survive, seed):
    handed, o = run(L, n, n_waves, static_rounds, chunk_tiles, survive, seed)
    assert np.all(handed == 1), "launch indices handed out %s times: %s" % (np.unique(handed), np.nonzero(handed != 1)[0][:8])
    assert o["out_of_range"] == 0
    assert o["leftover"] == 0
    assert o["gen_lanes"] == n
    assert o["partial_gens"] == (1 if n % 64 else 0)
    assert o["gen_passes"] == (n + 63) // 64
    return o


# n: 1, 63, 64, 65, ragged multiples, whole multiples
SIZES = [1, 63, 64, 65, 127, 128, 129, 64 * 7 + 5, 64 * 40, 64 * 40 + 63, 9216, 128 * 72, 1000 * 37 + 11]
SURVIVE = [0, 375, 900]   # per mille of the running paths that keep their lane across a refill (the Cornell box: about 3 in 8)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("static_rounds", [0, 1, 3])
@pytest.mark.parametrize("chunk_tiles", [1, 4, 4 | GUIDED, 16 | GUIDED])
def test_every_index_exactly_once(lib, n, static_rounds, chunk_tiles):
    for n_waves in (1, 4, 12):
        for survive in SURVIVE:
            check(lib, n, n_waves, static_rounds, chunk_tiles, survive, seed=n * 131 + static_rounds * 17 + chunk_tiles + n_waves + survive)


@pytest.mark.parametrize("static_rounds", [0, 2])
@pytest.mark.parametrize("chunk_tiles", [1, 4 | GUIDED])
def test_more_waves_than_tiles(lib, static_rounds, chunk_tiles):
    """A grid larger than the batch (a 1-frame launch of a small image on 256 CUs): most waves get no tile at all and stop at once."""
    for n in (1, 65, 64 * 5, 64 * 5 + 1):
        for n_waves in (8, 64, 3072):
            check(lib, n, n_waves, static_rounds, chunk_tiles, 375, seed=n + n_waves)


def test_headline_shape(lib):
    """1920x1080, the grid of 256 CUs x 3 blocks x 4 waves, the schedule of a long batch's frame: 4 tiles per atomic, guided."""
    o = check(lib, 1920 * 1080, 3072, 2, 4 | GUIDED, 375, seed=9)
    assert o["counter_adds"] >= 3072   # every wave meets the counter at least once (its last, failed, request)


def test_no_tile_counter_without_need(lib):
    """Static rounds that cover the batch: the counter is only asked once per wave, for the request that finds nothing."""
    n_waves = 6
    o = check(lib, 64 * n_waves * 2, n_waves, 2, 4, 375, seed=3)
    assert o["counter_adds"] == n_waves
