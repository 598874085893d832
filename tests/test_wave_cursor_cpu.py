"""How a persistent wave takes its work from a stream (vulkan-path-tracer_amd/csrc/wave_cursor.hpp: DealCursor of the traversal kernels and the finisher,
StrideCursor of the shading stages), walked on the host by tests/tools/wave_cursor_driver.cpp — a stand-alone program, built once with the host compiler
and once more with -fsanitize=address,undefined.  The driver runs a grid of G waves through the cursors' wave-uniform arithmetic with an ordinary
counter as the head word and the waves' steps interleaved round-robin, reversed, and with one wave racing ahead; the dealing cursor's idle masks walk
through popcounts 0, 1, 63, 64 and a pseudo-random sequence.  Per case: every entry of [0, n) is handed out exactly once and none at or beyond n, no
lane computes an index further than fetch_chunk's largest chunk past the end of its run, and every wave reaches the end of the stream.
What this checks is fetch_chunk, the cursors' arithmetic and a host model of their statements; the device structs and the kernels' written-out copies
are exercised by the GPU stream tests (tests/test_gpu_trace_stream.py beyond the grid's static part)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vulkan-path-tracer_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "tools", "wave_cursor_driver.cpp")
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ORDERS = (0, 1, 2)            # round-robin, reversed, wave 0 races ahead
GRIDS = (1, 7)
STATIC_RUNS = (64, 80, 96, 128)   # k_trace_vote / k_trace_shadow / k_finish, the pool's 80 and 96 slots, the pool's and the pair's 128
CHUNKS = (64, 1024, 0)        # the finisher's, fetch_chunk's largest, fetch_chunk(n)


def fetch_chunk(n):
    """wave.hpp's rule in words: n / 8192 entries per fetch, rounded up to whole waves, between 64 and 1024."""
    return min(max(((n >> 13) + 63) // 64 * 64, 64), 1024)


# n on both sides of each of fetch_chunk's clamps: below 8192 the rule says 0 and the lower clamp makes it 64, from 8192 the rule itself says 64 and
# from 65 * 8192 on 128 (the first chunk that is not the lower bound); it says 1024 from 961 * 8192 and the upper clamp holds it there from 1025 * 8192
CLAMP_SIZES = (8191, 8192, 8193, 65 * 8192 - 1, 65 * 8192, 961 * 8192 - 1, 961 * 8192, 1025 * 8192 - 1, 1025 * 8192)


def sizes(static, chunk):
    return sorted({0, 1, 63, 64, 65, static - 1, static, static + 1, static + chunk - 1, static + chunk + 77})


def compile_driver(out, extra=()):
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, DRIVER, "-o", out] + list(extra))
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return compile_driver(str(tmp_path_factory.mktemp("wave_cursor") / "wave_cursor_driver"))


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return compile_driver(str(tmp_path_factory.mktemp("wave_cursor_san") / "wave_cursor_driver_san"), SANITIZE)


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    return {k: int(v) for k, v in zip(words[0::2], words[1::2])}


def check(o, n, what):
    assert o["handed"] == n and o["dup"] == 0 and o["missing"] == 0 and o["beyond"] == 0, (what, o)   # every entry exactly once, none at or beyond n
    assert o["past"] <= o["chunk_max"] == 1024, (what, o)
    assert o["unexhausted"] == 0, (what, o)


def test_fetch_chunk_is_n_over_8192_in_whole_waves_between_64_and_1024(exe):
    for n in (0, 1, 64, 8191, 8192, 8193, 2 * 8192, 2 * 8192 + 1) + CLAMP_SIZES + (1 << 24, (1 << 32) - 1):
        assert run(exe, "chunk", n)["chunk"] == fetch_chunk(n), n
    assert [fetch_chunk(n) for n in CLAMP_SIZES] == [64, 64, 64, 64, 128, 960, 1024, 1024, 1024]


@pytest.mark.parametrize("static", STATIC_RUNS)
@pytest.mark.parametrize("grid", GRIDS)
def test_dealing_cursor_hands_out_every_entry_once(exe, grid, static):
    for chunk in CHUNKS:
        for n in sizes(grid * static, chunk or 64):
            for order in ORDERS:
                check(run(exe, "deal", grid, static, chunk, n, order), n, ("deal", grid, static, chunk, n, order))


@pytest.mark.parametrize("n", CLAMP_SIZES)
def test_dealing_cursor_with_fetch_chunk_on_both_sides_of_its_clamps(exe, n):
    for order in ORDERS:
        check(run(exe, "deal", 7, 64, 0, n, order), n, ("deal", n, order))
    check(run(exe, "deal", 1, 128, 0, n, 0), n, ("deal, one wave", n))


@pytest.mark.parametrize("grid", GRIDS)
def test_striding_cursor_hands_out_every_entry_once(exe, grid):
    """The sizes around the static part include active * 64 >= n (no chunk is ever reserved) and the first entry behind it."""
    for n in sizes(grid * 64, 64) + list(CLAMP_SIZES):
        for order in ORDERS:
            check(run(exe, "stride", grid, n, order), n, ("stride", grid, n, order))


def test_driver_is_clean_under_address_and_undefined_behaviour_sanitizers(exe_san):
    for grid, static, chunk, n in ((1, 64, 64, 0), (7, 64, 64, 7 * 64 + 64 + 77), (7, 80, 0, 7 * 80 + 1), (7, 128, 1024, 7 * 128 + 1023), (1, 96, 0, 65 * 8192), (7, 64, 0, 1025 * 8192)):
        for order in ORDERS:
            check(run(exe_san, "deal", grid, static, chunk, n, order), n, ("deal", grid, static, chunk, n, order))
    for grid, n in ((1, 0), (1, 65), (7, 7 * 64), (7, 7 * 64 + 1), (7, 65 * 8192 - 1)):
        for order in ORDERS:
            check(run(exe_san, "stride", grid, n, order), n, ("stride", grid, n, order))
