"""How a whole-path launch with a screen rectangle deals its launch indices (vulkan-path-tracer_amd/csrc/whole_deal.hpp), held against a walk over the
pixels by tests/tools/whole_deal_driver.cpp — a stand-alone program, built once as the product is compiled and once more with
-fsanitize=address,undefined.  Per shape, shard count (1, 3, 8) and rank: every launch index of 3 frames decodes to a slot of its own, inside the
rectangle, on one of the rank's rows, with the (x, y, f) pixel_of_slot makes of that slot; together they are the rank's samples inside the rectangle;
the culled-ray constant is the walked count of the others; and the runs of zero frame sums the launch's waves write hold every other slot of the
launch exactly once and none beyond it.  (The multiply-shift dividers the decode was also built with did not clear the
project's bar and are not in the tree: profiles/REJECTED.md r21.)  The GPU side: tests/test_gpu_whole_deal.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vulkan-path-tracer_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "tools", "whole_deal_driver.cpp")
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
FRAMES = 3
SHARDS = (1, 3, 8)
# name: (width, height, (x0, y0, x1, y1))
SHAPES = {
    "inside_97x53": (97, 53, (23, 5, 71, 40)),
    "cornell_1080p": (1920, 1080, (470, 47, 1453, 1019)),          # the rectangle vpt_get_whole_cull reports for bench.py's camera
    "left_top_97x53": (97, 53, (0, 0, 60, 30)),
    "right_bottom_97x53": (97, 53, (40, 20, 96, 52)),
    "left_bottom_1080p": (1920, 1080, (0, 500, 700, 1079)),
    "right_top_1080p": (1920, 1080, (1000, 0, 1919, 300)),
    "whole_image_97x53": (97, 53, (0, 0, 96, 52)),                    # a rectangle that happens to be the image (not "everything": it is still dealt)
    "one_column_97x53": (97, 53, (50, 3, 50, 47)),                    # rw == 1
    "one_column_1080p": (1920, 1080, (1919, 0, 1919, 1079)),
    "one_row_97x53": (97, 53, (10, 7, 80, 7)),                        # row 7 belongs to one rank of 3 and of 8: the others have no row inside
    "one_row_1080p": (1920, 1080, (470, 1079, 1453, 1079)),
    "one_pixel_97x53": (97, 53, (96, 52, 96, 52)),                    # rect_px == 1 on its rank, 0 on the others
    "two_rows_97x53": (97, 53, (5, 20, 90, 21)),                      # 8 shards: six ranks with no row inside
    "nothing_97x53": (97, 53, (1, 1, 0, 0)),                          # camera_cull.hpp's empty rectangle
}


def compile_driver(out, extra=()):
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC, DRIVER, "-o", out] + list(extra))
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return compile_driver(str(tmp_path_factory.mktemp("whole_deal") / "whole_deal_driver"))


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return compile_driver(str(tmp_path_factory.mktemp("whole_deal_san") / "whole_deal_driver_san"), SANITIZE)


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    return {k: int(v) for k, v in zip(words[0::2], words[1::2])}


def walked(w, h, rect, count):
    """(samples inside, samples outside, ranks with no row inside) of one frame, over every rank of the shard count."""
    x0, y0, x1, y1 = rect
    cols = x1 - x0 + 1 if x0 <= x1 else 0
    rows = [sum(1 for y in range(rank, h, count) if y0 <= y <= y1) for rank in range(count)]
    inside = cols * sum(rows)
    return inside, w * h - inside, sum(1 for r in rows if r * cols == 0)


@pytest.mark.parametrize("count", SHARDS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_every_launch_index_is_one_sample_inside_the_rectangle(exe, name, count):
    w, h, rect = SHAPES[name]
    o = run(exe, "shape", w, h, *rect, count, FRAMES)
    inside, outside, empty = walked(w, h, rect, count)
    assert o["wrong"] == 0 and o["ranks"] == count
    assert o["indices"] == o["inside"] == FRAMES * inside      # distinct slots (the driver's check), as many as there are samples inside: each exactly once
    assert o["culled"] == FRAMES * outside and o["empty_ranks"] == empty


def test_the_shapes_hold_what_they_are_named_for():
    assert walked(*SHAPES["one_row_97x53"][:3], 3)[2] == 2 and walked(*SHAPES["one_row_97x53"][:3], 8)[2] == 7    # shards with no row inside
    assert walked(*SHAPES["two_rows_97x53"][:3], 8)[2] == 6 and walked(*SHAPES["nothing_97x53"][:3], 3) == (0, 97 * 53, 3)
    assert walked(*SHAPES["cornell_1080p"][:3], 1)[0] == 984 * 973 == 957432 and walked(*SHAPES["inside_97x53"][:3], 1)[2] == 0


@pytest.mark.parametrize("size,rect,split,frames,base", [((97, 53), (23, 5, 71, 40), 2, 9, 0), ((100, 75), (24, 2, 77, 73), 2, 8, 3), ((97, 53), (0, 0, 60, 30), 3, 11, 7),
                                                         ((97, 53), (50, 3, 50, 47), 4, 17, 0), ((97, 53), (1, 1, 0, 0), 2, 4, 0)])
def test_split_screen_dispatches_deal_their_chunk_of_the_rectangle(exe, size, rect, split, frames, base):
    """Split-screen dispatch: dispatch k holds chunk (base + k) % S^2 of the rectangle, its pixels exactly once — and of the whole image what
    launch_pixel's split branch holds."""
    o = run(exe, "split", size[0], size[1], *rect, split, frames, base)
    assert o["wrong"] == 0
    x0, y0, x1, y1 = rect
    chunks = [(base + k) % (split * split) for k in range(frames)]
    count = lambda a0, a1, c: len([v for v in range(a0, a1 + 1) if v % split == c])
    want = sum(count(x0, x1, c % split) * count(y0, y1, c // split) + count(0, size[0] - 1, c % split) * count(0, size[1] - 1, c // split) for c in chunks)
    assert o["indices"] == want


def test_driver_is_clean_under_address_and_undefined_behaviour_sanitizers(exe_san):
    """The same program built with -fsanitize=address,undefined: a shape per kind, the empty rectangle, split-screen dispatch."""
    for name, count in (("inside_97x53", 3), ("one_column_97x53", 8), ("one_row_97x53", 3), ("one_pixel_97x53", 3), ("nothing_97x53", 1), ("right_bottom_97x53", 1)):
        w, h, rect = SHAPES[name]
        assert run(exe_san, "shape", w, h, *rect, count, FRAMES)["wrong"] == 0
    assert run(exe_san, "split", 97, 53, 23, 5, 71, 40, 2, 9, 1)["wrong"] == 0
