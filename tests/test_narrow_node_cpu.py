"""The two-slot node step of a tree staged into LDS (vulkan-path-tracer_amd/csrc/node_step.hpp), held to the four-wide step on the host.

The whole-path kernel's PLAIN instantiation flags, in the LDS copy of the tree, every child word that names a node whose slots 0 and 1 are used and
whose slots 2 and 3 are not (traverse.hpp stage_scene<true, true>, node_step.hpp narrow_child), and a closest-hit search that stands at flagged nodes
only takes a step of two box tests and one exchange.  tests/tools/narrow_node_host.cpp compiles the kernels' own functions for the host with -ffp-contract=off:
  (a) the flag rule over every child word of the product builder's trees — the Cornell box, tests/whole_spill_scene.py's 16-sheet chain, the compact
      scene of tests/material_scenes.py, a chain of 12 sheets (used slots 4, 4, 3, 2) — and of hand-made nodes with 1, 2, 3 and 4 used slots, a node
      whose used slots are 0 and 2 (never flagged) and a half-empty node under a half-empty node, against the rule stated from bvh_refit.hpp slot_used;
  (b) on every half-empty node of those trees, 10^5 rays per tree through both steps, origins inside and beyond kSlabFmaReach scene sizes so that the
      fma form and the subtract form both run: the same entry distances before and after ordering bit for bit, the same word descended into and the
      same words pushed; rays whose origin lies in both boxes (both entries clamped to tmin: t0 == t1) are part of the set wherever
      the two boxes overlap;
  (c) flagged, unflagged and leaf words through a model of the kernel's stack (kWholeStackRows LDS rows, the overflow region behind them).
Every class is counted and a generator that does not reach one fails.  The GPU side of the same claim: tests/test_gpu_narrow_node.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import material_scenes
import whole_spill_scene as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "narrow_node_host.cpp")
BUILDER = os.path.join(ROOT, "vulkan-path-tracer_amd", "csrc", "bvh_build.cpp")
F32 = np.float32
RAYS = 100000
UNUSED = F32(1.0e30)
COUNT_KEYS = ("fma_cases", "sub_cases", "differing", "both_entered", "none_entered", "ties", "swapped", "pushes", "upper_slots_entered")


class StepCounts(C.Structure):
    _fields_ = [(k, C.c_int64) for k in COUNT_KEYS]


def compile_driver(out, extra):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-march=x86-64-v3", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), SRC, BUILDER, "-o", out, "-lpthread"] + extra)
    return out


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = C.CDLL(compile_driver(str(tmp_path_factory.mktemp("narrow_node") / "libnarrow_node_host.so"), ["-shared", "-fPIC"]))
    L.nn_narrow_bit.restype = C.c_int
    L.nn_reach.restype = C.c_float
    L.nn_build.restype = C.c_int
    L.nn_build.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.nn_stage.restype = None
    L.nn_stage.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.nn_steps.restype = None
    L.nn_steps.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.POINTER(StepCounts)]
    L.nn_stack.restype = C.c_int
    L.nn_stack.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    return L


def build_tree(lib, tris):
    """The builder's fp32 nodes: n x 32 dwords (minx miny minz maxx maxy maxz child pad, four each), as floats."""
    nodes = np.zeros((64, 32), F32)
    n = lib.nn_build(tris.ctypes.data, len(tris), nodes.ctypes.data, len(nodes))
    assert 0 < n <= len(nodes)
    return np.ascontiguousarray(nodes[:n])


def stage(lib, nodes):
    """(staged copy, flagged, expect: n x 4 bool, used: n masks)"""
    staged = np.ascontiguousarray(nodes.copy())
    n = len(staged)
    flagged, expect, used = np.zeros((n, 4), np.uint8), np.zeros((n, 4), np.uint8), np.zeros(n, np.uint8)
    lib.nn_stage(staged.ctypes.data, n, flagged.ctypes.data, expect.ctypes.data, used.ctypes.data)
    return staged, flagged.astype(bool), expect.astype(bool), used


def children(nodes):
    return nodes.view(np.int32)[:, 24:28]


def handmade():
    """Seven nodes: a root over inner nodes with 1, 2, 3 and 4 used slots; node 2's first child is another half-empty node (5); node 6 uses slots 0
    and 2.  Boxes overlap, so a ray can stand in both boxes of a half-empty node."""
    nodes = np.full((7, 32), UNUSED, F32)
    ch = children(nodes)
    ch[:] = 0
    nodes[:, 28:] = 0.0

    def box(i, k, lo, hi, child):
        nodes[i, 0 + k], nodes[i, 4 + k], nodes[i, 8 + k] = lo, lo * 0.5, lo - 0.25
        nodes[i, 12 + k], nodes[i, 16 + k], nodes[i, 20 + k] = hi, hi * 0.5 + 1.0, hi + 0.25
        ch[i, k] = child
    leaf = lambda first, cnt=1: ~((first << 3) | (cnt - 1))
    for k in range(4): box(0, k, -2.0 + k, -1.0 + k, 1 + k)
    box(1, 0, -2.0, -1.5, leaf(0))
    box(2, 0, -1.0, -0.4, 5); box(2, 1, -0.7, 0.0, leaf(1))
    for k in range(3): box(3, k, 0.3 * k, 0.5 + 0.3 * k, leaf(2 + k))
    for k in range(4): box(4, k, 1.0 + 0.2 * k, 1.4 + 0.2 * k, 6 if k == 3 else leaf(5 + k))
    box(5, 0, -1.0, -0.8, leaf(8)); box(5, 1, -0.9, -0.4, leaf(9))
    box(6, 0, 1.6, 1.8, leaf(10)); box(6, 2, 1.7, 2.0, leaf(11))
    return nodes


TREES = ("cornell", "chain", "chain12", "compact", "handmade")


@pytest.fixture(scope="module")
def trees(lib, scenes, vpt):
    cache = {}

    def get(name):
        if name not in cache:
            if name == "handmade":
                cache[name] = (handmade(), 2.25)
            else:
                sc = scenes("cornell_box") if name == "cornell" else W.chain_scene(vpt) if name == "chain" else W.chain_scene(vpt, 12) if name == "chain12" else material_scenes.variant("compact")[0]
                tris = W.world_triangles(sc)
                p = tris[:, 0:3]
                extent = max(float(np.abs(q).max()) for q in (p, p + tris[:, 3:6], p + tris[:, 6:9]))
                nodes = build_tree(lib, tris)
                assert nodes.nbytes + tris.nbytes <= 3072 or name != "cornell"
                cache[name] = (nodes, extent)
        return cache[name]
    return get


@pytest.mark.parametrize("name", TREES)
def test_flag_rule_over_every_child_word(lib, trees, name):
    nodes, _ = trees(name)
    bit = lib.nn_narrow_bit()
    assert bit == 1 << 30
    staged, flagged, expect, used = stage(lib, nodes)
    before, after = children(nodes), children(staged)
    slots = [bin(int(u)).count("1") for u in used]
    print("%s: %d nodes, used slots %s, flagged words %s" % (name, len(nodes), slots, [(int(i), int(k)) for i, k in zip(*np.nonzero(flagged))]))
    assert np.array_equal(flagged, expect)
    # by hand, from the planes: the word names an inner node with minx = {used, used, 1e30, 1e30}
    for i in range(len(nodes)):
        for k in range(4):
            w = int(before[i, k])
            by_hand = w >= 0 and bool((nodes[w, 0:2] != UNUSED).all() and (nodes[w, 2:4] == UNUSED).all())
            assert bool(flagged[i, k]) == by_hand, (i, k, w)
    assert (after[flagged] == (before[flagged] | bit)).all() and (after[flagged] >= 0).all()
    assert np.array_equal(after[~flagged], before[~flagged])
    assert (after[before < 0] == before[before < 0]).all(), "a leaf word was touched"
    assert np.array_equal(staged[:, :24], nodes[:, :24]), "the pass wrote a plane"
    in_use = np.array([[(int(u) >> k) & 1 for k in range(4)] for u in used], bool)
    assert not (before[in_use] == 0).any(), "no used slot names the root: it is entered as cur = 0 and carries no flag"   # (an unused slot's word is 0; no search reads it)
    assert (before[before >= 0] < len(nodes)).all() and len(nodes) < (1 << 30) // 128
    if name == "cornell":
        assert len(nodes) == 3 and list(used) == [15, 3, 3]                     # (tests/test_gpu_lds_node_step.py: three nodes, two of them half-empty)
        assert sorted(int(w) for w in before[flagged]) == [1, 2] and flagged[0].sum() == 2
    if name == "chain12":
        assert slots == [4, 4, 3, 2] and flagged.sum() == 1      # the GPU case with a three-slot node beside a half-empty one (tests/narrow_node_cases.py)
    if name == "handmade":
        assert slots == [4, 1, 2, 3, 4, 2, 2] and used[6] == 5
        assert [(int(i), int(k)) for i, k in zip(*np.nonzero(flagged))] == [(0, 1), (2, 0)]   # the words that name nodes 2 and 5; node 6 (slots 0 and 2) stays unflagged


def rays_at(rng, nodes, j, extent, reach, n):
    """n rays for the half-empty node j: origins in its boxes, in BOTH boxes where they overlap, around the scene, and beyond the fma form's reach;
    directions towards the boxes or anywhere, some with zero components; tlimit the search's tmax or a hit somewhere around."""
    lo = np.stack([nodes[j, 0:2], nodes[j, 4:6], nodes[j, 8:10]], axis=1).astype(np.float64)      # [slot, axis]
    hi = np.stack([nodes[j, 12:14], nodes[j, 16:18], nodes[j, 20:22]], axis=1).astype(np.float64)
    ulo, uhi = lo.min(axis=0), hi.max(axis=0)
    ilo, ihi = lo.max(axis=0), hi.min(axis=0)
    overlap = bool((ilo < ihi).all())
    cls = rng.choice(4, n, p=[0.3, 0.2, 0.3, 0.2])          # in the union box, in both boxes, around the scene, beyond reach
    o = rng.uniform(ulo, uhi, (n, 3))
    if overlap:
        o[cls == 1] = rng.uniform(ilo, ihi, (int((cls == 1).sum()), 3))
    o[cls == 2] = rng.uniform(-2.0, 2.0, (int((cls == 2).sum()), 3)) * extent
    far = rng.uniform(-1.0, 1.0, (int((cls == 3).sum()), 3)) * extent
    ax = rng.integers(0, 3, len(far))
    far[np.arange(len(far)), ax] = np.where(rng.random(len(far)) < 0.5, -1.0, 1.0) * reach * extent * 10.0 ** rng.uniform(0.01, 2.0, len(far))
    o[cls == 3] = far
    o = o.astype(F32)
    slot = rng.integers(0, 2, n)
    target = lo[slot] + rng.random((n, 3)) * (hi[slot] - lo[slot])
    d = np.where((rng.random(n) < 0.7)[:, None], target - o, rng.normal(size=(n, 3)))
    d[(d == 0.0).all(axis=1)] = (0.0, 0.0, 1.0)
    d = d / np.linalg.norm(d, axis=1)[:, None]
    d[rng.random((n, 3)) < 0.05] = 0.0
    d[(d == 0.0).all(axis=1)] = (0.0, 1.0, 0.0)
    d = d.astype(F32)
    rng_t = np.empty((n, 2), F32)
    rng_t[:, 0] = np.where(rng.random(n) < 0.5, 0.01, 1.0e-4)
    dist = np.linalg.norm(target - o, axis=1)
    rng_t[:, 1] = np.where(rng.random(n) < 0.5, 1.0e5, np.maximum(rng_t[:, 0], dist * rng.uniform(0.5, 1.5, n))).astype(F32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d), np.ascontiguousarray(rng_t), overlap, cls


@pytest.mark.parametrize("name", TREES)
def test_two_slot_step_is_the_four_wide_step(lib, trees, name):
    nodes, extent = trees(name)
    staged, flagged, _, used = stage(lib, nodes)
    half = [i for i in range(len(nodes)) if used[i] == 3 and i != 0]
    assert sorted(set(int(w) for w in children(nodes)[flagged])) == half
    print("%s: half-empty nodes %s of %d" % (name, half, len(nodes)))
    if name in ("cornell", "handmade"):
        assert len(half) == 2
    rng = np.random.default_rng(20241022)
    total = dict.fromkeys(COUNT_KEYS, 0)
    overlapping = 0
    for j in half:
        n = -(-RAYS // len(half))
        o, d, rt, overlap, cls = rays_at(rng, staged, j, extent, float(lib.nn_reach()), n)
        c = StepCounts()
        lib.nn_steps(staged.ctypes.data, j, n, o.ctypes.data, d.ctypes.data, rt.ctypes.data, extent, C.byref(c))
        got = {k: int(getattr(c, k)) for k in COUNT_KEYS}
        print("  node %d (boxes overlap: %s): %r" % (j, overlap, got))
        assert got["sub_cases"] == n and got["fma_cases"] <= int((cls != 3).sum())
        assert got["fma_cases"] >= n // 2 and got["sub_cases"] - got["fma_cases"] >= n // 10, "both forms must run"
        assert got["both_entered"] >= n // 100 and got["none_entered"] >= n // 100 and got["swapped"] >= n // 100 and got["pushes"] == got["both_entered"]
        if overlap:
            overlapping += 1
            assert got["ties"] >= n // 20, "origins inside both boxes enter both at tmin"
        for k in COUNT_KEYS: total[k] += got[k]
    # a tree without a half-empty node flags nothing, and its searches never leave the four-wide step
    assert total["differing"] == 0 and total["upper_slots_entered"] == 0, total
    assert (total["sub_cases"] >= RAYS) == bool(half)
    if name == "handmade":
        assert overlapping == 2 and total["ties"] > 0


def test_a_flagged_word_survives_the_stack(lib):
    src = open(os.path.join(ROOT, "vulkan-path-tracer_amd", "csrc", "traverse.hpp")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    rows = const("kWholeStackRows")
    overflow = const("kStackDepth") + const("kStackOverflow") - rows
    assert rows == 6
    bit = lib.nn_narrow_bit()
    rng = np.random.default_rng(3)
    for depth in (1, rows, rows + 1, 20, rows + overflow):
        kind = rng.integers(0, 3, depth)
        idx = rng.integers(1, 24, depth)
        words = np.where(kind == 0, idx | bit, np.where(kind == 1, idx, ~(idx << 3))).astype(np.int64).astype(np.int32).view(np.uint32)
        words[0] = np.uint32(5 | bit)
        words[-1] = np.uint32(7 | bit)          # (the deepest entry: in the overflow region wherever the stack reaches it)
        spilled = C.c_int(0)
        bad = lib.nn_stack(np.ascontiguousarray(words).ctypes.data, depth, rows, overflow, C.byref(spilled))
        assert bad == 0 and spilled.value == max(0, depth - rows), (depth, bad, spilled.value)


def test_driver_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same driver as a stand-alone program over hand-made nodes and its own generator, built with -fsanitize=address,undefined."""
    exe = compile_driver(str(tmp_path / "narrow_node_san"), ["-g", "-DNNH_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "flag words differing 0" in r.stdout and " differing 0 " in r.stdout and "upper slots entered 0" in r.stdout
