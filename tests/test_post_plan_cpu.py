"""What the case table of tests/test_gpu_post_shapes.py reaches, checked without a GPU against tests/post_plan.py, the plain restatement
of enqueue_post's fused schedule: a census of the launch kinds, level counts and odd-size classes a sweep of image sizes can produce
(the table must reach all of them), the LDS bounds of the tail and of the two chain kernels over the same sweep, and the agreement of
the two CPU references (the scalar oracle and the vectorised numpy restatement) at every case of the table."""
import itertools

import numpy as np
import pytest

import post_plan
from post_plan import K
from test_gpu_post_shapes import CASES, CUSTOM, SPECIAL_CASES, hdr_image
from test_oracle_post import np_post

# thin strips, sizes around the tile widths (64, 8, 4), odd chains (511, 1023: odd at every level), 1080p- and 4K-like sizes
SWEEP = [2, 3, 4, 5, 7, 8, 10, 16, 17, 18, 33, 64, 65, 68, 97, 131, 135, 255, 256, 301, 511, 541, 1001, 1023, 1080, 1297, 1920, 2047, 2160, 3401, 3840]
SWEEP_CASES = [(w, h, m) for w, h in itertools.product(SWEEP, SWEEP) for m in range(1, post_plan.MAX_MIPS + 1)]


def test_constants_come_from_the_sources():
    for name in post_plan.PLAN_CONSTANTS + ("kTailMaxLevels", "kTailMaxTexels", "kTileW", "kChainTileH", "kChainW1", "kChainRows", "kChainMax",
                                            "kDcMax", "kDcTW", "kDcTH", "kDcW0", "kDcH0", "kDcW1", "kDcH1"):
        assert isinstance(K.get(name), int) and K[name] > 0, name
    # the host's limits (kernels.hpp) and the kernels' own (kernels_post.hip) describe the same launches
    assert K["kBloomChainMax"] == K["kChainMax"] and K["kBloomDownChainMax"] == K["kDcMax"]
    assert K["kBloomTailMaxLevels"] <= K["kTailMaxLevels"]
    assert (K["kDcW0"], K["kDcH0"], K["kDcW1"], K["kDcH1"]) == (41, 25, 19, 11)


def test_plan_of_the_baseline_size():
    """1920x1080 with all ten mips: the launches tests/test_gpu_post.py counts on the device (1 + 1 + 1 + 1 bloom, 1 tonemap)."""
    assert post_plan.plan(1920, 1080, 10) == ["first", "down_chain 3", "tail staged 5", "up_chain 4", "final up"]
    assert post_plan.predicted_launches(1920, 1080, 10) == (4, 1) and post_plan.reference_launches(1920, 1080, 10) == (19, 1)
    assert post_plan.plan(64, 64, 1) == ["final noup"] and post_plan.predicted_launches(64, 64, 1) == (0, 1)


def test_case_table_reaches_everything_the_sweep_reaches():
    reachable = set()
    for c in SWEEP_CASES:
        reachable |= post_plan.census(*c)
    table = set()
    for c in CASES:
        table |= post_plan.census(*c)
    missing = sorted(reachable - table)
    assert not missing, "no case of test_gpu_post_shapes.CASES reaches: " + "; ".join(missing)
    # the sweep itself is wide enough: every level count of the chain kernels, both final kernels, and the single launches
    wanted = ["down_chain %d" % n for n in range(2, K["kDcMax"] + 1)] + ["up_chain %d" % n for n in range(2, K["kChainMax"] + 1)]
    for e in wanted + ["first", "down", "up", "final up", "final noup"]:
        assert e in reachable, e
    assert any(e.startswith("tail staged") for e in reachable)


def test_no_chained_launch_is_a_single_block():
    """Every level a chained launch tiles has more than kBloomTailMaxTexels texels (smaller ones belong to the tail), which is more than
    one tile of either chain kernel: the table can hold one block row or one block column, never one block.  If a change of the
    constants makes a one-block chain possible this fails, and a case for it belongs in the table."""
    fewest = {}
    for w, h, m in SWEEP_CASES:
        sizes = post_plan.mip_sizes(w, h)
        for entry, levels in post_plan.launches(w, h, m):
            kind = entry.split()[0]
            if kind in ("down_chain", "up_chain"):
                gx, gy = post_plan.chain_grid(kind, sizes, levels)
                fewest[kind] = min(fewest.get(kind, gx * gy), gx * gy)
    assert set(fewest) == {"down_chain", "up_chain"} and min(fewest.values()) > 1, fewest


def test_special_value_cases_reach_both_tails_and_the_final_without_up_sample():
    reached = set().union(*(post_plan.plan(*c) for c in SPECIAL_CASES))
    assert any(e.startswith("tail plain") for e in reached) and any(e.startswith("tail staged") for e in reached) and "final noup" in reached


def test_lds_bounds_over_the_sweep():
    """What the kernels keep in LDS fits, for every launch of every swept case: the tail's levels (and a staged tail's base), and the
    tile of every level a block of a chained launch evaluates — the restated nlx/nhx/nly/nhy and lox/hix/loy/hiy, all blocks."""
    seen = set()
    for w, h, m in SWEEP_CASES:
        sizes = post_plan.mip_sizes(w, h)
        for entry, levels in post_plan.launches(w, h, m):
            key = (entry, tuple(sizes[i] for i in range(levels[0] - 1, min(levels[-1] + 2, len(sizes)))))
            if key in seen:
                continue
            seen.add(key)
            what = "%dx%d mips %d: %s" % (w, h, m, entry)
            kind = entry.split()[0]
            if kind == "tail":
                assert len(levels) <= K["kTailMaxLevels"], what
                assert sum(sizes[i][0] * sizes[i][1] for i in levels) <= K["kTailMaxTexels"], what
                bw, bh = sizes[levels[0] - 1]
                assert (bw * bh <= K["kTailMaxBase"]) == (entry.split()[1] == "staged"), what
            elif kind == "down_chain":
                n = len(levels)
                assert 2 <= n <= K["kDcMax"], what
                xs = post_plan.down_chain_axis([sizes[i][0] for i in levels], K["kDcTW"])
                ys = post_plan.down_chain_axis([sizes[i][1] for i in levels], K["kDcTH"])
                for j in range(n):
                    for axis, size in ((xs, sizes[levels[j]][0]), (ys, sizes[levels[j]][1])):
                        ol, oh, nl, nh = axis[j]
                        # the owned ranges of the blocks partition the level; what a block evaluates contains what it owns
                        assert ol[0] == 0 and oh[-1] == size - 1 and (ol[1:] == oh[:-1] + 1).all() and (ol <= oh).all(), (what, j)
                        assert (nl <= ol).all() and (nh >= oh).all(), (what, j)
                        if j + 1 < n:   # every tap of the next level's evaluated texels lies inside this level's tile
                            _, _, unl, unh = axis[j + 1]
                            up = sizes[levels[j + 1]][0 if axis is xs else 1]
                            assert (2 * np.clip(unl, 0, up - 1) - 2 >= nl).all() and (2 * np.clip(unh, 0, up - 1) + 1 <= nh).all(), (what, j)
                    if j < n - 1:   # levels below the top are kept in LDS: level 0 in tile0, level 1 (of three) in tile1
                        tw = int((xs[j][3] - xs[j][2] + 1).max())
                        th = int((ys[j][3] - ys[j][2] + 1).max())
                        cap_w, cap_h = (K["kDcW0"], K["kDcH0"]) if j == 0 else (K["kDcW1"], K["kDcH1"])
                        assert tw <= cap_w and th <= cap_h, (what, j, tw, th)
            elif kind == "up_chain":
                n = len(levels)
                assert 2 <= n <= K["kChainMax"], what
                lv = list(range(levels[0], levels[0] + n + 1))   # mip[0 .. n] of the launch
                xs = post_plan.up_chain_axis([sizes[i][0] for i in lv], n, K["kTileW"])
                ys = post_plan.up_chain_axis([sizes[i][1] for i in lv], n, K["kChainTileH"])
                for j in range(1, n):
                    tw = int((xs[j][1] - xs[j][0] + 1).max())
                    th = int((ys[j][1] - ys[j][0] + 1).max())
                    # one entry per thread: a tile of more than 256 entries would silently leave texels unevaluated
                    assert tw * th <= 256 and tw * th <= K["kChainRows"] * (K["kChainW1"] + 1), (what, j, tw, th)
                    # the taps of the level below (x / 2 - 1 .. x / 2 + 2 of its clamped texels) lie inside this tile
                    for axis, d in ((xs, 0), (ys, 1)):
                        below = sizes[lv[j - 1]][d]
                        assert (np.clip(axis[j - 1][0], 0, below - 1) // 2 - 1 >= axis[j][0]).all(), (what, j)
                        assert (np.clip(axis[j - 1][1], 0, below - 1) // 2 + 2 <= axis[j][1]).all(), (what, j)
    kinds = {k[0].split()[0] for k in seen}
    assert {"tail", "down_chain", "up_chain"} <= kinds


@pytest.mark.parametrize("w,h,mips", CASES, ids=["%dx%d-m%d" % c for c in CASES])
def test_oracle_and_numpy_agree_at_every_case(oracle, vpt, w, h, mips):
    """The GPU test's reference is checked by a second, independent one where the GPU test looks: bloom mip 0 of the scalar oracle
    equals the vectorised numpy restatement bit for bit, with the default parameters and with the table's other set."""
    img = hdr_image(w, h, 3 * w + h)
    for kw in ({}, CUSTOM):
        pp = vpt.default_post_params(mip_count=mips, **kw)
        _, bloom = oracle.postprocess(img, pp)
        ref = np_post(img, pp)
        assert np.array_equal(bloom[..., :3].view(np.uint32), np.ascontiguousarray(ref).view(np.uint32)), kw
        assert (bloom[..., 3] == 1).all()
