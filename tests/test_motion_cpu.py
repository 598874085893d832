"""The temporal history across instance moves (vpt_temporal_options.instance_motion = 1) without a device: csrc/temporal.hpp's temporal_pixel_motion,
instance_motion_of and MotionSnapshot compiled for the host (tests/tools/motion_driver.cpp, driven as api_post.hip and api_scene.hip drive them), held to
  * the existing host compiles: without a table, or with every visible instance still, image, record, moments and variance are temporal_driver's and
    svgf_driver's bits;
  * a float64 restatement written from the rule alone (tests/ref_motion64.py), on every hit pixel but those where that restatement's own decisions are
    marginal (at most 5 % of the hit pixels per step, asserted on the restatement alone);
  * the exact properties: what is carried, what is fresh, what the table decides, what a singular matrix costs, how moves compose;
  * AddressSanitizer / UBSan: the same driver built with -fsanitize=address,undefined, as a stand-alone program, on the 7 x 5 sequences.
The inputs are analytic (tests/motion_host.py): a room (instance 0), a rectangle floating in front of its wall (instance 1) that is translated, rotated in and
out of its plane and scaled non-uniformly about its centre, and a panel at 45 degrees (instance 2).  The same function on the device, against this host compile
bit for bit: tests/test_gpu_motion.py.

Host compile against float64, measured on these inputs (x86-64-v3, g++ -O2) over every size, flag set, camera setting and step, on the hit pixels that are not
left out (at most 3.6 % of them per step: one of 28 at 7 x 5): the largest absolute error of the image is 2.07e-05 (150 x 9, moving camera) and of the stored
history colour 2.31e-05 (150 x 9, still camera, demodulated) on values up to 1, of the history length 1.74e-05 frames (45 x 37, the pan) on values up to 8, and
of the motion 5.17e-04 pixels (150 x 9, the pan, where the motion reaches 248 pixels: points that leave the image near the previous camera's plane, whose
clip.w is small).  As in test_temporal_cpu.py the first three are the error of the reprojected position times the difference between neighbouring history
pixels.  The bounds below are 4 x those figures."""
import numpy as np
import pytest

import motion_host as MH
import ref_motion64 as M64
import ref_temporal64 as R64
import svgf_host as SH
import temporal_host as TH
from refit_moves import about, rotate, scale, translate

F32 = np.float32
SIZES = [(7, 5), (45, 37), (150, 9)]
FLAG_SETS = [0, TH.DEMODULATE, TH.MATCH_INSTANCE, TH.DEMODULATE | TH.MATCH_INSTANCE]
BOTH = TH.DEMODULATE | TH.MATCH_INSTANCE
P = MH.DEFAULTS
MEASURED = dict(image=2.07e-5, record=2.31e-5, length=1.74e-5, motion=5.17e-4)
TOL = {k: 4.0 * v for k, v in MEASURED.items()}
LEFT_OUT_CAP = 0.05
IDENTITY2 = np.stack([np.eye(4), np.eye(4)]).astype(F32)


def size_id(k):
    return "%dx%d" % k


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("motion")
    return MH.compile_driver(str(d / "motion_driver")), d


@pytest.fixture(scope="module")
def sequences():
    """(size, moving camera) -> (frames, start matrices)."""
    return {(key, cam): MH.sequence(key[0], key[1], cam) for key in SIZES for cam in (False, True)}


@pytest.fixture(scope="module")
def host_results(driver, sequences):
    exe, d = driver
    return {(key, cam, fl): MH.run_sequence(exe, d, frames, start, tag="seq_%d_%d_%d_%d" % (key[0], key[1], cam, fl), flags=fl)
            for (key, cam), (frames, start) in sequences.items() for fl in FLAG_SETS}


def run(driver, frames, start, tag="p", **params):
    return MH.run_sequence(driver[0], driver[1], frames, start, tag=tag, **params)


def state_of(frame, record):
    return R64.State(record[..., :3].astype(np.float64), record[..., 3].astype(np.float64), frame.normal[..., :3].astype(np.float64), frame.depth.astype(np.float64),
                     frame.inst, frame.view_inv, frame.proj_inv)


def reference_step(frames, start, results, k, flags, normal_rule="nt", **over):
    """Frame k in float64, its history being what the host compile left behind frame k - 1, its previous matrices those of frame k - 1."""
    p = dict(P, **over)
    mats = MH.matrices_after(start, frames)
    prev = state_of(frames[k - 1], results[k - 1]["record"]) if k > 0 else None
    fr = frames[k]
    return M64.temporal64(prev, mats[k - 1] if k > 0 else None, mats[k], fr.view_inv, fr.proj_inv, fr.m, fr.radiance, fr.normal, fr.albedo, fr.depth, fr.inst,
                          p["max_history"], p["depth_tolerance"], p["normal_threshold"], flags, normal_rule)


# ---- no table, or every visible instance still: the existing drivers' bits
@pytest.mark.parametrize("variance", [0, 1])
@pytest.mark.parametrize("key", SIZES, ids=size_id)
def test_without_a_move_the_bits_are_the_existing_drivers(driver, tmp_path, key, variance):
    """temporal_host.analytic_sequence under all four flag sets: (a) no move at all — no table; (b) vpt_set_instance_transforms with the matrices the instances
    have — no table either; (c) a third instance that no pixel shows moves — a table, in which every visible instance is still."""
    frames = TH.analytic_sequence(*key)
    t_exe = TH.compile_driver(str(tmp_path / "temporal_driver"))
    s_exe = SH.compile_driver(str(tmp_path / "svgf_driver"))
    three = np.stack([np.eye(4), np.eye(4), np.eye(4)]).astype(F32)
    same = [MH.with_moves(fr, [(0, [np.eye(4), np.eye(4)])] if k else []) for k, fr in enumerate(frames)]
    other = [MH.with_moves(fr, [(2, [translate(0.1 * k, 0.0, 0.0)])] if k else []) for k, fr in enumerate(frames)]
    tables = 0
    for fl in FLAG_SETS:
        want_t = TH.run_sequence(t_exe, tmp_path, frames, tag="t", flags=fl)
        want_s = SH.run_sequence(s_exe, tmp_path, frames, tag="s", flags=fl, variance=1) if variance else None
        for name, seq, start, table in (("none", frames, IDENTITY2, False), ("same", same, IDENTITY2, False), ("other", other, three, True)):
            got = MH.run_sequence(driver[0], tmp_path, seq, start, tag="m", flags=fl, variance=variance)
            for k in range(len(frames)):
                assert got[k]["table"] == (table and k > 0) and not got[k]["state"][:2].any(), (name, fl, k)
                tables += got[k]["table"]
                assert np.array_equal(MH.bits(got[k]["image"]), MH.bits(want_t[k][0])) and np.array_equal(MH.bits(got[k]["record"]), MH.bits(want_t[k][1])), (name, fl, k)
                if variance:
                    for what in ("image", "record", "moments", "variance"):
                        assert np.array_equal(MH.bits(got[k][what]), MH.bits(want_s[k][what])), (name, fl, k, what)
    assert tables == 3 * len(FLAG_SETS)


# ---- against float64
def test_the_inputs_hold_what_they_are_for(sequences, host_results):
    """By the restatement alone: every step of every sequence keeps its marginal share under the cap, and over each sequence the rectangle's pixels are carried
    (four taps counted) and the wall it uncovered is fresh."""
    for (key, cam), (frames, start) in sequences.items():
        carried = fresh = 0
        for k in range(1, len(frames)):
            info = reference_step(frames, start, host_results[(key, cam, BOTH)], k, BOTH)[3]
            hit = frames[k].depth >= 0
            share = info["marginal"].sum() / hit.sum()
            rect = frames[k].inst == 1
            carried += int((rect & (info["counted"] == 4 if key != (7, 5) else info["has"])).sum())      # (at 7 x 5 the rectangle is two pixels)
            fresh += int((hit & ~rect & ~info["has"]).sum())
            print(key, "moving camera" if cam else "still camera", "step", k, "left out %.4f" % share, "state", info["state"], "rectangle pixels", int(rect.sum()))
            assert share <= LEFT_OUT_CAP, (key, cam, k, share)
            assert info["state"][1] == M64.MOVED and info["state"][0] == M64.STILL
        assert carried >= (2 if key == (7, 5) else 10 if key == (150, 9) else 50) and fresh >= 1, (key, cam, carried, fresh)


@pytest.mark.parametrize("flags", FLAG_SETS)
@pytest.mark.parametrize("cam", [False, True], ids=["still_camera", "moving_camera"])
@pytest.mark.parametrize("key", SIZES, ids=size_id)
def test_host_compile_against_float64(sequences, host_results, key, cam, flags):
    """Image, stored history colour, length and motion on every hit pixel the restatement does not call marginal; the bounds are 4 x the measured figures."""
    frames, start = sequences[(key, cam)]
    results = host_results[(key, cam, flags)]
    for k in range(len(frames)):
        image, length, state, info = reference_step(frames, start, results, k, flags)
        hit = frames[k].depth >= 0
        keep = hit & ~info["marginal"]
        got = results[k]
        err = dict(image=np.abs(got["image"].astype(np.float64) - image)[keep].max(), length=np.abs(got["record"][..., 3].astype(np.float64) - length)[keep].max(),
                   record=np.abs(got["record"][..., :3].astype(np.float64) - state.e)[keep].max(), motion=np.abs(got["motion"].astype(np.float64) - info["motion"])[keep].max())
        print("%s %s flags %d step %d: max |host - float64| %s; left out %d of %d" % (key, "moving" if cam else "still", flags, k, " ".join("%s %.3g" % kv for kv in err.items()),
                                                                                        info["marginal"].sum(), hit.sum()))
        assert np.isfinite(got["image"]).all()
        assert np.array_equal(got["state"], info["state"]) and got["table"] == (k > 0)
        for what, e in err.items():
            assert e <= TOL[what], (what, e)
        assert not got["motion"][~info["reprojected"] & ~info["marginal"]].any()      # (0, 0) wherever nothing was reprojected: misses, the first frame


# ---- what is carried and what is fresh
@pytest.mark.parametrize("cam", [False, True], ids=["still_camera", "moving_camera"])
@pytest.mark.parametrize("key", [(45, 37), (150, 9)], ids=size_id)
def test_the_moved_instance_is_carried_and_the_wall_it_uncovered_is_fresh(sequences, host_results, key, cam):
    """Pixels of the rectangle all four taps of which count: length = previous + m exactly (the previous lengths of a frame's rectangle pixels are one value, so
    sl / sw gives it back), and the history colour — recovered from the record, e = hist + (e_cur - hist) a — is the previous record sampled bilinearly at
    pixel + motion: where the surface WAS.  Wall pixels whose four taps all land on the rectangle's old place are fresh under MATCH_INSTANCE."""
    frames, start = sequences[(key, cam)]
    res = host_results[(key, cam, TH.MATCH_INSTANCE)]
    h, w = frames[0].depth.shape
    carried = fresh = 0
    for k in range(1, len(frames)):
        info = reference_step(frames, start, res, k, TH.MATCH_INSTANCE)[3]
        got, before = res[k], res[k - 1]
        yy, xx = np.mgrid[0:h, 0:w]
        fx, fy = xx + got["motion"][..., 0].astype(np.float64), yy + got["motion"][..., 1].astype(np.float64)
        x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
        full = (frames[k].inst == 1) & (info["counted"] == 4) & ~info["marginal"] & ~info["near_integer"]
        prev_len = before["record"][..., 3]
        for (y, x) in zip(*np.nonzero(full)):
            taps = [(y0[y, x] + j, x0[y, x] + i) for j in (0, 1) for i in (0, 1)]
            assert all(frames[k - 1].inst[t] == 1 for t in taps)
            lens = {float(prev_len[t]) for t in taps}
            if len(lens) == 1:      # (sl / sw gives a common length back to within the rounding of its products: 6 b is not exact)
                assert abs(got["record"][y, x, 3] - min(lens.pop() + frames[k].m, P["max_history"])) <= 1e-5
            ax, ay = fx[y, x] - x0[y, x], fy[y, x] - y0[y, x]
            wts = [(1 - ax) * (1 - ay), ax * (1 - ay), (1 - ax) * ay, ax * ay]
            hist = sum(wt * before["record"][t][:3].astype(np.float64) for wt, t in zip(wts, taps))
            a = frames[k].m / float(got["record"][y, x, 3])
            want = hist + (frames[k].radiance[y, x, :3].astype(np.float64) - hist) * a
            assert np.abs(got["record"][y, x, :3] - want).max() <= 1e-4      # (the motion is a float32 difference of values up to 150: 1.5e-5 of a pixel, times a neighbour difference of order 1)
            carried += 1
        # the wall behind the rectangle's old place
        wall = (frames[k].inst == 0) & info["reprojected"]      # (pixel + motion is the host compile's own fx, fy exactly: the taps below are the ones it read)
        for (y, x) in zip(*np.nonzero(wall)):
            taps = [(y0[y, x] + j, x0[y, x] + i) for j in (0, 1) for i in (0, 1)]
            if all(0 <= ty < h and 0 <= tx < w and frames[k - 1].inst[ty, tx] == 1 for ty, tx in taps):
                assert got["record"][y, x, 3] == frames[k].m and np.array_equal(MH.bits(got["image"][y, x]), MH.bits(frames[k].radiance[y, x]))
                fresh += 1
    print(key, cam, "carried", carried, "fresh", fresh)
    assert carried > (50 if key == (45, 37) else 10) and fresh > (20 if key == (45, 37) else 3)


@pytest.mark.parametrize("key", SIZES, ids=size_id)
def test_the_table_is_what_decides(driver, sequences, host_results, key):
    """The same sequence with the table withheld from the pixels: the rectangle's pixels come out otherwise, the room's do not change where no tap of theirs
    is on the rectangle (under MATCH_INSTANCE a room pixel never counts a rectangle tap)."""
    frames, start = sequences[(key, False)]
    with_table = host_results[(key, False, BOTH)]
    without = run(driver, frames, start, tag="withheld", flags=BOTH, withhold=True)
    differ = 0
    for k in range(1, len(frames)):
        assert without[k]["table"]
        rect = frames[k].inst == 1
        d = (MH.bits(with_table[k]["record"]) != MH.bits(without[k]["record"])).any(-1)
        differ += int((d & rect).sum())
        if k == 1:   # (later steps start from different histories)
            assert not (d & ~rect).any()
            assert (with_table[k]["record"][..., 3][rect] > without[k]["record"][..., 3][rect]).any()
    assert differ >= (2 if key == (7, 5) else 10 if key == (150, 9) else 50)


# ---- normals under a non-uniform scale
def test_normals_go_with_the_inverse_transpose(driver):
    """The panel at 45 degrees squashed to a third along z about its centre: its normal turns towards z while its tangents turn away from it.  Turned by nt, the
    current normal IS the previous one (cosine 1); turned by D's own linear part it is 53 degrees off (cosine 0.6 < 0.9) — found with the restatement, which
    under that rule gives these pixels no history.  The host compile follows nt."""
    w, h = 45, 37
    cam = MH.STILL_CAMERA
    f0 = MH.frame_of(w, h, cam, 2, seed=1, xforms=MH.START)
    cur = MH.START.copy()
    cur[2] = (MH.PANEL_SQUASH @ MH.START[2].astype(np.float64)).astype(F32)
    f1 = MH.frame_of(w, h, cam, 1, seed=2, xforms=cur, moves=[(2, [cur[2]])])
    res = run(driver, [f0, f1], MH.START, tag="squash", flags=BOTH)
    by_nt = reference_step([f0, f1], MH.START, res, 1, BOTH)[3]
    by_linear = reference_step([f0, f1], MH.START, res, 1, BOTH, normal_rule="linear")[3]
    panel = (f1.inst == 2) & ~by_nt["marginal"] & ~by_linear["marginal"]
    opposite = panel & by_nt["has"] & ~by_linear["has"]
    print("panel pixels", int(panel.sum()), "with history by nt and none by the linear part", int(opposite.sum()))
    assert opposite.sum() > 20
    assert (res[1]["record"][..., 3][opposite] == f0.m + f1.m).all()
    assert res[1]["state"][2] == MH.MOVED


# ---- a singular or non-finite matrix
@pytest.mark.parametrize("case", ["singular_current", "infinite_current", "nan_previous"])
def test_an_instance_without_a_regular_motion_has_no_history_and_costs_nothing_else(driver, sequences, case):
    """The rectangle's current matrix singular or infinite, or its previous one NaN (the guides are those of the regular sequence: the driver takes them as
    given): state 2, its pixels come back as a first frame's, every other pixel keeps the bits of the run in which the rectangle did not move at all."""
    frames, start = sequences[((45, 37), True)]
    f0, f1 = frames[0], frames[1]
    bad = np.array(start[1])
    if case == "singular_current":
        bad[:3, 2] = 0.0
    elif case == "infinite_current":
        bad[0, 3] = np.inf
    else:
        bad[1, 1] = np.nan
    regular = np.array(start[1])
    if case == "nan_previous":
        begin = np.array(start); begin[1] = bad
        moved = [f0, MH.with_moves(f1, [(1, [regular])])]
    else:
        begin = np.array(start)
        moved = [f0, MH.with_moves(f1, [(1, [bad])])]
    got = run(driver, moved, begin, tag=case, flags=BOTH, variance=1)
    still = run(driver, [f0, MH.with_moves(f1, [])], begin, tag=case + "_still", flags=BOTH, variance=1)
    alone = run(driver, [MH.with_moves(f1, [])], begin, tag=case + "_alone", flags=BOTH, variance=1)
    assert got[1]["table"] and list(got[1]["state"]) == [0, 2, 0] and not still[1]["table"]
    rect = f1.inst == 1
    assert rect.sum() > 40 and (~rect & (f1.depth >= 0)).sum() > 50
    for what in ("image", "record", "moments", "variance", "motion"):
        assert np.array_equal(MH.bits(got[1][what])[rect], MH.bits(alone[0][what])[rect]), what
        assert np.array_equal(MH.bits(got[1][what])[~rect], MH.bits(still[1][what])[~rect]), what
    assert (got[1]["record"][..., 3][rect] == f1.m).all() and not got[1]["motion"][rect].any()
    assert (still[1]["record"][..., 3][~rect & (f1.depth >= 0)] > f1.m).sum() > 50


# ---- how moves compose
def test_moves_compose_and_a_move_there_and_back_is_no_move(driver, sequences):
    """The previous transform is the matrix at the latest record, however many calls lie between: A -> B -> C in two calls before one temporal call gives the
    bits of A -> C in one; A -> B -> A builds no table and gives the bits of the run without a move; the same matrix set again is state 0 beside a moved one."""
    frames, start = sequences[((45, 37), False)]
    f0, f1 = frames[0], frames[1]
    C = f1.moves[0][1][0]
    B = (about(MH.RECT_CENTRE, rotate((1.0, 0.3, 0.0), 40.0) @ scale(2.0, 0.5, 1.5)) @ start[1].astype(np.float64)).astype(F32)
    direct = run(driver, [f0, f1], start, tag="direct", flags=BOTH, variance=1)
    through = run(driver, [f0, MH.with_moves(f1, [(1, [B]), (0, [start[0], C])])], start, tag="through", flags=BOTH, variance=1)
    assert direct[1]["table"] and through[1]["table"] and list(through[1]["state"]) == [0, 1, 0]
    for what in ("image", "record", "moments", "variance", "motion"):
        assert np.array_equal(MH.bits(direct[1][what]), MH.bits(through[1][what])), what
    # there and back: the guides of a frame in which nothing moved
    g1 = MH.frame_of(45, 37, MH.STILL_CAMERA, 1, seed=5, xforms=start)
    back = run(driver, [f0, MH.with_moves(g1, [(1, [B]), (1, [start[1]])])], start, tag="back", flags=BOTH)
    never = run(driver, [f0, g1], start, tag="never", flags=BOTH)
    assert not back[1]["table"] and not never[1]["table"]
    for what in ("image", "record", "motion"):
        assert np.array_equal(MH.bits(back[1][what]), MH.bits(never[1][what])), what
    assert (never[1]["record"][..., 3][g1.depth >= 0] == f0.m + g1.m).all()
    # a drop forgets the snapshot: after it the frame is a first frame, whatever moved before
    dropped = run(driver, [f0, MH.with_moves(f1, f1.moves, drop=True)], start, tag="dropped", flags=BOTH)
    assert not dropped[1]["table"] and (dropped[1]["record"][..., 3][f1.depth >= 0] == f1.m).all() and not dropped[1]["motion"].any()


def test_the_driver_is_clean_under_address_and_undefined_behaviour_sanitizers(sequences, host_results, tmp_path):
    """Host code in a stand-alone program, on the 7 x 5 sequences (and a singular matrix, and two moves before a call); the bits are the plain build's."""
    exe = MH.compile_driver(str(tmp_path / "motion_driver_san"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    for cam in (False, True):
        frames, start = sequences[((7, 5), cam)]
        for fl in FLAG_SETS:
            got = MH.run_sequence(exe, tmp_path, frames, start, tag="san", flags=fl)
            for g, want in zip(got, host_results[((7, 5), cam, fl)]):
                for what in ("image", "record", "motion"):
                    assert np.array_equal(MH.bits(g[what]), MH.bits(want[what])), (cam, fl, what)
    frames, start = sequences[((7, 5), False)]
    bad = np.zeros((4, 4), F32)
    got = MH.run_sequence(exe, tmp_path, [frames[0], MH.with_moves(frames[1], [(1, [bad]), (0, [start[0], bad, start[2]])])], start, tag="san_singular", flags=3, variance=1)
    assert list(got[1]["state"]) == [0, 2, 0]
