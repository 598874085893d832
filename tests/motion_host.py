"""What the tests of the temporal history across instance moves share: the host compile of csrc/temporal.hpp's temporal_pixel_motion
(tests/tools/motion_driver.cpp) built and run on a sequence of frames with instance moves between them, and an analytic scene whose planes belong to three
instances and take a matrix per step.  Not a test module."""
import os
import struct
import subprocess

import numpy as np

import ref_temporal64 as R64
import temporal_host as TH
from refit_moves import about, rotate, scale, translate

ROOT = TH.ROOT
F32 = np.float32
DEFAULTS = dict(TH.DEFAULTS, variance=0, min_history=4)
STILL, MOVED, NO_HISTORY = 0, 1, 2


def compile_driver(exe, extra=()):
    """(the flags of temporal_host.compile_driver)"""
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math", "-march=x86-64-v3"] + list(extra) +
                          ["-I" + TH.CSRC, os.path.join(ROOT, "tests", "tools", "motion_driver.cpp"), "-o", exe])
    return exe


class Frame(TH.Frame):
    """temporal_host.Frame and the vpt_set_instance_transforms calls made before this temporal call: moves = [(first, [matrix, ...])], math matrices
    (row, column) of float32 values."""
    def __init__(self, view_inv, proj_inv, m, radiance, normal, albedo, depth, inst, drop=False, moves=()):
        TH.Frame.__init__(self, view_inv, proj_inv, m, radiance, normal, albedo, depth, inst, drop)
        self.moves = [(int(first), [np.asarray(x, F32) for x in mats]) for first, mats in moves]


def with_moves(frame, moves=(), drop=None):
    """A temporal_host.Frame (or a Frame) with these moves before it."""
    return Frame(frame.view_inv, frame.proj_inv, frame.m, frame.radiance, frame.normal, frame.albedo, frame.depth, frame.inst, frame.drop if drop is None else drop, moves)


def run_sequence(exe, workdir, frames, start, tag="m", withhold=False, **params):
    """start: the instances' matrices before the first frame, [n, 4, 4].  -> per frame a dict: image, record [h, w, 4], moments [h, w, 2], variance [h, w],
    motion [h, w, 2], table (bool: a table was built), state uint32 [n] — what vpt_temporal_accumulate computes with instance_motion = 1, call after call,
    on the host.  withhold: the table is built but the pixels do not get it."""
    p = dict(DEFAULTS, **params)
    h, w = frames[0].depth.shape
    start = np.ascontiguousarray(start, F32)
    n_inst = len(start)
    src, dst = os.path.join(str(workdir), tag + ".in"), os.path.join(str(workdir), tag + ".out")
    with open(src, "wb") as f:
        f.write(struct.pack("<9I4f", w, h, len(frames), p["flags"], p["max_history"], p["variance"], p["min_history"], n_inst, 1 if withhold else 0,
                            p["depth_tolerance"], p["normal_threshold"], p["focus_distance"], p["dof_strength"]))
        f.write(np.ascontiguousarray(start.transpose(0, 2, 1)).tobytes())              # column-major
        for fr in frames:
            assert fr.radiance.shape == fr.normal.shape == fr.albedo.shape == (h, w, 4) and fr.depth.shape == fr.inst.shape == (h, w)
            f.write(fr.view_inv.T.tobytes()); f.write(fr.proj_inv.T.tobytes())
            moves = getattr(fr, "moves", [])
            f.write(struct.pack("<fII", fr.m, 1 if fr.drop else 0, len(moves)))
            for first, mats in moves:
                f.write(struct.pack("<II", first, len(mats)))
                for x in mats:
                    f.write(np.ascontiguousarray(np.asarray(x, F32).T).tobytes())
            for a in (fr.radiance, fr.normal, fr.albedo, fr.depth, fr.inst):
                f.write(a.tobytes())
    subprocess.check_call([exe, src, dst])
    raw = np.fromfile(dst, "<u4")
    n = h * w
    per = n * (4 + 4 + 2 + 1 + 2) + 1 + n_inst
    assert raw.size == per * len(frames)
    out = []
    for k in range(len(frames)):
        a = raw[k * per:(k + 1) * per]
        fl = a[:13 * n].view(F32)
        out.append(dict(image=fl[:4 * n].reshape(h, w, 4), record=fl[4 * n:8 * n].reshape(h, w, 4), moments=fl[8 * n:10 * n].reshape(h, w, 2),
                        variance=fl[10 * n:11 * n].reshape(h, w), motion=fl[11 * n:13 * n].reshape(h, w, 2), table=bool(a[13 * n]), state=a[13 * n + 1:].copy()))
    return out


def matrices_after(start, frames):
    """The instances' matrices at every frame: [frames][n, 4, 4] float32."""
    cur = np.array(start, F32)
    out = []
    for fr in frames:
        for first, mats in getattr(fr, "moves", []):
            for j, x in enumerate(mats):
                cur[first + j] = x
        out.append(cur.copy())
    return out


# ---- the analytic scene: instance 0 is the room (a back wall and a floor, never moved by the tests' visible moves), instance 1 a rectangle floating in front
# of the wall, instance 2 a panel standing at 45 degrees to the wall on the left.  Every plane is given in its instance's OBJECT space and placed by the
# instance's matrix; anything else is a miss.
# (unit normal, a point, what of the plane belongs to the surface) in object space
OBJECTS = {
    0: [((0.0, 0.0, 1.0), (0.0, 0.0, -5.0), lambda P: (np.abs(P[..., 0]) <= 40.0) & (P[..., 1] >= -1.0) & (P[..., 1] <= 2.2)),
        ((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), lambda P: (np.abs(P[..., 0]) <= 40.0) & (P[..., 2] >= -5.0) & (P[..., 2] <= 1.5))],
    1: [((0.0, 0.0, 1.0), (0.0, 0.0, 0.0), lambda P: (np.abs(P[..., 0]) <= 0.8) & (np.abs(P[..., 1]) <= 0.6))],
    2: [((0.0, 0.0, 1.0), (0.0, 0.0, 0.0), lambda P: (np.abs(P[..., 0]) <= 0.7) & (np.abs(P[..., 1]) <= 0.7))],
}
RECT_CENTRE, PANEL_CENTRE = (0.1, 0.3, -3.5), (-1.5, 0.2, -4.0)
START = np.stack([np.eye(4), translate(*RECT_CENTRE), translate(*PANEL_CENTRE) @ rotate((0.0, 1.0, 0.0), 45.0)]).astype(F32)


def trace(view_inv, proj_inv, w, h, xforms):
    """Depth (float64 ray / plane intersection along the CENTER ray, rounded to float32; -1 on a miss), normal [h, w, 4], instance id."""
    o, d = R64.camera_rays(view_inv, proj_inv, w, h)
    best = np.full((h, w), np.inf)
    normal = np.zeros((h, w, 4), F32)
    inst = np.full((h, w), 0xffffffff, np.uint32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for ident, planes in OBJECTS.items():
            M = np.asarray(xforms[ident], np.float64)
            Mi = np.linalg.inv(M)
            for nrm, p0, inside in planes:
                nw = Mi[:3, :3].T @ np.asarray(nrm, np.float64)       # normals go with the inverse transpose
                nw /= np.linalg.norm(nw)
                pw = M[:3, :3] @ np.asarray(p0, np.float64) + M[:3, 3]
                t = ((pw - o) @ nw) / (d @ nw)
                X = o + t[..., None] * d
                P = np.nan_to_num(X) @ Mi[:3, :3].T + Mi[:3, 3]
                ok = np.isfinite(t) & (t > 0.01) & (t < best) & inside(P)
                best = np.where(ok, t, best)
                normal[ok, :3] = np.where((d[ok] @ nw)[:, None] < 0, nw, -nw)     # facing the camera, as a shading normal does
                inst[ok] = ident
    return np.where(np.isfinite(best), best, -1.0).astype(F32), normal, inst


def frame_of(w, h, camera, m, seed, xforms, moves=(), drop=False, tan_half_y=0.57735):
    """temporal_host.analytic_frame's colours and albedo (random; alpha 1; misses as k_first_hit writes them) over this scene under these matrices."""
    view_inv, proj_inv = TH.look_at_inverse(*camera), TH.projection_inverse(w / h, tan_half_y)
    depth, normal, inst = trace(view_inv, proj_inv, w, h, xforms)
    rng = np.random.default_rng(seed)
    hit = depth >= 0
    albedo = rng.uniform(0.25, 1.0, (h, w, 4)).astype(F32)
    albedo[~hit] = 0.0
    colour = np.ones((h, w, 4), F32)
    colour[..., :3] = rng.uniform(0.0, 1.0, (h, w, 3)).astype(F32) * np.maximum(albedo[..., :3], F32(1e-3))
    colour[~hit, :3] = rng.uniform(0.0, 1.0, (int((~hit).sum()), 3)).astype(F32)
    return Frame(view_inv, proj_inv, m, colour, normal, albedo, depth, inst, drop, moves)


# world transforms applied to an instance's current matrix, step after step: the rectangle translated; rotated in its plane and out of it; scaled non-uniformly
# about its centre; and the panel scaled along z about its centre — under which its normal turns, and turns the other way than its tangents
RECT_STEPS = [translate(0.95, 0.4, 0.1),
              lambda c: about(c, rotate((0.0, 0.0, 1.0), 7.0) @ rotate((0.0, 1.0, 0.0), 9.0)),
              lambda c: about(c, scale(1.25, 0.8, 1.0))]
PANEL_SQUASH = about(PANEL_CENTRE, scale(1.0, 1.0, 1.0 / 3.0))
STILL_CAMERA = TH.CAMERAS[0]
M_OF_STEP = (2, 1, 3, 2)


def sequence(w, h, moving_camera, squash_panel_at=None):
    """Four frames: the start, then the three RECT_STEPS of the rectangle, one per step (the panel squashed too at step `squash_panel_at`); under one camera
    or under temporal_host's cameras of this size.  -> (frames, START)."""
    tan_half_y, cams = TH.SETUPS.get((w, h), (0.57735, TH.CAMERAS))
    cur = START.astype(np.float64)
    centre = np.asarray(RECT_CENTRE, np.float64)
    frames = []
    for k in range(4):
        moves = []
        if k > 0:
            step = RECT_STEPS[k - 1]
            W = step(centre) if callable(step) else step
            cur[1] = (W @ cur[1]).astype(F32)
            centre = cur[1][:3, 3].copy()
            moves.append((1, [cur[1].astype(F32)]))
            if squash_panel_at == k:
                cur[2] = (PANEL_SQUASH @ cur[2]).astype(F32)
                moves.append((2, [cur[2].astype(F32)]))
        cam = cams[k] if moving_camera else cams[0]
        frames.append(frame_of(w, h, cam, M_OF_STEP[k], seed=7000 * w + 30 * h + k + (500 if moving_camera else 0), xforms=cur.astype(F32), moves=moves, tan_half_y=tan_half_y))
    return frames, START


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)
