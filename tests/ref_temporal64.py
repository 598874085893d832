"""vpt_temporal_accumulate restated in float64 numpy, from the description in include/vpt.h and the head of csrc/temporal.hpp and not from its code:
reproject the previous result through the first hit of the current frame, keep it where the same surface is still seen, blend the new samples in.
Vectorised over pixels, one tap at a time; divisions where the description has divisions.  Besides image and length it reports, per pixel, how many taps
counted and how close any of its decisions was to going the other way — tests/test_temporal_cpu.py leaves out the pixels where THIS restatement is marginal.
Matrices are math matrices (row, column), float32 values as the library stores them."""
import numpy as np

DEMODULATE, MATCH_INSTANCE = 1, 2
MIN_WEIGHT = 0.01


def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def camera_rays(view_inv, proj_inv, w, h):
    """The CENTER ray of every pixel: origin [3], unit directions [h, w, 3]."""
    vi, pi = np.asarray(view_inv, np.float64), np.asarray(proj_inv, np.float64)
    y, x = np.mgrid[0:h, 0:w]
    dx, dy = (x + 0.5) / w * 2.0 - 1.0, (y + 0.5) / h * 2.0 - 1.0
    tg = np.stack([dx, dy, np.ones_like(dx), np.ones_like(dx)], -1) @ pi.T
    tn = _unit(tg[..., :3])
    d = _unit(tn @ vi[:3, :3].T)
    return vi[:3, 3].copy(), d


def prev_clip(view_inv, proj_inv):
    """projection * view of a camera given by its two inverses, rounded to float32 as the description has it; None: singular."""
    try:
        m = np.linalg.inv(np.asarray(proj_inv, np.float64)) @ np.linalg.inv(np.asarray(view_inv, np.float64))
    except np.linalg.LinAlgError:
        return None
    return m.astype(np.float32).astype(np.float64) if np.isfinite(m).all() else None


class State:
    """What one call leaves for the next: history (e.rgb), length, normal, depth, instance, and the camera."""
    def __init__(self, e, length, normal, depth, inst, view_inv, proj_inv):
        self.e, self.length, self.normal, self.depth, self.inst, self.view_inv, self.proj_inv = e, length, normal, depth, inst, view_inv, proj_inv


def temporal64(prev, view_inv, proj_inv, m, cur, normal, albedo, depth, inst, max_history, depth_tolerance, normal_threshold, flags):
    """prev: State or None.  cur, normal, albedo [h, w, 4]; depth [h, w] (t, < 0 on a miss); inst [h, w].
    -> image float64 [h, w, 4], length [h, w], the next State, info dict (counted [h, w] int, inside_hit [h, w] int, marginal [h, w] bool,
    mixed [h, w] bool: some inside hit tap has another instance id than the pixel, behind / behind_would_tap [h, w] bool, dots [4, h, w])."""
    c = np.asarray(cur, np.float64)
    n = np.asarray(normal, np.float64)[..., :3]
    t = np.asarray(depth, np.float64)
    inst = np.asarray(inst)
    h, w = t.shape
    hit = t >= 0
    scale = np.maximum(np.asarray(albedo, np.float64)[..., :3], 1e-3) if flags & DEMODULATE else np.ones((h, w, 3))
    e_cur = c[..., :3] / scale
    sw = np.zeros((h, w)); sc = np.zeros((h, w, 3)); sl = np.zeros((h, w))
    counted = np.zeros((h, w), int); inside_hit = np.zeros((h, w), int)
    marginal = np.zeros((h, w), bool); mixed = np.zeros((h, w), bool)
    behind = np.zeros((h, w), bool); behind_would_tap = np.zeros((h, w), bool)
    dots = np.full((4, h, w), np.nan)      # n_p . n_q of every inside hit tap
    clip_m = prev_clip(prev.view_inv, prev.proj_inv) if prev is not None else None
    if clip_m is not None:
        o, d = camera_rays(view_inv, proj_inv, w, h)
        X = o + np.where(hit, t, 1.0)[..., None] * d
        clip = np.concatenate([X, np.ones((h, w, 1))], -1) @ clip_m.T
        front = hit & (clip[..., 3] > 0)
        cw = np.where(front, clip[..., 3], 1.0)
        fx = ((clip[..., 0] / cw + 1.0) * 0.5) * w - 0.5
        fy = ((clip[..., 1] / cw + 1.0) * 0.5) * h - 0.5
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0, fy - y0
        near_integer = (np.minimum(ax, 1.0 - ax) < 1e-3) | (np.minimum(ay, 1.0 - ay) < 1e-3)
        o_prev = np.asarray(prev.view_inv, np.float64)[:3, 3]
        te = np.sqrt(((X - o_prev) ** 2).sum(-1))
        # (for the tests only: where a point BEHIND the previous camera would land if the sign of clip.w were not looked at — the division mirrors it through
        # the image centre — and whether a hit pixel of the previous image lies there)
        behind = hit & (clip[..., 3] < 0)
        bw = np.where(behind, clip[..., 3], -1.0)
        mx, my = np.floor(((clip[..., 0] / bw + 1.0) * 0.5) * w - 0.5), np.floor(((clip[..., 1] / bw + 1.0) * 0.5) * h - 0.5)
        for (i, j) in ((0, 0), (1, 0), (0, 1), (1, 1)):
            ins = behind & (mx + i >= 0) & (mx + i < w) & (my + j >= 0) & (my + j < h)
            behind_would_tap |= ins & (prev.depth[np.where(ins, my + j, 0).astype(int), np.where(ins, mx + i, 0).astype(int)] >= 0)
        for tap, (i, j) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
            qx, qy = x0 + i, y0 + j
            inside = front & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            ix, iy = np.where(inside, qx, 0).astype(int), np.where(inside, qy, 0).astype(int)
            tq, nq, iq = prev.depth[iy, ix], prev.normal[iy, ix], prev.inst[iy, ix]
            cand = inside & (tq >= 0)
            resid = np.abs(tq - te) / te
            nd = (n * nq).sum(-1)
            dots[tap] = np.where(cand, nd, np.nan)
            ok = cand & (resid <= depth_tolerance) & (nd >= normal_threshold)
            if flags & MATCH_INSTANCE:
                ok &= iq == inst
            b = (ax if i else 1.0 - ax) * (ay if j else 1.0 - ay)
            sw += np.where(ok, b, 0.0)
            sc += np.where(ok[..., None], b[..., None] * prev.e[iy, ix], 0.0)   # (a tap that does not count is left out, not multiplied by 0)
            sl += np.where(ok, b * prev.length[iy, ix], 0.0)
            counted += ok; inside_hit += cand
            marginal |= cand & ((np.abs(resid - depth_tolerance) < 1e-4) | (np.abs(nd - normal_threshold) < 1e-4))
            mixed |= cand & (iq != inst)
        marginal |= front & near_integer
    has = hit & (sw > MIN_WEIGHT)
    swd = np.where(has, sw, 1.0)
    hist, nlen = sc / swd[..., None], sl / swd
    n_new = np.minimum(nlen + m, float(max_history))
    a = np.minimum(m / n_new, 1.0)
    e = np.where(has[..., None], hist + (e_cur - hist) * a[..., None], e_cur)
    length = np.where(hit, np.where(has, n_new, min(float(m), float(max_history))), 0.0)
    image = c.copy()
    image[..., :3] = np.where(hit[..., None], e * scale, c[..., :3])
    state = State(np.where(hit[..., None], e, 0.0), length, n, t, inst, view_inv, proj_inv)
    return image, length, state, {"counted": counted, "inside_hit": inside_hit, "marginal": marginal & hit, "mixed": mixed & hit, "has": has,
                                  "behind": behind, "behind_would_tap": behind_would_tap, "dots": dots}
