"""vpt_temporal_accumulate with vpt_temporal_options.instance_motion = 1 restated in float64 numpy, from the rule in include/vpt.h and not from the code:
the previous transform of an instance is the matrix it had when the previous record was made; D = M_prev M_cur^-1 and nt = the inverse transpose of D's upper
3 x 3, both formed in float64 and rounded to float32 once; a hit pixel of a moved instance is reprojected from Xp = D (X, 1) — in the clip transform and in the
depth |Xp - o_prev| — and tested with the normal normalize(nt n_p); an instance whose matrices are equal byte for byte is left as it is, and one whose M_cur or
D is singular or not finite has no history.  Everything else is ref_temporal64's: the same taps, weights, blend.  Vectorised over pixels, one tap at a time.
Besides image and length it reports the motion image and, per pixel, how close any of its decisions was to going the other way: `marginal` is a tap test (depth,
normal, the least weight) within 1e-4 of its threshold.  A reprojected position within 1e-3 of a pixel centre is NOT marginal — under a still camera every pixel
that did not move is one: rounding moves a tap of weight below 1e-5 in or out, which changes the result continuously, by that weight — but it is reported as
`near_integer` for the tests that count taps."""
import numpy as np

import ref_temporal64 as R64

DEMODULATE, MATCH_INSTANCE = R64.DEMODULATE, R64.MATCH_INSTANCE
MIN_WEIGHT = R64.MIN_WEIGHT
STILL, MOVED, NO_HISTORY = 0, 1, 2


def instance_motion(prev_xform, cur_xform):
    """-> (state, D [4, 4], nt [3, 3]) of one instance; math matrices (row, column) of float32 values."""
    a, b = np.asarray(prev_xform, np.float32), np.asarray(cur_xform, np.float32)
    if a.tobytes() == b.tobytes():
        return STILL, np.eye(4), np.eye(3)
    with np.errstate(all="ignore"):
        try:
            if not np.isfinite(b).all() or abs(np.linalg.det(b.astype(np.float64))) == 0.0:
                return NO_HISTORY, None, None
            D = a.astype(np.float64) @ np.linalg.inv(b.astype(np.float64))
            if not np.isfinite(D).all() or abs(np.linalg.det(D[:3, :3])) == 0.0:
                return NO_HISTORY, None, None
            nt = np.linalg.inv(D[:3, :3]).T
        except np.linalg.LinAlgError:
            return NO_HISTORY, None, None
        D32, nt32 = D.astype(np.float32), nt.astype(np.float32)
    if not (np.isfinite(D32).all() and np.isfinite(nt32).all()):
        return NO_HISTORY, None, None
    return MOVED, D32.astype(np.float64), nt32.astype(np.float64)


def temporal64(prev, prev_xforms, cur_xforms, view_inv, proj_inv, m, cur, normal, albedo, depth, inst, max_history, depth_tolerance, normal_threshold, flags,
               normal_rule="nt"):
    """prev: ref_temporal64.State or None; prev_xforms / cur_xforms [n, 4, 4]: the matrices at the previous record and now (None: no instance moved).
    normal_rule "linear" (for a test alone): the normal goes through D's own linear part, as a tangent would.
    -> image float64 [h, w, 4], length [h, w], the next State, info dict (ref_temporal64's counted, inside_hit, marginal, has; motion [h, w, 2];
    reprojected [h, w] bool: fx, fy were computed; state [n])."""
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
    marginal = np.zeros((h, w), bool); near = np.zeros((h, w), bool)
    motion = np.zeros((h, w, 2)); reprojected = np.zeros((h, w), bool)
    n_inst = 0 if cur_xforms is None else len(cur_xforms)
    state = np.zeros(n_inst, int)
    clip_m = R64.prev_clip(prev.view_inv, prev.proj_inv) if prev is not None else None
    if clip_m is not None:
        o, d = R64.camera_rays(view_inv, proj_inv, w, h)
        X = o + np.where(hit, t, 1.0)[..., None] * d
        n_test = n.copy()
        alive = hit.copy()
        for i in range(n_inst):
            state[i], D, nt = instance_motion(prev_xforms[i], cur_xforms[i])
            mine = hit & (inst == i)
            if state[i] == NO_HISTORY:
                alive &= ~mine
            elif state[i] == MOVED:
                X = np.where(mine[..., None], X @ D[:3, :3].T + D[:3, 3], X)
                turned = n @ (nt if normal_rule == "nt" else D[:3, :3]).T
                norm = np.sqrt((turned * turned).sum(-1, keepdims=True))
                n_test = np.where(mine[..., None], turned / np.where(mine[..., None], norm, 1.0), n_test)
        clip = np.concatenate([X, np.ones((h, w, 1))], -1) @ clip_m.T
        front = alive & (clip[..., 3] > 0)
        cw = np.where(front, clip[..., 3], 1.0)
        fx = ((clip[..., 0] / cw + 1.0) * 0.5) * w - 0.5
        fy = ((clip[..., 1] / cw + 1.0) * 0.5) * h - 0.5
        yy, xx = np.mgrid[0:h, 0:w]
        motion = np.where(front[..., None], np.stack([fx - xx, fy - yy], -1), 0.0)
        reprojected = front
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0, fy - y0
        near_integer = (np.minimum(ax, 1.0 - ax) < 1e-3) | (np.minimum(ay, 1.0 - ay) < 1e-3)
        o_prev = np.asarray(prev.view_inv, np.float64)[:3, 3]
        te = np.sqrt(((X - o_prev) ** 2).sum(-1))
        for (i, j) in ((0, 0), (1, 0), (0, 1), (1, 1)):
            qx, qy = x0 + i, y0 + j
            inside = front & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            ix, iy = np.where(inside, qx, 0).astype(int), np.where(inside, qy, 0).astype(int)
            tq, nq, iq = prev.depth[iy, ix], prev.normal[iy, ix], prev.inst[iy, ix]
            cand = inside & (tq >= 0)
            resid = np.abs(tq - te) / te
            nd = (n_test * nq).sum(-1)
            ok = cand & (resid <= depth_tolerance) & (nd >= normal_threshold)
            if flags & MATCH_INSTANCE:
                ok &= iq == inst
            b = (ax if i else 1.0 - ax) * (ay if j else 1.0 - ay)
            sw += np.where(ok, b, 0.0)
            sc += np.where(ok[..., None], b[..., None] * prev.e[iy, ix], 0.0)
            sl += np.where(ok, b * prev.length[iy, ix], 0.0)
            counted += ok; inside_hit += cand
            marginal |= cand & ((np.abs(resid - depth_tolerance) < 1e-4) | (np.abs(nd - normal_threshold) < 1e-4))
        near = front & near_integer
    has = hit & (sw > MIN_WEIGHT)
    marginal |= hit & (np.abs(sw - MIN_WEIGHT) < 1e-4)
    swd = np.where(has, sw, 1.0)
    hist, nlen = sc / swd[..., None], sl / swd
    n_new = np.minimum(nlen + m, float(max_history))
    a = np.minimum(m / n_new, 1.0)
    e = np.where(has[..., None], hist + (e_cur - hist) * a[..., None], e_cur)
    length = np.where(hit, np.where(has, n_new, min(float(m), float(max_history))), 0.0)
    image = c.copy()
    image[..., :3] = np.where(hit[..., None], e * scale, c[..., :3])
    nxt = R64.State(np.where(hit[..., None], e, 0.0), length, n, t, inst, view_inv, proj_inv)
    return image, length, nxt, {"counted": counted, "inside_hit": inside_hit, "marginal": marginal & hit, "has": has, "motion": motion, "reprojected": reprojected,
                                "state": state, "near_integer": near & hit}
