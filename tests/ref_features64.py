"""float64 restatement of what vpt_render_features writes at a first hit: the camera ray through a pixel centre (RayGen.slang:35-50 with both
jitter draws 0.5 and no lens offset), SurfaceFrame's normal (Surface.slang:26-147) and Material.Initialize's base colour (Material.slang:44), with
the MARGIN of every branch the chain takes — so that a test can leave out the pixels at which an fp32 evaluation may legitimately take the other
branch.  The scene, its textures and the brute-force closest hit are tests/ref_integrator64.py's Scene64; the surface expressions are those of its
closest_hit, restated here because that function runs on into the BSDF and returns nothing.  Written from the Slang sources, not from the
device code.  Not a test module."""
import numpy as np

from ref_integrator64 import FLAG_FURNACE, FLAG_GEOMETRY_NORMALS, Scene64  # noqa: F401
from test_oracle_bsdf_fp64 import _norm

TMIN, TMAX = 0.01, 100000.0   # RayGen.slang:70's TraceRay range


def center_ray(S, x, y):
    """-> (origin, direction): one_sample's camera ray (ref_integrator64.py) with j0 = j1 = 0 (the draws are 0.5) and a zero lens offset."""
    d2 = np.array([(x + 0.5) / S.W, (y + 0.5) / S.H]) * 2.0 - 1.0
    origin = (S.view_inv @ np.array([0.0, 0.0, 0.0, 1.0]))[:3]
    target = (S.proj_inv @ np.array([d2[0], d2[1], 1.0, 1.0]))[:3]
    direction = (S.view_inv @ np.append(_norm(target), 0.0))[:3]
    return origin, _norm(direction)   # normalize(focus - origin) with focus = origin + direction * f


def tap_margin(S, ti, uv):
    """Distance of a bilinear tap's two weights from a texel edge (0 or 1), in texels: inf for a 1x1 texture (one texel whatever the uv)."""
    h, w = S.textures[ti].shape[:2]
    if h == 1 and w == 1:
        return np.inf
    m = np.inf
    for c, n in ((uv[0], w), (uv[1], h)):
        f = c * n - 0.5
        f -= np.floor(f)
        m = min(m, f, 1.0 - f)
    return m


def first_hit(S, x, y, flags=0, hit=None):
    """The CENTER ray of pixel (x, y) — and, if given, `hit` = (t, u, v, global triangle id) in place of its float64 closest hit: what the two shader
    functions are handed — -> None on a miss, else a dict: t, u, v, gid, instance, primitive, material, mesh, ng (geometric normal towards the viewer), normal (4: SurfaceFrame N | inside), albedo (4: base colour | transmission), margin (the smallest distance of any branch predicate
    from flipping: dot(Ng, view), dot(N, view), dot(reflect, Ng), |N.z| against 0.9999999, the tap weights of the normal and base-colour textures)."""
    o, rd = center_ray(S, x, y)
    hit = S.closest(o, rd, TMIN, TMAX) if hit is None else hit
    if hit is None:
        return None
    t, hu, hv, gid = hit
    inst_id, prim = S.ids[gid]
    mesh, mat_id, M, Minv = S.inst[inst_id]
    vert, idx = S.meshes[mesh]
    i1, i2, i3 = (int(k) for k in idx.reshape(-1, 3)[prim])
    P1, P2, P3 = (vert["position"][k].astype(np.float64) for k in (i1, i2, i3))
    N1, N2, N3 = (vert["normal"][k].astype(np.float64) for k in (i1, i2, i3))
    b = np.array([1.0 - hu - hv, hu, hv])
    uv = sum(vert["texcoord"][k].astype(np.float64) * w_ for k, w_ in zip((i1, i2, i3), b))
    md = S.materials[mat_id]
    margins = []
    # ---- Surface.Initialize
    Ng = _norm(np.cross(P2 - P1, P3 - P1)); Ng = _norm(Ng @ Minv)
    geo = bool(flags & FLAG_GEOMETRY_NORMALS)
    N = Ng.copy() if geo else _norm(_norm(N1 * b[0] + N2 * b[1] + N3 * b[2]) @ Minv)
    view = -rd
    margins.append(abs(np.dot(Ng, view)))
    inside = bool(np.dot(Ng, view) < 0.0)
    if inside:
        N, Ng = -N, -Ng
    margins.append(abs(abs(N[2]) - 0.9999999))
    up = np.array([0.0, 0.0, 1.0]) if abs(N[2]) < 0.9999999 else np.array([1.0, 0.0, 0.0])
    T = _norm(np.cross(up, N)); B = _norm(np.cross(N, T))
    if not geo:
        margins.append(tap_margin(S, md["normal_texture"], uv))
        nm = S.tex(md["normal_texture"], uv)[:3] * 2.0 - 1.0
        N = _norm(nm[0] * T + nm[1] * B + nm[2] * N)
    margins.append(abs(np.dot(N, view)))
    if np.dot(N, view) < 0.0:
        N = _norm(N - view * (np.dot(N, view) - 0.01))
    refl = _norm(-view - 2.0 * np.dot(N, -view) * N)
    margins.append(abs(np.dot(refl, Ng)))
    if np.dot(refl, Ng) < 0.0:
        N = _norm(N + Ng * (0.1 + np.dot(N, Ng)))
    # ---- Material.Initialize: BaseColor (Material.slang:44; FURNACE_TEST_MODE :78-86)
    margins.append(tap_margin(S, md["base_color_texture"], uv))
    base = np.array(md["base_color"], np.float64) * S.tex(md["base_color_texture"], uv)[:3] ** 2.2
    if flags & FLAG_FURNACE:
        base = np.ones(3)
    return dict(t=t, u=hu, v=hv, gid=gid, instance=inst_id, primitive=prim, material=mat_id, mesh=mesh, ng=Ng, origin=o, direction=rd,
                normal=np.append(N, 1.0 if inside else 0.0), albedo=np.append(base, float(md["transmission"])), margin=float(min(margins)))


def image(S, flags=0):
    """first_hit at every pixel -> (hit mask [H, W], normal [H, W, 4], albedo [H, W, 4], margin [H, W], records [H][W])."""
    hit = np.zeros((S.H, S.W), bool)
    normal = np.zeros((S.H, S.W, 4)); albedo = np.zeros((S.H, S.W, 4)); margin = np.full((S.H, S.W), np.inf)
    recs = [[None] * S.W for _ in range(S.H)]
    for y in range(S.H):
        for x in range(S.W):
            r = first_hit(S, x, y, flags)
            recs[y][x] = r
            if r is not None:
                hit[y, x] = True; normal[y, x] = r["normal"]; albedo[y, x] = r["albedo"]; margin[y, x] = r["margin"]
    return hit, normal, albedo, margin, recs
