"""Scenes that exercise the texture slots and instance transforms no shipped fixture uses: per-hit and 1x1 non-default normal maps,
emissive textures on lights (per-hit, strip, 1x1 coloured, 1x1 black), and affine instances (non-uniform scale, shear, mirroring).
Built from the Cornell box with the glass sphere (tests/golden/cornell_box_glass.npz) plus a procedural box mesh.  A plain helper
module for tests/test_oracle_material_textures_fp64.py and tests/test_gpu_material_textures.py.

Every builder returns (scene, info): `info` names the instances and textures each variant is meant to exercise, so a test can assert
its own preconditions (which textures are 1x1, which transforms are mirrored or non-uniformly scaled) from the scene it renders."""
import copy
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VARIANTS = ("normal_map", "emissive_texture", "affine_instances", "combined")


def rot(axis, deg):
    """4x4 rotation about x / y / z by `deg` degrees."""
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]
    m = np.eye(4)
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def scale(x, y, z):
    return np.diag([x, y, z, 1.0])


def translate(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def xf(*ms):
    """The product of the matrices, as the float32 instance transform."""
    r = np.eye(4)
    for m in ms:
        r = r @ m
    return r.astype(np.float32)


def box_mesh(sc, uv_lo=-0.4, uv_hi=1.6):
    """The cube [-1, 1]^3: 24 vertices (flat faces), outward normals, winding with cross(p2 - p1, p3 - p1) outward, and uvs from uv_lo
    to uv_hi on every face (outside [0, 1] on both sides: REPEAT addressing)."""
    pos, nrm, uvs, idx = [], [], [], []
    for ax in range(3):
        for sgn in (-1.0, 1.0):
            n = np.zeros(3); n[ax] = sgn
            a, b = (ax + 1) % 3, (ax + 2) % 3
            base = len(pos)
            for (s, t) in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = np.zeros(3); p[ax] = sgn; p[a] = s; p[b] = t
                pos.append(p); nrm.append(n)
                uvs.append((uv_lo + (s + 1) * 0.5 * (uv_hi - uv_lo), uv_lo + (t + 1) * 0.5 * (uv_hi - uv_lo)))
            # e_a x e_b = +e_ax, so (0, 1, 2) winds outward on the + face
            idx += [base, base + 1, base + 2, base, base + 2, base + 3] if sgn > 0 else [base, base + 2, base + 1, base, base + 3, base + 2]
    return sc.add_mesh(np.array(pos, np.float32), np.array(nrm, np.float32), np.array(uvs, np.float32), np.array(idx, np.uint32))


def quad_mesh(sc, half, uvs):
    """A quad in the xz plane facing +y (down, in the reference's Y-down world), corner uvs as given."""
    p = np.array([[-half, 0, -half], [half, 0, -half], [half, 0, half], [-half, 0, half]], np.float32)
    n = np.tile(np.array([0, 1, 0], np.float32), (4, 1))
    # cross(p2 - p1, p3 - p1) = +y for (0, 2, 1)
    return sc.add_mesh(p, n, np.array(uvs, np.float32), np.array([0, 2, 1, 0, 3, 2], np.uint32))


def normal_map_texture(w=37, h=23, seed=11):
    """RGBA8 tangent-space normal map, w x h (not powers of two): one smooth bump per period (so the wrap of REPEAT is smooth too), one
    column of texels tilted past 80 degrees (mapped z ~ 0.12) and one row whose mapped z is negative; both corrections of the surface frame
    fire on those.  The walls sample a window round the wrap corner, away from the extreme texels: a path that bounces between surfaces whose
    normal map varies fast in world space is chaotic (each bounce multiplies a float32 rounding of the hit point by 2 t |dN/dx|), and no float32
    implementation could then follow the float64 one sample by sample."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    nx = 0.3 * np.sin(2.0 * np.pi * x / w) * np.cos(2.0 * np.pi * y / h)
    ny = 0.3 * np.sin(2.0 * np.pi * y / h + 0.7)
    nz = np.ones_like(nx)
    nx[:, 18] = 1.0; ny[:, 18] = 0.2; nz[:, 18] = 0.12             # ~83 degrees of tilt
    nx[11, :] = -0.6; ny[11, :] = 0.7; nz[11, :] = -0.35           # below the tangent plane
    nz += rng.uniform(-0.02, 0.02, nz.shape)
    v = np.stack([nx, ny, nz], -1)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    t = np.full((h, w, 4), 255, np.uint8)
    t[..., :3] = np.clip(np.round((v * 0.5 + 0.5) * 255.0), 0, 255).astype(np.uint8)
    return t


def panel_texture(w=16, h=9, seed=5):
    """RGBA8 emissive texture of the ceiling light: mid-grey to white texels, a few black ones and one hot (white) texel among dimmer ones."""
    rng = np.random.RandomState(seed)
    t = np.full((h, w, 4), 255, np.uint8)
    t[..., :3] = rng.randint(60, 200, (h, w, 3))
    t[rng.rand(h, w) < 0.2, :3] = 0
    t[4, 11, :3] = 255
    return t


def base_scene():
    from importlib import import_module
    S = import_module("vulkan-path-tracer_amd").scenes
    return S, copy.deepcopy(S.Scene.load(os.path.join(GOLDEN, "cornell_box_glass.npz")))


def wall_uvs(sc, origin, span):
    """Gives the five Cornell walls (meshes 0 .. 4, whose fixtures carry no uvs) uvs on the wall's two long axes: from `origin` to `origin + span`."""
    for mi in range(5):
        v, idx = sc.meshes[mi]
        v = v.copy()
        p = v["position"].astype(np.float64)
        axes = np.argsort(p.max(0) - p.min(0))[1:]
        lo, hi = p.min(0), p.max(0)
        v["texcoord"] = np.array(origin) + np.array(span) * (p[:, axes] - lo[axes]) / (hi[axes] - lo[axes])
        sc.meshes[mi] = (v, idx)


def build(normal_map=False, emissive=False, affine=False, env=False, compact=False):
    """The Cornell box with the glass sphere, two boxes, and whatever the flags add.  -> (scene, info).
    compact: no sphere and one box (mirrored, non-uniformly scaled), so that the BVH is small enough to ride in LDS and the
    whole-path / fused per-bounce kernels serve the scene."""
    S, sc = base_scene()
    info = dict(per_hit_normal=[], normal_1x1=[], mirrored=[], nonuniform=[], sheared=[], z_normal=[], emitters={})
    # u in [-0.12, 0.12], v in [-0.15, 0.15] (negative: REPEAT, a window round the normal map's wrap corner)
    wall_uvs(sc, (-0.12, -0.15), (0.24, 0.3))
    m_box = box_mesh(sc)
    mats = sc.materials
    glass = 4
    box_a = len(mats); mats.append(S.material(base_color=(0.75, 0.75, 0.7), roughness=0.8, name="box_a"))
    box_b = len(mats); mats.append(S.material(base_color=(0.3, 0.5, 0.8), roughness=0.35, metallic=0.7, anisotropy=0.6, anisotropy_rotation=30.0, name="box_b"))
    if compact:
        del sc.instances[6]
        boxes = [(box_b, xf(translate(2.2, 3.6, -6.0), rot("z", 25.0), scale(-0.9, 1.7, 0.6)))]               # mirrored; +-z faces stay exactly +-z
        info["mirrored"] += [6]; info["nonuniform"] += [6]; info["z_normal"] += [6]
    elif not affine:
        # rotation + uniform scale, as in every shipped scene
        boxes = [(box_a, xf(translate(-2.6, 3.9, -7.4), rot("y", 20.0), scale(1.6, 1.6, 1.6))),
                 (box_b, xf(translate(2.7, 4.4, -4.2), rot("y", -35.0), scale(1.1, 1.1, 1.1)))]
    else:
        boxes = [(box_a, xf(translate(-2.6, 3.6, -6.8), rot("z", 25.0), scale(0.9, 1.7, 0.4))),                      # +-z faces stay exactly +-z
                 (box_b, xf(translate(2.6, 3.9, -4.4), rot("y", -35.0), rot("x", 20.0), scale(1.5, 0.6, 1.1))),
                 (box_a, xf(translate(-2.4, -2.6, -8.6), np.array([[1, 0.6, 0, 0], [0, 1, 0.3, 0], [0, 0, 1, 0], [0, 0, 0, 1]]), scale(0.8, 0.9, 0.8))),   # sheared
                 (box_b, xf(translate(3.4, -1.2, -8.8), rot("y", 40.0), scale(-0.8, 1.0, 1.2)))]                        # mirrored
    for mat, m in boxes:
        sc.add_instance(m_box, mat, m)
    if affine and not compact:
        n = len(sc.instances)
        info["z_normal"] += [n - 4]; info["nonuniform"] += [n - 4, n - 3]; info["sheared"] += [n - 2]; info["mirrored"] += [n - 1]
        # the glass sphere: mirrored and non-uniformly scaled (inside flag, refraction)
        sc.instances[6] = (6, glass, xf(translate(0.0, 0.9, -5.8), rot("y", 20.0), scale(-2.2, 1.6, 1.3)))
        info["mirrored"].append(6); info["nonuniform"].append(6)
    if affine:
        # the lamp: rotated, non-uniformly scaled, tilted (the light pdf's world area and the light normal); lowered so it clears the ceiling
        sc.instances[5] = (5, 3, xf(translate(0.0, -5.0, -5.8), rot("y", 30.0), rot("x", 12.0), scale(1.7, 1.0, 0.9)))
        info["nonuniform"].append(5)
    if normal_map:
        tn = sc.add_texture(normal_map_texture())
        t1 = sc.add_texture(np.array([[[200, 90, 180, 255]]], np.uint8))
        flat = 0 if compact else box_a      # (the compact scene has no box_a: the left wall takes the 1x1 map)
        mapped = [k for k in (0, 1, 2, box_b) if k != flat]
        for k in mapped:
            mats[k]["normal_texture"] = tn
        mats[flat]["normal_texture"] = t1
        info["per_hit_normal"] = mapped; info["normal_1x1"] = [flat]
    if emissive:
        # the ceiling light: a 16 x 9 texture over uvs that cover it once
        v, idx = sc.meshes[5]
        v = v.copy()
        p = v["position"].astype(np.float64)
        v["texcoord"] = (p[:, [0, 2]] - p[:, [0, 2]].min(0)) / (p[:, [0, 2]].max(0) - p[:, [0, 2]].min(0))
        sc.meshes[5] = (v, idx)
        mats[3]["emissive_texture"] = sc.add_texture(panel_texture())
        mats[3]["emissive_color"] = (90.0, 90.0, 90.0)
        # a strip lamp on the left wall: 1 x 7, R8 (the emissive slot reads (r, 0, 0, 1)), uvs across the strip
        strip = sc.add_texture(np.array([30, 255, 0, 120, 200, 60, 255], np.uint8).reshape(7, 1))
        m_strip = quad_mesh(sc, 0.8, [(0.3, -0.2), (0.3, 0.9), (0.7, 1.6), (0.7, 0.1)])
        e_strip = len(mats); mats.append(S.material(emissive_color=(60.0, 40.0, 20.0), emissive_texture=strip, name="strip"))
        sc.add_instance(m_strip, e_strip, xf(translate(-5.4, -1.5, -6.5), rot("z", -90.0)))         # faces +x
        # a lamp on the right wall with a 1x1 orange texel (uniform light sampler)
        orange = sc.add_texture(np.array([[[255, 180, 90, 255]]], np.uint8))
        m_lamp = quad_mesh(sc, 0.7, [(0, 0)] * 4)
        e_orange = len(mats); mats.append(S.material(emissive_color=(40.0, 40.0, 40.0), emissive_texture=orange, name="orange"))
        sc.add_instance(m_lamp, e_orange, xf(translate(5.5, 0.5, -7.0), rot("z", 90.0)))           # faces -x
        # emissive_color set, texel black: in the emissive-mesh list, never a light when hit
        black = sc.add_texture(np.array([[[0, 0, 0, 255]]], np.uint8))
        e_black = len(mats); mats.append(S.material(base_color=(0.6, 0.6, 0.6), emissive_color=(30.0, 30.0, 30.0), emissive_texture=black, name="black_emitter"))
        sc.add_instance(m_lamp, e_black, xf(translate(0.0, -5.4, -9.5)))
        info["emitters"] = dict(textured=3, strip=e_strip, uniform=e_orange, black=e_black)
    if env:
        # the 16 x 8 environment of the fp64 'environment' case: one hot sun texel and a dim gradient
        rng = np.random.RandomState(3)
        e = np.zeros((8, 16, 4), np.float32)
        e[..., :3] = rng.gamma(0.8, 0.4, (8, 16, 3))
        e[2, 5, :3] = (60.0, 50.0, 40.0)
        sc.env = e
    sc.name = "material_scene"
    return sc, info


def variant(name):
    """normal_map | emissive_texture | emissive_texture_environment | affine_instances | combined (all of them under the environment)."""
    return {"normal_map": lambda: build(normal_map=True),
            "emissive_texture": lambda: build(emissive=True),
            "emissive_texture_environment": lambda: build(emissive=True, env=True),
            "affine_instances": lambda: build(affine=True),
            "combined": lambda: build(normal_map=True, emissive=True, affine=True, env=True),
            "compact": lambda: build(normal_map=True, emissive=True, affine=True, compact=True),
            "compact_environment": lambda: build(normal_map=True, emissive=True, affine=True, env=True, compact=True)}[name]()


def check_preconditions(sc, info):
    """What the variant is meant to exercise, asserted from the scene itself (the device has no per-path counters of these)."""
    one = lambda t: sc.textures[t].shape[:2] == (1, 1)
    for k in info["per_hit_normal"]:
        assert not one(sc.materials[k]["normal_texture"])
    for k in info["normal_1x1"]:
        t = sc.textures[sc.materials[k]["normal_texture"]]
        assert one(sc.materials[k]["normal_texture"]) and tuple(t[0, 0, :3]) != (128, 128, 255)
    if info["per_hit_normal"]:
        assert any(sc.materials[k]["anisotropy"] > 0 and sc.materials[k]["anisotropy_rotation"] != 0 for k in info["per_hit_normal"])
        t = sc.textures[sc.materials[info["per_hit_normal"][0]]["normal_texture"]].astype(np.float64) / 255.0 * 2.0 - 1.0
        assert (t[..., 2] < 0).any() and (t[..., 2] < np.cos(np.radians(80.0))).sum() > (t[..., 2] < 0).sum()
    for inst in info["mirrored"]:
        assert np.linalg.det(sc.instances[inst][2][:3, :3].astype(np.float64)) < 0
    for inst in info["nonuniform"]:
        s = np.linalg.svd(sc.instances[inst][2][:3, :3].astype(np.float64), compute_uv=False)
        assert s.max() / s.min() > 1.3
    for inst in info["sheared"]:
        m = sc.instances[inst][2][:3, :3].astype(np.float64)
        g = m.T @ m
        assert np.abs(g - np.diag(np.diag(g))).max() > 0.1            # columns not orthogonal
    for inst in info["z_normal"]:
        m = sc.instances[inst][2]
        assert m[0, 2] == m[1, 2] == m[2, 0] == m[2, 1] == 0          # the z faces' world normals are exactly +-z
    e = info["emitters"]
    if e:
        shape = lambda k: sc.textures[sc.materials[k]["emissive_texture"]].shape
        assert shape(e["textured"])[:2] != (1, 1) and shape(e["strip"])[1] == 1 and shape(e["strip"])[0] > 1
        assert shape(e["uniform"])[:2] == (1, 1) and tuple(sc.textures[sc.materials[e["uniform"]]["emissive_texture"]][0, 0, :3]) != (255, 255, 255)
        assert any(sc.materials[e["black"]]["emissive_color"]) and not sc.textures[sc.materials[e["black"]]["emissive_texture"]][0, 0, :3].any()
