"""Instance moves shared by tests/test_refit_cpu.py (the refit's arithmetic on the host) and tests/test_gpu_instance_transforms.py
(vpt_set_instance_transforms on the device): world-space transforms, copies of a scene with some instance matrices replaced, a seeded triangle
soup with a few slivers, and the moves both files use.  Not a test module."""
import copy

import numpy as np

F32 = np.float32


def translate(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def scale(x, y, z):
    return np.diag([x, y, z, 1.0])


def rotate(axis, degrees):
    """Rodrigues: a rotation about an arbitrary axis through the origin."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.radians(degrees)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * (k @ k)
    return m


def about(point, m):
    """m applied about `point` instead of the origin."""
    p = np.asarray(point, np.float64)
    return translate(*p) @ m @ translate(*-p)


def moved_matrices(scene, moves):
    """{instance: world transform W} -> {instance: W @ the instance's matrix}, float32 (what vpt_instance.transform takes, in math layout)."""
    return {i: (np.asarray(w, np.float64) @ np.asarray(scene.instances[i][2], np.float64)).astype(F32) for i, w in moves.items()}


def with_matrices(scene, matrices):
    """A copy of the scene (arrays shared, the instance list its own) with these instances' matrices replaced."""
    sc = copy.copy(scene)
    sc.instances = [(me, ma, np.asarray(matrices.get(i, x), F32)) for i, (me, ma, x) in enumerate(scene.instances)]
    return sc


def soup_scene(vpt, seed=11, triangles=300, slivers=5):
    """A seeded soup in three instances: random small triangles in a cube of half width 4, and a few exact slivers (three collinear points, which
    every affine map keeps collinear) that the builder drops."""
    S = vpt.scenes
    rng = np.random.default_rng(seed)
    sc = S.Scene()
    sc.luts = S.load_luts()
    sc.materials.append(S.material(base_color=(0.7, 0.6, 0.5)))
    per = triangles // 3
    for k in range(3):
        c = rng.uniform(-4, 4, (per, 1, 3))
        p = (c + rng.uniform(-0.6, 0.6, (per, 3, 3))).astype(F32)
        n_sl = slivers // 3 + (1 if k < slivers % 3 else 0)
        for j in range(n_sl):          # p1 = p0 + d, p2 = p0 + 2 d with small integers: exact in fp32
            p0 = np.array([j - 1.0, 2.0 * k, 1.0], F32)
            d = np.array([1.0, 0.5, -0.25], F32)
            p[7 * j + 3] = np.stack([p0, p0 + d, p0 + 2 * d])
        pos = p.reshape(-1, 3)
        nrm = np.tile(np.array([0, 0, 1], F32), (len(pos), 1))
        m = sc.add_mesh(pos, nrm, np.zeros((len(pos), 2), F32), np.arange(len(pos), dtype=np.uint32))
        sc.add_instance(m, 0, translate(0.5 * k, -0.25 * k, 0.0))
    return sc


# ---- the moves (world transforms per instance).  In the Cornell scenes instance 5 is the lamp (emissive; the world is y-down: lowering it raises y),
# instances 0-4 are the walls, instance 6 of cornell_box_glass is the glass sphere; in the chain scenes instance 1 is the stack of sheets.
LAMP = 5
CORNELL_WALL = {2: about((0.0, 0.0, -11.5), rotate((0.3, 1.0, 0.1), 9.0)) @ translate(0.4, 0.0, 1.5)}      # the back wall, translated and rotated
CORNELL_LAMP = {LAMP: about((0.0, -5.65, -5.84), scale(1.6, 1.0, 0.7)) @ translate(0.3, 1.2, 0.0)}        # the lamp, lowered and scaled (non-uniform)
GLASS_SPHERE = {6: about((0.0, 0.6, -5.84), rotate((1.0, 2.0, -0.5), 33.0)) @ translate(-0.8, 0.3, 0.6)}  # rotation about an arbitrary axis
GLASS_LAMP_AND_SPHERE = {LAMP: translate(0.5, 0.8, -0.4), 6: about((0.0, 0.6, -5.84), scale(0.8, 1.2, 0.9))}
CHAIN_GROWS = {1: translate(7.5, 0.25, 0.5)}     # carries the stack past the floor's edge (half width 6): the scene's extent, and so the padding, grows
CHAIN_TILT = {1: rotate((1.0, 0.2, 0.0), 12.0), 2: translate(0.0, 0.5, 0.0)}
