"""The ray sets of the traversal tests, seeded and made without a GPU: tests/test_gpu_traversal.py, test_gpu_edge_cases.py and
test_gpu_material_textures.py send them through vpt_trace_rays (k_first_hit), tests/test_gpu_trace_stream.py sends the same rays through the
ray-stream kernels (k_trace_vote, k_trace_shadow) by way of the laboratory's hooks.  Every set has ONE tmin / tmax (vpt_lab_set_rays takes ray 0's).
Rays are float32 [n, 8] = origin, tmin, direction, tmax.  Not a test module."""
import copy
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
WALL = 5.709264755249023     # a wall plane of the Cornell boxes, exactly
WINDOW = (2.0, 9.0)          # tmin beyond near hits, tmax before far hits
SCALES = (1e-3, 1e3, 3.7e4)
FAR = (30.0, 1000.0)


def random_rays(n, seed, scale=12.0):
    rng = np.random.RandomState(seed)
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3] = (rng.rand(n, 3) * 2 - 1) * scale
    d = rng.randn(n, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r[:, 4:7] = d
    r[:, 3] = 1e-4
    r[:, 7] = 1e6
    return r


def axis_aligned_rays():
    """Zero direction components (0 * inf in slab tests), origins on walls, rays along box edges; then the same rays from the exact wall
    coordinate (coplanar rays)."""
    rays = []
    for ax in range(3):
        for sgn in (-1.0, 1.0):
            for ox in np.linspace(-6, 6, 25):
                for oy in np.linspace(-6, 6, 25):
                    o = [ox, oy, -5.8]
                    d = [0.0, 0.0, 0.0]
                    d[ax] = sgn
                    rays.append(o + [1e-4] + d + [1e6])
    rays = np.array(rays, np.float32)
    extra = rays.copy()
    extra[:, 0] = np.float32(WALL)
    return np.concatenate([rays, extra])


def window_rays():
    rays = random_rays(50000, 8, 6.0)
    rays[:, 3] = WINDOW[0]
    rays[:, 7] = WINDOW[1]
    return rays


def scaled(sc, k):
    """The scene with every instance (and the camera's position) scaled by k about the origin."""
    s = copy.deepcopy(sc)
    s.instances = [(m, mat, (np.diag([k, k, k, 1.0]) @ x).astype(np.float32)) for m, mat, x in s.instances]
    cam = s.view_inverse.astype(np.float64).copy(); cam[:3, 3] *= k
    s.view_inverse = cam.astype(np.float32)
    return s


def scaled_rays(k, n=60000):
    """Random rays through a scene of radius ~2 scaled by k, the window scaled with it."""
    rng = np.random.default_rng(3)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = rng.uniform(-2 * k, 2 * k, (n, 3))
    d = rng.normal(size=(n, 3)); rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 3] = 1e-4 * k; rays[:, 7] = 1e6 * k
    return rays


def far_rays(far, n=40000):
    """Origins `far` scene radii (of 2) away, aimed at the scene."""
    rng = np.random.default_rng(11)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    target = rng.uniform(-0.8, 0.8, (n, 3))
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = target - d * far * 2.0
    rays[:, 4:7] = d
    rays[:, 3] = 1e-4; rays[:, 7] = 1e9
    return rays


def affine_rays(sc, info):
    """Random rays, and rays aimed into the mirrored, sheared and non-uniformly scaled instances of material_scenes.variant("affine_instances")."""
    rng = np.random.default_rng(9)
    parts = [random_rays(100000, 13, 8.0)]
    for inst in sorted(set(info["mirrored"] + info["sheared"] + info["nonuniform"])):
        M = sc.instances[inst][2].astype(np.float64)
        v = sc.meshes[sc.instances[inst][0]][0]["position"].astype(np.float64)
        lo, hi = v.min(0), v.max(0)
        n = 20000
        target = rng.uniform(lo, hi, (n, 3)) @ M[:3, :3].T + M[:3, 3]
        origin = rng.uniform(-5.5, 5.5, (n, 3)) + np.array([0.0, 0.0, -5.8])
        d = target - origin
        r = np.zeros((n, 8), np.float32)
        r[:, 0:3] = origin; r[:, 3] = 1e-4; r[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True); r[:, 7] = 1e6
        parts.append(r)
    return np.concatenate(parts)


def chain_rays(n=6000):
    """From the floor of whole_spill_scene.memory_chain_scene towards its light, over the kernels' closest-hit range: searches that go deeper than
    the 14 LDS stack rows (tests/test_stack_bound_cpu.py)."""
    from test_stack_bound_cpu import floor_to_light_rays
    o, d = floor_to_light_rays(np.random.default_rng(21), n)
    return np.concatenate([o, np.full((n, 1), 0.01), d, np.full((n, 1), 100000.0)], axis=1).astype(np.float32)


# ---- how many rays a launch gets (tests/test_gpu_trace_stream.py): a lone ray, around one wave, more than a block, more than one block's waves can start on,
# and one size beyond the static part of the stream kernels' grids, so that their cursor and fetch_chunk run
SCHEDULE_SIZES = (1, 63, 64, 65, 257, 4097)
SHADOW_SIZES = (1, 63, 65, 4097)


def beyond_static(compute_units):
    """2048 * CUs bounds gridDim.x * 256 of a persistent grid at 8 blocks of 256 per CU; half as much again lies beyond it."""
    return 3 * 2048 * compute_units // 2


RAGGED = 77


def beyond_static_sizes(compute_units):
    """The size the static part is left at, and one whose last cursor chunk is cut short by the end of the stream (fetch_chunk's chunks are
    multiples of 64, and so are the first size and the static part)."""
    n = beyond_static(compute_units)
    return n, n + RAGGED


def orders(n, seed=29):
    """Visiting orders of n rays: as they lie, reversed, a seeded permutation."""
    ident = np.arange(n, dtype=np.uint32)
    return {"identity": None, "reversed": ident[::-1].copy(), "permuted": np.random.default_rng(seed).permutation(n).astype(np.uint32)}


# ---- light rays, as the shade stage queues them for k_trace_shadow<light>
LIGHT_SCENES = ("cornell_box_glass", "chain")
SHADOW_WINDOW = {1: (1e-4, 1e6), 0: (1e-5, 1000.0)}   # k_trace_shadow's own window, by ray_queries
HOLE_EVERY = 7


def hole_mask(n):
    """One entry in seven is a hole."""
    return (np.arange(n) % HOLE_EVERY == 3).astype(np.uint8)


def light_scene(vpt, name):
    if name == "chain":
        import whole_spill_scene
        return whole_spill_scene.memory_chain_scene(vpt)
    return vpt.scenes.Scene.load(os.path.join(GOLDEN, name + ".npz"))


def light_rays(vpt, name, n=8190):
    """(rays, expect, media) of n light rays on a scene of LIGHT_SCENES, in triples: ray 3k aims from a random interior origin at a random point of an
    emissive triangle and expects that triangle (global id, the flattened instance-major order); ray 3k + 1 is the same ray expecting the emissive
    triangle next to it; ray 3k + 2 is media-flagged, leaves the same origin and aims, every other time, past the light — into the light's plane
    beside it — still expecting that triangle.  Origins: where part of the rays towards the light meet an occluder (the glass sphere; the stack
    of sheets)."""
    import whole_spill_scene
    sc = light_scene(vpt, name)
    tris = whole_spill_scene.world_triangles(sc)
    ids = tris[:, 9:12].view(np.uint32)
    lamp = [i for i, (_, mat, _) in enumerate(sc.instances) if max(sc.materials[mat]["emissive_color"][:3]) > 0.0]
    em = np.nonzero(np.isin(ids[:, 1], lamp))[0]
    assert len(em) >= 2
    rng = np.random.default_rng(17)
    m = n // 3
    assert n == 3 * m
    if name == "chain":     # between the floor (z = -4.5) and the lowest sheet (z = -1.5), out to the floor's edge: the stack (half width 1) hides part of the light (z = 4, half width 3)
        origin = np.stack([rng.uniform(-5.5, 5.5, m), rng.uniform(-5.5, 5.5, m), rng.uniform(-4.4, -1.6, m)], axis=1)
    else:                   # anywhere in the box below the lamp (the world is y-down: the lamp hangs at y = -5.65), the glass sphere and the blocks between
        origin = np.stack([rng.uniform(-5.0, 5.0, m), rng.uniform(-4.5, 5.3, m), rng.uniform(-11.0, -0.5, m)], axis=1)
    pick = rng.integers(0, len(em), m)
    a, b = rng.random(m), rng.random(m)
    flip = a + b > 1.0
    a[flip], b[flip] = 1.0 - a[flip], 1.0 - b[flip]
    a, b = 0.01 + 0.97 * a, 0.01 + 0.97 * b            # strictly inside the triangle
    t = tris[em[pick]].astype(np.float64)
    target = t[:, 0:3] + a[:, None] * t[:, 3:6] + b[:, None] * t[:, 6:9]
    # beside the light, in its plane: the target pushed away from the lamp's centre, 2.5 to 4 times as far
    centre = (tris[em, 0:3].astype(np.float64) + (tris[em, 3:6] + tris[em, 6:9]) / 3.0).mean(axis=0)
    past = centre + (target - centre) * rng.uniform(2.5, 4.0, (m, 1))
    aim_past = np.arange(m) % 2 == 1
    rays = np.zeros((n, 8), np.float32)
    expect = np.zeros(n, np.uint32)
    media = np.zeros(n, np.uint8)
    for k, tgt in enumerate((target, target, np.where(aim_past[:, None], past, target))):
        d = tgt - origin
        rays[k::3, 0:3] = origin
        rays[k::3, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 3], rays[:, 7] = SHADOW_WINDOW[1]
    gid = ids[em[pick], 2]
    neighbour = ids[em[(pick + 1) % len(em)], 2]
    expect[0::3], expect[1::3], expect[2::3] = gid, neighbour, gid
    media[2::3] = 1
    return rays, expect, media


def light_visible(ref_gid, expect, media):
    """k_trace_shadow<light>'s answer from the brute-force closest hit's global id (-1: nothing hit)."""
    return ((ref_gid == expect.astype(np.int64)) | ((media != 0) & (ref_gid < 0))).astype(np.uint8)


def hit_gid(tris, ref):
    """Global triangle id of each closest hit (-1: a miss), `tris` being Oracle.triangles()."""
    ids = tris[:, 9:12].view(np.uint32).astype(np.int64)
    first = np.full(int(ids[:, 1].max()) + 2, -1, np.int64)
    for inst in np.unique(ids[:, 1]):
        sel = ids[:, 1] == inst
        assert np.array_equal(ids[sel, 2] - ids[sel, 2].min(), ids[sel, 0]), "instance-major ids"
        first[inst] = ids[sel, 2].min()
    hit = ref["t"] >= 0
    inst = np.where(hit, ref["instance"].astype(np.int64), len(first) - 1)
    return np.where(hit, first[inst] + ref["primitive"].astype(np.int64), -1)


# ---- the sets by name: (scene, rays), for the tests that run every one of them
SKY_SETS = ("axis_aligned", "far_30", "far_1000", "scaled_0.001", "scaled_1000", "scaled_37000")   # ... as sky rays through k_trace_shadow
SKY_SETS_NO_RAY_QUERIES = ("axis_aligned", "far_30")   # ... and without ray queries, where the window ends at 1000 on the normalised direction
SETS = ("random_glass", "random_viking", "axis_aligned", "window", "scaled_0.001", "scaled_1000", "scaled_37000", "far_30", "far_1000", "affine", "chain")
_CACHE = {}


def load(vpt, name):
    """(scene, rays) of the set `name`; built once per process."""
    if name in _CACHE:
        return _CACHE[name]
    golden = lambda f: vpt.scenes.Scene.load(os.path.join(GOLDEN, f + ".npz"))
    if name == "random_glass":
        r = golden("cornell_box_glass"), random_rays(200000, 5, 8.0)
    elif name == "random_viking":
        r = golden("viking_room"), random_rays(60000, 5, 2.0)
    elif name == "axis_aligned":
        r = golden("cornell_box_glass"), axis_aligned_rays()
    elif name == "window":
        r = golden("cornell_box_glass"), window_rays()
    elif name.startswith("scaled_"):
        k = float(name[len("scaled_"):])
        r = scaled(golden("viking_room"), k), scaled_rays(k)
    elif name.startswith("far_"):
        r = golden("viking_room"), far_rays(float(name[len("far_"):]))
    elif name == "affine":
        import material_scenes
        sc, info = material_scenes.variant("affine_instances")
        r = sc, affine_rays(sc, info)
    elif name == "chain":
        import whole_spill_scene
        r = whole_spill_scene.memory_chain_scene(vpt), chain_rays()
    else:
        raise KeyError(name)
    assert len(np.unique(r[1][:, 3])) == 1 and len(np.unique(r[1][:, 7])) == 1, "one tmin / tmax per set"
    _CACHE[name] = r
    return r


# ---- the reference: the oracle's brute-force closest hit (no tree on that side at all), once per process and question
_REF = {}


def brute_force(vpt, oracle, sc, rays, strict=False):
    o = oracle.Oracle(sc, 8, 8)
    if strict:   # VPT_FLAG_LOCAL_HITS on the oracle's side, as tests/test_bvh_host.py sets it
        p = vpt.default_params()
        p.flags |= vpt._abi.FLAG_LOCAL_HITS
        o.set_params(p)
    o.set_brute_force(True)
    ref = o.trace_rays(rays)
    o.close()
    return ref


def reference(vpt, oracle, name, strict=False):
    """The closest hits of the set `name` over its own tmin / tmax."""
    key = ("set", name, strict)
    if key not in _REF:
        _REF[key] = brute_force(vpt, oracle, *load(vpt, name), strict=strict)
    return _REF[key]


def shadow_rays(oracle, rays, ray_queries=1):
    """The rays as k_trace_shadow traces them: its own window, and without ray queries the direction normalised (vpt_fp32.h normalize)."""
    r = np.array(rays, np.float32)
    if not ray_queries:
        r[:, 4:7] = oracle.leaf_eval("normalize", r[:, 4:7])
    r[:, 3], r[:, 7] = SHADOW_WINDOW[ray_queries]
    return r


def sky_reference(vpt, oracle, name, strict=False, ray_queries=1):
    """k_trace_shadow<sky>'s answer for the set `name`: 1 where the brute-force search over the kernel's window finds nothing."""
    key = ("sky", name, strict, ray_queries)
    if key not in _REF:
        sc, rays = load(vpt, name)
        _REF[key] = (brute_force(vpt, oracle, sc, shadow_rays(oracle, rays, ray_queries), strict)["t"] < 0).astype(np.uint8)
    return _REF[key]


def light_reference(vpt, oracle, name, strict=False):
    """(k_trace_shadow<light>'s answer for light_rays(name), the closest hits' global ids)."""
    key = ("light", name, strict)
    if key not in _REF:
        sc = light_scene(vpt, name)
        rays, expect, media = light_rays(vpt, name)
        o = oracle.Oracle(sc, 8, 8); tris = o.triangles(); o.close()
        gid = hit_gid(tris, brute_force(vpt, oracle, sc, shadow_rays(oracle, rays), strict))
        _REF[key] = light_visible(gid, expect, media), gid
    return _REF[key]


def check_conditions(vpt, oracle):
    """What the shadow tests' ray sets must be for their results to mean something, from the reference alone: in each light set both answers make up
    at least 10 % of the rays — also among the rays that expect the triangle they aim at — and each sky set keeps the hit fractions the
    vpt_trace_rays tests assert of it.  Returns the figures."""
    out = {}
    for name in LIGHT_SCENES:
        vis, gid = light_reference(vpt, oracle, name)
        rays, expect, media = light_rays(vpt, name)
        out["light_" + name] = {"visible": float(vis.mean()), "visible_right_expectation": float(vis[0::3].mean()), "visible_wrong_expectation": float(vis[1::3].mean()),
                                "visible_media": float(vis[2::3].mean()), "media_visible_on_a_miss": int(((gid < 0) & (media != 0)).sum())}
        assert 0.1 <= vis.mean() <= 0.9, (name, vis.mean())
        assert 0.1 <= vis[0::3].mean() <= 0.9, (name, vis[0::3].mean())
        assert len(np.unique(expect)) >= 2
    assert out["light_chain"]["media_visible_on_a_miss"] > 100   # the open scene: rays past the light leave it
    for name in SKY_SETS:
        hit = 1.0 - float(sky_reference(vpt, oracle, name).mean())
        out["sky_" + name] = {"hit": hit}
        assert hit > (0.2 if name.startswith("far_") else 0.02 if name.startswith("scaled_") else 0.05), (name, hit)
        assert hit < 0.95, (name, hit)
    for name in SKY_SETS_NO_RAY_QUERIES:
        hit = 1.0 - float(sky_reference(vpt, oracle, name, ray_queries=0).mean())
        out["sky_%s_norq" % name] = {"hit": hit}
        assert 0.05 < hit < 0.95, (name, hit)
    return out
