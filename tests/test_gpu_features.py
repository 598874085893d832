"""vpt_render_features / vpt_pick: what the camera sees first through every pixel — depth, ids, shading normal, albedo — from one kernel that runs
the integrator's camera-ray query and the head of the closest-hit shader, and stops there.
Ids and depth are held EXACTLY against the oracle's camera rays (Oracle.pixel_rays at max_depth 1) in SAMPLE mode; normals and albedo against a
float64 restatement of Surface.slang / Material.Initialize (tests/ref_features64.py) in CENTER mode, leaving out only the pixels at which that
restatement ALONE sits within 1e-4 of taking another branch.  Images are 45 x 37: partial 8 x 8 tiles on both edges and a last wave that is mostly
outside the image.  The layouts of the two structs without a device: tests/test_features_abi_cpu.py."""
import copy
import ctypes as C
import os
import subprocess
from importlib import import_module

import numpy as np
import pytest
import torch   # before the first context exists: torch brings a HIP runtime of its own, and the one the process loads FIRST serves both (test 8 shares pointers)

import material_scenes
import ref_features64 as RF
import refit_moves as RM
import whole_spill_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LUTS = os.path.join(ROOT, "vulkan-path-tracer_amd", "assets", "lookup_tables.bin")
W, H = 45, 37
MISS = 0xffffffff
FLAG_LOCAL_HITS, FLAG_GEOMETRY_NORMALS, FLAG_FURNACE = 256, 8, 32
NO_SCENE, INVALID = "VPT_ERR_NO_SCENE", "VPT_ERR_INVALID_ARGUMENT"
ALL = ("depth", "ids", "normal", "albedo")
_CACHE = {}


def look(vpt, sc, eye, at):
    sc.view_inverse = np.linalg.inv(vpt.scenes.look_at(eye, at, (0.0, 1.0, 0.0))).astype(np.float32)
    return sc


def scene(vpt, name):
    """The scenes of this file, each with a camera chosen for what its test needs (see the tests); built once."""
    if name not in _CACHE:
        S = vpt.scenes
        if name == "cornell_gltf":      # 12 triangles, rides in LDS; seen from outside, past its right edge: hits on every wall and the lamp, and misses
            sc = look(vpt, S.load_gltf(os.path.join(GOLDEN, "cornell_box.gltf")), (9.0, -3.0, 14.0), (0.0, 0.0, -5.0))
        elif name == "chain84":         # the tree lives in memory; from just above the floor UP through the 40 sheets: the searches overflow the 14 LDS rows
            sc = look(vpt, whole_spill_scene.memory_chain_scene(vpt), (0.15, -0.1, -4.4), (0.3, 0.2, 4.0))
        elif name == "combined":        # affine instances (mirrored, sheared, non-uniformly scaled); its own camera sees past the box's edges
            sc = material_scenes.variant("combined")[0]
        elif name == "normal_map":      # from inside the box towards the right wall and the two boxes: per-hit normal maps on most of the image
            sc = look(vpt, material_scenes.variant("normal_map")[0], (-3.0, 1.0, -2.0), (4.0, 2.5, -7.0))
        elif name == "textured_boxes":  # 64 x 64 base-colour texture on the boxes, its own camera
            sc = S.load_gltf(os.path.join(GOLDEN, "textured_boxes.gltf"))
        elif name == "quad":            # one quad at z = -5 facing the camera at the origin; corners at powers of two, so its geometric normal is (0, 0, 1) to the bit
            sc = S.Scene(); sc.luts = S.load_luts()
            p = np.array([[-4, -4, -5], [4, -4, -5], [4, 4, -5], [-4, 4, -5]], np.float32)
            m = sc.add_mesh(p, np.tile(np.array([0, 0, 1], np.float32), (4, 1)), np.zeros((4, 2), np.float32), np.array([0, 1, 2, 0, 2, 3], np.uint32))
            sc.materials.append(S.material(base_color=(0.25, 0.5, 0.8125)))
            sc.add_instance(m, 0)
        else:
            raise KeyError(name)
        _CACHE[name] = sc
    return _CACHE[name]


def context(vpt, sc, w=W, h=H, flags=0, **cfg):
    g = vpt.PathTracer(w, h, **cfg)
    g.set_scene(sc)
    P = vpt.default_params(max_depth=4)
    P.flags |= flags
    g.set_params(P)
    return g


def reference64(vpt, name, flags=0):
    """ref_features64.image of a scene of this file, once."""
    key = ("ref64", name, flags)
    if key not in _CACHE:
        with np.errstate(all="ignore"):
            _CACHE[key] = RF.image(RF.Scene64(scene(vpt, name), W, H), flags)
    return _CACHE[key]


def oracle_camera_hits(vpt, oracle, name, frames):
    """(t [frames, H, W] float32, gid [frames, H, W] int64 or -1, triangle table) of the oracle's camera rays."""
    key = ("oracle", name)
    if key not in _CACHE:
        o = oracle.Oracle(scene(vpt, name), W, H)
        try:
            o.set_params(vpt.default_params(max_depth=1))
            tri = o.triangles()
            rows = np.array([[[o.pixel_rays(x, y, f, cap=8)[0] for x in range(W)] for y in range(H)] for f in frames])
        finally:
            o.close()
        assert np.array_equal(tri[:, 11].view(np.uint32), np.arange(len(tri), dtype=np.uint32))
        _CACHE[key] = (np.ascontiguousarray(rows[..., 8]), rows[..., 9].astype(np.int64), tri)
    return _CACHE[key]


# ---- 1. ids and depth, exact, against the oracle (SAMPLE mode)
@pytest.mark.parametrize("local_hits", [False, True], ids=["default_flags", "local_hits"])
@pytest.mark.parametrize("name", ["cornell_gltf", "chain84", "combined"])
def test_ids_and_depth_equal_the_oracles_camera_rays(vpt, oracle, name, local_hits):
    frames = (0, 3)
    sc = scene(vpt, name)
    t_ref, gid_ref, tri = oracle_camera_hits(vpt, oracle, name, frames)
    prim, inst = tri[:, 9].view(np.uint32), tri[:, 10].view(np.uint32)
    inst_mesh = np.array([me for me, _, _ in sc.instances], np.uint32)
    inst_mat = np.array([ma for _, ma, _ in sc.instances], np.uint32)
    g = context(vpt, sc, flags=FLAG_LOCAL_HITS if local_hits else 0)
    try:
        assert g.stats()["bvh_node_bytes"] == (128 if name == "cornell_gltf" else 64)
        for k, frame in enumerate(frames):
            hit = t_ref[k] >= 0
            assert hit.any() and (~hit).any(), "the view must hold hits and misses"
            assert (gid_ref[k] >= 0).tolist() == hit.tolist()
            f = g.render_features(vpt.FEATURES_SAMPLE, frame, which=("depth", "ids"))
            assert np.array_equal(f["depth"].view(np.uint32), t_ref[k].view(np.uint32)), "depth differs from the oracle's t in %d pixels" % (f["depth"] != t_ref[k]).sum()
            want = np.full((H, W, 4), MISS, np.uint32)
            gi = gid_ref[k][hit]
            want[hit] = np.stack([inst[gi], prim[gi], inst_mat[inst[gi]], inst_mesh[inst[gi]]], axis=1)
            assert np.array_equal(f["ids"], want)
        if name == "chain84":
            assert g.stats()["stack_spills"][0] > 0, "the camera rays were meant to overflow the LDS part of the stack"
        assert not np.array_equal(t_ref[0], t_ref[1]), "frames 0 and 3 must draw different jitter"
    finally:
        g.close()


# ---- 2. closed form (CENTER mode)
def test_a_quad_facing_the_camera_in_closed_form(vpt):
    """depth = D / |dir.z| from the same matrices in float64; albedo = base_color exactly (the texel is 1: pow(1, 2.2) = 1).
    The normal: the reference's default normal map is the texel (128, 128, 255), which decodes to (0.0039, 0.0039, 1) and not to (0, 0, 1) — no UNORM8
    texel does — so the mapped normal is held against its own closed form, normalize(nx * T + ny * B + N) with T = (0, -1, 0), B = (1, 0, 0)
    (Surface.slang's frame for N = +z), and (0, 0, 1, 0) EXACTLY is asserted where it is the exact answer: under VPT_FLAG_GEOMETRY_NORMALS."""
    sc = scene(vpt, "quad")
    S = RF.Scene64(sc, W, H)
    d = np.array([[RF.center_ray(S, x, y)[1] for x in range(W)] for y in range(H)])
    want_depth = 5.0 / np.abs(d[..., 2])
    n = 128.0 / 255.0 * 2.0 - 1.0
    mapped = np.array([n, -n, 1.0]) / np.linalg.norm([n, -n, 1.0])
    for flags in (0, FLAG_GEOMETRY_NORMALS):
        g = context(vpt, sc, flags=flags)
        try:
            f = g.render_features(vpt.FEATURES_CENTER, 0)
        finally:
            g.close()
        assert (f["depth"] > 0).all()
        assert np.abs(f["depth"] / want_depth - 1.0).max() <= 1e-5
        assert (f["ids"][..., 0] == 0).all() and np.isin(f["ids"][..., 1], (0, 1)).all() and (f["ids"][..., 2] == 0).all() and (f["ids"][..., 3] == 0).all()
        assert set(np.unique(f["ids"][..., 1])) == {0, 1}
        assert np.array_equal(f["albedo"], np.broadcast_to(np.array([0.25, 0.5, 0.8125, 0.0], np.float32), (H, W, 4)))
        if flags:
            assert np.array_equal(f["normal"], np.broadcast_to(np.array([0, 0, 1, 0], np.float32), (H, W, 4)))
        else:
            assert np.abs(f["normal"][..., :3] - mapped).max() <= 1e-6 and (f["normal"][..., 3] == 0).all()


# ---- 3. normals and albedo under textures
TOL = 1e-5   # O(1) values, a few dozen fp32 operations (2^-24 each) and a pow within 4 ulp (tests/test_fp32_contract.py)


@pytest.mark.parametrize("name", ["normal_map", "textured_boxes"])
def test_normals_and_albedo_against_float64(vpt, name):
    """Surface.slang / Material.Initialize restated in float64 (tests/ref_features64.py) at every hit pixel, 1e-5 absolute.
    What the two shader functions are GIVEN — the hit's triangle and barycentrics — is the device's own hit, read per pixel through vpt_pick (the
    same kernel; t and the ids equal the buffers' bit for bit, and the traversal is held bit-exact against the oracle by test 1 and the vpt_trace_rays
    tests).  Measured with the hit recomputed in float64 as well (printed below), the textured faces miss 1e-5 — normal 6.45e-05 on 'normal_map' (3.4e-05
    from the oracle's fp32 barycentrics alone, on the host), albedo 5.13e-04 on 'textured_boxes' — while the chain itself is within 3.3e-06 and 3.0e-06:
    a box face spans 74 texels of a random normal map (64 of the colour texture), so the 1e-7 .. 1e-5 the fp32 ray-triangle test leaves in (t, u, v) is
    worth that much in the looked-up texel — the sensitivity of the map, not an error of the chain this tolerance is about.
    The float64 closest hit still decides which pixels hit and which triangle they see, and the 2 % cap holds for it alone and for the evaluation used."""
    hit, normal, albedo, margin, recs = reference64(vpt, name)
    sc = scene(vpt, name)
    per_hit = lambda key: sum(1 for row in recs for r in row if r and sc.textures[sc.materials[r["material"]][key]].shape[:2] != (1, 1))
    if name == "normal_map":
        assert per_hit("normal_texture") > 0.5 * hit.sum(), "most of the image was meant to lie on normal-mapped materials"
    else:
        assert per_hit("base_color_texture") > 0.2 * hit.sum() and (~hit).any()
    out = hit & (margin < 1e-4)
    assert out.sum() <= 0.02 * hit.sum(), "the reference alone leaves out %d of %d hit pixels" % (out.sum(), hit.sum())
    S64 = RF.Scene64(sc, W, H)
    gid_of = {ip: k for k, ip in enumerate(S64.ids)}
    g = context(vpt, sc)
    try:
        f = g.render_features(vpt.FEATURES_CENTER, 0)
        picks = {(x, y): g.pick(x, y) for y in range(H) for x in range(W) if f["ids"][y, x, 0] != MISS}
    finally:
        g.close()
    assert np.array_equal(f["ids"][..., 0] != MISS, hit) and np.array_equal(f["depth"] >= 0, hit)
    want_ids = np.array([[[r["instance"], r["primitive"], r["material"], r["mesh"]] if r else [MISS] * 4 for r in row] for row in recs], np.uint32)
    assert np.array_equal(f["ids"], want_ids)
    assert not f["normal"][~hit].any() and not f["albedo"][~hit].any()
    en = ea = eh = 0.0
    left_out = 0
    with np.errstate(all="ignore"):
        for (x, y), p in picks.items():
            assert np.float32(p["t"]).view(np.uint32) == f["depth"][y, x].view(np.uint32)
            r64 = recs[y][x]
            eh = max(eh, abs(p["u"] - r64["u"]), abs(p["v"] - r64["v"]), abs(p["t"] / r64["t"] - 1.0))
            r = RF.first_hit(S64, x, y, hit=(float(p["t"]), float(p["u"]), float(p["v"]), gid_of[(p["instance"], p["primitive"])]))
            if r["margin"] < 1e-4:
                left_out += 1
                continue
            en = max(en, np.abs(f["normal"][y, x] - r["normal"]).max())
            ea = max(ea, np.abs(f["albedo"][y, x] - r["albedo"]).max())
    print("%s: %d hit pixels, %d left out (%d by the float64 hit alone), max |normal error| %.3g, max |albedo error| %.3g; with the hit recomputed in float64: "
          "%.3g, %.3g (hit differs by up to %.3g)" % (name, hit.sum(), left_out, out.sum(), en, ea, np.abs(f["normal"][hit & ~out] - normal[hit & ~out]).max(),
                                                    np.abs(f["albedo"][hit & ~out] - albedo[hit & ~out]).max(), eh))
    assert left_out <= 0.02 * hit.sum()
    assert en <= TOL and ea <= TOL


# ---- 4. flags
def test_geometry_normals_and_furnace(vpt):
    sc = scene(vpt, "normal_map")
    hit, _, _, _, recs = reference64(vpt, "normal_map")
    ng = np.array([[r["ng"] if r else np.zeros(3) for r in row] for row in recs])
    inside = np.array([[r["normal"][3] if r else 0.0 for r in row] for row in recs])
    g = context(vpt, sc, flags=FLAG_GEOMETRY_NORMALS)
    try:
        f = g.render_features(vpt.FEATURES_CENTER, 0, which=("normal",))
    finally:
        g.close()
    assert list(f) == ["normal"]
    assert np.abs(f["normal"][..., :3] - ng).max() <= 1e-6 and np.array_equal(f["normal"][..., 3], inside.astype(np.float32))
    for name in ("normal_map", "textured_boxes"):
        hit = reference64(vpt, name)[0]
        g = context(vpt, scene(vpt, name), flags=FLAG_FURNACE)
        try:
            f = g.render_features(vpt.FEATURES_CENTER, 0, which=("albedo",))
        finally:
            g.close()
        assert (f["albedo"][hit][:, :3] == 1.0).all() and not f["albedo"][~hit].any()


# ---- 5. vpt_pick
def test_pick_equals_the_center_buffers(vpt):
    sc = scene(vpt, "textured_boxes")
    hit, _, _, _, recs = reference64(vpt, "textured_boxes")
    ys, xs = np.nonzero(hit); ym, xm = np.nonzero(~hit)
    pixels = [(0, 0), (W - 1, H - 1), (int(xs[len(xs) // 2]), int(ys[len(ys) // 2])), (int(xm[len(xm) // 2]), int(ym[len(ym) // 2]))]
    g = context(vpt, sc)
    try:
        f = g.render_features(vpt.FEATURES_CENTER, 0, which=("depth", "ids"))
        for x, y in pixels:
            p = g.pick(x, y)
            assert [p["instance"], p["primitive"], p["material"], p["mesh"]] == f["ids"][y, x].tolist(), (x, y)
            assert np.float32(p["t"]).view(np.uint32) == f["depth"][y, x].view(np.uint32), (x, y)
            r = recs[y][x]
            if r is None:
                assert p["instance"] == MISS and p["t"] == -1.0
            else:
                assert np.abs(p["position"] - (r["origin"] + np.float64(p["t"]) * r["direction"])).max() <= 1e-5
                assert 0.0 <= p["u"] <= 1.0 and 0.0 <= p["v"] <= 1.0 and p["u"] + p["v"] <= 1.0 + 1e-6
        assert hit[pixels[2][1], pixels[2][0]] and not hit[pixels[3][1], pixels[3][0]]
        for x, y in ((W, 0), (0, H)):
            with pytest.raises(vpt.VptError, match=INVALID):
                g.pick(x, y)
        assert np.array_equal(g.render_features(vpt.FEATURES_CENTER, 0, which=("depth",))["depth"], f["depth"])   # the context is still usable
    finally:
        g.close()


# ---- 6. it disturbs nothing
@pytest.mark.parametrize("use_async", [False, True], ids=["blocking", "async_batch_in_flight"])
def test_a_call_between_batches_changes_no_image_and_no_counter(vpt, oracle, scenes, use_async):
    sc = scenes("cornell_box")
    w, h = 32, 24
    P = vpt.default_params(max_depth=4)
    key = ("oracle6", w, h)
    if key not in _CACHE:
        o = oracle.Oracle(sc, w, h); o.set_params(P); o.render(6); _CACHE[key] = o.radiance(); o.close()

    def run(interrupt):
        g = vpt.PathTracer(w, h); g.set_scene(sc); g.set_params(P)
        try:
            render = (lambda n: g.render_async(n)) if use_async else g.render
            render(3)
            if interrupt:
                a = g.render_features(vpt.FEATURES_CENTER, 0)
                b = g.render_features(vpt.FEATURES_SAMPLE, 2)
                g.pick(7, 5)
                assert (a["depth"] > 0).any() and not np.array_equal(a["depth"], b["depth"])
            render(3)
            g.wait()
            st = g.stats()
            return g.radiance(), [st[k] for k in ("samples", "frames", "dispatches", "closest_rays")]
        finally:
            g.close()
    img, st = run(True)
    img0, st0 = run(False)
    assert np.array_equal(img, img0) and np.array_equal(img, _CACHE[key])
    assert st == st0 and st[1] == 6


# ---- 7. it follows edits
def test_buffers_follow_moved_instances_and_edited_materials(vpt, scenes):
    sc = copy.deepcopy(scenes("cornell_box_glass"))
    moved = RM.moved_matrices(sc, RM.GLASS_LAMP_AND_SPHERE)
    g = context(vpt, sc, flags=FLAG_LOCAL_HITS)
    try:
        before = g.render_features(vpt.FEATURES_CENTER, 0)
        for i, m in moved.items():
            g.set_instance_transforms(i, [m])
        m = g.get_material(1)
        m.base_color[:] = (0.1, 0.9, 0.3); m.transmission = 0.25
        g.set_material(1, m)
        got = [g.render_features(mode, 5) for mode in (vpt.FEATURES_CENTER, vpt.FEATURES_SAMPLE)]
    finally:
        g.close()
    sc2 = RM.with_matrices(sc, moved)
    sc2.materials = copy.deepcopy(sc.materials)
    sc2.materials[1]["base_color"] = (0.1, 0.9, 0.3); sc2.materials[1]["transmission"] = 0.25
    g = context(vpt, sc2, flags=FLAG_LOCAL_HITS)
    try:
        want = [g.render_features(mode, 5) for mode in (vpt.FEATURES_CENTER, vpt.FEATURES_SAMPLE)]
    finally:
        g.close()
    for a, b in zip(got, want):
        for k in ALL:
            assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(before["depth"], got[0]["depth"]) and not np.array_equal(before["albedo"], got[0]["albedo"]), "the edits were meant to be visible"
    assert (got[0]["ids"][..., 2] == 1).any()


# ---- 8. shards and memory kinds
def test_shard_contexts_and_device_pointers(vpt):
    sc = scene(vpt, "textured_boxes")
    g = context(vpt, sc)
    try:
        want = {mode: g.render_features(mode, 1) for mode in (vpt.FEATURES_CENTER, vpt.FEATURES_SAMPLE)}
        dev = {k: torch.zeros((H, W) + (() if k == "depth" else (4,)), dtype=torch.int32 if k == "ids" else torch.float32, device="cuda:0") for k in ALL}
        for mode in want:
            g.render_features_device(mode, 1, **{k: t.data_ptr() for k, t in dev.items()})
            torch.cuda.synchronize()
            for k in ALL:
                assert np.array_equal(dev[k].cpu().numpy().view(want[mode][k].dtype), want[mode][k]), (mode, k)
        only = torch.full((H, W, 4), 7.0, device="cuda:0")
        g.render_features_device(vpt.FEATURES_CENTER, 0, normal=only.data_ptr())      # one buffer alone
        assert np.array_equal(only.cpu().numpy(), want[vpt.FEATURES_CENTER]["normal"])
    finally:
        g.close()
    for rank in (0, 1):
        s = context(vpt, sc, shard_rank=rank, shard_count=2)
        try:
            for mode in want:
                f = s.render_features(mode, 1)
                for k in ALL:
                    assert np.array_equal(f[k], want[mode][k]), (rank, mode, k)
        finally:
            s.close()


# ---- 9. errors
def test_errors_leave_the_context_usable(vpt, oracle, scenes):
    sc = scenes("cornell_box")
    w, h = 32, 24
    P = vpt.default_params(max_depth=4)
    o = oracle.Oracle(sc, w, h); o.set_params(P); o.render(2); ref = o.radiance(); o.close()
    g = vpt.PathTracer(w, h)
    try:
        with pytest.raises(vpt.VptError, match=NO_SCENE):
            g.render_features(vpt.FEATURES_CENTER, 0)
        with pytest.raises(vpt.VptError, match=NO_SCENE):
            g.pick(0, 0)
        g.set_scene(sc); g.set_params(P)
        with pytest.raises(vpt.VptError, match=INVALID):
            g.render_features(vpt.FEATURES_CENTER, 0, which=())          # all four pointers NULL
        with pytest.raises(vpt.VptError, match=INVALID):
            g.render_features(2, 0)                                      # an unknown mode
        lib = vpt.load_library()
        assert lib.vpt_render_features(g.ctx, 0, 0, None) == -1 and lib.vpt_render_features(None, 0, 0, C.byref(vpt._abi.FeatureBuffers())) == -1
        assert lib.vpt_pick(g.ctx, 0, 0, None) == -1 and lib.vpt_pick(None, 0, 0, C.byref(vpt._abi.PickResult())) == -1
        g.render(2)
        assert np.array_equal(g.radiance(), ref)
    finally:
        g.close()


# ---- 10. the command-line tool
def test_cli_writes_the_guide_buffers(vpt, tmp_path):
    from test_host_cpp import CLI, HOST
    import fcntl
    vpt.load_library()
    with open(os.path.join(HOST, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-C", HOST, "vpt_render"], stdout=subprocess.DEVNULL)
    gltf = os.path.join(GOLDEN, "cornell_box.gltf")
    w, h = 32, 24
    prefix, cam = str(tmp_path / "aov"), str(tmp_path / "c.f32")
    subprocess.check_output([CLI, "--scene", gltf, "--luts", LUTS, "--size", "%dx%d" % (w, h), "--spp", "2", "--depth", "3", "--camera", cam, "--aov", prefix])
    m = np.fromfile(cam, "<f4").reshape(2, 4, 4)
    g = vpt.PathTracer(w, h)
    try:
        g.set_scene(vpt.scenes.load_gltf(gltf))
        g.set_camera(m[0].T, m[1].T)   # column-major dumps -> math matrices
        f = g.render_features(vpt.FEATURES_CENTER, 0, which=("normal", "albedo"))
    finally:
        g.close()
    assert (f["albedo"][..., :3] > 0).any()
    for name, v in (("normal", f["normal"] * np.float32(0.5) + np.float32(0.5)), ("albedo", f["albedo"])):
        want = (np.clip(v, np.float32(0.0), np.float32(1.0)) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
        want[..., 3] = 255
        got = np.asarray(import_module("vulkan-path-tracer_amd.imagecodec").load_image("%s_%s.png" % (prefix, name)))
        assert got.shape == (h, w, 4) and np.array_equal(got, want), name
