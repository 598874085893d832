"""The material sets of tests/material_sweep.py through every shading kernel: all three BSDF lobes live at once (also under a per-hit
metallic texture: material_finish's renormalisation), roughness 0 and next to it, ior at and below the clamp and beyond the LUT's last
layer, anisotropy 1 with rotations outside [0, 90), black base and specular colours, emitters that also transmit or are metallic (the
class priority of k_classify_instances, k_precompute_lights with several emissive meshes), media at anisotropy 1, -1 and 0.

a. parity with the oracle, bit for bit: every set under the black (PLAIN instantiations) and the lit environment, on the Cornell walls
   (the tree in LDS: k_whole, k_bounce, PLAIN and general) and on the walls with a set member on the sphere (the tree in memory: the
   stream kernels, k_shade_stream per class, k_finish), plus the STRICT and COUNT instantiations on three sets;
b. nothing vacuous, from the oracle alone: every member of every set changes the image; the emitters are in the light table; the media
   set is not depth-bounded and its anisotropy-1 member alone is (the fixed schedule and its captured graphs then run);
c. the device straight against tests/ref_integrator64.py, sample by sample, without the oracle: the one check where a BSDF error the
   device shares with the oracle could not hide;
d. whole sets installed by vpt_set_material on a context that has rendered: shade class, light table and depth_bounded change under it."""
import copy
import os

import numpy as np
import pytest

import material_sweep as M
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

W, H, FRAMES = 96, 54, 3
ENVS = ("black", "lit")
# name: (PathTracer keywords, samples_per_frame, size, batches)
WALL_CONFIGS = {
    "auto": (dict(pipeline=0), 1, (W, H), [FRAMES]),
    "auto_ragged": (dict(pipeline=0), 1, (63, 37), [FRAMES]),
    "fused": (dict(pipeline=1), 1, (W, H), [FRAMES]),
    "general_kernels": (dict(pipeline=0, build_flags=2), 1, (W, H), [FRAMES]),          # VPT_BUILD_GENERAL_KERNELS
    "auto_2spf": (dict(pipeline=0), 2, (W, H), [FRAMES]),                               # not a whole-path batch
}
SPHERE_CONFIGS = {
    "auto": (dict(pipeline=0), 1, (W, H), [FRAMES]),
    "auto_ragged": (dict(pipeline=0), 1, (63, 37), [FRAMES]),
    "fused": (dict(pipeline=1), 1, (W, H), [FRAMES]),
    "staged": (dict(pipeline=2), 1, (W, H), [FRAMES]),
    "staged_streams_only": (dict(pipeline=2, build_flags=4), 1, (W, H), [FRAMES]),      # VPT_BUILD_STREAMS_ONLY
    "staged_sorted": (dict(pipeline=4), 1, (W, H), [FRAMES]),
    "finisher": (dict(pipeline=0, frames_in_flight=2), 1, (W, H), [2, 1]),              # small batches: three bounces, then k_finish
}
_ORACLE = {}
THREADS = min(16, os.cpu_count() or 1)      # (images this small: more oracle threads than that only cost their start-up)


def scene_of(place, name, env, mats=None):
    """place: 'walls' | 'sphere0' | 'sphere2' | 'sphere4'."""
    return M.walls(name, env, mats) if place == "walls" else M.sphere(name, int(place[-1]), env, mats)


def oracle_image(oracle, key, sc, w, h, P, frames):
    """The oracle's image and counters, once per (scene key, size, parameters, frames); handed out read-only."""
    k = (key, w, h, bytes(P), frames)
    if k not in _ORACLE:
        o = oracle.Oracle(sc, w, h, threads=THREADS); o.set_params(P); o.render(frames)
        img, ctr = o.radiance(), o.counters(); o.close()
        img.setflags(write=False)
        _ORACLE[k] = (img, ctr)
    return _ORACLE[k]


def render(vpt, sc, w, h, P, batches, **kw):
    g = vpt.PathTracer(w, h, **kw)
    g.set_scene(sc); g.set_params(P)
    for n in batches:
        g.render(n)
    img, st = g.radiance(), g.stats(); g.close()
    return img, st


def emissive_instances(sc):
    return sum(1 for _, m, _ in sc.instances if any(sc.materials[m]["emissive_color"]))


def parity_case(vpt, oracle, place, name, env, config):
    kw, spf, (w, h), batches = (WALL_CONFIGS if place == "walls" else SPHERE_CONFIGS)[config]
    sc = scene_of(place, name, env)
    if name in M.TEXTURED:
        M.check_texture(sc, name)
    assert sc.env.any() == (env == "lit")
    P = M.params(vpt, env, samples_per_frame=spf)
    ref, _ = oracle_image(oracle, (place, name, env), sc, w, h, P, FRAMES)
    assert (ref[..., :3].sum(axis=2) > 0).mean() > 0.3
    img, st = render(vpt, sc, w, h, P, batches, **kw)
    assert_parity(img, ref)
    kl = st["kernel_launches"]
    if config == "auto" and place == "walls":
        assert st["bvh_node_bytes"] == 128 and kl["primary"] > 0 and kl["extend"] == 0, kl
    if config == "auto" and place != "walls":
        assert st["bvh_node_bytes"] == 64 and kl["extend"] > 0 and kl["join"] > 0, kl
    if config == "finisher":
        assert st["finish_paths"] > 0
    if config == "staged_streams_only":
        assert st["finish_paths"] == 0


# ------------------------------------------------------------------ a. parity
@pytest.mark.parametrize("config", list(WALL_CONFIGS))
@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("name", list(M.SETS))
def test_walls_equal_the_oracle(vpt, oracle, name, env, config):
    parity_case(vpt, oracle, "walls", name, env, config)


@pytest.mark.parametrize("config", list(SPHERE_CONFIGS))
@pytest.mark.parametrize("k", M.SPHERE_MEMBERS)
@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("name", list(M.SETS))
def test_sphere_equals_the_oracle(vpt, oracle, name, env, k, config):
    parity_case(vpt, oracle, "sphere%d" % k, name, env, config)


@pytest.mark.parametrize("mode", ["local_hits", "count_traversal"])
@pytest.mark.parametrize("place", ["walls", "sphere2"])
@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("name", ["three_lobes", "ior_edges", "medium_edges"])
def test_strict_and_counting_instantiations(vpt, oracle, name, env, place, mode):
    """VPT_FLAG_LOCAL_HITS (the STRICT kernels) and vpt_config.count_traversal (the COUNT kernels), AUTO pipeline.  The counting context's
    closest rays are the oracle's where only surfaces scatter."""
    sc = scene_of(place, name, env)
    P = M.params(vpt, env)
    if mode == "local_hits":
        P.flags |= vpt._abi.FLAG_LOCAL_HITS
    ref, ctr = oracle_image(oracle, (place, name, env), sc, W, H, P, FRAMES)
    img, st = render(vpt, sc, W, H, P, [FRAMES], count_traversal=(mode == "count_traversal"))
    assert_parity(img, ref)
    assert st["samples"] == W * H * FRAMES == ctr["samples"]
    if mode == "count_traversal":
        assert st["nodes_visited"] > 0 and st["tris_tested"] > 0
        if name != "medium_edges":
            assert st["closest_rays"] == ctr["closest"], (st["closest_rays"], ctr["closest"])


# ------------------------------------------------------------------ b. nothing vacuous
@pytest.mark.parametrize("place", ["walls", "sphere2"])
@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("name", list(M.SETS))
def test_every_member_changes_the_image(vpt, oracle, name, env, place):
    """Oracle only: the image must change when one member is replaced by the default material — a member no path reaches would pass
    whatever the kernels did."""
    P = M.params(vpt, env)
    full, _ = oracle_image(oracle, (place, name, env), scene_of(place, name, env), W, H, P, FRAMES)
    for i in range(5):
        mats = M.members(name)
        mats[i] = M.default_material()
        other, _ = oracle_image(oracle, (place, name, env, "without", i), scene_of(place, name, env, mats), W, H, P, FRAMES)
        assert not np.array_equal(full, other), "member %d of %s changes nothing on %s under the %s environment" % (i, name, place, env)


@pytest.mark.parametrize("place", ["walls", "sphere0", "sphere2"])
def test_the_emitters_are_lights(vpt, oracle, place):
    sc = scene_of(place, "emitters", "black")
    g = vpt.PathTracer(W, H); g.set_scene(sc); st = g.stats(); g.close()
    o = oracle.Oracle(sc, 8, 8); info = o.scene_info(); o.close()
    # three emissive walls and the lamp; the sphere too: members 0 and 2 both emit
    want = emissive_instances(sc)
    assert want == (4 if place == "walls" else 5)
    assert want >= 3 and st["emissive_mesh_count"] == want == info["emissive_meshes"]
    assert st["emissive_triangle_count"] == info["emissive_tris"]


def async_frames(g, frames):
    """One frame per vpt_render_async with the host a frame ahead, as tests/test_gpu_async.py does."""
    prev = 0
    for _ in range(frames):
        g.render_async(1)
        cur = g.postprocess_device()
        if prev:
            g.wait(prev)
        prev = cur
    g.wait()


@pytest.mark.parametrize("env", ENVS)
def test_medium_at_anisotropy_one_is_depth_bounded(vpt, oracle, env):
    """scene::depth_bounded: a medium at anisotropy exactly 1 never scatters (shade_core.hpp), so a scene whose only medium is that one keeps
    the fixed schedule of vpt_render_async and its captured graphs; the set as a whole does not.  Per-bounce kernels (VPT_PIPELINE_FUSED:
    a fixed batch enqueues max_depth bounces and nothing after them), one frame per call.  Then the sphere takes the set's
    anisotropy -0.8 member on the live context: depth_bounded flips, and a schedule that stayed fixed would cut those paths short."""
    frames = 6
    mats = M.members("medium_edges")
    assert not M.depth_bounded(mats)
    assert [M.depth_bounded([m]) for m in mats] == [True, False, False, False, False]
    assert mats[0]["medium_anisotropy"] == 1.0 and mats[0]["medium_density"] > 0 and mats[0]["transmission"] > 0
    P = M.params(vpt, env)
    fused = vpt._abi.PIPELINE_FUSED
    # the whole set: no fixed schedule, no graph
    sc_all = M.sphere("medium_edges", 2, env)
    assert not M.depth_bounded(sc_all.materials)
    ref_all, _ = oracle_image(oracle, ("sphere2", "medium_edges", env), sc_all, W, H, P, frames)
    g = vpt.PathTracer(W, H, frames_in_flight=1, pipeline=fused)
    g.set_scene(sc_all); g.set_params(P)
    async_frames(g, frames)
    img, st = g.radiance(), g.stats(); g.close()
    assert np.array_equal(img, ref_all)
    assert st["graph_launches"] == 0 and st["frames"] == frames
    # its anisotropy-1 member alone, on the sphere between the fixture's walls
    sc_one = M.sphere("medium_edges", 0, env, mats=M.fixture_walls("cornell_box_glass"), ball=mats[0])
    assert M.depth_bounded(sc_one.materials)
    ref_one, _ = oracle_image(oracle, ("sphere", "medium_edges", env, "only_anisotropy_one"), sc_one, W, H, P, frames)
    plain_glass, _ = oracle_image(oracle, ("sphere", "fixture", env), M.sphere("medium_edges", 0, env, mats=M.fixture_walls("cornell_box_glass"), ball=M.load_fixture("cornell_box_glass").materials[4]), W, H, P, frames)
    assert not np.array_equal(ref_one, plain_glass), "the medium should change the image"
    g = vpt.PathTracer(W, H, frames_in_flight=1, pipeline=fused)
    g.set_scene(sc_one); g.set_params(P)
    async_frames(g, frames)
    img, st = g.radiance(), g.stats()
    assert np.array_equal(img, ref_one)
    assert st["graph_launches"] >= frames - 3, "the fixed 1-frame batches were not replayed from a graph: %r" % (st["graph_launches"],)
    blocking, _ = render(vpt, sc_one, W, H, P, [frames])
    assert np.array_equal(blocking, ref_one)
    # the flip, on the live context
    ball = sc_one.instances[6][1]
    g.set_material(ball, M.to_abi(vpt, mats[1]))
    async_frames(g, frames)
    img2, st2 = g.radiance(), g.stats(); g.close()
    sc_two = M.sphere("medium_edges", 1, env, mats=M.fixture_walls("cornell_box_glass"), ball=mats[1])
    assert not M.depth_bounded(sc_two.materials)
    ref_two, _ = oracle_image(oracle, ("sphere", "medium_edges", env, "only_member_1"), sc_two, W, H, P, frames)
    assert np.array_equal(img2, ref_two)
    assert st2["graph_launches"] == st["graph_launches"], "a graph captured for the depth-bounded scene was replayed after the edit"


# ------------------------------------------------------------------ c. straight against float64
@pytest.mark.parametrize("place", ["walls", "sphere2"])
@pytest.mark.parametrize("name", list(M.SETS))
def test_device_samples_match_the_float64_integrator(vpt, name, place):
    """One frame of one sample per pixel: the radiance IS the sample value.  64 x 36, lit environment, AUTO pipeline, 150 pixels against
    ref_integrator64.sample_value under the rule of tests/test_oracle_integrator_fp64.py (2e-3 relative / 1e-6 absolute per sample, at
    most 1 % of the samples differing outright, more than half of them lit)."""
    sc = scene_of(place, name, "lit")
    P = M.params(vpt, "lit")
    xs, ys = M.window("lit", 150, 4)
    img, st = render(vpt, sc, M.W64, M.H64, P, [1])
    assert st["samples"] == M.W64 * M.H64 and np.isfinite(img).all()
    got = img[ys, xs, :3]
    ref = M.ref64_samples(vpt, (name, place, "device"), sc, "lit", xs, ys, 1)
    bad, total, lit, worst = M.compare64(got, ref[:, 0])
    print("%s %s: %d of %d samples differ, %d lit, worst relative deviation %.2e" % (name, place, bad, total, lit, worst))
    assert total >= 150
    assert lit > 0.5 * total
    assert bad <= 0.01 * total, (bad, total)


# ------------------------------------------------------------------ d. edits on a live context
@pytest.mark.parametrize("place,pipeline", [("walls", 0), ("sphere2", 0), ("sphere2", 4)])
@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("name", ["three_lobes", "emitters", "medium_edges"])
def test_a_set_installed_by_set_material(vpt, oracle, name, env, place, pipeline):
    """The walls (and the sphere) start on material slots of their own that hold the fixture's values; the context renders 2 frames, takes
    the whole set through vpt_set_material, renders 3: the image is the oracle's under the same edits and a fresh context's that got the
    set with vpt_set_scene.  three_lobes: the walls go from the plain to the glass shade class; emitters: the light table grows from one
    mesh to four or five; medium_edges: depth_bounded flips.  A second edit back restores the first image."""
    fixture = "cornell_box" if place == "walls" else "cornell_box_glass"
    start = M.fixture_walls(fixture)
    if place == "walls":
        sc0 = M.walls(name, env, mats=start)
    else:
        sc0 = M.sphere(name, 2, env, mats=start, ball=M.load_fixture(fixture).materials[4])
    slots = [sc0.instances[i][1] for i in range(5)] + ([sc0.instances[6][1]] if place != "walls" else [])
    assert len(set(slots)) == len(slots)
    before = [copy.deepcopy(sc0.materials[s]) for s in slots]
    after = M.members(name) + ([M.members(name)[2]] if place != "walls" else [])
    assert M.depth_bounded(before) and (M.depth_bounded(after) == (name != "medium_edges"))
    P = M.params(vpt, env)
    g = vpt.PathTracer(W, H, pipeline=pipeline)
    g.set_scene(sc0); g.set_params(P); g.render(2)
    first, st0 = g.radiance(), g.stats()
    o = oracle.Oracle(sc0, W, H, threads=THREADS); o.set_params(P); o.render(2)
    assert np.array_equal(first, o.radiance())
    for s, m in zip(slots, after):
        mm = M.to_abi(vpt, m)
        g.set_material(s, mm); o.set_material(s, mm)
        assert bytes(g.get_material(s)) == bytes(mm)
    g.render(FRAMES); o.render(FRAMES)
    img, st1 = g.radiance(), g.stats()
    assert np.array_equal(img, o.radiance()), "differs from the oracle under the same edits"
    o.close()
    sc1 = scene_of(place, name, env)
    ref, _ = oracle_image(oracle, (place, name, env), sc1, W, H, P, FRAMES)
    fresh, st_fresh = render(vpt, sc1, W, H, P, [FRAMES], pipeline=pipeline)
    assert_parity(fresh, ref)
    assert np.array_equal(img, fresh), "differs from a fresh context that got the set with set_scene"
    assert st1["emissive_mesh_count"] == st_fresh["emissive_mesh_count"] and st1["emissive_triangle_count"] == st_fresh["emissive_triangle_count"]
    assert st0["emissive_mesh_count"] == 1
    assert st1["emissive_mesh_count"] == emissive_instances(sc1)
    if name == "emitters":
        assert emissive_instances(sc1) == (4 if place == "walls" else 5)       # (member 2, on the sphere, emits too)
    for s, m in zip(slots, before):
        mm = M.to_abi(vpt, m)
        g.set_material(s, mm)
        assert bytes(g.get_material(s)) == bytes(mm)
    g.render(2)
    again, st2 = g.radiance(), g.stats(); g.close()
    assert np.array_equal(again, first), "the edit back did not restore the first image"
    assert st2["emissive_mesh_count"] == 1
