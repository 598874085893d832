"""Every traversal schedule through its stack-SPILL path.  A lane's stack is 14 LDS entries (traverse.hpp kStackDepth); deeper entries go to a
per-thread region in global memory that every kernel addresses with a stride of its own (the vote and trace kernels 82 words, k_trace_pair
2 x 82 on half the blocks), one region per lane and a second one for the kernels of the main lane's second stream.  tests/test_gpu_spills.py
takes that path on the default schedule with a 40,000-triangle scene; this file takes it everywhere else the product can schedule a scene
whose BVH lives in memory, on tests/whole_spill_scene.py's memory_chain_scene: 84 triangles, a chain-shaped tree, and 7 % of the rays that
go up through its sheets hold up to 22 entries (tests/test_stack_bound_cpu.py checks that on the host) — in closest-hit and any-hit
searches alike, and at every bounce, because paths keep bouncing between the floor and the underside of the stack.

Every case asserts (a) its premise — vpt_stats.stack_spills, the words written to the first regions of all lanes and to the main lane's
second region, is non-zero for the regions the schedule uses, and the schedule's own kernels ran; (b) the image is the oracle's bit for
bit; (c) the ray statistics are the oracle's or a twin's.  The spill counter is cumulative per region and cannot say WHICH kernel wrote:
where several kernels share a region (k_finish behind three bounces of the stream kernels; the three lanes of asynchronous frames, summed
in the first figure) the premise rests on the host measurement above holding for every bounce and every frame alike."""
import copy
import ctypes as C

import numpy as np
import pytest

import whole_spill_scene
from test_stack_bound_cpu import floor_to_light_rays, random_rays

pytestmark = pytest.mark.gpu
W, H = 96, 54
BUILD_SBVH, BUILD_STREAMS_ONLY = 1, 4          # include/vpt.h VPT_BUILD_*
VISITS = ("nodes_visited", "tris_tested", "shadow_nodes_visited", "shadow_tris_tested")


@pytest.fixture(scope="module")
def scene(vpt):
    return whole_spill_scene.memory_chain_scene(vpt)


@pytest.fixture(scope="module")
def reference(oracle):
    """The oracle's image and counters per (scene, frames, parameters, media), computed once and handed out read-only."""
    cache = {}

    def get(sc, frames, P, volumes=(), atm=None, key=None):
        k = (id(sc) if key is None else key, frames, bytes(P), tuple(bytes(v) for v in volumes), bytes(atm) if atm is not None else None)
        if k not in cache:
            o = oracle.Oracle(sc, W, H)
            o.set_params(P); o.set_volumes(list(volumes)); o.set_atmosphere(atm)
            o.render(frames)
            img, ctr = o.radiance(), o.counters()
            o.close()
            img.setflags(write=False)
            assert img[..., :3].max() > 0
            cache[k] = (img, ctr)
        return cache[k]
    return get


def render(vpt, sc, P, batches, volumes=(), atm=None, **kw):
    g = vpt.PathTracer(W, H, **kw)
    g.set_scene(sc); g.set_params(P)
    if volumes:
        g.set_volumes(list(volumes))
    if atm is not None:
        g.set_atmosphere(atm)
    for n in batches:
        g.render(n)
    img, st = g.radiance(), g.stats()
    g.close()
    return img, st


def spilled(st, second):
    """(a): the first region always; the main lane's second one exactly when the schedule runs the shadow kernels beside the next extend."""
    print("stack_spills %r, finish_paths %d, graph_launches %d, launches %r" % (st["stack_spills"], st["finish_paths"], st["graph_launches"], st["kernel_launches"]))
    assert st["bvh_node_bytes"] == 64, "the tree should live in memory"
    assert st["stack_spills"][0] > 0, "no spills: %r" % (st["stack_spills"],)
    assert (st["stack_spills"][1] > 0) == second, "second region: %r" % (st["stack_spills"],)


def same_rays(st, ctr, frames):
    """(c) against the oracle, as tests/test_gpu_transitions.py holds them: closest rays equal; the oracle counts every visibility query of
    its loop, the library the shadow rays it launches — never more than the oracle asked."""
    print("closest %d (oracle %d), shadow %d (oracle %d)" % (st["closest_rays"], ctr["closest"], st["shadow_rays"], ctr["shadow"]))
    assert st["samples"] == W * H * frames == ctr["samples"]
    assert st["closest_rays"] == ctr["closest"], (st["closest_rays"], ctr["closest"])
    assert 0 < st["shadow_rays"] <= ctr["shadow"], (st["shadow_rays"], ctr["shadow"])


def hit_rays(o, d, tmin, tmax):
    n = len(o)
    return np.concatenate([o, np.full((n, 1), tmin), d, np.full((n, 1), tmax)], axis=1).astype(np.float32)


@pytest.mark.parametrize("window", ["kernel_range", "mid_stack"])
def test_trace_rays_against_brute_force(vpt, oracle, scene, window):
    """k_trace_rays (vpt_trace_rays) on a fresh context: the only traversal kernel that has run when the spill words are counted, on the main
    lane's first region.  Rays from the floor towards the light and random rays through the stack, over the kernels' closest-hit range and
    over a window that begins and ends between the sheets (for a vertical ray the stack spans t = 3 .. 6): such searches still hold up to
    19 entries (tests/test_stack_bound_cpu.py)."""
    rng = np.random.default_rng(21)
    tmin, tmax = (0.01, 100000.0) if window == "kernel_range" else whole_spill_scene.MID_STACK_WINDOW
    o1, d1 = floor_to_light_rays(rng, 6000)
    o2, d2 = random_rays(rng, whole_spill_scene.world_triangles(scene), 6000)
    rays = np.concatenate([hit_rays(o1, d1, tmin, tmax), hit_rays(o2, d2, tmin, tmax)])
    o = oracle.Oracle(scene, 8, 8)
    o.set_brute_force(True)
    ref = o.trace_rays(rays)
    o.close()
    g = vpt.PathTracer(8, 8)
    g.set_scene(scene)
    assert g.stats()["stack_spills"] == [0, 0]
    got = g.trace_rays(rays)
    st = g.stats()
    g.close()
    spilled(st, False)
    for k in ("t", "u", "v", "primitive", "instance"):
        assert np.array_equal(got[k], ref[k]), k
    hit = ref["t"] >= 0
    assert hit[:6000].any() and hit[6000:].any() and (~hit).any()
    if window == "mid_stack":
        assert (ref["t"][hit] > tmin).all() and (ref["t"][hit] < tmax).all()
        assert (ref["instance"][:6000][hit[:6000]] == 1).all(), "from the floor, only sheets lie inside the window"


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("count", [False, True])
def test_finisher_instantiations(vpt, scene, reference, count, strict):
    """k_finish<COUNT, STRICT> behind small batches of the streams pipeline (finish_at = 3 bounces) at depth 8: it aliases a TravStack and a
    LaneStack on the same LDS rows and the same region and runs three searches per bounce.  Against the oracle and against a twin that runs
    every bounce on the stream kernels (VPT_BUILD_STREAMS_ONLY), as tests/test_gpu_transitions.py test_finisher_instantiations.  Bounces 3
    to 7 start on the floor or on the underside of the stack like the bounces before them, so k_finish's searches spill like theirs."""
    frames = 4
    P = vpt.default_params(max_depth=8)
    if strict:
        P.flags |= vpt._abi.FLAG_LOCAL_HITS
    ref, ctr = reference(scene, frames, P)
    stats = []
    for build in (0, BUILD_STREAMS_ONLY):
        img, st = render(vpt, scene, P, [2, 2], frames_in_flight=2, count_traversal=count, build_flags=build)
        spilled(st, not count)                              # (counting contexts run one kernel at a time, on one stream)
        assert np.array_equal(img, ref), build
        same_rays(st, ctr, frames)
        stats.append(st)
    fin, streams = stats
    assert fin["finish_paths"] > 0 and streams["finish_paths"] == 0
    assert fin["finish_closest_rays"] > 0 and fin["finish_shadow_rays"] > 0
    assert fin["kernel_launches"]["extend"] < streams["kernel_launches"]["extend"]
    assert fin["shadow_rays"] == streams["shadow_rays"], (fin["shadow_rays"], streams["shadow_rays"])
    if count:
        for k in VISITS:
            assert fin[k] > 0 and fin[k] == streams[k], (k, fin[k], streams[k])
    else:
        assert all(fin[k] == 0 for k in VISITS)


def test_regeneration(vpt, scene, reference):
    """Eight frames with two frames of paths resident: refills run beside spilling searches, and a lane's slot in the spill region serves
    one path after another."""
    frames = 8
    P = vpt.default_params(max_depth=6)
    ref, ctr = reference(scene, frames, P)
    img, st = render(vpt, scene, P, [frames], frames_in_flight=frames, resident_frames=2)
    spilled(st, True)
    assert st["resident_frames"] == 2 and st["frames_allocated"] == frames
    assert st["kernel_launches"]["primary"] > 1, "the camera-ray launch and refills"
    assert np.array_equal(img, ref)
    same_rays(st, ctr, frames)


def test_async_lanes_and_graph_replay(vpt, oracle, scene, reference):
    """One frame per vpt_render_async with the host a frame ahead, as tests/test_gpu_whole.py test_async_frames_are_whole_path_launches: on a
    scene in memory every such batch is three bounces of the stream kernels and k_finish on ONE stream, dealt to the lanes — each with a
    spill region of its own — and replayed from captured graphs."""
    frames = 10
    P = vpt.default_params(max_depth=6)
    ref, ctr = reference(scene, frames, P)
    g = vpt.PathTracer(W, H, frames_in_flight=1)
    g.set_scene(scene); g.set_params(P)
    prev = 0
    for _ in range(frames):
        done, _t = g.render_async(1)
        assert not done
        cur = g.postprocess_device()
        if prev:
            g.wait(prev)
        prev = cur
    g.wait()
    st = g.stats()
    img, out8 = g.radiance(), g.output_to_host()
    g.close()
    # (a captured batch and a batch on an extra lane stay on one stream; the plain launches before the replays begin go to the main lane with
    # its shadow kernels on the second stream, and the regions keep what was written)
    spilled(st, True)
    assert st["graph_launches"] > 0, "the 1-frame batches were not replayed from a captured graph"
    assert st["finish_paths"] > 0 and st["kernel_launches"]["extend"] > 0 and st["kernel_launches"]["resolve"] == frames
    assert np.array_equal(img, ref)
    assert np.array_equal(out8, oracle.postprocess(ref, vpt.default_post_params())[0])
    same_rays(st, ctr, frames)


@pytest.mark.parametrize("medium", ["volume", "atmosphere"])
def test_media_on_the_streams(vpt, scene, reference, medium):
    """kernels_media.hip on the streams (AUTO on a scene in memory): the distance query and the extend on k_trace_vote, the shadow kernels,
    all on one stream and one region.  A homogeneous volume that encloses the stack, set up as tests/test_gpu_volumes.py does; the
    atmosphere as tests/test_gpu_atmosphere.py does.  The fused media kernel (k_bounce on the tree in memory, its own TravStack) is the twin."""
    frames = 3
    if medium == "volume":
        P = vpt.default_params(max_depth=6)
        vols, atm = [vpt.volume(corner_min=(-2.0, -2.0, -2.5), corner_max=(2.0, 2.0, 2.5), color=(0.9, 0.85, 0.8), density=0.3, anisotropy=0.3)], None
    else:
        P = vpt.default_params(max_depth=6, sky_altitude=-50.0, sky_azimuth=150.0)
        vols, atm = [], vpt.atmosphere()
    ref, ctr = reference(scene, frames, P, vols, atm)
    plain, _ = reference(scene, frames, vpt.default_params(max_depth=6))
    assert not np.array_equal(ref, plain), "the medium should change the image"
    img, st = render(vpt, scene, P, [frames], vols, atm)
    spilled(st, False)
    kl = st["kernel_launches"]
    assert kl["bounce"] == 0 and kl["extend"] > 0 and kl["extend"] == kl["shade"] and kl["shadow"] > 0 and kl["join"] > 0, kl   # (distance + extend, scatter + shade per bounce)
    assert np.array_equal(img, ref)
    assert st["samples"] == W * H * frames == ctr["samples"]
    fused, sf = render(vpt, scene, P, [frames], vols, atm, pipeline=vpt._abi.PIPELINE_FUSED)
    spilled(sf, False)
    assert sf["kernel_launches"]["bounce"] > 0 and sf["kernel_launches"]["extend"] == 0
    assert np.array_equal(fused, ref)
    assert sf["samples"] == st["samples"]


def assemble(parts):
    hip = C.CDLL("libamdhip64.so")
    n = parts[0].shard_floats()
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), n * 4 * len(parts)) == 0
    for r, g in enumerate(parts):
        g.shard_to_device(C.c_void_p(buf.value + r * n * 4))
    parts[0].assemble_shards(buf, len(parts))
    img = parts[0].radiance()
    hip.hipFree(buf)
    return img


@pytest.mark.parametrize("which", ["sorted", "fused", "sbvh", "sbvh_fused"])
def test_other_pipelines_and_builds(vpt, scene, reference, which):
    """The class-sorted streams (one stream), the fused per-bounce kernel on the tree in memory (and round 1's stage kernels in the laboratory
    build), and a tree built with spatial splits under both."""
    A = vpt._abi
    frames = 4
    P = vpt.default_params(max_depth=6)
    ref, ctr = reference(scene, frames, P)
    kw = {"sorted": dict(pipeline=A.PIPELINE_STAGED_SORTED), "fused": dict(pipeline=A.PIPELINE_FUSED), "sbvh": dict(build_flags=BUILD_SBVH),
          "sbvh_fused": dict(build_flags=BUILD_SBVH, pipeline=A.PIPELINE_FUSED)}[which]
    img, st = render(vpt, scene, P, [3, 1], frames_in_flight=3, **kw)
    spilled(st, which == "sbvh")
    kl = st["kernel_launches"]
    if "fused" in which:
        assert kl["bounce"] > 0 and kl["extend"] == 0
    else:
        assert kl["extend"] > 0 and kl["join"] > 0 and st["finish_paths"] > 0
    assert st["build_flags"] & BUILD_SBVH == kw.get("build_flags", 0)
    assert np.array_equal(img, ref)
    same_rays(st, ctr, frames)
    if which == "fused" and vpt.has_lab():
        img, st = render(vpt, scene, P, [3, 1], frames_in_flight=3, pipeline=A.PIPELINE_STAGED_R1)
        spilled(st, False)
        assert np.array_equal(img, ref)


def test_two_row_shards(vpt, scene, reference):
    frames = 4
    P = vpt.default_params(max_depth=6)
    ref, ctr = reference(scene, frames, P)
    parts = []
    for r in range(2):
        g = vpt.PathTracer(W, H, shard_rank=r, shard_count=2)
        g.set_scene(scene); g.set_params(P); g.render(frames)
        parts.append(g)
    stats = [g.stats() for g in parts]
    for st in stats:
        spilled(st, True)
    img = assemble(parts)
    for g in parts:
        g.close()
    assert np.array_equal(img, ref)
    total = {k: sum(s[k] for s in stats) for k in ("samples", "closest_rays", "shadow_rays")}
    same_rays(total, ctr, frames)


def test_counted_visits_do_not_depend_on_the_schedule(vpt, scene, reference):
    """vpt_config.count_traversal: node and triangle visits are per ray, so streams (+ k_finish) and the fused kernel count the same — with
    every entry that went through the spill region popped again, no more and no less (tests/test_gpu_whole.py's counting test)."""
    frames = 4
    P = vpt.default_params(max_depth=6)
    ref, ctr = reference(scene, frames, P)
    a, sa = render(vpt, scene, P, [frames], count_traversal=True)
    b, sb = render(vpt, scene, P, [frames], count_traversal=True, pipeline=vpt._abi.PIPELINE_FUSED)
    spilled(sa, False); spilled(sb, False)
    assert sa["kernel_launches"]["extend"] > 0 and sb["kernel_launches"]["bounce"] > 0 and sb["kernel_launches"]["extend"] == 0
    assert np.array_equal(a, ref) and np.array_equal(b, ref)
    same_rays(sa, ctr, frames); same_rays(sb, ctr, frames)
    for k in VISITS + ("closest_rays", "shadow_rays", "samples"):
        assert sa[k] == sb[k] and sa[k] > 0, (k, sa[k], sb[k])


@pytest.mark.parametrize("flags", ["no_ray_queries", "no_mis", "local_hits", "furnace"])
def test_flags_that_pick_other_instantiations(vpt, scene, reference, flags):
    """k_trace_vote / k_trace_shadow as the parameter flags instantiate them, with k_finish behind three bounces (AUTO) and on every bounce
    (VPT_BUILD_STREAMS_ONLY).  Without ray queries no light rays exist (shade_core.hpp), so that case gets a sun-and-sky environment: its
    shadow kernels then run the sky rays, up through the sheets."""
    A = vpt._abi
    frames = 3
    P = vpt.default_params(max_depth=6)
    P.flags = {"no_ray_queries": A.FLAGS_DEFAULT & ~A.FLAG_RAY_QUERIES, "no_mis": A.FLAGS_DEFAULT & ~A.FLAG_SKY_MIS & ~A.FLAG_MESH_MIS,
               "local_hits": A.FLAGS_DEFAULT | A.FLAG_LOCAL_HITS, "furnace": A.FLAGS_DEFAULT | A.FLAG_FURNACE}[flags]
    sc = scene
    if flags == "no_ray_queries":
        sc = copy.deepcopy(scene)
        sc.env = vpt.scenes.sun_sky_env(32, 16, seed=6, sun_peak=60.0)
    ref, ctr = reference(sc, frames, P, key=flags)
    if flags == "no_mis":
        assert not np.array_equal(ref, reference(scene, frames, vpt.default_params(max_depth=6))[0]), "the flag should change the image"
    for build in (0, BUILD_STREAMS_ONLY):
        img, st = render(vpt, sc, P, [frames], build_flags=build)
        print("closest %d (oracle %d), shadow %d (oracle %d)" % (st["closest_rays"], ctr["closest"], st["shadow_rays"], ctr["shadow"]))
        spilled(st, st["shadow_rays"] > 0)                  # (without NEE there is nothing for the second stream's kernels to trace)
        assert (st["finish_paths"] > 0) == (build == 0)
        assert np.array_equal(img, ref), (flags, build)
        assert st["samples"] == W * H * frames == ctr["samples"]
        assert st["closest_rays"] == ctr["closest"], (st["closest_rays"], ctr["closest"])
        assert st["shadow_rays"] <= ctr["shadow"]
        if flags != "no_mis":
            assert st["shadow_rays"] > 0


def test_two_contexts_alive_at_once(vpt, scene, reference):
    """Two contexts render the scene in alternating batches: each owns its regions, neither sees the other's entries."""
    P = vpt.default_params(max_depth=6)
    ref, ctr = reference(scene, 4, P)
    ctxs = [vpt.PathTracer(W, H, frames_in_flight=2) for _ in range(2)]
    for g in ctxs:
        g.set_scene(scene); g.set_params(P)
    for n in (1, 2, 1):
        for g in ctxs:
            g.render(n)
    for g in ctxs:
        st = g.stats()
        spilled(st, True)
        assert np.array_equal(g.radiance(), ref)
        same_rays(st, ctr, 4)
    for g in ctxs:
        g.close()
