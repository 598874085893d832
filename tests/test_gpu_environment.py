"""vpt_set_environment: the environment map of an installed scene is replaced without a rebuild, and the context is the one vpt_set_scene
would have produced from the same description with that map.  The same calls go to a vpt.PathTracer and — the Lockstep idea of
tests/test_gpu_transitions.py — to an oracle.Oracle; a swap on the oracle's side is a NEW Oracle built from a copy of the scene with
.env replaced, carrying the state the context keeps (parameters, volumes, atmosphere, material edits, camera).  Images compare with
np.array_equal.  Before a pair of environments is relied on, the oracle's two images are shown to differ: in a scene where no ray reaches
the sky every test here would pass whatever the swap did."""
import copy

import numpy as np
import pytest

from test_environment_cpu import swap_environments

pytestmark = pytest.mark.gpu
W, H, FRAMES = 96, 54, 3
NO_SCENE, INVALID = "VPT_ERR_NO_SCENE", "VPT_ERR_INVALID_ARGUMENT"
FUSED, STAGED = 1, 2                                        # include/vpt.h VPT_PIPELINE_*
FLAG_LOCAL_HITS = 256


def fog(vpt):
    return vpt.volume(corner_min=(-5.0, -10.5, -5.0), corner_max=(5.0, -0.5, 5.0), color=(0.9, 0.85, 0.8), density=0.12, anisotropy=0.3)


class Swapper:
    """One context and the oracle's restatement of what it holds."""

    def __init__(self, vpt, oracle, sc, w=W, h=H, P=None, **cfg):
        self.vpt, self.oracle, self.w, self.h = vpt, oracle, w, h
        self.sc = copy.deepcopy(sc)
        self.P = P if P is not None else vpt.default_params(max_depth=6)
        self.vols, self.atm, self.edits, self.camera = [], None, {}, None
        self.g = vpt.PathTracer(w, h, **cfg)
        self.g.set_scene(self.sc); self.g.set_params(self.P)

    def close(self):
        self.g.close()

    def set_volumes(self, vols):
        self.vols = list(vols); self.g.set_volumes(self.vols)

    def set_atmosphere(self, atm):
        self.atm = atm; self.g.set_atmosphere(atm)

    def set_params(self, P):
        self.P = P; self.g.set_params(P)

    def set_material(self, i, **kw):
        m = self.g.get_material(i)
        for k, v in kw.items():
            getattr(m, k)[:] = v
        self.g.set_material(i, m); self.edits[i] = m

    def set_camera(self, view_inverse, projection_inverse):
        self.camera = (view_inverse, projection_inverse); self.g.set_camera(view_inverse, projection_inverse)

    def swap(self, env):
        self.g.set_environment(env)
        self.sc.env = np.array(env, np.float32)
        assert self.g.stats()["frames"] == 0, "the swap did not reset the accumulation"

    def reference(self, frames, rows=slice(None)):
        """(image, closest rays) of a new Oracle holding everything this context holds."""
        o = self.oracle.Oracle(self.sc, self.w, self.h)
        try:
            o.set_params(self.P); o.set_volumes(self.vols); o.set_atmosphere(self.atm)
            for i, m in self.edits.items():
                o.set_material(i, m)
            if self.camera:
                o.set_camera(*self.camera)
            o.render(frames)
            return o.radiance()[rows], o.counters()["closest"]
        finally:
            o.close()

    def render_and_compare(self, frames=FRAMES, what=""):
        self.g.reset_stats()
        self.g.render(frames)
        img, st = self.g.radiance(), self.g.stats()
        ref, closest = self.reference(frames)
        diff = (img != ref).any(axis=2)
        assert not diff.any(), "%s: %d pixels differ from the oracle" % (what, int(diff.sum()))
        assert st["frames"] == frames, (what, st["frames"])
        if not self.vols and self.atm is None:              # (surfaces: the suite holds the closest-ray counts equal, tests/test_gpu_transitions.py)
            assert st["closest_rays"] == closest, (what, st["closest_rays"], closest)
        return img, st


def walk(vpt, S):
    """black -> sky 64x32 -> constant 48x20 -> black, three frames and parity after every swap; the images, which must differ from
    one step to the next (else the scene shows no sky and the walk proves nothing), and the statistics."""
    envs = swap_environments(vpt)
    out = []
    for name in ("black_1x1", "sky_64x32", "constant_48x20", "black_1x1"):
        S.swap(envs[name])
        out.append(S.render_and_compare(what=name))
    for (a, _), (b, _) in zip(out, out[1:]):
        assert not np.array_equal(a, b), "two environments give the same image: no ray of this scene reaches the sky"
    assert np.array_equal(out[-1][0], out[0][0]), "back on the black environment the image is not the first step's"
    return out


@pytest.mark.parametrize("pipeline", [0, FUSED], ids=["auto", "fused"])
def test_walk_on_the_lds_scene(vpt, oracle, scenes, pipeline):
    """cornell_box: whole-path launches under AUTO, k_bounce under FUSED; black <-> lit flips the PLAIN / general instantiation both ways."""
    S = Swapper(vpt, oracle, scenes("cornell_box"), pipeline=pipeline)
    try:
        out = walk(vpt, S)
        for _, st in out:
            assert st["kernel_launches"]["primary"] > 0 and st["kernel_launches"]["extend"] == 0
    finally:
        S.close()


@pytest.mark.parametrize("pipeline", [0, STAGED], ids=["auto", "staged"])
def test_walk_on_the_streams_without_a_rebuild(vpt, oracle, scenes, pipeline):
    """viking_room (BVH in memory).  A rebuild would change the two wall-clock doubles of vpt_set_scene: that they, the tree's counts and the
    spill counters are EXACTLY what vpt_set_scene left shows, without a timing threshold, that none happened."""
    S = Swapper(vpt, oracle, scenes("viking_room"), pipeline=pipeline)
    keys = ("bvh_build_ms", "set_scene_ms", "bvh_nodes", "bvh_triangles", "stack_spills")
    try:
        st0 = S.g.stats()
        assert st0["set_scene_ms"] > 0 and st0["bvh_build_ms"] > 0 and st0["set_environment_ms"] == 0
        envs = swap_environments(vpt)
        imgs = []
        for name in ("black_1x1", "sky_64x32", "constant_48x20", "black_1x1"):
            S.swap(envs[name])
            after_swap = S.g.stats()
            img, st = S.render_and_compare(what=name)
            imgs.append(img)
            for s in (after_swap, st):
                assert {k: s[k] for k in keys} == {k: st0[k] for k in keys}, name
                assert s["set_environment_ms"] > 0
            assert st["kernel_launches"]["extend"] > 0 and st["kernel_launches"]["join"] > 0, "the streams should run this scene"
        for a, b in zip(imgs, imgs[1:]):
            assert not np.array_equal(a, b), "two environments give the same image: no ray of this scene reaches the sky"
        assert np.array_equal(imgs[-1], imgs[0])
    finally:
        S.close()


@pytest.mark.parametrize("medium", ["surfaces", "fog", "atmosphere"])
def test_twin_of_a_context_that_got_the_environment_with_its_scene(vpt, oracle, scenes, medium):
    """A: set_scene(S with env B).  B: set_scene(S), then set_environment(B).  Equal images — through fog (sky NEE through media asks
    sample_env for a direction even where the map is black) and under an atmosphere, where the map is unused: the swap leaves the image as
    it was and still resets the accumulation."""
    sc = scenes("cornell_box")
    env = swap_environments(vpt)["sky_64x32"]
    P = vpt.default_params(max_depth=6, sky_altitude=-40.0, sky_azimuth=120.0) if medium == "atmosphere" else vpt.default_params(max_depth=6)

    def install(S):
        if medium == "fog":
            S.set_volumes([fog(vpt)])
        if medium == "atmosphere":
            S.set_atmosphere(vpt.atmosphere())

    with_env = copy.deepcopy(sc); with_env.env = env
    A = Swapper(vpt, oracle, with_env, P=P)
    B = Swapper(vpt, oracle, sc, P=P)
    try:
        install(A); install(B)
        before, _ = B.render_and_compare(what="own environment")
        B.swap(env)
        b, _ = B.render_and_compare(what="swapped")
        a, _ = A.render_and_compare(what="installed with the scene")
        assert np.array_equal(a, b)
        if medium == "atmosphere":
            assert np.array_equal(b, before), "under an atmosphere the environment map is unused"
            assert b[..., :3].any()
        else:
            assert not np.array_equal(b, before), "no ray of this scene reaches the sky"
        # and the other direction: back to black with the medium installed
        B.swap(np.zeros((1, 1, 4), np.float32))
        c, _ = B.render_and_compare(what="back to black")
        assert np.array_equal(c, before)
    finally:
        A.close(); B.close()


def test_state_set_before_the_swap_survives_it(vpt, oracle, scenes):
    sc = scenes("cornell_box")
    P = vpt.default_params(max_depth=6, sky_azimuth=70.0, sky_altitude=-25.0, sky_intensity=2.5)
    P.flags |= FLAG_LOCAL_HITS
    S = Swapper(vpt, oracle, sc, P=P)
    try:
        S.set_material(0, emissive_color=(3.0, 2.0, 1.0), base_color=(0.2, 0.7, 0.4))
        vi = np.array(sc.view_inverse, np.float32).copy()
        vi[:3, 3] += np.float32(0.25) * vi[:3, 0] + np.float32(0.1) * vi[:3, 1]          # a moved camera: a quarter unit right, a tenth up
        S.set_camera(vi, sc.projection_inverse(W / H))
        before, st = S.render_and_compare(what="before the swap")
        assert st["emissive_mesh_count"] > 0
        S.swap(swap_environments(vpt)["sky_64x32"])
        after, st = S.render_and_compare(what="after the swap")
        assert not np.array_equal(after, before), "no ray of this scene reaches the sky"
        m = S.g.get_material(0)
        assert tuple(m.emissive_color) == (3.0, 2.0, 1.0)
        # each piece of state is one the image depends on: an oracle without it gives another image
        for drop in ("params", "material", "camera"):
            T = copy.copy(S)
            if drop == "params":
                T.P = vpt.default_params(max_depth=6)
            if drop == "material":
                T.edits = {}
            if drop == "camera":
                T.camera = None
            assert not np.array_equal(T.reference(FRAMES)[0], after), "the image does not depend on the %s" % drop
    finally:
        S.close()


@pytest.mark.parametrize("env_name", ["sky_64x32", "constant_48x20"], ids=["same_dimensions", "other_dimensions"])
def test_swap_behind_asynchronous_frames_replayed_from_a_graph(vpt, oracle, scenes, env_name):
    """One-frame render_async + postprocess_device batches until they replay from a captured hipGraph (which bakes the tables' addresses
    in), a swap with work still in flight and no wait, three more asynchronous frames."""
    sc = copy.deepcopy(scenes("cornell_box"))
    sc.env = vpt.scenes.constant_env((0.9, 0.4, 0.2), w=64, h=32)
    S = Swapper(vpt, oracle, sc, frames_in_flight=1, pipeline=FUSED)
    g = S.g
    try:
        for _ in range(12):
            g.render_async(1); g.postprocess_device()
            if g.stats()["graph_launches"] > 0:             # (drains)
                break
        assert g.stats()["graph_launches"] > 0, "the 1-frame batches were not replayed from a captured graph"
        old, _ = S.reference(FRAMES)
        g.render_async(1); g.postprocess_device()            # in flight when the swap arrives
        S.swap(swap_environments(vpt)[env_name])
        replays = g.stats()["graph_launches"]
        for _ in range(FRAMES):
            g.render_async(1); g.postprocess_device()
        g.wait()
        ref, _ = S.reference(FRAMES)
        assert not np.array_equal(ref, old), "no ray of this scene reaches the sky"
        assert np.array_equal(g.radiance(), ref)
        ref8, _ = oracle.postprocess(ref, vpt.default_post_params())
        assert np.array_equal(g.output_to_host(), ref8)
        st = g.stats()
        assert st["frames"] == FRAMES
        assert st["graph_launches"] <= replays + FRAMES - 1, "a frame after the swap replayed a graph captured before it"
    finally:
        S.close()


def test_rejections_leave_the_installed_environment(vpt, oracle, scenes):
    lib = vpt.load_library()
    sky = swap_environments(vpt)["sky_64x32"]
    g = vpt.PathTracer(W, H)
    try:
        with pytest.raises(vpt.VptError, match=NO_SCENE + " no scene"):
            g.set_environment(sky)
    finally:
        g.close()
    sc = copy.deepcopy(scenes("cornell_box"))
    sc.env = swap_environments(vpt)["constant_48x20"]
    S = Swapper(vpt, oracle, sc)
    try:
        S.g.render(2)
        for data, w, h in ((None, 64, 32), (sky.ctypes.data, 0, 32), (sky.ctypes.data, 64, 0)):
            assert lib.vpt_set_environment(S.g.ctx, data, w, h) == -1
            assert lib.vpt_last_error(S.g.ctx) == b"incomplete environment map"
        with pytest.raises(vpt.VptError, match=INVALID):
            S.g.set_environment(np.zeros((0, 4, 4), np.float32))
        assert S.g.stats()["frames"] == 2, "a rejected call reset the accumulation"
        S.g.reset()
        img, st = S.render_and_compare(what="after the rejected calls")
        assert st["set_environment_ms"] == 0
        S.sc.env = sky
        assert not np.array_equal(S.reference(FRAMES)[0], img), "no ray of this scene reaches the sky"
    finally:
        S.close()


def test_two_row_shards_each_swap(vpt, oracle, scenes):
    """shard_count = 2 (rows y % 2 == k on context k): each context swaps its own replica, and each shard's rows are the oracle's."""
    import ctypes as C
    sc = scenes("cornell_box")
    shards = [Swapper(vpt, oracle, sc, shard_rank=k, shard_count=2) for k in range(2)]
    hip = C.CDLL("libamdhip64.so")
    n = shards[0].g.shard_floats()
    assert n == len(range(0, H, 2)) * W * 4
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), n * 4 * 2) == 0
    try:
        refs = []
        for name in ("sky_64x32", "constant_48x20"):
            env = swap_environments(vpt)[name]
            for k, S in enumerate(shards):
                S.swap(env)
                S.g.render(FRAMES)
                S.g.shard_to_device(C.c_void_p(buf.value + k * n * 4))
            ref, _ = shards[0].reference(FRAMES)
            refs.append(ref)
            rows = np.empty((2, n // (4 * W), W, 4), np.float32)
            assert hip.hipMemcpy(C.c_void_p(rows.ctypes.data), buf, n * 4 * 2, 2) == 0       # hipMemcpyDeviceToHost
            for k in range(2):
                assert np.array_equal(rows[k][:len(range(k, H, 2))], ref[k::2]), (name, "shard %d" % k)
            shards[0].g.assemble_shards(buf, 2)
            assert np.array_equal(shards[0].g.radiance(), ref), name
        assert not np.array_equal(refs[0], refs[1]), "no ray of this scene reaches the sky"
    finally:
        hip.hipFree(buf)
        for S in shards:
            S.close()
