"""vpt_set_instance_transforms: instances of an installed scene move by a BVH refit on the device — no tree build, no geometry upload — and the
context renders what vpt_set_scene would have installed from the moved description.  The same calls go to a vpt.PathTracer and to a NEW
oracle.Oracle built from a copy of the scene with the instance matrices replaced (tests/test_gpu_environment.py's Swapper, with a move where it
has a swap).  Images compare with np.array_equal, closest-ray counts too where there are no media.  Before a walk is relied on, the ORACLE's
images are shown to differ from step to step: a move nobody sees would pass whatever the refit did.
The refit's arithmetic without a device: tests/test_refit_cpu.py."""
import copy
import ctypes as C

import numpy as np
import pytest

import refit_moves as RM
import whole_spill_scene
from test_gpu_environment import FRAMES, FUSED, H, STAGED, W, Swapper, fog
from test_gpu_spill_schedules import hit_rays
from test_stack_bound_cpu import floor_to_light_rays, random_rays

pytestmark = pytest.mark.gpu
FLAG_LOCAL_HITS = 256
BUILD_SBVH = 1
NO_SCENE, INVALID, UNSUPPORTED = "VPT_ERR_NO_SCENE", "VPT_ERR_INVALID_ARGUMENT", "VPT_ERR_UNSUPPORTED"


class Mover(Swapper):
    def __init__(self, vpt, oracle, sc, **kw):
        super().__init__(vpt, oracle, sc, **kw)
        self.original = [np.array(x, np.float32) for _, _, x in self.sc.instances]

    def move(self, moves):
        """{instance: world transform}, applied to the ORIGINAL matrices; instances not named go back to theirs.  One call per run of consecutive
        instances whose matrix changes, so partial ranges and first > 0 are what the walks use."""
        target = RM.moved_matrices(RM.with_matrices(self.sc, dict(enumerate(self.original))), moves)
        new = [np.asarray(target.get(i, self.original[i]), np.float32) for i in range(len(self.original))]
        changed = [i for i in range(len(new)) if not np.array_equal(new[i], self.sc.instances[i][2])]
        runs = []
        for i in changed:
            if runs and runs[-1][-1] == i - 1:
                runs[-1].append(i)
            else:
                runs.append([i])
        for run in runs:
            self.g.set_instance_transforms(run[0], [new[i] for i in run])
            assert self.g.stats()["frames"] == 0, "the move did not reset the accumulation"
        self.sc = RM.with_matrices(self.sc, dict(enumerate(new)))
        return len(runs)


def walk(S, steps):
    """A render with parity after every step; the oracle's images differ from one step to the next; back at the start the image is the first."""
    st0 = S.g.stats()
    assert st0["set_scene_ms"] > 0 and st0["bvh_build_ms"] > 0 and st0["set_transforms_ms"] == 0
    out, refs = [], []
    for name, moves in steps:
        moved = S.move(moves)
        refs.append(S.reference(FRAMES)[0])
        if len(refs) > 1:
            assert not np.array_equal(refs[-1], refs[-2]), "%s: the oracle's image did not change: the walk proves nothing" % name
        img, st = S.render_and_compare(what=name)
        out.append(img)
        for k in ("set_scene_ms", "bvh_build_ms", "bvh_nodes", "bvh_triangles"):
            assert st[k] == st0[k], (name, k)                                       # to the bit: nothing was rebuilt
        assert (st["set_transforms_ms"] > 0) == (moved > 0 or len(out) > 1), name
    for a, b in zip(out, out[1:]):
        assert not np.array_equal(a, b)
    assert np.array_equal(out[-1], out[0]), "back on the original matrices the image is not the first step's"
    return out


CORNELL_STEPS = [("original", {}), ("wall", RM.CORNELL_WALL), ("lamp", RM.CORNELL_LAMP), ("original again", {})]
GLASS_STEPS = [("original", {}), ("sphere", RM.GLASS_SPHERE), ("lamp and sphere", RM.GLASS_LAMP_AND_SPHERE), ("original again", {})]
CHAIN_STEPS = [("original", {}), ("tilt", RM.CHAIN_TILT), ("grows", RM.CHAIN_GROWS), ("original again", {})]


@pytest.mark.parametrize("pipeline", [0, FUSED], ids=["auto", "fused"])
def test_walk_on_the_lds_scene(vpt, oracle, scenes, pipeline):
    """cornell_box rides in LDS (wide nodes are refitted too): whole-path launches under AUTO, k_bounce under FUSED.  The back wall is translated and
    rotated, the lamp (instance 5, emissive: the light tables follow) lowered and scaled, then everything goes back."""
    S = Mover(vpt, oracle, scenes("cornell_box"), pipeline=pipeline)
    try:
        assert S.g.stats()["bvh_node_bytes"] == 128
        walk(S, CORNELL_STEPS)
        st = S.g.stats()
        assert st["kernel_launches"]["primary"] > 0 and st["kernel_launches"]["extend"] == 0
    finally:
        S.close()


@pytest.mark.parametrize("local_hits", [True, False], ids=["local_hits", "default_flags"])
@pytest.mark.parametrize("pipeline", [0, STAGED], ids=["auto", "staged"])
@pytest.mark.parametrize("which", ["glass", "chain84"])
def test_walk_in_memory(vpt, oracle, scenes, which, pipeline, local_hits):
    sc, steps = (scenes("cornell_box_glass"), GLASS_STEPS) if which == "glass" else (whole_spill_scene.memory_chain_scene(vpt), CHAIN_STEPS)
    P = vpt.default_params(max_depth=6)
    if local_hits:
        P.flags |= FLAG_LOCAL_HITS
    S = Mover(vpt, oracle, sc, P=P, pipeline=pipeline)
    try:
        assert S.g.stats()["bvh_node_bytes"] == 64
        walk(S, steps)
    finally:
        S.close()


@pytest.mark.parametrize("which", ["glass", "chain84"])
def test_walk_on_a_spatial_split_tree(vpt, oracle, scenes, which):
    """VPT_BUILD_SBVH: a clipped reference is refitted with the bounds of its whole triangle; with VPT_FLAG_LOCAL_HITS the image is the oracle's."""
    sc, steps = (scenes("cornell_box_glass"), GLASS_STEPS) if which == "glass" else (whole_spill_scene.memory_chain_scene(vpt), CHAIN_STEPS)
    P = vpt.default_params(max_depth=6)
    P.flags |= FLAG_LOCAL_HITS
    S = Mover(vpt, oracle, sc, P=P, build_flags=BUILD_SBVH)
    try:
        assert S.g.stats()["build_flags"] & BUILD_SBVH
        walk(S, steps)
    finally:
        S.close()


def test_equals_a_context_given_the_moved_description(vpt, oracle, scenes):
    sc = scenes("cornell_box_glass")
    P = vpt.default_params(max_depth=6)
    P.flags |= FLAG_LOCAL_HITS
    A = Mover(vpt, oracle, sc, P=P)
    try:
        A.move(RM.GLASS_LAMP_AND_SPHERE)
        B = Swapper(vpt, oracle, A.sc, P=P)          # vpt_set_scene of the moved description
        try:
            a, sa = A.render_and_compare(what="moved")
            b, sb = B.render_and_compare(what="installed moved")
            assert np.array_equal(a, b)
            assert (sa["closest_rays"], sa["shadow_rays"]) == (sb["closest_rays"], sb["shadow_rays"])
            assert sa["emissive_triangle_count"] == sb["emissive_triangle_count"] > 0
        finally:
            B.close()
    finally:
        A.close()


def test_trace_rays_after_a_move_against_brute_force(vpt, oracle):
    """The move of tests/test_refit_cpu.py whose extent grows (the stack leaves the floor's outline): the padding and scene_extent follow."""
    sc = whole_spill_scene.memory_chain_scene(vpt)
    moved = RM.with_matrices(sc, RM.moved_matrices(sc, RM.CHAIN_GROWS))
    rng = np.random.default_rng(33)
    o1, d1 = floor_to_light_rays(rng, 3000)
    o2, d2 = random_rays(rng, whole_spill_scene.world_triangles(moved), 3000)
    rays = np.concatenate([hit_rays(o1, d1, 0.01, 100000.0), hit_rays(o2, d2, 0.01, 100000.0)])
    assert len(rays) == 6000
    o = oracle.Oracle(moved, 8, 8)
    o.set_brute_force(True)
    ref = o.trace_rays(rays)
    o.close()
    o = oracle.Oracle(sc, 8, 8)
    o.set_brute_force(True)
    unmoved = o.trace_rays(rays)
    o.close()
    assert not np.array_equal(ref["t"], unmoved["t"]), "the move changes no hit of these rays"
    g = vpt.PathTracer(8, 8)
    try:
        g.set_scene(sc)
        g.set_instance_transforms(1, [moved.instances[1][2]])
        got = g.trace_rays(rays)
    finally:
        g.close()
    for k in ("t", "u", "v", "primitive", "instance"):
        assert np.array_equal(got[k], ref[k]), k
    hit = ref["t"] >= 0
    assert (ref["instance"][hit] == 1).any() and (~hit).any()


@pytest.mark.parametrize("medium", ["fog", "atmosphere"])
def test_media_state_survives_a_move(vpt, oracle, scenes, medium):
    P = vpt.default_params(max_depth=6, sky_altitude=-40.0, sky_azimuth=120.0) if medium == "atmosphere" else vpt.default_params(max_depth=6)
    S = Mover(vpt, oracle, scenes("cornell_box"), P=P)
    try:
        if medium == "fog":
            S.set_volumes([fog(vpt)])
        else:
            S.set_atmosphere(vpt.atmosphere())
        before, _ = S.render_and_compare(what="before")
        S.move(RM.CORNELL_LAMP)
        after, _ = S.render_and_compare(what="moved under " + medium)
        assert not np.array_equal(after, before)
        T = copy.copy(S)
        T.vols, T.atm = [], None
        assert not np.array_equal(T.reference(FRAMES)[0], after), "the image does not depend on the medium"
    finally:
        S.close()


def test_move_behind_asynchronous_frames_replayed_from_a_graph(vpt, oracle, scenes):
    S = Mover(vpt, oracle, scenes("cornell_box"), frames_in_flight=1, pipeline=FUSED)
    g = S.g
    try:
        for _ in range(12):
            g.render_async(1); g.postprocess_device()
            if g.stats()["graph_launches"] > 0:             # (drains)
                break
        assert g.stats()["graph_launches"] > 0, "the 1-frame batches were not replayed from a captured graph"
        old, _ = S.reference(FRAMES)
        g.render_async(1); g.postprocess_device()            # in flight when the move arrives
        S.move(RM.CORNELL_LAMP)
        replays = g.stats()["graph_launches"]
        for _ in range(FRAMES):
            g.render_async(1); g.postprocess_device()
        g.wait()
        ref, _ = S.reference(FRAMES)
        assert not np.array_equal(ref, old)
        assert np.array_equal(g.radiance(), ref)
        st = g.stats()
        assert st["frames"] == FRAMES
        assert st["graph_launches"] <= replays + FRAMES - 1, "a frame after the move replayed a graph captured before it"
    finally:
        S.close()


def test_partial_range_leaves_the_other_instances(vpt, oracle, scenes):
    """first = 2, count = 1: the back wall alone; every other instance (the emissive lamp included) keeps its matrix."""
    S = Mover(vpt, oracle, scenes("cornell_box"))
    try:
        before, _ = S.render_and_compare(what="before")
        m = RM.moved_matrices(S.sc, RM.CORNELL_WALL)[2]
        S.g.set_instance_transforms(2, [m])
        S.sc = RM.with_matrices(S.sc, {2: m})
        after, st = S.render_and_compare(what="instance 2 alone")
        assert not np.array_equal(after, before)
        assert st["emissive_mesh_count"] == 1
    finally:
        S.close()


def test_rejections_leave_the_installed_transforms(vpt, oracle, scenes):
    lib = vpt.load_library()
    one = [np.eye(4, dtype=np.float32)]
    g = vpt.PathTracer(W, H)
    try:
        with pytest.raises(vpt.VptError, match=NO_SCENE + " no scene"):
            g.set_instance_transforms(0, one)
    finally:
        g.close()
    S = Mover(vpt, oracle, scenes("cornell_box"))
    try:
        unmoved, _ = S.render_and_compare(what="unmoved")
        flat = (C.c_float * 16)(*vpt.scenes.colmajor(RM.moved_matrices(S.sc, {2: RM.scale(1.0, 0.0, 0.0)})[2]))
        rows = [((0, 1, None), -1, b"no instance transforms"), ((6, 1, flat), -1, b"instance range out of bounds"), ((2, 5, flat), -1, b"instance range out of bounds"),
                ((0xffffffff, 2, flat), -1, b"instance range out of bounds"), ((2, 1, flat), -6, None)]
        for (first, count, data), code, msg in rows:
            S.g.reset(); S.g.render(2)
            assert lib.vpt_set_instance_transforms(S.g.ctx, first, count, data) == code, (first, count)
            if msg is not None:
                assert lib.vpt_last_error(S.g.ctx) == msg
            else:
                assert b"vpt_set_scene" in lib.vpt_last_error(S.g.ctx)              # the sliver rule says where to go
            assert S.g.stats()["frames"] == 2, "a rejected call reset the accumulation"
            S.g.reset()
            img, st = S.render_and_compare(what="after a rejected call")
            assert np.array_equal(img, unmoved)
            assert st["set_transforms_ms"] == 0
        with pytest.raises(vpt.VptError, match=UNSUPPORTED):
            S.g.set_instance_transforms(2, [RM.moved_matrices(S.sc, {2: RM.scale(1.0, 0.0, 0.0)})[2]])
        S.g.reset(); S.g.render(2)
        assert lib.vpt_set_instance_transforms(S.g.ctx, 3, 0, None) == 0             # nothing to do: not even a reset
        assert S.g.stats()["frames"] == 2
        S.g.reset()
        S.move(RM.CORNELL_WALL)                                                       # and the context keeps working
        moved, _ = S.render_and_compare(what="a move after the rejections")
        assert not np.array_equal(moved, unmoved)
    finally:
        S.close()


def test_two_row_shards_each_move(vpt, oracle, scenes):
    """shard_count = 2 (rows y % 2 == k on context k): each context moves its own replica, and each shard's rows are the oracle's."""
    sc = scenes("cornell_box")
    shards = [Mover(vpt, oracle, sc, shard_rank=k, shard_count=2) for k in range(2)]
    hip = C.CDLL("libamdhip64.so")
    n = shards[0].g.shard_floats()
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), n * 4 * 2) == 0
    try:
        refs = []
        for moves in (RM.CORNELL_WALL, RM.CORNELL_LAMP):
            for k, S in enumerate(shards):
                S.move(moves)
                S.g.render(FRAMES)
                S.g.shard_to_device(C.c_void_p(buf.value + k * n * 4))
            ref, _ = shards[0].reference(FRAMES)
            refs.append(ref)
            rows = np.empty((2, n // (4 * W), W, 4), np.float32)
            assert hip.hipMemcpy(C.c_void_p(rows.ctypes.data), buf, n * 4 * 2, 2) == 0       # hipMemcpyDeviceToHost
            for k in range(2):
                assert np.array_equal(rows[k][:len(range(k, H, 2))], ref[k::2]), "shard %d" % k
            shards[0].g.assemble_shards(buf, 2)
            assert np.array_equal(shards[0].g.radiance(), ref)
        assert not np.array_equal(refs[0], refs[1])
    finally:
        hip.hipFree(buf)
        for S in shards:
            S.close()
