"""The ray-stream traversal kernels that trace every ray of the stream pipelines, held to the oracle's brute force ray by ray: k_trace_vote (the
closest-hit search: vote.hpp's node and triangle steps, LaneStack spills, a wave-level scheduler with static first entries, cursor chunks, ray
replacement, holes, the validating re-trace) and k_trace_shadow<sky> / <light> (the staged tree top, the light predicate).  vpt_trace_rays shares
none of that — it is k_first_hit's per-lane loop — so the ray classes of tests/test_gpu_traversal.py, test_gpu_edge_cases.py and
test_gpu_material_textures.py (tests/trace_ray_sets.py holds them for both) reach these kernels here, through the laboratory's hooks:
vpt_lab_trace with VPT_TRACE_VOTE and the default vote parameter launches the product's instantiations of k_trace_vote, vpt_lab_trace_shadow
calls the product's launch_trace_shadow.  tests/gpu_trace_stream_run.py makes every launch in one process of its own (VPT_LAB=1); the tests compare
what it left with references computed here.  Every comparison is bit-exact: (t, u, v, primitive, instance) under np.array_equal, visibility bytes
equal.  k_finish's own loops over the vote steps and the LDS-tree searches of k_whole / k_bounce have no per-ray hook and stay with the image tests."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import trace_ray_sets as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("t", "u", "v", "primitive", "instance")
RULES = ("default", "strict")   # VPT_FLAG_LOCAL_HITS off / on: the product and the validating instantiations, the reference with the same rule


@pytest.fixture(scope="module")
def runs(vpt, oracle, tmp_path_factory):
    print(json.dumps(T.check_conditions(vpt, oracle)))   # the ray sets are what the tests need them to be, before the GPU is involved
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    vpt.build(lab=True)
    out = str(tmp_path_factory.mktemp("trace_stream") / "runs.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_trace_stream_run.py"), out, str(cus)], env=dict(os.environ, VPT_LAB="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    z = np.load(out)
    info = json.loads(str(z["info"]))
    assert info["compute_units"] == cus
    return z, info


@pytest.fixture(scope="module")
def big(vpt, oracle, runs):
    """The scheduling tests' rays — beyond the static part of a persistent grid of 8 blocks per CU — and their closest hits."""
    sizes = T.beyond_static_sizes(runs[1]["compute_units"])
    sc, _ = T.load(vpt, "random_glass")
    rays = T.random_rays(sizes[1], 5, 8.0)
    return sizes, T.brute_force(vpt, oracle, sc, rays)


def ran(info, group):
    """The runner's group of launches went through: the library refused none of them (a launch that writes beyond its ray set is refused)."""
    assert group not in info["errors"], info["errors"][group]


def assert_hits(got, ref, what, only=None):
    for f in FIELDS:
        a, b = (got[f], ref[f]) if only is None else (got[f][only], ref[f][only])
        assert np.array_equal(a, b), "%s: %s differs for %d of %d rays" % (what, f, int((a != b).sum()), len(a))


def assert_holes(got, full, what):
    """A launch over the hole mask: a hole's result stays the 0xAA fill, every other ray keeps the result it has without the mask."""
    hole = T.hole_mask(len(full)) != 0
    assert hole.any() or len(full) < T.HOLE_EVERY
    raw = np.frombuffer(got.tobytes(), np.uint8).reshape(len(got), -1)
    assert (raw[hole] == 0xAA).all(), what
    assert raw[~hole].tobytes() == np.frombuffer(full.tobytes(), np.uint8).reshape(len(full), -1)[~hole].tobytes(), what


@pytest.mark.parametrize("name", T.SETS)
def test_closest_hits_equal_brute_force_in_every_instantiation(vpt, oracle, runs, name):
    """k_trace_vote's product, counting, validating and validating + counting instantiations on every shared ray set."""
    z, info = runs
    ran(info, "vote_" + name)
    rec = info["vote_" + name]
    for rule in RULES:
        ref = T.reference(vpt, oracle, name, strict=rule == "strict")
        assert_hits(z["vote_%s_%s" % (name, rule)], ref, "%s, %s" % (name, rule))
        assert rec[rule]["counting_same"], "the counting instantiation returns other hits (%s)" % rule
        assert rec[rule]["visits"][0] > 0 and rec[rule]["visits"][1] > 0, rec[rule]["visits"]
    hit = T.reference(vpt, oracle, name)["t"] >= 0
    assert hit.any() and (~hit).any() or name == "chain"   # (from the chain scene's floor every ray towards the light ends on a sheet or the light)
    if name == "chain":   # the searches went deeper than the LDS rows: the spill path did run
        assert rec["stack_spills"][0] == [0, 0] and rec["stack_spills"][1][0] > 0, rec["stack_spills"]


@pytest.mark.parametrize("name", T.SETS)
def test_holes_keep_their_sentinel_and_change_no_other_ray(runs, name):
    z, info = runs
    ran(info, "vote_" + name)
    assert_holes(z["vote_%s_holes" % name], z["vote_%s_default" % name], name)


@pytest.mark.parametrize("name", ["axis_aligned", "far_30", "far_1000"])
def test_any_hit_search_stops_exactly_where_a_closest_hit_exists(vpt, oracle, runs, name):
    """The laboratory's any-hit k_trace_vote shares vote_node_step<true> and the staged tree top with the shadow kernels: t = 1 where brute force
    finds a hit in the set's window, -1 elsewhere."""
    ran(runs[1], "vote_" + name)
    ref = T.reference(vpt, oracle, name)
    want = np.where(ref["t"] >= 0, np.float32(1.0), np.float32(-1.0))
    got = runs[0]["any_" + name]
    assert np.array_equal(got, want), "%d of %d rays" % (int((got != want).sum()), len(want))


def sizes(runs):
    return T.SCHEDULE_SIZES + T.beyond_static_sizes(runs[1]["compute_units"])


@pytest.mark.parametrize("which", range(len(T.SCHEDULE_SIZES) + 2))
def test_results_and_visits_do_not_depend_on_the_schedule(runs, big, which):
    """n rays as they lie, reversed and permuted: the same hits per ray, and the same {nodes, triangles} totals — a ray's visits do not depend on
    the lane or the chunk that served it.  The last two sizes lie beyond the grid's static part: the cursor and fetch_chunk run, and the very
    last one ends inside a chunk.  (The library refuses a launch that writes beyond its set: the buffers end in a guard, include/vpt_lab.h.)"""
    z, info = runs
    n = sizes(runs)[which]
    ran(info, "sched_%d" % n)
    rec = info["sched_%d" % n]
    print(n, {o: rec[o]["visits"] for o in T.orders(1)})
    assert_hits(z["sched_%d" % n], big[1][:n], "%d rays" % n)
    for o in T.orders(1):
        assert rec[o]["same_as_identity"], (n, o)
        assert rec[o]["counting_same"], (n, o)
        assert rec[o]["visits"] == rec["identity"]["visits"] and rec[o]["visits"][0] > 0, (n, o, rec[o]["visits"], rec["identity"]["visits"])
    if n >= 4097:
        assert_holes(z["sched_%d_holes" % n], z["sched_%d" % n], "%d rays" % n)
        assert rec["holes_reversed_same"], "holes named by a visiting order"


def test_the_largest_sizes_leave_the_static_part(runs, big):
    cus = runs[1]["compute_units"]
    assert big[0] == (3072 * cus, 3072 * cus + T.RAGGED) and big[0][0] > 2048 * cus >= 4097
    assert big[0][1] % 64 != 0   # fetch_chunk's chunks and the static part are multiples of 64: the last chunk of this size is cut short


@pytest.mark.parametrize("name", ["random_glass", "random_viking"])
def test_spatial_split_tree(vpt, oracle, runs, name):
    """VPT_BUILD_SBVH: leaves share triangles, the same hits (ties in t go to the smaller global id)."""
    z, info = runs
    ran(info, "sbvh_" + name)
    assert info["sbvh_" + name]["build_flags"] == 1 and info["sbvh_" + name]["bvh_triangles"] >= T.load(vpt, name)[0].triangle_count()
    assert_hits(z["sbvh_" + name], T.reference(vpt, oracle, name), name)
    if name == "random_viking":
        assert info["sbvh_" + name]["bvh_triangles"] > T.load(vpt, name)[0].triangle_count()   # references multiplied


def test_refitted_tree_after_an_instance_move(vpt, oracle, runs):
    """vpt_set_instance_transforms moves the lamp and the glass sphere: the refitted boxes are looser, the hits are the moved scene's."""
    import refit_moves as RM
    ran(runs[1], "moved_glass")
    sc, rays = T.load(vpt, "random_glass")
    moved = RM.with_matrices(sc, RM.moved_matrices(sc, RM.GLASS_LAMP_AND_SPHERE))
    ref = T.brute_force(vpt, oracle, moved, rays)
    assert_hits(runs[0]["moved_glass"], ref, "moved")
    before = T.reference(vpt, oracle, "random_glass")
    assert (ref["t"] != before["t"]).sum() > 1000   # the move is seen


@pytest.mark.parametrize("name", T.SKY_SETS)
def test_sky_rays(vpt, oracle, runs, name):
    """k_trace_shadow<sky>, four instantiations: visible <=> brute force finds nothing in the kernel's window [1e-4, 1e6]."""
    z, info = runs
    ran(info, "sky_" + name)
    for rule in RULES:
        want = T.sky_reference(vpt, oracle, name, strict=rule == "strict")
        got = z["sky_%s_%s" % (name, rule)]
        assert np.array_equal(got, want), "%s, %s: %d of %d rays" % (name, rule, int((got != want).sum()), len(want))
        assert info["sky_" + name][rule]["counting_same"] and min(info["sky_" + name][rule]["visits"]) > 0
    assert_holes(z["sky_%s_holes" % name], z["sky_%s_default" % name], name)


@pytest.mark.parametrize("name", T.SKY_SETS_NO_RAY_QUERIES)
def test_sky_rays_without_ray_queries(vpt, oracle, runs, name):
    """... and [1e-5, 1000] on the normalised direction."""
    z, info = runs
    ran(info, "sky_" + name)
    for rule in RULES:
        want = T.sky_reference(vpt, oracle, name, strict=rule == "strict", ray_queries=0)
        got = z["sky_%s_norq_%s" % (name, rule)]
        assert np.array_equal(got, want), "%s, %s: %d of %d rays" % (name, rule, int((got != want).sum()), len(want))
        assert info["sky_%s_norq" % name][rule]["counting_same"]


@pytest.mark.parametrize("name", T.LIGHT_SCENES)
def test_light_rays(vpt, oracle, runs, name):
    """k_trace_shadow<light>, four instantiations: visible <=> the closest hit is the expected triangle, or the ray is media-flagged and hits
    nothing; with the right expectation, the neighbouring triangle's, and media-flagged rays past the light."""
    z, info = runs
    ran(info, "light_" + name)
    o = oracle.Oracle(T.light_scene(vpt, name), 8, 8); tris = o.triangles(); o.close()
    import whole_spill_scene
    assert np.array_equal(tris.view(np.uint32), whole_spill_scene.world_triangles(T.light_scene(vpt, name)).view(np.uint32))   # the ids the rays expect are the oracle's
    for rule in RULES:
        want, _ = T.light_reference(vpt, oracle, name, strict=rule == "strict")
        got = z["light_%s_%s" % (name, rule)]
        assert np.array_equal(got, want), "%s, %s: %d of %d rays" % (name, rule, int((got != want).sum()), len(want))
        assert info["light_" + name][rule]["counting_same"] and min(info["light_" + name][rule]["visits"]) > 0
    assert_holes(z["light_%s_holes" % name], z["light_%s_default" % name], name)


@pytest.mark.parametrize("which", range(len(T.SHADOW_SIZES) + 2))
def test_shadow_kernels_at_every_size(vpt, oracle, runs, big, which):
    """Light rays at 1, 63, 65, 4097 entries and at the two sizes beyond the static part (the set over and over), with and without holes; the sky
    form at those two sizes on the scheduling tests' rays."""
    z, info = runs
    n = (T.SHADOW_SIZES + big[0])[which]
    ran(info, "light_n%d" % n)
    want, _ = T.light_reference(vpt, oracle, "cornell_box_glass")
    want = want[np.arange(n) % len(want)]
    got = z["light_n%d" % n]
    assert np.array_equal(got, want), "%d of %d rays" % (int((got != want).sum()), n)
    assert_holes(z["light_n%d_holes" % n], want, "%d light rays" % n)
    if n in big[0]:
        ran(info, "sky_n%d" % n)
        sky = (big[1]["t"][:n] < 0).astype(np.uint8)   # (random_rays' window is the kernel's)
        assert np.array_equal(z["sky_n%d" % n], sky), "%d of %d rays" % (int((z["sky_n%d" % n] != sky).sum()), n)
        assert_holes(z["sky_n%d_holes" % n], sky, "%d sky rays" % n)
