"""Edge cases: tiny and ragged image sizes, a scene with no triangles, degenerate triangles, depth 1, very large and
very small scene scales (the quantised BVH boxes must stay conservative), post-processing of images too small for
a full bloom chain; a rejected scene description leaves the installed scene as it was."""
import copy
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import assert_parity
from trace_ray_sets import far_rays, scaled, scaled_rays

pytestmark = pytest.mark.gpu


def both(vpt, oracle, sc, w, h, P, frames, **kw):
    o = oracle.Oracle(sc, w, h); o.set_params(P); o.render(frames)
    ref = o.radiance(); o.close()
    g = vpt.PathTracer(w, h, **kw); g.set_scene(sc); g.set_params(P); g.render(frames)
    img = g.radiance(); out8 = g.postprocess(); g.close()
    ref8, _ = oracle.postprocess(ref, vpt.default_post_params())
    return img, ref, out8, ref8


@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (5, 3), (2, 2), (63, 65), (257, 3)])
@pytest.mark.parametrize("pipeline", [1, 2])
def test_tiny_and_ragged_image_sizes(vpt, oracle, scenes, w, h, pipeline):
    img, ref, out8, ref8 = both(vpt, oracle, scenes("cornell_box"), w, h, vpt.default_params(max_depth=5), 3, pipeline=pipeline, build_flags=4 if pipeline == 2 else 0)
    assert_parity(img, ref)
    assert np.array_equal(out8, ref8)       # bloom chain stops when a mip would fall below 2 px (PostProcessor.cpp:136-157)


@pytest.mark.parametrize("k", [1e-3, 1e3, 3.7e4])
def test_scene_scale_does_not_break_the_quantised_bvh(vpt, oracle, scenes, k):
    """Random rays against the viking room scaled by k: closest hits equal the oracle's (its own BVH / brute force)."""
    sc = scaled(scenes("viking_room"), k)
    rays = scaled_rays(k)
    o = oracle.Oracle(sc, 8, 8); ref = o.trace_rays(rays); o.close()
    g = vpt.PathTracer(8, 8); g.set_scene(sc); got = g.trace_rays(rays); g.close()
    for f in ("t", "u", "v", "primitive", "instance"):
        assert np.array_equal(got[f], ref[f]), f
    assert (ref["t"] >= 0).mean() > 0.02


def test_depth_one_and_degenerate_triangles(vpt, oracle, scenes):
    sc = copy.deepcopy(scenes("cornell_box"))
    S = vpt.scenes
    pos = np.array([[0, -5, 0], [0, -5, 0], [0, -5, 0],            # a point
                    [-1, -6, 0], [0, -6, 0], [1, -6, 0]], np.float32)  # a segment (collinear)
    m = sc.add_mesh(pos, np.tile([0, 0, 1], (6, 1)).astype(np.float32), np.zeros((6, 2), np.float32), np.arange(6, dtype=np.uint32))
    sc.add_instance(m, 0)
    for depth in (1, 2):
        img, ref, _, _ = both(vpt, oracle, sc, 96, 54, vpt.default_params(max_depth=depth), 2)
        assert_parity(img, ref)


def test_scene_without_triangles(vpt, oracle):
    """Only an environment: every ray misses; with the env shown directly the image is the env, bit for bit."""
    S = vpt.scenes
    sc = S.Scene()
    m = sc.add_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32), np.zeros(0, np.uint32))
    sc.materials.append(S.material()); sc.add_instance(m, 0)
    sc.env = S.sun_sky_env(64, 32, seed=1, sun_peak=100.0); sc.luts = S.load_luts()
    sc.view_inverse = np.linalg.inv(S.look_at((0, 0, 0), (0, -0.2, -1), (0, 1, 0))).astype(np.float32)
    img, ref, out8, ref8 = both(vpt, oracle, sc, 64, 36, vpt.default_params(max_depth=4), 2)
    assert_parity(img, ref)
    assert img[..., :3].max() > 0 and np.array_equal(out8, ref8)


@pytest.mark.parametrize("far", [30.0, 1000.0])
def test_rays_from_far_outside_the_scene(vpt, oracle, scenes, far):
    """Origins `far` scene radii away, aimed at the scene: the slab test's rounding grows with the distance to the box,
    the build-time padding does not — the traversal must still find every hit the shared triangle test accepts.
    (Holds up to ~1e3 scene radii.  At 3e4 radii about 0.1 % of the rays differ from brute force: there one ulp of the
    ray origin is larger than the triangles, and no fixed box padding can follow what the fp32 triangle test accepts;
    the integrator never starts a ray that far from the geometry it can hit: DESIGN.md §6.)"""
    sc = scenes("viking_room")
    rays = far_rays(far)
    o = oracle.Oracle(sc, 8, 8); o.set_brute_force(True); ref = o.trace_rays(rays); o.close()   # no box test on the oracle side at all
    g = vpt.PathTracer(8, 8); g.set_scene(sc); got = g.trace_rays(rays); g.close()
    for f in ("t", "u", "v", "primitive", "instance"):
        assert np.array_equal(got[f], ref[f]), (f, int((got[f] != ref[f]).sum()))
    assert (ref["t"] >= 0).mean() > 0.2


def rejected_descriptions(vpt):
    """(name, scene, what to do to its description, error code, message): one ordinary rejection of scene_prep.hpp's check (the whole table:
    tests/test_scene_prep_cpu.py) and the one that used to be noticed only after the installed scene had been freed."""
    S = vpt.scenes
    tri = S.Scene()
    m = tri.add_mesh([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 0, 1)] * 3, None, [0, 1, 2])
    tri.materials.append(S.material())
    tri.add_instance(m, 0)
    lamps = copy.deepcopy(tri)
    lamps.materials[0]["emissive_color"] = (3.0, 3.0, 3.0)
    lamps.instances = lamps.instances * 10001            # VPT_MAX_EMISSIVE_MESHES + 1 instances of an emissive material

    def bad_index(desc):
        idx = (C.c_uint32 * 3)(0, 1, 3)
        desc.meshes[0].indices = C.cast(idx, C.c_void_p).value
        return idx

    return [("mesh index out of range", tri, bad_index, -1, "mesh index out of range"),
            ("too many emissive meshes", lamps, lambda desc: None, -7, "too many emissive meshes")]


def test_a_rejected_scene_leaves_the_installed_one_untouched(vpt, scenes):
    sc = scenes("cornell_box")
    frames = 3
    g = vpt.PathTracer(64, 36); g.set_scene(sc); g.set_params(vpt.default_params(max_depth=5)); g.render(frames)
    first = g.radiance()
    assert first[..., :3].max() > 0
    keys = ("total_vertex_count", "total_index_count", "bvh_nodes", "bvh_triangles", "bvh_node_bytes", "emissive_mesh_count", "emissive_triangle_count", "frames")
    before = {k: g.stats()[k] for k in keys}
    assert before["bvh_triangles"] == sc.triangle_count() and before["emissive_mesh_count"] >= 1 and before["frames"] == frames
    for name, bad, mutate, code, message in rejected_descriptions(vpt):
        desc, keep = bad.to_desc()
        keep.append(mutate(desc))
        assert g.lib.vpt_set_scene(g.ctx, C.byref(desc)) == code, name
        assert g.lib.vpt_last_error(g.ctx).decode() == message, name
        assert {k: g.stats()[k] for k in keys} == before, name          # the old scene, and the frames accumulated on it
        assert np.array_equal(g.radiance(), first), name
        g.reset(); g.render(frames)
        assert np.array_equal(g.radiance(), first), name                # ... which still renders what it rendered
    g.close()
