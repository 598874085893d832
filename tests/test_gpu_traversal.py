"""vpt_trace_rays against the oracle's brute-force closest hit: (t,u,v) bit-exact, primitive/instance identical, ties and degenerate rays
included.  vpt_trace_rays is k_first_hit (kernels_aux.hip), a per-lane trace_closest loop out of traverse.hpp; the kernels that trace the rays of
the stream pipelines (k_trace_vote, k_trace_shadow) take the same ray sets (tests/trace_ray_sets.py) in tests/test_gpu_trace_stream.py."""
import numpy as np
import pytest

from trace_ray_sets import axis_aligned_rays, random_rays, window_rays

pytestmark = pytest.mark.gpu


def compare(vpt, oracle, sc, rays):
    o = oracle.Oracle(sc, 8, 8)
    o.set_brute_force(True)
    ref = o.trace_rays(rays)
    o.close()
    g = vpt.PathTracer(8, 8)
    g.set_scene(sc)
    got = g.trace_rays(rays)
    st = g.stats()
    g.close()
    for k in ("t", "u", "v", "primitive", "instance"):
        assert np.array_equal(got[k], ref[k]), k
    return ref, st


@pytest.mark.parametrize("name,scale,n", [("cornell_box", 8.0, 400000), ("cornell_box_glass", 8.0, 200000), ("viking_room", 2.0, 60000)])
def test_random_rays(vpt, oracle, scenes, name, scale, n):
    ref, st = compare(vpt, oracle, scenes(name), random_rays(n, 5, scale))
    assert (ref["t"] >= 0).mean() > 0.05
    assert st["bvh_triangles"] == scenes(name).triangle_count()
    # vpt_trace_rays always walks the 64 B quantised nodes; the render kernels of an LDS-resident scene use 128 B fp32 ones
    assert st["bvh_node_bytes"] in (64, 128) and st["bvh_tri_bytes"] == 48


def test_axis_aligned_and_degenerate_rays(vpt, oracle, scenes):
    """Zero direction components (0 * inf in slab tests), origins on walls, rays along box edges."""
    compare(vpt, oracle, scenes("cornell_box"), axis_aligned_rays())


def test_tmin_tmax_window(vpt, oracle, scenes):
    ref, _ = compare(vpt, oracle, scenes("cornell_box_glass"), window_rays())   # tmin 2.0 beyond near hits, tmax 9.0 before far hits
    hit = ref["t"] >= 0
    assert hit.any() and (ref["t"][hit] > 2.0).all() and (ref["t"][hit] < 9.0).all()


def test_empty_ray_list(vpt, scenes):
    g = vpt.PathTracer(8, 8)
    g.set_scene(scenes("cornell_box"))
    assert len(g.trace_rays(np.zeros((0, 8), np.float32))) == 0
    g.close()


def test_spatial_split_tree_renders_the_same_image(vpt, oracle, scenes):
    """vpt_config.build_flags = VPT_BUILD_SBVH: the tree built with spatial splits references some triangles from several leaves;
    closest hits, light-identity queries and therefore the image stay bit-identical to the oracle's (ties in t -> smaller global id)."""
    sc = scenes("viking_room")
    P = vpt.default_params(max_depth=6)
    o = oracle.Oracle(sc, 160, 90); o.set_params(P); o.render(3); ref = o.radiance(); o.close()
    g = vpt.PathTracer(160, 90, build_flags=1); g.set_scene(sc); g.set_params(P); g.render(3)   # VPT_BUILD_SBVH
    img = g.radiance(); st = g.stats(); g.close()
    h = vpt.PathTracer(160, 90); h.set_scene(sc); h.set_params(P); h.render(3); st0 = h.stats(); h.close()
    assert st["build_flags"] == 1 and st0["build_flags"] == 0
    assert np.array_equal(img, ref)
    assert st["bvh_triangles"] > st0["bvh_triangles"] == sc.triangle_count()   # references multiplied, triangles did not
