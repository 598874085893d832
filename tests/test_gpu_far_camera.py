"""The box test of a tree in LDS has two forms (vulkan-path-tracer_amd/csrc/slab.hpp): one fma per plane for waves whose ray origins all lie within
kSlabFmaReach (16) x the scene's largest |coordinate| of the world's origin, subtract-and-multiply for the others.  A box test only prunes, so the
image must be the oracle's bit for bit whichever form a search ran: the Cornell box (largest |coordinate| 11.56, reach 184.9) seen from its own
camera, from 0.9 x the reach (every search takes the fma form) and from 1.1 x the reach (the camera rays' searches take the subtract form; in the
whole-path kernel so do the bounce rays that share a wave with a freshly started camera ray).  Host side of the same claim:
tests/test_box_entry_fma_cpu.py."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EXTENT, REACH = 11.558207513143259, 16.0


def render_pair(vpt, oracle, sc, w, h, depth, frames, pipeline):
    p = vpt.default_params(max_depth=depth)
    o = oracle.Oracle(sc, w, h)
    o.set_params(p)
    o.render(frames)
    ref = o.radiance()
    o.close()
    g = vpt.PathTracer(w, h, pipeline=pipeline, frames_in_flight=frames)
    g.set_scene(sc); g.set_params(p)
    g.render(frames)
    img, st = g.radiance(), g.stats()
    g.close()
    return img, ref, st


@pytest.mark.parametrize("pipeline", ["WHOLE", "FUSED"])
@pytest.mark.parametrize("where,camera_z", [("own", None), ("inside_reach", 0.9 * REACH * EXTENT), ("beyond_reach", 1.1 * REACH * EXTENT)])
def test_cornell_box_from_inside_and_beyond_the_fma_reach_equals_the_oracle(vpt, oracle, scenes, where, camera_z, pipeline):
    sc = copy.deepcopy(scenes("cornell_box"))
    pos = np.concatenate([(np.c_[sc.meshes[mesh][0]["position"], np.ones(len(sc.meshes[mesh][0]))] @ np.asarray(m, np.float64).T)[:, :3] for mesh, _, m in sc.instances])
    assert abs(float(np.abs(pos).max()) - EXTENT) < 1e-3
    w, h = (160, 90)
    if camera_z is not None:
        sc.view_inverse = np.array(sc.view_inverse, np.float32)
        sc.view_inverse[2, 3] = camera_z      # straight back along the viewing axis: the box is ~60 of 720 rows from there
        w, h = (1280, 720)
        assert (abs(float(sc.view_inverse[2, 3])) > REACH * EXTENT) == (where == "beyond_reach")
    img, ref, st = render_pair(vpt, oracle, sc, w, h, 8, 2, getattr(vpt._abi, "PIPELINE_" + pipeline))
    lit = int((ref[..., :3].max(axis=2) > 0).sum())
    assert lit >= 1500, "the box is hardly in the picture: %d lit pixels" % lit
    assert np.array_equal(img, ref), "%d px differ" % int((np.abs(img - ref).max(axis=2) > 0).sum())
    assert st["kernel_launches"]["bounce" if pipeline == "FUSED" else "primary"] > 0
