"""The reference's asynchronous per-frame contract behind the C-ABI (include/vpt.h vpt_render_async / vpt_postprocess_device /
vpt_wait: PathTracer::PathTrace(cmd) records and returns, PathTracer.cpp:122-156; Editor.cpp:116,129) and the lazily grown path
buffers: every image must equal the blocking path's — and the oracle's — bit for bit."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def oracle_image(oracle, sc, w, h, params, frames):
    o = oracle.Oracle(sc, w, h)
    o.set_params(params)
    o.render(frames)
    ref = o.radiance()
    o.close()
    return ref


def test_async_frames_equal_blocking_frames_and_replay_from_a_graph(vpt, oracle, scenes):
    """Cornell box, depth 8, the per-bounce pipeline (VPT_PIPELINE_FUSED; AUTO would run a 1-frame batch as one whole-path launch,
    tests/test_gpu_whole.py): a fixed schedule (no medium scatters, 8 <= VPT_ASYNC_MAX_BOUNCES) — frames are enqueued back to back, the
    third identical call onwards replays a captured hipGraph, and the accumulated image equals vpt_render's and the oracle's."""
    sc, w, h, frames = scenes("cornell_box"), 160, 90, 12
    p = vpt.default_params(max_depth=8)
    ref = oracle_image(oracle, sc, w, h, p, frames)
    blocking = vpt.PathTracer(w, h, frames_in_flight=1, pipeline=vpt._abi.PIPELINE_FUSED)
    blocking.set_scene(sc); blocking.set_params(p)
    for _ in range(frames):
        blocking.render(1)
    img_b = blocking.radiance(); out_b = blocking.postprocess(); blocking.close()
    g = vpt.PathTracer(w, h, frames_in_flight=1, pipeline=vpt._abi.PIPELINE_FUSED)
    g.set_scene(sc); g.set_params(p)
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
    img_a = g.radiance()
    out_dev = g.output_to_host()
    assert np.array_equal(img_a, img_b) and np.array_equal(img_a, ref)
    assert np.array_equal(out_dev, out_b), "vpt_postprocess_device differs from vpt_postprocess"
    assert st["frames"] == frames and st["samples"] == w * h * frames
    assert st["graph_launches"] >= frames - 3, "the fused 1-frame batch was not replayed from a graph: %r" % (st["graph_launches"],)
    assert st["kernel_launches"]["primary"] == frames and st["kernel_launches"]["bounce"] == frames * 7 and st["kernel_launches"]["resolve"] == frames
    g.close()


def test_async_renders_interleaved_with_material_edits(vpt, oracle, scenes):
    """SetMaterial between asynchronous frames (it drains, patches the tables, resets the accumulation): same images as the blocking path."""
    sc, w, h = copy.deepcopy(scenes("cornell_box")), 128, 72
    p = vpt.default_params(max_depth=6)

    def run(use_async):
        g = vpt.PathTracer(w, h, frames_in_flight=1)
        g.set_scene(sc); g.set_params(p)
        imgs = []
        for edit in range(3):
            for _ in range(4):
                if use_async:
                    g.render_async(1); g.postprocess_device()
                else:
                    g.render(1)
            m = g.get_material(1)
            m.base_color[:] = (0.2 + 0.3 * edit, 0.9 - 0.2 * edit, 0.3)
            m.roughness = 0.3 + 0.2 * edit
            imgs.append(g.radiance())          # drains
            g.set_material(1, m)               # resets the accumulation
        for _ in range(3):
            if use_async:
                g.render_async(1)
            else:
                g.render(1)
        imgs.append(g.radiance())
        st = g.stats(); g.close()
        return imgs, st

    a, sa = run(True)
    b, sb = run(False)
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert sa["samples"] == sb["samples"]
    # the last image against the oracle with the final material
    sc2 = copy.deepcopy(sc)
    sc2.materials[1].update(base_color=(0.2 + 0.3 * 2, 0.9 - 0.2 * 2, 0.3), roughness=0.3 + 0.2 * 2)
    assert np.array_equal(a[-1], oracle_image(oracle, sc2, w, h, p, 3))


@pytest.mark.parametrize("name,depth,pipeline", [("cornell_box", 200, 0), ("cornell_box_glass", 12, 0), ("cornell_box_glass", 40, 0), ("cornell_box", 6, 2)])
def test_async_batches_that_may_outlive_their_enqueued_bounces(vpt, oracle, scenes, name, depth, pipeline):
    """Deeper than VPT_ASYNC_MAX_BOUNCES, the streams pipeline (also forced on a scene that rides in LDS): the enqueued part is the first bounces and the
    next call finishes the batch as vpt_render would have; multi-frame batches included."""
    sc, w, h = scenes(name), 96, 54
    p = vpt.default_params(max_depth=depth)
    g = vpt.PathTracer(w, h, pipeline=pipeline, frames_in_flight=3)
    g.set_scene(sc); g.set_params(p)
    g.render_async(3)
    g.render_async(2)      # finishes the first batch, then enqueues
    g.postprocess_device() # finishes the second
    g.render_async(1)
    img = g.radiance()     # drains
    st = g.stats(); g.close()
    assert st["frames"] == 6
    assert np.array_equal(img, oracle_image(oracle, sc, w, h, p, 6))


def test_async_with_a_scattering_medium_inside_glass(vpt, oracle, scenes):
    """A transmissive material with a dense medium: scattering events inside it do not raise the depth, so the batch is not a fixed
    schedule whatever max_depth says."""
    sc = copy.deepcopy(scenes("cornell_box_glass"))
    for m in sc.materials:
        if m["transmission"] > 0:
            m.update(medium_density=6.0, medium_anisotropy=0.3, medium_color=(0.9, 0.6, 0.4))
    w, h, p = 96, 54, vpt.default_params(max_depth=5)
    g = vpt.PathTracer(w, h, frames_in_flight=2)
    g.set_scene(sc); g.set_params(p)
    for _ in range(3):
        g.render_async(2)
    img = g.radiance(); g.close()
    assert np.array_equal(img, oracle_image(oracle, sc, w, h, p, 6))


def test_path_buffers_grow_with_the_batches_asked_for(vpt, scenes):
    """vpt_create holds the records of ONE frame (the verdict's interactive host: < 2 GB at 1080p with AUTO); the buffers grow to the
    largest batch requested, never beyond frames_in_flight, and the image does not depend on how they grew."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value
    sc = scenes("cornell_box")
    free0 = free_bytes()
    g = vpt.PathTracer(1920, 1080)            # AUTO: the cap is ~448M paths (226 frames)
    g.set_scene(sc); g.set_params(vpt.default_params(max_depth=4))
    st = g.stats()
    free1 = free_bytes()
    assert st["frames_allocated"] == 1 and st["frames_in_flight"] >= 64
    assert free0 - free1 < 2 * 1024 ** 3, "vpt_create + vpt_set_scene took %.2f GB" % ((free0 - free1) / 2 ** 30)
    g.render(1)
    assert g.stats()["frames_allocated"] == 1
    g.render(5)
    assert g.stats()["frames_allocated"] == 5
    g.render(2)
    assert g.stats()["frames_allocated"] == 5
    img = g.radiance(); g.close()
    ref = vpt.PathTracer(1920, 1080, frames_in_flight=8)
    ref.set_scene(sc); ref.set_params(vpt.default_params(max_depth=4))
    ref.render(8)
    assert ref.stats()["frames_allocated"] == 8
    assert np.array_equal(img, ref.radiance())
    ref.close()
    free2 = free_bytes()
    assert free0 - free2 < 1024 ** 3, "device memory not returned by vpt_destroy"


def test_async_edge_cases(vpt, oracle, scenes):
    """Camera moves between asynchronous frames (every move invalidates the captured batches: frames fall back to plain launches), max_samples
    reached (PathTrace's `true`: nothing more is launched), a resize with frames in flight, output getters before / after a post-process,
    and tickets of work long finished."""
    sc, w, h = scenes("cornell_box"), 96, 54
    p = vpt.default_params(max_depth=5, max_samples=7)
    g = vpt.PathTracer(w, h, frames_in_flight=1)
    g.set_scene(sc); g.set_params(p)
    assert g.output_device() is None
    with pytest.raises(vpt.VptError):
        g.output_to_host()
    tickets = []
    for k in range(10):
        done, t = g.render_async(1)
        tickets.append(t)
        assert done == (k >= 7)
    g.wait(tickets[0]); g.wait(tickets[3]); g.wait(10 ** 9)     # long finished; in the ring; beyond what was issued (= everything)
    st = g.stats()
    assert st["frames"] == 7 and st["samples"] == 7 * w * h
    ref = oracle_image(oracle, sc, w, h, p, 7)
    assert np.array_equal(g.radiance(), ref)
    # a moving camera: accumulation restarts with every move, each image is a 1-frame render of that view
    views = []
    for k in range(4):
        vi = np.array(sc.view_inverse, np.float32).copy(); vi[0, 3] += 0.05 * k
        g.set_camera(vi, sc.projection_inverse(w / h))
        g.render_async(1); g.postprocess_device()
        views.append((vi, g.radiance(), g.output_to_host()))
    for vi, img, out8 in views[1:]:
        o = oracle.Oracle(sc, w, h); o.set_camera(vi, sc.projection_inverse(w / h)); o.set_params(p); o.render(1)
        r = o.radiance(); o.close()
        assert np.array_equal(img, r)
        ref8, _ = oracle.postprocess(r, vpt.default_post_params())
        assert np.array_equal(out8, ref8)
    # resize with frames in flight: drains, the lanes' buffers of the old size go, rendering goes on at the new size
    g.set_camera(sc.view_inverse, sc.projection_inverse(w / h))
    for _ in range(3):
        g.render_async(1)
    g.resize(64, 36)
    g.set_camera(sc.view_inverse, sc.projection_inverse(64 / 36))
    for _ in range(5):
        g.render_async(1)
    assert np.array_equal(g.radiance(), oracle_image(oracle, sc, 64, 36, p, 5))
    g.close()


def test_fixed_stream_batches_are_replayed_from_a_graph(vpt, oracle, scenes):
    """A frame per call on a scene whose BVH lives in memory: the streams pipeline's small batch — three bounces on the streams, then ONE launch that
    runs what is left to its end (k_finish) — is a fixed schedule whatever max_depth is: dealt to the lanes, captured once per lane and replayed;
    a parameter change in between re-captures.  Same image as the oracle's."""
    sc, w, h = scenes("cornell_box_glass"), 96, 54
    p = vpt.default_params(max_depth=8)
    g = vpt.PathTracer(w, h, frames_in_flight=1)
    g.set_scene(sc); g.set_params(p)
    for _ in range(7):
        g.render_async(1); g.postprocess_device()
    img = g.radiance()
    st = g.stats()
    assert st["frames"] == 7 and st["graph_launches"] >= 2 and st["kernel_launches"]["join"] == 7 * 3 and st["kernel_launches"]["bounce"] == 7
    assert np.array_equal(img, oracle_image(oracle, sc, w, h, p, 7))
    p2 = vpt.default_params(max_depth=200)   # far beyond VPT_ASYNC_MAX_BOUNCES: still one fixed schedule per frame
    g.set_params(p2)
    for _ in range(5):
        g.render_async(1)
    assert np.array_equal(g.radiance(), oracle_image(oracle, sc, w, h, p2, 5))
    g.close()


@pytest.mark.parametrize("name,depth", [("cornell_box_glass", 12), ("viking_room", 6)])
def test_small_stream_batches_finish_in_one_launch_and_large_ones_at_their_tail(vpt, oracle, scenes, name, depth):
    """k_finish (kernels_finish.hip) behind blocking batches too: a small batch runs three bounces on the streams and ONE launch for the rest, whatever
    its depth (the class-sorted pipeline likewise); ray statistics as the oracle counts them.  (Large batches hand over once the host sees fewer than
    262,144 paths alive: the 1080p cases of test_gpu_configs.py.)"""
    sc = copy.deepcopy(scenes(name))
    sc.env = vpt.scenes.sun_sky_env(32, 16, seed=6, sun_peak=60.0)
    w, h, frames = 160, 90, 4
    p = vpt.default_params(max_depth=depth)
    o = oracle.Oracle(sc, w, h); o.set_params(p); o.render(frames); ref, ctr = o.radiance(), o.counters(); o.close()
    for pipeline in (0, 4):
        g = vpt.PathTracer(w, h, pipeline=pipeline, frames_in_flight=frames)
        g.set_scene(sc); g.set_params(p); g.render(frames)
        st = g.stats()
        assert np.array_equal(g.radiance(), ref), pipeline
        assert st["closest_rays"] == ctr["closest"] and st["kernel_launches"]["bounce"] == 1 and st["kernel_launches"]["extend"] == 3
        g.close()
