"""One long-lived context walked through changes of schedule class, in lockstep with the oracle: the same call sequence goes to a
vpt.PathTracer and an oracle.Oracle, and after every render step the images are equal bit for bit.  The host layer (api_render.hip) picks a
schedule per batch from the context's history — whole-path launch, fused k_bounce, streams with regeneration, media streams, the k_finish
tail; the path buffers' frames_alloc / resident_alloc; media_frames, class queues, captured graphs — and every other GPU test builds a fresh
context per configuration.  Also the four instantiations of k_finish<COUNT, STRICT> (kernels_finish.hip): image, ray statistics and visit
counts against the oracle and against a twin context without the finisher (VPT_BUILD_STREAMS_ONLY)."""
import copy

import numpy as np
import pytest

from test_oracle_volumes import cloud_grid

pytestmark = pytest.mark.gpu
W, H = 96, 54
BUILD_STREAMS_ONLY = 4          # include/vpt.h VPT_BUILD_STREAMS_ONLY


def params(vpt, **kw):
    d = dict(max_depth=8)
    d.update(kw)
    return vpt.default_params(**d)


def fog(vpt, **kw):
    d = dict(corner_min=(-5.0, -10.5, -5.0), corner_max=(5.0, -0.5, 5.0), color=(0.9, 0.85, 0.8), density=0.12, anisotropy=0.3)
    d.update(kw)
    return vpt.volume(**d)


class Lockstep:
    """The same calls to the library and to the oracle.  set_scene / resize construct a new Oracle (both reset the accumulation) and hand it
    the state the context keeps; every render step compares the images and, where the suite holds them equal (surfaces, whole-frame
    dispatches), the closest-ray counts of the step."""

    def __init__(self, vpt, oracle, w, h, **cfg):
        self.vpt, self.oracle, self.w, self.h = vpt, oracle, w, h
        self.g = vpt.PathTracer(w, h, **cfg)
        self.o = None
        self.P, self.vols, self.atm, self.phase, self.grids, self.sc = None, [], None, 0, [], None
        self.steps = 0

    def close(self):
        self.g.close()
        if self.o:
            self.o.close()

    def _new_oracle(self):
        if self.o:
            self.o.close()
        self.o = self.oracle.Oracle(self.sc, self.w, self.h)
        for grid in self.grids:
            self.o.add_density_grid(grid)
        if self.P is not None:
            self.o.set_params(self.P)
        self.o.set_volumes(self.vols); self.o.set_atmosphere(self.atm); self.o.set_phase_function(self.phase)

    def set_scene(self, sc):
        assert not self.grids
        self.sc = copy.deepcopy(sc)
        self.g.set_scene(sc)
        for f in (lambda x: x.set_volumes(self.vols), lambda x: x.set_atmosphere(self.atm), lambda x: x.set_phase_function(self.phase)):
            f(self.g)
        if self.P is not None:
            self.g.set_params(self.P)
        self._new_oracle()

    def resize(self, w, h):
        assert not self.grids
        self.w, self.h = w, h
        self.g.resize(w, h)
        self.g.set_camera(self.sc.view_inverse, self.sc.projection_inverse(w / h))
        self._new_oracle()

    def set_params(self, P):
        self.P = P
        self.g.set_params(P); self.o.set_params(P)

    def set_max_samples(self, n, frames_done):
        """A change of max_samples alone keeps the accumulation (PathTracer.cpp:1003-1006); the oracle resets on every set_params, so it
        gets its own image back."""
        keep = self.o.radiance()
        self.P = type(self.P).from_buffer_copy(self.P); self.P.max_samples = n
        self.g.set_params(self.P); self.o.set_params(self.P); self.o.set_radiance(keep, frames_done)

    def set_volumes(self, vols):
        self.vols = list(vols)
        self.g.set_volumes(self.vols); self.o.set_volumes(self.vols)

    def add_density_grid(self, grid):
        a, b = self.g.add_density_grid(grid), self.o.add_density_grid(grid)
        assert a == b
        self.grids.append(grid)
        return a

    def clear_density_grids(self):
        self.set_volumes([])
        self.grids = []
        self.g.clear_density_grids(); self.o.clear_density_grids()

    def set_atmosphere(self, atm):
        self.atm = atm
        self.g.set_atmosphere(atm); self.o.set_atmosphere(atm)

    def set_phase_function(self, phase):
        self.phase = phase
        self.g.set_phase_function(phase); self.o.set_phase_function(phase)

    def set_material(self, i, **kw):
        m = self.g.get_material(i)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(m, k)[:] = v
            else:
                setattr(m, k, v)
        self.g.set_material(i, m); self.o.set_material(i, m)

    def set_radiance(self, img, frames):
        self.g.set_radiance(img, frames); self.o.set_radiance(img, frames)

    def radiance(self):
        return self.g.radiance()

    def render(self, n, use_async=False):
        self.steps += 1
        self.g.reset_stats()
        c0 = self.o.counters()
        if use_async:
            for _ in range(n):
                self.g.render_async(1)
            self.g.wait(0)
        else:
            self.g.render(n)
        self.o.render(n)
        img, ref = self.g.radiance(), self.o.radiance()
        st = self.g.stats()
        diff = (img != ref).any(axis=2)
        assert not diff.any(), "step %d (render %d%s): %d pixels differ, %d of them black here only" % (
            self.steps, n, " async" if use_async else "", int(diff.sum()), int((diff & (img[..., :3] == 0).all(axis=2)).sum()))
        c1 = self.o.counters()
        closest, shadow = c1["closest"] - c0["closest"], c1["shadow"] - c0["shadow"]
        if not self.vols and self.atm is None and self.P.screen_chunk_count == 1:   # (surfaces, whole-frame dispatches)
            assert st["closest_rays"] == closest, ("step %d" % self.steps, st["closest_rays"], closest)
            # the oracle counts every visibility query of its loop, the library the shadow rays it launches (tests/test_gpu_transitions.py
            # test_finisher_instantiations): never more than the oracle asked
            assert st["shadow_rays"] <= shadow, ("step %d" % self.steps, st["shadow_rays"], shadow)
        return st


CONTEXTS = {   # pipeline, frames_in_flight, resident_frames, count_traversal
    "auto_library_sized": dict(pipeline=0, frames_in_flight=0, resident_frames=0, count_traversal=False),
    "fused_explicit": dict(pipeline=1, frames_in_flight=2, resident_frames=0, count_traversal=False),
    "fused_explicit_counting": dict(pipeline=1, frames_in_flight=3, resident_frames=0, count_traversal=True),
    "staged_explicit_all_resident": dict(pipeline=2, frames_in_flight=3, resident_frames=0, count_traversal=False),
    "staged_resident1": dict(pipeline=2, frames_in_flight=3, resident_frames=1, count_traversal=False),
    "staged_sorted_resident1_counting": dict(pipeline=4, frames_in_flight=4, resident_frames=1, count_traversal=True),
}


@pytest.mark.parametrize("ctx", sorted(CONTEXTS))
def test_schedule_transitions_in_lockstep_with_the_oracle(vpt, oracle, scenes, ctx):
    cfg = CONTEXTS[ctx]
    F = cfg["frames_in_flight"] or 5       # (a library-sized context takes batches of thousands of frames here: these counts all fit one)
    cornell, glass = scenes("cornell_box"), scenes("cornell_box_glass")
    L = Lockstep(vpt, oracle, W, H, **cfg)
    try:
        P = params(vpt)
        L.set_scene(cornell); L.set_params(P)
        # frame counts across batch boundaries on the LDS scene (whole-path launches under AUTO)
        for n in (1, max(F - 1, 1), F + 1, 2 * F + 1):
            L.render(n)
        # LDS scene -> scene in memory (streams + finisher under AUTO / STAGED), and back
        L.set_scene(glass)
        L.render(1); L.render(F + 1)
        L.set_scene(cornell)
        L.render(2)
        # samples_per_frame 1 -> 3 (leaves the whole-path launch) -> 1
        L.set_params(params(vpt, samples_per_frame=3)); L.render(2); L.render(F + 1)
        L.set_params(P); L.render(F + 1)
        # split-screen dispatch 2 and 3 (no regeneration: residency grows), on both scenes, and back
        for sc in (glass, cornell):
            L.set_scene(sc)
            L.render(F + 1)                                  # (a regenerating batch first, where the scene allows one)
            for S in (2, 3):
                L.set_params(params(vpt, screen_chunk_count=S)); L.render(S * S + 1); L.render(S * S * (F + 1) - 1)
            L.set_params(P); L.render(F + 1)
        # surface -> homogeneous volume (phase functions), grid volume, atmosphere, and back — on the scene in memory and the LDS one
        for sc in {0: (glass, cornell), 1: (glass, cornell), 2: (glass,)}.get(cfg["pipeline"], ()):   # (media on the fused kernel or, in memory, the streams: VPT_ERR_UNSUPPORTED otherwise)
            L.set_scene(sc)
            L.render(F + 1)
            L.set_volumes([fog(vpt)]); L.render(2); L.render(F + 1)
            L.set_phase_function(1); L.render(1)
            L.set_phase_function(2); L.render(2)
            L.set_phase_function(0)
            gi = L.add_density_grid(cloud_grid(seed=5))
            L.set_volumes([vpt.volume(corner_min=(-4.0, -9.0, -4.0), corner_max=(4.0, -2.0, 4.0), color=(0.9, 0.9, 0.9), density=1.0, density_data_index=gi)])
            L.render(2)
            L.clear_density_grids(); L.render(F + 1)
            L.set_params(params(vpt, sky_altitude=-50.0, sky_azimuth=150.0)); L.set_atmosphere(vpt.atmosphere()); L.render(2)
            L.set_atmosphere(None); L.set_params(P); L.render(F + 1)
        # max_depth 8 -> 1 -> 200 -> 8
        for d in (1, 200, 8):
            L.set_params(params(vpt, max_depth=d)); L.render(2)
        # flags: strict hits, furnace (re-resolves the materials), default
        for flags in (P.flags | 256, P.flags | 32, P.flags):   # VPT_FLAG_LOCAL_HITS, VPT_FLAG_FURNACE
            L.set_params(params(vpt, flags=flags)); L.render(F + 1)
        # accumulation: a material edit mid-run (emissive list rebuilt), max_samples alone, past max_samples, a checkpoint
        L.set_scene(glass); L.render(3)
        L.set_material(0, emissive_color=(4.0, 3.0, 2.0)); L.render(2)
        L.set_material(0, emissive_color=(0.0, 0.0, 0.0), base_color=(0.3, 0.6, 0.9)); L.render(F + 1)
        L.set_params(P); L.render(3)
        L.set_max_samples(5, 3); L.render(4)                # two more frames, then nothing
        before = L.radiance()
        L.render(2)                                          # past max_samples: renders nothing
        assert np.array_equal(L.radiance(), before)
        L.set_max_samples(P.max_samples, 5); L.render(2)   # (max_samples alone again: the accumulation goes on)
        L.set_radiance(before, 5); L.render(F + 1)          # resume from a checkpoint
        # asynchronous frames interleaved with the changes above; a captured-graph replay, then a resize and buffers that regrow
        L.set_scene(cornell)
        L.render(6, use_async=True)
        L.set_params(params(vpt, samples_per_frame=2)); L.render(3, use_async=True)
        if cfg["pipeline"] in (0, 1):
            L.set_params(P); L.set_volumes([fog(vpt)]); L.render(3, use_async=True)
            L.set_volumes([]); L.render(2, use_async=True)
        L.set_scene(glass); L.render(4, use_async=True)
        L.set_params(params(vpt, screen_chunk_count=2)); L.render(5, use_async=True)
        L.set_params(P); L.set_scene(cornell)
        L.resize(64, 36)                                     # the path buffers of one frame again
        st = L.render(6, use_async=True)
        if not cfg["count_traversal"] and cfg["pipeline"] in (0, 1):   # (counting contexts launch plainly)
            assert st["graph_launches"] > 0, "the 1-frame batches were not replayed from a captured graph"
        L.render(2 * F + 1)                                  # and regrow behind the replays
        L.render(3, use_async=True)
    finally:
        L.close()


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("count", [False, True])
def test_finisher_instantiations(vpt, oracle, scenes, count, strict):
    """k_finish<COUNT, STRICT> behind small batches of the streams pipeline (finish_at = 3 bounces): it runs, the image is the oracle's, its
    ray statistics are the oracle's, and with counting on its visit counts equal those of a twin that runs every bounce on the stream kernels."""
    sc = copy.deepcopy(scenes("cornell_box_glass"))
    sc.env = vpt.scenes.sun_sky_env(32, 16, seed=6, sun_peak=60.0)
    w, h, frames = 128, 72, 4
    P = vpt.default_params(max_depth=12)
    if strict:
        P.flags |= 256                                       # VPT_FLAG_LOCAL_HITS
    o = oracle.Oracle(sc, w, h); o.set_params(P); o.render(frames); ref, ctr = o.radiance(), o.counters(); o.close()
    stats = []
    for build in (0, BUILD_STREAMS_ONLY):
        g = vpt.PathTracer(w, h, frames_in_flight=2, count_traversal=count, build_flags=build)
        g.set_scene(sc); g.set_params(P); g.render(frames)
        st = g.stats()
        assert np.array_equal(g.radiance(), ref), build
        assert st["closest_rays"] == ctr["closest"], (build, st["closest_rays"], ctr["closest"])
        assert st["samples"] == ctr["samples"]
        stats.append(st); g.close()
    fin, streams = stats
    assert fin["finish_paths"] > 0 and streams["finish_paths"] == 0
    assert fin["kernel_launches"]["extend"] < streams["kernel_launches"]["extend"]
    # (shadow_rays: the oracle counts every visibility query of its own loop — 78881 against the library's 57835 launched shadow rays here, in
    # every pipeline — so no test holds them equal to it; the finisher must count what the stream kernels count)
    assert fin["shadow_rays"] == streams["shadow_rays"], (fin["shadow_rays"], streams["shadow_rays"])
    assert 0.6 * ctr["shadow"] <= fin["shadow_rays"] <= ctr["shadow"], (fin["shadow_rays"], ctr["shadow"])   # (0.733 of the oracle's queries here)
    keys = ("nodes_visited", "tris_tested", "shadow_nodes_visited", "shadow_tris_tested")
    if count:
        for k in keys:
            assert fin[k] > 0 and fin[k] == streams[k], (k, fin[k], streams[k])
    else:
        assert all(fin[k] == 0 for k in keys)
