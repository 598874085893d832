"""MI355X wavefront render backend for the Vulkan-Path-Tracer hot path.

This package is a thin ctypes shim over the C-ABI in include/vpt.h (libvpt_hip.so, hand-written HIP for
gfx950).  All compute happens in the library; there is no Python or CPU fallback: if the library or a
HIP device is missing, loading / vpt_create fail loudly.
"""
import ctypes as C
import os

import numpy as np

from . import _abi, imagefiles, scenes  # noqa: F401
from ._abi import default_params, default_post_params, volume, atmosphere  # noqa: F401
from ._abi import PHASE_HENYEY_GREENSTEIN, PHASE_DRAINE, PHASE_HENYEY_GREENSTEIN_PLUS_DRAINE  # noqa: F401
from ._abi import FEATURES_CENTER, FEATURES_SAMPLE  # noqa: F401
from ._abi import default_denoise_params, DENOISE_DEMODULATE, DENOISE_MAX_ITERATIONS, POST_SOURCE_RADIANCE, POST_SOURCE_DENOISED  # noqa: F401
from ._abi import default_temporal_params, TEMPORAL_DEMODULATE, TEMPORAL_MATCH_INSTANCE, DENOISE_SOURCE_RADIANCE, DENOISE_SOURCE_TEMPORAL  # noqa: F401
from ._abi import SvgfOptions, default_svgf_options  # noqa: F401
from ._abi import SvgfSpatialOptions, default_svgf_spatial_options  # noqa: F401
from ._abi import FireflyOptions, FireflyState, default_firefly_options  # noqa: F401
from ._abi import TemporalOptions, default_temporal_options  # noqa: F401
from ._abi import ExposureOptions, ExposureState, default_exposure_options, EXPOSURE_BINS  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class VptError(RuntimeError):
    pass


def _want_lab():
    """VPT_LAB=1 in the environment selects the LABORATORY build (libvpt_hip_lab.so: include/vpt_lab.h, the measured-and-rejected kernel
    variants, round 1's stage kernels).  It chooses which LIBRARY is loaded — a measuring tool's choice — never a behaviour of the product library."""
    return os.environ.get("VPT_LAB", "0") not in ("", "0")


def library_path(lab=None):
    lab = _want_lab() if lab is None else lab
    return os.path.join(_HERE, "libvpt_hip_lab.so" if lab else "libvpt_hip.so")


def build(force=False, verbose=False, lab=None):
    from . import _build as _b
    return _b.build(force=force, verbose=verbose, lab=_want_lab() if lab is None else lab)


def load_library():
    """Loads libvpt_hip.so — or libvpt_hip_lab.so with VPT_LAB=1 — building it first when hipcc is available and sources are newer."""
    global _LIB
    if _LIB is None:
        path = library_path()
        try:
            path = build()
        except Exception as e:  # no hipcc on this box: the prebuilt in-tree .so must exist
            if not os.path.exists(path):
                raise VptError("%s is missing and cannot be built: %s" % (os.path.basename(path), e))
        _LIB = _abi.bind(C.CDLL(path))
    return _LIB


def has_lab():
    """True when the loaded library is the laboratory build (exports vpt_lab_*, accepts VPT_PIPELINE_STAGED_R1)."""
    return bool(load_library().has_lab)


def _check(lib, ctx, rc, what):
    if rc != 0:
        msg = lib.vpt_last_error(ctx).decode() if ctx else ""
        raise VptError("%s failed: %s %s" % (what, _abi.ERR_NAMES.get(rc, rc), msg))


LUT_REFLECT, LUT_REFRACT_ABOVE, LUT_REFRACT_BELOW = 0, 1, 2


def calculate_lut(kind, size, sample_count, time_ms=0, device=0):
    """LookupTableCalculator::CalculateTable (LookupTableCalculator.cpp:44) on the GPU: returns float32 [z, y, x].
    kind: LUT_REFLECT (LookupReflect.slang), LUT_REFRACT_ABOVE / _BELOW (LookupRefract.slang + define)."""
    lib = load_library()
    sx, sy, sz = (int(v) for v in size)
    out = np.zeros((sz, sy, sx), np.float32)
    _check(lib, None, lib.vpt_lut_calculate(device, kind, sx, sy, sz, sample_count, time_ms, out.ctypes.data), "vpt_lut_calculate")
    return out


def bricks_of(grid):
    """A dense float32 [z, y, x] grid as 8x8x8 bricks, every brick whose voxels are all 0 dropped: ((dim_x, dim_y, dim_z), uint32 [n, 3] coordinates
    (bx, by, bz), float32 [n, 8, 8, 8] values [brick, z, y, x]; a partial brick's voxels outside the box hold 0) — the arguments of add_density_bricks."""
    g = np.ascontiguousarray(grid, np.float32)
    dz, dy, dx = g.shape
    cz, cy, cx = (-(-n // 8) for n in g.shape)
    padded = np.zeros((cz * 8, cy * 8, cx * 8), np.float32)
    padded[:dz, :dy, :dx] = g
    cells = padded.reshape(cz, 8, cy, 8, cx, 8).transpose(0, 2, 4, 1, 3, 5)   # [cell z, cell y, cell x, z, y, x]
    bz, by, bx = np.nonzero((cells != 0).any(axis=(3, 4, 5)))
    return (dx, dy, dz), np.stack([bx, by, bz], axis=1).astype(np.uint32), np.ascontiguousarray(cells[bz, by, bx])


class PathTracer:
    """Mirror of the reference's PathTracer + PostProcessor call surface over the C-ABI."""

    def __init__(self, width, height, device=0, shard_rank=0, shard_count=1, frames_in_flight=0, profile=False,
                 count_traversal=False, pipeline=0, build_flags=0, resident_frames=0):
        self.lib = load_library()
        cfg = _abi.Config(device, width, height, shard_rank, shard_count, frames_in_flight, int(profile), int(count_traversal), int(pipeline), int(build_flags), int(resident_frames))
        err = C.c_int(0)
        self.ctx = self.lib.vpt_create(C.byref(cfg), C.byref(err))
        if not self.ctx:
            raise VptError("vpt_create failed: %s (no CPU fallback exists)" % _abi.ERR_NAMES.get(err.value, err.value))
        self.width, self.height = width, height
        self.shard_rank, self.shard_count = shard_rank, shard_count

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.vpt_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- PathTracer API
    def set_scene(self, scene, set_camera=True):
        desc, keep = scene.to_desc()
        _check(self.lib, self.ctx, self.lib.vpt_set_scene(self.ctx, C.byref(desc)), "vpt_set_scene")
        del keep
        if set_camera:
            self.set_camera(scene.view_inverse, scene.projection_inverse(self.width / self.height))

    def set_camera(self, view_inverse, projection_inverse):
        _check(self.lib, self.ctx, self.lib.vpt_set_camera(self.ctx, scenes.colmajor(view_inverse), scenes.colmajor(projection_inverse)), "vpt_set_camera")

    def set_params(self, params):
        _check(self.lib, self.ctx, self.lib.vpt_set_params(self.ctx, C.byref(params)), "vpt_set_params")

    def set_volumes(self, volumes):
        """AddVolume / RemoveVolume / SetVolume (PathTracer.h:157-159): replaces the whole list."""
        arr = (_abi.Volume * max(len(volumes), 1))(*volumes)
        _check(self.lib, self.ctx, self.lib.vpt_set_volumes(self.ctx, arr, len(volumes)), "vpt_set_volumes")

    def add_density_grid(self, grid):
        """AddDensityDataToVolume with the .vdb already decoded: float32 [z, y, x] raw densities -> grid index."""
        g = np.ascontiguousarray(grid, np.float32)
        rc = self.lib.vpt_add_density_grid(self.ctx, g.shape[2], g.shape[1], g.shape[0], g.ctypes.data)
        if rc < 0:
            _check(self.lib, self.ctx, rc, "vpt_add_density_grid")
        return rc

    def add_density_bricks(self, dims, coords, values):
        """vpt_add_density_bricks: the grid as a NanoVDB tree holds it.  dims: (dim_x, dim_y, dim_z) of the index box; coords: uint32 [n, 3] brick
        coordinates (bx, by, bz); values: float32 [n, 8, 8, 8] = [brick, z, y, x] raw densities -> grid index (the index space of add_density_grid)."""
        c = np.ascontiguousarray(coords, np.uint32).reshape(-1, 3)
        v = np.ascontiguousarray(values, np.float32).reshape(-1, 8, 8, 8)
        if len(c) != len(v):
            raise ValueError("%d brick coordinates for %d bricks of values" % (len(c), len(v)))
        rc = self.lib.vpt_add_density_bricks(self.ctx, int(dims[0]), int(dims[1]), int(dims[2]), len(c), c.ctypes.data if len(c) else None, v.ctypes.data if len(c) else None)
        if rc < 0:
            _check(self.lib, self.ctx, rc, "vpt_add_density_bricks")
        return rc

    def add_density_grid_sparse(self, grid):
        """add_density_grid's image from the bricks of `grid` (float32 [z, y, x]) that hold a value other than 0: see bricks_of."""
        return self.add_density_bricks(*bricks_of(grid))

    def density_grid_info(self, index):
        """vpt_get_density_grid_info -> {"dim": (x, y, z), "brick_count" (0: dense), "device_bytes", "max_density"}."""
        i = _abi.DensityGridInfo()
        _check(self.lib, self.ctx, self.lib.vpt_get_density_grid_info(self.ctx, index, C.byref(i)), "vpt_get_density_grid_info")
        return {"dim": tuple(i.dim), "brick_count": i.brick_count, "device_bytes": i.device_bytes, "max_density": np.float32(i.max_density)}

    def read_density_grid(self, index, ijk):
        """vpt_read_density_grid (test hook): the raw values the device lookup returns at voxels ijk (int32 [..., 3] = x, y, z; clamped to the index box)."""
        q = np.ascontiguousarray(ijk, np.int32)
        if q.ndim < 1 or q.shape[-1] != 3:
            raise ValueError("ijk must be [..., 3], got %r" % (q.shape,))
        out = np.zeros(q.shape[:-1], np.float32)
        _check(self.lib, self.ctx, self.lib.vpt_read_density_grid(self.ctx, index, q.ctypes.data, out.size, out.ctypes.data), "vpt_read_density_grid")
        return out

    def clear_density_grids(self):
        _check(self.lib, self.ctx, self.lib.vpt_clear_density_grids(self.ctx), "vpt_clear_density_grids")

    def set_atmosphere(self, atm):
        """SetEnableAtmosphere(True) + the planet/density setters; None disables (PathTracer.h:168-179)."""
        _check(self.lib, self.ctx, self.lib.vpt_set_atmosphere(self.ctx, C.byref(atm) if atm is not None else None), "vpt_set_atmosphere")

    def set_phase_function(self, phase):
        _check(self.lib, self.ctx, self.lib.vpt_set_phase_function(self.ctx, phase), "vpt_set_phase_function")

    def set_material(self, index, mat):
        _check(self.lib, self.ctx, self.lib.vpt_set_material(self.ctx, index, C.byref(mat)), "vpt_set_material")

    def get_material(self, index):
        m = _abi.Material()
        _check(self.lib, self.ctx, self.lib.vpt_get_material(self.ctx, index, C.byref(m)), "vpt_get_material")
        return m

    def set_environment(self, env):
        """SetEnvMapFilepath with the .hdr already decoded (vpt_set_environment): float32 [h, w, 4], alpha ignored.  Replaces the
        environment of the installed scene only: no BVH build, no geometry upload."""
        env = np.ascontiguousarray(env, np.float32)
        if env.ndim != 3 or env.shape[2] != 4:
            raise ValueError("environment must be [h, w, 4], got %r" % (env.shape,))
        _check(self.lib, self.ctx, self.lib.vpt_set_environment(self.ctx, env.ctypes.data, env.shape[1], env.shape[0]), "vpt_set_environment")

    def set_instance_transforms(self, first, matrices):
        """vpt_set_instance_transforms: instances first, first + 1, ... take these 4x4 matrices (math layout, as Scene.instances holds them).  The
        installed scene's BVH is refitted on the device: no tree build, no geometry upload."""
        flat = [v for x in matrices for v in scenes.colmajor(x)]
        arr = (C.c_float * max(len(flat), 1))(*flat)
        _check(self.lib, self.ctx, self.lib.vpt_set_instance_transforms(self.ctx, first, len(matrices), arr if flat else None), "vpt_set_instance_transforms")

    def resize(self, w, h):
        _check(self.lib, self.ctx, self.lib.vpt_resize(self.ctx, w, h), "vpt_resize")
        self.width, self.height = w, h

    def reset(self):
        _check(self.lib, self.ctx, self.lib.vpt_reset(self.ctx), "vpt_reset")

    def render(self, dispatches):
        done = C.c_int(0)
        _check(self.lib, self.ctx, self.lib.vpt_render(self.ctx, dispatches, C.byref(done)), "vpt_render")
        return bool(done.value)

    # ---- the asynchronous per-frame form (PathTrace(cmd) / PostProcess(cmd) record and return; include/vpt.h)
    def render_async(self, dispatches):
        """vpt_render_async: enqueues and returns (done, ticket)."""
        done, ticket = C.c_int(0), C.c_uint64(0)
        _check(self.lib, self.ctx, self.lib.vpt_render_async(self.ctx, dispatches, C.byref(done), C.byref(ticket)), "vpt_render_async")
        return bool(done.value), int(ticket.value)

    def postprocess_device(self, post_params=None, rgba8_device=None):
        """vpt_postprocess_device: the post chain behind the render, RGBA8 left on the device (output_device()); returns the ticket."""
        pp = post_params or default_post_params()
        ticket = C.c_uint64(0)
        _check(self.lib, self.ctx, self.lib.vpt_postprocess_device(self.ctx, C.byref(pp), rgba8_device, C.byref(ticket)), "vpt_postprocess_device")
        return int(ticket.value)

    def wait(self, ticket=0):
        """vpt_wait.  ticket 0: everything enqueued so far; otherwise the work up to that ticket (a host that runs one frame ahead of the
        device waits for the PREVIOUS frame's post-process ticket)."""
        _check(self.lib, self.ctx, self.lib.vpt_wait(self.ctx, ticket), "vpt_wait")

    def lab_set(self, key, value):
        """Measurement hooks of include/vpt_lab.h (VPT_LAB_*; laboratory build only): scheduling only, images never depend on them."""
        if not self.lib.has_lab:
            raise VptError("vpt_lab_set: the product library has no laboratory entry points (run with VPT_LAB=1)")
        _check(self.lib, self.ctx, self.lib.vpt_lab_set(self.ctx, key, value), "vpt_lab_set")

    def whole_cull(self):
        """vpt_get_whole_cull: (x0, y0, x1, y1), inclusive — the pixels a whole-path batch rendered now would start paths for."""
        r = (C.c_uint32 * 4)()
        _check(self.lib, self.ctx, self.lib.vpt_get_whole_cull(self.ctx, r), "vpt_get_whole_cull")
        return tuple(int(v) for v in r)

    def lab_whole_culled(self):
        """vpt_lab_whole_culled (laboratory build only): samples the latest vpt_render batch finished without a path."""
        if not self.lib.has_lab:
            raise VptError("vpt_lab_whole_culled: the product library has no laboratory entry points (run with VPT_LAB=1)")
        n = C.c_uint64(0)
        _check(self.lib, self.ctx, self.lib.vpt_lab_whole_culled(self.ctx, C.byref(n)), "vpt_lab_whole_culled")
        return int(n.value)

    def output_device(self):
        """GetOutputImageView(): device pointer of the RGBA8 image (None before the first post-process)."""
        return self.lib.vpt_output_device(self.ctx)

    def output_to_host(self):
        """vpt_get_output: the RGBA8 image the last post-process left on the device, read back (drains)."""
        out = np.empty((self.height, self.width, 4), np.uint8)
        _check(self.lib, self.ctx, self.lib.vpt_get_output(self.ctx, out.ctypes.data), "vpt_get_output")
        return out

    def radiance(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        _check(self.lib, self.ctx, self.lib.vpt_get_radiance(self.ctx, out.ctypes.data), "vpt_get_radiance")
        return out

    def radiance_to_device(self, ptr):
        _check(self.lib, self.ctx, self.lib.vpt_get_radiance_device(self.ctx, ptr), "vpt_get_radiance_device")

    def set_radiance(self, img, frame_count):
        img = np.ascontiguousarray(img, np.float32)
        assert img.shape == (self.height, self.width, 4)
        _check(self.lib, self.ctx, self.lib.vpt_set_radiance(self.ctx, img.ctypes.data, frame_count), "vpt_set_radiance")

    def shard_floats(self):
        return int(self.lib.vpt_shard_floats(self.ctx))

    def shard_to_device(self, ptr):
        _check(self.lib, self.ctx, self.lib.vpt_get_shard_device(self.ctx, ptr), "vpt_get_shard_device")

    def assemble_shards(self, gathered_ptr, shard_count):
        _check(self.lib, self.ctx, self.lib.vpt_assemble_shards(self.ctx, gathered_ptr, shard_count), "vpt_assemble_shards")

    # ---- PostProcessor API
    def postprocess(self, post_params=None, want_bloom=False):
        pp = post_params or default_post_params()
        out = np.empty((self.height, self.width, 4), np.uint8)
        bloom = np.empty((self.height, self.width, 4), np.float32) if want_bloom else None
        _check(self.lib, self.ctx, self.lib.vpt_postprocess(self.ctx, C.byref(pp), out.ctypes.data, bloom.ctypes.data if want_bloom else None), "vpt_postprocess")
        return (out, bloom) if want_bloom else out

    def stats(self):
        s = _abi.Stats()
        _check(self.lib, self.ctx, self.lib.vpt_get_stats(self.ctx, C.byref(s)), "vpt_get_stats")
        d = {k: getattr(s, k) for k, _ in _abi.Stats._fields_ if k not in ("kernel_launches", "kernel_ms", "stack_spills")}
        d["stack_spills"] = [int(s.stack_spills[0]), int(s.stack_spills[1])]
        ms = C.c_double(0.0)                   # kept beside vpt_stats, not in it (vpt.h vpt_get_set_transforms_ms)
        _check(self.lib, self.ctx, self.lib.vpt_get_set_transforms_ms(self.ctx, C.byref(ms)), "vpt_get_set_transforms_ms")
        d["set_transforms_ms"] = ms.value
        d["kernel_launches"] = {n: int(s.kernel_launches[i]) for i, n in enumerate(_abi.KERNEL_NAMES)}
        d["kernel_ms"] = {n: float(s.kernel_ms[i]) for i, n in enumerate(_abi.KERNEL_NAMES)}
        return d

    def reset_stats(self):
        _check(self.lib, self.ctx, self.lib.vpt_reset_stats(self.ctx), "vpt_reset_stats")

    def trace_rays(self, rays):
        rays = np.ascontiguousarray(rays, np.float32)
        hits = np.zeros(len(rays), HIT_DTYPE)
        _check(self.lib, self.ctx, self.lib.vpt_trace_rays(self.ctx, rays.ctypes.data, len(rays), hits.ctypes.data), "vpt_trace_rays")
        return hits

    # ---- picking and guide buffers (include/vpt.h vpt_render_features / vpt_pick)
    FEATURES = ("depth", "ids", "normal", "albedo")

    def render_features(self, mode=FEATURES_CENTER, frame=0, which=FEATURES):
        """vpt_render_features to host memory: {name: array} for the names in `which` — depth float32 [h, w] (t, -1 on a miss), ids uint32 [h, w, 4]
        (instance, primitive, material, mesh; 0xffffffff on a miss), normal and albedo float32 [h, w, 4].  Always the whole image."""
        which = tuple(which)
        bad = [n for n in which if n not in self.FEATURES]
        if bad:
            raise ValueError("unknown feature buffers %r (known: %r)" % (bad, self.FEATURES))
        out = {n: np.zeros((self.height, self.width) + (() if n == "depth" else (4,)), np.uint32 if n == "ids" else np.float32) for n in which}
        fb = _abi.FeatureBuffers(**{n: a.ctypes.data for n, a in out.items()})
        _check(self.lib, self.ctx, self.lib.vpt_render_features(self.ctx, mode, frame, C.byref(fb)), "vpt_render_features")
        return out

    def render_features_device(self, mode=FEATURES_CENTER, frame=0, depth=None, ids=None, normal=None, albedo=None):
        """vpt_render_features into device memory of the context's device: each argument is a device pointer (e.g. a torch tensor's data_ptr()) to
        width*height floats (depth) or width*height*4 words (the others, 16-byte aligned), or None."""
        fb = _abi.FeatureBuffers(depth, ids, normal, albedo, 1, 0)
        _check(self.lib, self.ctx, self.lib.vpt_render_features(self.ctx, mode, frame, C.byref(fb)), "vpt_render_features")

    def pick(self, x, y):
        """vpt_pick: what the FEATURES_CENTER ray of pixel (x, y) hits first -> {"instance", "primitive", "material", "mesh", "t", "u", "v", "position"};
        a miss has the four ids 0xffffffff and t = -1."""
        r = _abi.PickResult()
        _check(self.lib, self.ctx, self.lib.vpt_pick(self.ctx, x, y, C.byref(r)), "vpt_pick")
        return {"instance": r.instance, "primitive": r.primitive, "material": r.material, "mesh": r.mesh, "t": np.float32(r.t), "u": np.float32(r.u),
                "v": np.float32(r.v), "position": np.array(list(r.position), np.float32)}

    # ---- denoising (include/vpt.h vpt_denoise / vpt_denoise_device / vpt_set_post_source)
    def denoise(self, params=None):
        """vpt_denoise: the accumulation image through the edge-avoiding a-trous filter -> float32 [h, w, 4].  The image also stays in the context
        (a snapshot) for set_post_source(POST_SOURCE_DENOISED)."""
        dp = params or default_denoise_params()
        out = np.empty((self.height, self.width, 4), np.float32)
        _check(self.lib, self.ctx, self.lib.vpt_denoise(self.ctx, C.byref(dp), out.ctypes.data), "vpt_denoise")
        return out

    def denoise_device(self, params=None, ptr=None):
        """vpt_denoise_device: enqueued behind the frames in flight; the image is copied to device pointer `ptr` (16-byte aligned, or None) on the
        context's device; returns the ticket."""
        dp = params or default_denoise_params()
        ticket = C.c_uint64(0)
        _check(self.lib, self.ctx, self.lib.vpt_denoise_device(self.ctx, C.byref(dp), ptr, C.byref(ticket)), "vpt_denoise_device")
        return int(ticket.value)

    def set_post_source(self, source):
        """vpt_set_post_source: POST_SOURCE_RADIANCE (default) or POST_SOURCE_DENOISED — the image postprocess / postprocess_device read."""
        _check(self.lib, self.ctx, self.lib.vpt_set_post_source(self.ctx, source), "vpt_set_post_source")

    # ---- temporal accumulation (include/vpt.h vpt_temporal_accumulate / _device / vpt_temporal_reset / vpt_get_temporal_history / vpt_set_denoise_source)
    def temporal_accumulate(self, params=None):
        """vpt_temporal_accumulate: the accumulation image blended with the reprojected previous result -> float32 [h, w, 4].  The image also stays in
        the context (a snapshot) for set_denoise_source(DENOISE_SOURCE_TEMPORAL), and becomes the history of the next call."""
        tp = params or default_temporal_params()
        out = np.empty((self.height, self.width, 4), np.float32)
        _check(self.lib, self.ctx, self.lib.vpt_temporal_accumulate(self.ctx, C.byref(tp), out.ctypes.data), "vpt_temporal_accumulate")
        return out

    def temporal_accumulate_device(self, params=None, ptr=None):
        """vpt_temporal_accumulate_device: enqueued behind the frames in flight; the image is copied to device pointer `ptr` (16-byte aligned, or None)
        on the context's device; returns the ticket."""
        tp = params or default_temporal_params()
        ticket = C.c_uint64(0)
        _check(self.lib, self.ctx, self.lib.vpt_temporal_accumulate_device(self.ctx, C.byref(tp), ptr, C.byref(ticket)), "vpt_temporal_accumulate_device")
        return int(ticket.value)

    def temporal_reset(self):
        """vpt_temporal_reset: drop the history; the next temporal_accumulate starts afresh."""
        _check(self.lib, self.ctx, self.lib.vpt_temporal_reset(self.ctx), "vpt_temporal_reset")

    def temporal_history(self):
        """vpt_get_temporal_history: the history length, in frames, of the latest temporal result -> float32 [h, w] (0 on a miss)."""
        out = np.empty((self.height, self.width), np.float32)
        _check(self.lib, self.ctx, self.lib.vpt_get_temporal_history(self.ctx, out.ctypes.data), "vpt_get_temporal_history")
        return out

    def set_denoise_source(self, source):
        """vpt_set_denoise_source: DENOISE_SOURCE_RADIANCE (default) or DENOISE_SOURCE_TEMPORAL — the image denoise / denoise_device filter."""
        _check(self.lib, self.ctx, self.lib.vpt_set_denoise_source(self.ctx, source), "vpt_set_denoise_source")

    # ---- SVGF (include/vpt.h vpt_set_base_seed / vpt_set_svgf_options / vpt_get_svgf_options / vpt_get_temporal_variance / vpt_get_temporal_moments)
    def set_base_seed(self, base_seed):
        """vpt_set_base_seed: other random numbers from the next frame on.  The accumulation restarts as after set_camera: the temporal history survives."""
        _check(self.lib, self.ctx, self.lib.vpt_set_base_seed(self.ctx, base_seed), "vpt_set_base_seed")

    def set_svgf_options(self, **kw):
        """vpt_set_svgf_options: the context's options with the fields given replaced (variance, sigma_luminance, min_history).  Changing `variance`
        drops the temporal history."""
        o = self.svgf_options()
        for k, v in kw.items():
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, v)
        _check(self.lib, self.ctx, self.lib.vpt_set_svgf_options(self.ctx, C.byref(o)), "vpt_set_svgf_options")

    def svgf_options(self):
        """vpt_get_svgf_options -> SvgfOptions."""
        o = _abi.SvgfOptions()
        _check(self.lib, self.ctx, self.lib.vpt_get_svgf_options(self.ctx, C.byref(o)), "vpt_get_svgf_options")
        return o

    def set_svgf_spatial_options(self, **kw):
        """vpt_set_svgf_spatial_options: the context's options with the fields given replaced (mode, radius, sigma_normal, sigma_depth, min_weight).  With
        mode = 1 and svgf variance = 1, temporal_accumulate gives a young pixel (variance -1) the variance of its neighbourhood's moments.  Keeps the history."""
        o = self.svgf_spatial_options()
        for k, v in kw.items():
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, v)
        _check(self.lib, self.ctx, self.lib.vpt_set_svgf_spatial_options(self.ctx, C.byref(o)), "vpt_set_svgf_spatial_options")

    def svgf_spatial_options(self):
        """vpt_get_svgf_spatial_options -> SvgfSpatialOptions."""
        o = _abi.SvgfSpatialOptions()
        _check(self.lib, self.ctx, self.lib.vpt_get_svgf_spatial_options(self.ctx, C.byref(o)), "vpt_get_svgf_spatial_options")
        return o

    def temporal_variance(self):
        """vpt_get_temporal_variance: the luminance variance of the latest temporal result made with variance = 1 -> float32 [h, w]
        (-1: history shorter than min_history images; 0 on a miss)."""
        out = np.empty((self.height, self.width), np.float32)
        _check(self.lib, self.ctx, self.lib.vpt_get_temporal_variance(self.ctx, out.ctypes.data), "vpt_get_temporal_variance")
        return out

    def temporal_moments(self):
        """vpt_get_temporal_moments: first and second luminance moment of the latest temporal result made with variance = 1 -> float32 [h, w, 2]."""
        out = np.empty((self.height, self.width, 2), np.float32)
        _check(self.lib, self.ctx, self.lib.vpt_get_temporal_moments(self.ctx, out.ctypes.data), "vpt_get_temporal_moments")
        return out

    # ---- outlier rejection ahead of the two filters (include/vpt.h vpt_set_firefly_options / vpt_get_firefly_options / vpt_get_firefly_state / vpt_get_firefly_image)
    def set_firefly_options(self, **kw):
        """vpt_set_firefly_options: the context's options with the fields given replaced (mode, radius, rank, threshold, floor).  With mode = 1
        temporal_accumulate and denoise (from the radiance source) first scale down every hit pixel whose luminance exceeds max(threshold * the rank-th largest
        of its neighbours, floor) and filter that image; the accumulation image keeps its bits.  A bias: the clamp removes energy.  Keeps the history."""
        o = self.firefly_options()
        for k, v in kw.items():
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, v)
        _check(self.lib, self.ctx, self.lib.vpt_set_firefly_options(self.ctx, C.byref(o)), "vpt_set_firefly_options")

    def firefly_options(self):
        """vpt_get_firefly_options -> FireflyOptions."""
        o = _abi.FireflyOptions()
        _check(self.lib, self.ctx, self.lib.vpt_get_firefly_options(self.ctx, C.byref(o)), "vpt_get_firefly_options")
        return o

    def firefly_state(self):
        """vpt_get_firefly_state -> FireflyState of the latest filtered call (waits for the work in flight): clamped and considered pixels, filtered calls
        since mode went to 1.  Zeros before the first filtered call of the current size."""
        s = _abi.FireflyState()
        _check(self.lib, self.ctx, self.lib.vpt_get_firefly_state(self.ctx, C.byref(s)), "vpt_get_firefly_state")
        return s

    def firefly_image(self):
        """vpt_get_firefly_image: the image the latest filtered call handed to its filter -> float32 [h, w, 4]."""
        out = np.empty((self.height, self.width, 4), np.float32)
        _check(self.lib, self.ctx, self.lib.vpt_get_firefly_image(self.ctx, out.ctypes.data), "vpt_get_firefly_image")
        return out

    # ---- the temporal history across instance moves (include/vpt.h vpt_set_temporal_options / vpt_get_temporal_options / vpt_get_temporal_motion)
    def set_temporal_options(self, **kw):
        """vpt_set_temporal_options: the context's options with the fields given replaced (instance_motion).  With instance_motion = 1
        set_instance_transforms keeps the temporal history and temporal_accumulate reprojects it through the move.  Changing it drops the history."""
        o = self.temporal_options()
        for k, v in kw.items():
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, v)
        _check(self.lib, self.ctx, self.lib.vpt_set_temporal_options(self.ctx, C.byref(o)), "vpt_set_temporal_options")

    def temporal_options(self):
        """vpt_get_temporal_options -> TemporalOptions."""
        o = _abi.TemporalOptions()
        _check(self.lib, self.ctx, self.lib.vpt_get_temporal_options(self.ctx, C.byref(o)), "vpt_get_temporal_options")
        return o

    def temporal_motion(self):
        """vpt_get_temporal_motion: where the previous image saw each pixel's surface, minus the pixel's own coordinates, of the latest temporal result
        made with instance_motion = 1 -> float32 [h, w, 2] ((0, 0) on a miss and wherever nothing was reprojected)."""
        out = np.empty((self.height, self.width, 2), np.float32)
        _check(self.lib, self.ctx, self.lib.vpt_get_temporal_motion(self.ctx, out.ctypes.data), "vpt_get_temporal_motion")
        return out

    # ---- auto-exposure (include/vpt.h vpt_set_exposure_options / vpt_get_exposure_options / vpt_get_exposure_state / vpt_get_exposure_histogram / vpt_exposure_reset)
    def set_exposure_options(self, **kw):
        """vpt_set_exposure_options: the context's options with the fields given replaced (mode, min_log2, max_log2, low_percentile, high_percentile, key,
        compensation_log2, min_exposure_log2, max_exposure_log2, rate_up, rate_down).  With mode = 1 every postprocess / postprocess_device meters its source
        image on the device and the tonemap multiplies by exposure * the adapted scale.  Changing `mode` starts the adapted state afresh; nothing else does."""
        o = self.exposure_options()
        for k, v in kw.items():
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, v)
        _check(self.lib, self.ctx, self.lib.vpt_set_exposure_options(self.ctx, C.byref(o)), "vpt_set_exposure_options")

    def exposure_options(self):
        """vpt_get_exposure_options -> ExposureOptions."""
        o = _abi.ExposureOptions()
        _check(self.lib, self.ctx, self.lib.vpt_get_exposure_options(self.ctx, C.byref(o)), "vpt_get_exposure_options")
        return o

    def exposure_state(self):
        """vpt_get_exposure_state -> ExposureState (waits for the work in flight).  scale 1 and valid 0 with the option off or before the first metering."""
        s = _abi.ExposureState()
        _check(self.lib, self.ctx, self.lib.vpt_get_exposure_state(self.ctx, C.byref(s)), "vpt_get_exposure_state")
        return s

    def exposure_histogram(self):
        """vpt_get_exposure_histogram: the 256 bin counts of the latest metering -> uint32 [256]."""
        out = np.empty(_abi.EXPOSURE_BINS, np.uint32)
        _check(self.lib, self.ctx, self.lib.vpt_get_exposure_histogram(self.ctx, out.ctypes.data), "vpt_get_exposure_histogram")
        return out

    def exposure_reset(self):
        """vpt_exposure_reset: the next metering jumps to its target instead of blending towards it."""
        _check(self.lib, self.ctx, self.lib.vpt_exposure_reset(self.ctx), "vpt_exposure_reset")


HIT_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("primitive", "<u4"), ("instance", "<u4")])
