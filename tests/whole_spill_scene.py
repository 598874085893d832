"""A scene that rides in LDS (at most 3 KB of fp32 nodes and triangles: scene_prep.hpp rides_in_lds) and whose tree is a CHAIN, for the tests of
the whole-path kernel's shorter LDS stack (traverse.hpp kWholeStackRows = 6; tests/test_stack_bound_cpu.py, tests/test_gpu_whole_refill.py).
Sheets stacked along z with gaps that halve towards the bottom: the SAH builder peels the lonely upper sheets off one at a time, so a four-wide
node holds three leaves and the rest of the stack, level after level, and a ray that comes from below crosses every box, goes down the chain
first and leaves three siblings on its stack per level.  Floor, light and camera as in tests/test_gpu_spills.py: the camera looks down at the
floor from under the stack, so bounce rays and the rays towards the light go up through the sheets.
memory_chain_scene is the same geometry with 40 sheets whose gaps shrink by 1.5 instead of 2: 84 triangles, too many for LDS, so the tree lives
in memory, and deep enough that searches overflow the 14 LDS rows of every other traversal kernel too (tests/test_gpu_spill_schedules.py; its
premise on the host: tests/test_stack_bound_cpu.py).  Not a test module."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SHEETS = 16
MID_STACK_WINDOW = (3.3, 4.5)    # (tmin, tmax) that begin and end between memory_chain_scene's sheets for rays from the floor (a vertical one crosses them at t = 3 .. 6)


def chain_scene(vpt, sheets=SHEETS):
    return sheets_scene(vpt, (-1.5 + 3.0 * 0.5 ** np.arange(sheets - 1, -1, -1)).astype(F32))       # gaps 3/2, 3/4, ... from the top down


def memory_chain_scene(vpt, sheets=40, ratio=1.5):
    return sheets_scene(vpt, (-1.5 + 3.0 * ratio ** (np.arange(sheets) - (sheets - 1))).astype(F32))


def sheets_scene(vpt, z):
    """Quads of half width 1 at the heights z, over the floor and under the light."""
    S = vpt.scenes
    sc = S.Scene()
    sc.luts = S.load_luts()
    sheets = len(z)
    corners = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], F32)
    pos = np.zeros((sheets, 4, 3), F32)
    pos[:, :, :2] = corners[None]
    pos[:, :, 2] = z[:, None]
    idx = (np.arange(sheets, dtype=np.uint32)[:, None] * 4 + np.array([0, 1, 2, 0, 2, 3], np.uint32)[None]).reshape(-1)
    nrm = np.tile(np.array([0, 0, -1], F32), (sheets * 4, 1))
    m_stack = sc.add_mesh(pos.reshape(-1, 3), nrm, np.zeros((sheets * 4, 2), F32), idx)

    def quad(zq, half, normal_z):
        p = np.array([[-half, -half, zq], [half, -half, zq], [half, half, zq], [-half, half, zq]], F32)
        order = [0, 1, 2, 0, 2, 3] if normal_z > 0 else [0, 2, 1, 0, 3, 2]
        return sc.add_mesh(p, np.tile(np.array([0, 0, normal_z], F32), (4, 1)), np.zeros((4, 2), F32), np.array(order, np.uint32))
    m_floor, m_light = quad(-4.5, 6.0, 1.0), quad(4.0, 3.0, -1.0)
    sc.materials.append(S.material(base_color=(0.7, 0.7, 0.65)))
    sc.materials.append(S.material(base_color=(0.2, 0.5, 0.8), roughness=0.6))
    sc.materials.append(S.material(base_color=(1, 1, 1), emissive_color=(40, 36, 30)))
    sc.add_instance(m_floor, 0); sc.add_instance(m_stack, 1); sc.add_instance(m_light, 2)
    sc.view_inverse = np.linalg.inv(S.look_at((0.0, 0.0, -1.7), (0.0, 0.0, -4.5), (0.0, 1.0, 0.0))).astype(F32)
    return sc


def world_triangles(sc):
    """The scene's triangles as the builder takes them: 12 dwords each (v0, e1, e2, prim, inst, gid), instance-major."""
    recs = []
    for inst, (mesh, _mat, m) in enumerate(sc.instances):
        v, idx = sc.meshes[mesh]
        p = np.concatenate([v["position"].astype(F32), np.ones((len(v), 1), F32)], axis=1) @ np.asarray(m, F32).T
        p = p[:, :3].astype(F32)
        for t, (i0, i1, i2) in enumerate(idx.reshape(-1, 3)):
            rec = np.zeros(12, F32)
            rec[0:3] = p[i0]; rec[3:6] = p[i1] - p[i0]; rec[6:9] = p[i2] - p[i0]
            rec[9:12] = np.array([t, inst, len(recs)], np.uint32).view(F32)
            recs.append(rec)
    return np.ascontiguousarray(np.stack(recs), F32)


def stack_bound_lib(out_dir):
    out = os.path.join(str(out_dir), "libstack_bound_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "stack_bound_host.cpp"),
                           os.path.join(ROOT, "vulkan-path-tracer_amd", "csrc", "bvh_build.cpp"), "-o", out])
    L = C.CDLL(out)
    L.sb_tree.restype = None
    L.sb_tree.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.sb_rays.restype = None
    L.sb_rays.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.sb_tree_ex.restype = None
    L.sb_tree_ex.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.sb_rays_ex.restype = None
    L.sb_rays_ex.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p]
    return L


def tree_facts(L, tris, sbvh=False):
    out = np.zeros(5, np.int32)
    L.sb_tree_ex(tris.ctypes.data, len(tris), int(sbvh), out.ctypes.data)
    return dict(zip(("nodes", "leaf_tris", "lds_bytes", "levels", "stack_bound"), (int(v) for v in out)))


def ray_depths(L, tris, o, d, prune, sbvh=False, tmin=0.01, tmax=100000.0):
    o, d = np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32)
    sp = np.zeros(len(o), np.int32)
    L.sb_rays_ex(tris.ctypes.data, len(tris), int(sbvh), len(o), o.ctypes.data, d.ctypes.data, tmin, tmax, int(prune), sp.ctypes.data)
    return sp
