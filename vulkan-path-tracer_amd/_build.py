"""Builds libvpt_hip.so (HIP kernels + C-ABI) for gfx950 with hipcc, in-tree.

-ffp-contract=off and no fast-math are part of the parity contract (include/vpt_fp32.h): the only
fused multiply-adds in the binary are the explicit vptfp::fma() calls.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libvpt_hip.so")
# The LABORATORY build: the same sources with -DVPT_LAB=1 plus LAB_SOURCES — every kernel variant that was measured against the product kernels and found
# slower, round 1's stage kernels (VPT_PIPELINE_STAGED_R1) and the vpt_lab_* entry points of include/vpt_lab.h (api_lab.hip).  The product library has none of it.
LIB_LAB = os.path.join(HERE, "libvpt_hip_lab.so")
SOURCES = ["kernels_whole.hip", "kernels_bounce.hip", "kernels_trace.hip", "kernels_stream.hip", "kernels_post.hip",
           "api_context.hip", "api_scene.hip", "api_render.hip", "api_post.hip", "api_comm.hip", "bvh_build.cpp"]   # (the api_*.hip files hold no kernel: no fat binary, no per-file flag)
LAB_SOURCES = ["kernels_lab_r1.hip", "api_lab.hip"]   # compiled and linked into the laboratory library only
# (kernels_lut.hip is a header here: kernels_post.hip includes it — the two share their flags, and one fat binary with its page padding less is 10 KB of the
# product's size bound, DESIGN.md "Library size"; kernels_finish.hip likewise inside kernels_stream.hip and kernels_aux.hip inside kernels_trace.hip, each pair
# with -fno-slp-vectorize on both sides: 8 KB each, the room auto-exposure needed; kernels_media.hip inside kernels_bounce.hip on the same terms: 12 KB, the
# firefly filter's room)
HEADERS = ["kernels_lut.hip", "kernels_finish.hip", "kernels_aux.hip", "kernels_media.hip", "firefly.hpp", "exposure.hpp", "post_plan.hpp", "device_types.hpp", "path_plan.hpp", "scene_prep.hpp", "grid_prep.hpp", "denoise.hpp", "temporal.hpp", "svgf_spatial.hpp", "kernels.hpp", "api_ctx.hpp", "shading.hpp", "traverse.hpp", "bvh_build.hpp", "bvh_refit.hpp", "volume.hpp", "atmosphere.hpp", "wave.hpp", "wave_cursor.hpp", "shade_core.hpp", "vote.hpp", "slab.hpp", "node_step.hpp", "whole_refill.hpp", "whole_args.hpp", "whole_deal.hpp", "camera.hpp", "camera_cull.hpp",
           os.path.join("..", "..", "include", "vpt.h"), os.path.join("..", "..", "include", "vpt_lab.h"), os.path.join("..", "..", "include", "vpt_fp32.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wno-unused-result", "-Wno-pass-failed"]
# Per-file additions.  The traversal kernels are VALU-issue-bound and their triangle test is 51 scalar fp32 operations: the SLP
# vectoriser turns 28 of them into 14 packed ones at the price of 20-30 register moves to pair the operands up
# (profiles/r03_trace_isa_budget.md), a net loss in issued instructions, so it is off for that file.  Values are unaffected:
# packed and scalar fp32 operations round identically and no contraction is allowed either way.
EXTRA_FLAGS = {f: ["-fno-slp-vectorize"] for f in ("kernels_trace.hip", "kernels_stream.hip", "kernels_media.hip", "kernels_whole.hip", "kernels_finish.hip", "kernels_bounce.hip", "kernels_aux.hip", "kernels_lab_r1.hip")}
# The host layer (no kernel in these files, nothing in them is timed) is compiled for size: the product library's size bound (tests/test_abi.py) is a few
# KB away, and -Os on these five takes ~10 KB off it.
EXTRA_FLAGS.update({f: ["-Os"] for f in ("api_context.hip", "api_scene.hip", "api_render.hip", "api_post.hip", "api_comm.hip")})
# The host BVH builder at -O2 (the later -O wins): 7 KB less of unrolled and vectorised loops; its time is what vpt_stats.bvh_build_ms reports.
EXTRA_FLAGS["bvh_build.cpp"] = ["-O2"]
# The post chain's launch wrappers (host code in a kernel file, 13 KB of it when this flag was taken, a handful of calls per vpt_postprocess; like every
# launch_* wrapper they pick a kernel's instantiation as a pointer and launch ONCE, each launch site being argument marshalling the size bound pays for:
# DESIGN.md §9) for size too, on the HOST pass alone:
# -Xarch_host keeps the flag from the device pass, so the kernels are compiled as before.  4.4 KB, which the camera cull's host code (camera_cull.hpp,
# 3 KB) needed under the size bound.
EXTRA_FLAGS["kernels_post.hip"] = ["-Xarch_host", "-Os"]


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _sources(lab):
    return SOURCES + (LAB_SOURCES if lab else [])


def source_id(defines=("-DVPT_LAB=0",)):
    """sha256 (16 hex digits) over everything the library is compiled from: kernel sources (LAB_SOURCES too when the -D list says -DVPT_LAB=1), headers,
    this file's flags and the build's -D list (the product's is -DVPT_LAB=0; the laboratory build and tests/tools/build_variant.py pass theirs, so a
    variant never carries the product's id).
    profiles/traffic.json carries the id of the build its rocprofv3 counters were collected on; bench.py copies an entry only when it equals the current one."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(_sources("-DVPT_LAB=1" in defines)) + sorted(HEADERS):
        h.update(open(os.path.join(CSRC, f), "rb").read())
    h.update(repr((FLAGS, sorted(EXTRA_FLAGS.items()), sorted(defines))).encode())
    return h.hexdigest()[:16]


def needs_build(lab=False):
    lib = LIB_LAB if lab else LIB
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    # (this file holds the compiler flags: a change here rebuilds too)
    return os.path.getmtime(__file__) > t or any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in _sources(lab) + HEADERS)


def build(force=False, verbose=False, lab=False):
    lib = LIB_LAB if lab else LIB
    if not force and not needs_build(lab):
        return lib
    import fcntl
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
    with open(os.path.join(HERE, "build", ".lock"), "w") as lock:   # one builder at a time (pytest-xdist workers, a bench beside a test run): the others find the library built
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not needs_build(lab):
            return lib
        return _build_locked(lib, force, verbose, lab)


def _build_locked(lib, force, verbose, lab):
    objs = []
    procs = []
    objdir = os.path.join(HERE, "build", "lab" if lab else "product")
    os.makedirs(objdir, exist_ok=True)
    newest_header = max([os.path.getmtime(__file__)] + [os.path.getmtime(os.path.join(CSRC, h)) for h in HEADERS])
    for src in _sources(lab):
        obj = os.path.join(objdir, src + ".o")
        objs.append(obj)
        if not force and os.path.exists(obj) and os.path.getmtime(obj) > max(newest_header, os.path.getmtime(os.path.join(CSRC, src))):
            continue   # this object is newer than its source and every header
        cmd = [hipcc()] + FLAGS + ["-DVPT_LAB=%d" % (1 if lab else 0)] + EXTRA_FLAGS.get(src, []) + (["-x", "hip"] if src.endswith(".cpp") else []) + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for src, p in procs:
        out = p.communicate()[0].decode()
        if p.returncode != 0:
            raise RuntimeError("hipcc failed on %s:\n%s" % (src, out))
        if verbose and out.strip():
            print(out)
    return link(lib, objs)


def link(lib, objs):
    """Links objs into lib.  Only the C ABI (vpt_*, vpt_lab_*) is exported: every source file is a fat binary of its own, padded to whole 4 KB pages inside
    the library, and the dynamic symbol table of the C++ launchers between them is what the product's size bound (tests/test_abi.py) does not have room for."""
    exports = os.path.join(HERE, "build", "exports.map")
    with open(exports, "w") as f:
        f.write("{ global: vpt_*; local: *; };\n")
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs +
                          ["-L/opt/rocm/lib", "-lrccl", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--strip-all", "-Wl,--gc-sections", "-Wl,--version-script=" + exports])
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True, lab="--lab" in sys.argv))
