"""Auto-exposure on the host: compiles tests/tools/exposure_driver.cpp (csrc/exposure.hpp's bin_of, meter and adapt) and runs it over a sequence of
meterings.  Shared by tests/test_exposure_cpu.py and tests/test_gpu_exposure.py, which holds the device to these bits."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vulkan-path-tracer_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "tools", "exposure_driver.cpp")
RESET_NONE, RESET_JUMP, RESET_ALL = 0, 1, 2   # exposure.hpp kReset*
STATE_FIELDS = ("scale", "cur_log2", "target_log2", "avg_log2", "valid", "meterings", "counted")
STATE_DTYPE = np.dtype([("scale", "<f4"), ("cur_log2", "<f4"), ("target_log2", "<f4"), ("avg_log2", "<f4"), ("valid", "<u4"), ("meterings", "<u4"), ("counted", "<u8")])
STEP_DTYPE = np.dtype([("state", STATE_DTYPE), ("hist", "<u4", 256), ("lo", "<u8"), ("hi", "<u8"), ("S", "<u8"), ("W", "<u8"), ("has_target", "<u4"), ("pad", "<u4")])


def compile_driver(exe, extra=()):
    """(the flags of denoise_host.compile_driver)"""
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math", "-march=x86-64-v3"] + list(extra) +
                          ["-I" + CSRC, DRIVER, "-o", exe])
    return exe


def write_input(path, options, steps):
    """steps: a list of (kind, payload, reset) with kind "image" (float32 [h, w, 4]), "hist" (uint32 [256]) or "bins" (float32 [h, w, 4])."""
    with open(path, "wb") as f:
        f.write(bytes(options))
        f.write(struct.pack("<I", len(steps)))
        for kind, payload, reset in steps:
            if kind == "hist":
                h = np.ascontiguousarray(payload, np.uint32)
                assert h.shape == (256,)
                f.write(struct.pack("<4I", 1, reset, 0, 0))
                f.write(h.tobytes())
            else:
                img = np.ascontiguousarray(payload, np.float32)
                assert img.ndim == 3 and img.shape[2] == 4
                f.write(struct.pack("<4I", 0 if kind == "image" else 2, reset, img.shape[1], img.shape[0]))
                f.write(img.tobytes())


def run(exe, tmp, options, steps):
    """-> one entry per step: a numpy record (STEP_DTYPE) for "image" / "hist" steps, a uint32 [h, w] array of bins for "bins" steps."""
    src, dst = os.path.join(str(tmp), "exposure.in"), os.path.join(str(tmp), "exposure.out")
    write_input(src, options, steps)
    subprocess.check_call([exe, src, dst])
    raw = open(dst, "rb").read()
    out, at = [], 0
    for kind, payload, _ in steps:
        if kind == "bins":
            h, w = payload.shape[:2]
            out.append(np.frombuffer(raw, "<u4", h * w, at).reshape(h, w).copy())
            at += h * w * 4
        else:
            out.append(np.frombuffer(raw, STEP_DTYPE, 1, at)[0].copy())
            at += STEP_DTYPE.itemsize
    assert at == len(raw)
    return out


def state_tuple(s):
    """A state — a driver record or the library's ExposureState — as raw words: floats by their bits, so equality is bit for bit."""
    get = (lambda k: s[k]) if isinstance(s, (np.void, np.ndarray)) else (lambda k: getattr(s, k))
    bits = tuple(int(np.float32(get(k)).view(np.uint32)) for k in STATE_FIELDS[:4])
    return bits + tuple(int(get(k)) for k in STATE_FIELDS[4:])


assert STATE_DTYPE.itemsize == 32 and STEP_DTYPE.itemsize == 32 + 1024 + 32 + 8
