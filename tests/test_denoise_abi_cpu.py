"""vpt_denoise_params: sizeof and every field offset, as gcc lays out include/vpt.h, against the ctypes mirror (the technique of tests/test_abi.py's
test_ctypes_mirror_matches_the_compiled_header), the constants, the defaults on both sides, and the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vpt_default_denoise_params", "vpt_denoise", "vpt_denoise_device", "vpt_set_post_source")


def test_denoise_params_match_the_compiled_header(vpt, tmp_path):
    a = vpt._abi
    cls = a.DenoiseParams
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vpt.h"', 'int main(void) {', 'printf("%zu", sizeof(vpt_denoise_params));']
    for fname, _ in cls._fields_:
        lines.append('printf(" %%zu", offsetof(vpt_denoise_params, %s));' % fname)
    lines += ['printf("\\n%u %u %u %u\\n", VPT_DENOISE_DEMODULATE, VPT_DENOISE_MAX_ITERATIONS, VPT_POST_SOURCE_RADIANCE, VPT_POST_SOURCE_DENOISED);', 'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.check_output([exe], text=True).strip().splitlines()
    tok = [int(t) for t in out[0].split()]
    assert tok[0] == C.sizeof(cls) == 24 and len(tok) == 1 + len(cls._fields_)
    assert [getattr(cls, f).offset for f, _ in cls._fields_] == tok[1:] == [0, 4, 8, 12, 16, 20]
    assert [int(t) for t in out[1].split()] == [a.DENOISE_DEMODULATE, a.DENOISE_MAX_ITERATIONS, a.POST_SOURCE_RADIANCE, a.POST_SOURCE_DENOISED] == [1, 6, 0, 1]
    assert (vpt.DENOISE_DEMODULATE, vpt.DENOISE_MAX_ITERATIONS, vpt.POST_SOURCE_RADIANCE, vpt.POST_SOURCE_DENOISED) == (1, 6, 0, 1)


def test_defaults_agree_on_both_sides(vpt):
    lib = vpt.load_library()
    p = vpt._abi.DenoiseParams(9, 9.0, 9.0, 9.0, 9, 9)
    lib.vpt_default_denoise_params(C.byref(p))
    q = vpt.default_denoise_params()
    for k, _ in vpt._abi.DenoiseParams._fields_:
        assert getattr(p, k) == getattr(q, k), k
    assert (p.iterations, p.flags, p.reserved) == (5, vpt.DENOISE_DEMODULATE, 0)
    assert (p.sigma_color, round(p.sigma_normal, 6), round(p.sigma_depth, 6)) == (1.0, 0.1, 0.05)
    lib.vpt_default_denoise_params(None)   # a NULL pointer is ignored
    assert vpt.default_denoise_params(iterations=2, flags=0).iterations == 2
    with pytest.raises(AttributeError):
        vpt.default_denoise_params(sigma=1.0)


def test_entry_points_are_declared_mirrored_and_exported(vpt):
    hdr = open(os.path.join(ROOT, "include", "vpt.h")).read()
    lib = vpt.load_library()
    for name in ENTRIES:
        assert re.search(r"\b(int|void) %s\(" % name, hdr) and name in vpt._abi.PROTOTYPES and hasattr(lib, name), name
    for m in ("denoise", "denoise_device", "set_post_source"):
        assert hasattr(vpt.PathTracer, m)


def test_null_arguments_are_refused_without_a_device(vpt):
    lib = vpt.load_library()
    p = vpt.default_denoise_params()
    assert lib.vpt_denoise(None, C.byref(p), None) == -1            # VPT_ERR_INVALID_ARGUMENT
    assert lib.vpt_denoise_device(None, C.byref(p), None, None) == -1
    assert lib.vpt_set_post_source(None, 0) == -1
