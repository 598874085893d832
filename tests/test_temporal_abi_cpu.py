"""vpt_temporal_params: sizeof and every field offset, as gcc lays out include/vpt.h, against the ctypes mirror (the technique of tests/test_abi.py's
test_ctypes_mirror_matches_the_compiled_header), the constants, the defaults on both sides, and the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vpt_default_temporal_params", "vpt_temporal_accumulate", "vpt_temporal_accumulate_device", "vpt_temporal_reset", "vpt_get_temporal_history", "vpt_set_denoise_source")


def test_temporal_params_match_the_compiled_header(vpt, tmp_path):
    a = vpt._abi
    cls = a.TemporalParams
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vpt.h"', 'int main(void) {', 'printf("%zu", sizeof(vpt_temporal_params));']
    for fname, _ in cls._fields_:
        lines.append('printf(" %%zu", offsetof(vpt_temporal_params, %s));' % fname)
    lines += ['printf("\\n%u %u %u %u\\n", VPT_TEMPORAL_DEMODULATE, VPT_TEMPORAL_MATCH_INSTANCE, VPT_DENOISE_SOURCE_RADIANCE, VPT_DENOISE_SOURCE_TEMPORAL);', 'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.check_output([exe], text=True).strip().splitlines()
    tok = [int(t) for t in out[0].split()]
    assert tok[0] == C.sizeof(cls) == 24 and len(tok) == 1 + len(cls._fields_)
    assert [getattr(cls, f).offset for f, _ in cls._fields_] == tok[1:] == [0, 4, 8, 12, 16]
    assert [int(t) for t in out[1].split()] == [a.TEMPORAL_DEMODULATE, a.TEMPORAL_MATCH_INSTANCE, a.DENOISE_SOURCE_RADIANCE, a.DENOISE_SOURCE_TEMPORAL] == [1, 2, 0, 1]
    assert (vpt.TEMPORAL_DEMODULATE, vpt.TEMPORAL_MATCH_INSTANCE, vpt.DENOISE_SOURCE_RADIANCE, vpt.DENOISE_SOURCE_TEMPORAL) == (1, 2, 0, 1)


def test_defaults_agree_on_both_sides(vpt):
    lib = vpt.load_library()
    p = vpt._abi.TemporalParams(9, 9.0, 9.0, 9, (9, 9))
    lib.vpt_default_temporal_params(C.byref(p))
    q = vpt.default_temporal_params()
    for k in ("max_history", "depth_tolerance", "normal_threshold", "flags"):
        assert getattr(p, k) == getattr(q, k), k
    assert list(p.reserved) == list(q.reserved) == [0, 0]
    assert (p.max_history, p.flags) == (32, vpt.TEMPORAL_DEMODULATE | vpt.TEMPORAL_MATCH_INSTANCE)
    assert (round(p.depth_tolerance, 6), round(p.normal_threshold, 6)) == (0.02, 0.9)
    lib.vpt_default_temporal_params(None)   # a NULL pointer is ignored
    assert vpt.default_temporal_params(max_history=4, flags=0).max_history == 4
    with pytest.raises(AttributeError):
        vpt.default_temporal_params(history=1)


def test_entry_points_are_declared_mirrored_and_exported(vpt):
    hdr = open(os.path.join(ROOT, "include", "vpt.h")).read()
    lib = vpt.load_library()
    for name in ENTRIES:
        assert re.search(r"\b(int|void) %s\(" % name, hdr) and name in vpt._abi.PROTOTYPES and hasattr(lib, name), name
    for m in ("temporal_accumulate", "temporal_accumulate_device", "temporal_reset", "temporal_history", "set_denoise_source"):
        assert hasattr(vpt.PathTracer, m)


def test_null_arguments_are_refused_without_a_device(vpt):
    lib = vpt.load_library()
    p = vpt.default_temporal_params()
    assert lib.vpt_temporal_accumulate(None, C.byref(p), None) == -1            # VPT_ERR_INVALID_ARGUMENT
    assert lib.vpt_temporal_accumulate_device(None, C.byref(p), None, None) == -1
    assert lib.vpt_temporal_reset(None) == -1
    assert lib.vpt_get_temporal_history(None, None) == -1
    assert lib.vpt_set_denoise_source(None, 0) == -1
