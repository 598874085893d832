"""vpt_svgf_options: sizeof and every field offset, as gcc lays out include/vpt.h, against the ctypes mirror (the technique of tests/test_temporal_abi_cpu.py),
the defaults on both sides, that every new entry point is declared, mirrored and exported, and the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vpt_set_base_seed", "vpt_default_svgf_options", "vpt_set_svgf_options", "vpt_get_svgf_options", "vpt_get_temporal_variance", "vpt_get_temporal_moments")


def test_svgf_options_match_the_compiled_header(vpt, tmp_path):
    cls = vpt._abi.SvgfOptions
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vpt.h"', 'int main(void) {', 'printf("%zu", sizeof(vpt_svgf_options));']
    for fname, _ in cls._fields_:
        lines.append('printf(" %%zu", offsetof(vpt_svgf_options, %s));' % fname)
    lines += ['printf("\\n%zu %zu %zu\\n", sizeof(vpt_temporal_params), sizeof(vpt_denoise_params), sizeof(vpt_stats));', 'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.check_output([exe], text=True).strip().splitlines()
    tok = [int(t) for t in out[0].split()]
    assert tok[0] == C.sizeof(cls) == 16 and len(tok) == 1 + len(cls._fields_)
    assert [getattr(cls, f).offset for f, _ in cls._fields_] == tok[1:] == [0, 4, 8, 12]
    # the structs the existing calls take keep their layout
    a = vpt._abi
    assert [int(t) for t in out[1].split()] == [C.sizeof(a.TemporalParams), C.sizeof(a.DenoiseParams), C.sizeof(a.Stats)]
    assert (C.sizeof(a.TemporalParams), C.sizeof(a.DenoiseParams)) == (24, 24)


def test_defaults_agree_on_both_sides(vpt):
    lib = vpt.load_library()
    p = vpt.SvgfOptions(9, 9.0, 9, 9)
    lib.vpt_default_svgf_options(C.byref(p))
    q = vpt.default_svgf_options()
    for k in ("variance", "sigma_luminance", "min_history", "reserved"):
        assert getattr(p, k) == getattr(q, k), k
    assert (p.variance, p.sigma_luminance, p.min_history, p.reserved) == (0, 4.0, 4, 0)
    lib.vpt_default_svgf_options(None)   # a NULL pointer is ignored
    assert vpt.default_svgf_options(variance=1, min_history=2).min_history == 2
    with pytest.raises(AttributeError):
        vpt.default_svgf_options(history=1)


def test_entry_points_are_declared_mirrored_and_exported(vpt):
    hdr = open(os.path.join(ROOT, "include", "vpt.h")).read()
    lib = vpt.load_library()
    for name in ENTRIES:
        assert re.search(r"\b(int|void) %s\(" % name, hdr) and name in vpt._abi.PROTOTYPES and hasattr(lib, name), name
    for m in ("set_base_seed", "set_svgf_options", "svgf_options", "temporal_variance", "temporal_moments"):
        assert hasattr(vpt.PathTracer, m)
    # the viewport loop is documented with the reseed in it
    assert "vpt_set_camera -> vpt_set_base_seed(frame_index) -> vpt_render(k) -> vpt_temporal_accumulate -> vpt_denoise -> vpt_postprocess" in hdr


def test_null_arguments_are_refused_without_a_device(vpt):
    lib = vpt.load_library()
    o = vpt.default_svgf_options()
    assert lib.vpt_set_base_seed(None, 7) == -1            # VPT_ERR_INVALID_ARGUMENT
    assert lib.vpt_set_svgf_options(None, C.byref(o)) == -1
    assert lib.vpt_get_svgf_options(None, C.byref(o)) == -1
    assert lib.vpt_get_temporal_variance(None, None) == -1
    assert lib.vpt_get_temporal_moments(None, None) == -1
