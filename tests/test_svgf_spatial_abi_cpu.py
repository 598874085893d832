"""vpt_svgf_spatial_options: sizeof and every field offset, as gcc lays out include/vpt.h, against the ctypes mirror (the technique of
tests/test_svgf_abi_cpu.py), the defaults on both sides, that the three entry points are declared, mirrored and exported, and the argument checks that need
no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vpt_default_svgf_spatial_options", "vpt_set_svgf_spatial_options", "vpt_get_svgf_spatial_options")
FIELDS = ("mode", "radius", "sigma_normal", "sigma_depth", "min_weight")
DEFAULTS = (0, 3, 0.1, 0.05, 4.0)


def test_spatial_options_match_the_compiled_header(vpt, tmp_path):
    cls = vpt._abi.SvgfSpatialOptions
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vpt.h"', 'int main(void) {', 'printf("%zu", sizeof(vpt_svgf_spatial_options));']
    for fname, _ in cls._fields_:
        lines.append('printf(" %%zu", offsetof(vpt_svgf_spatial_options, %s));' % fname)
    lines += ['printf("\\n%zu %zu %zu\\n", sizeof(vpt_svgf_options), sizeof(vpt_temporal_params), sizeof(vpt_stats));', 'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.check_output([exe], text=True).strip().splitlines()
    tok = [int(t) for t in out[0].split()]
    assert tok[0] == C.sizeof(cls) == 32 and len(tok) == 1 + len(cls._fields_)
    assert [f for f, _ in cls._fields_] == list(FIELDS) + ["reserved"]
    assert [getattr(cls, f).offset for f, _ in cls._fields_] == tok[1:] == [0, 4, 8, 12, 16, 20]
    # the structs the existing calls take keep their layout
    a = vpt._abi
    assert [int(t) for t in out[1].split()] == [C.sizeof(a.SvgfOptions), C.sizeof(a.TemporalParams), C.sizeof(a.Stats)]
    assert (C.sizeof(a.SvgfOptions), C.sizeof(a.TemporalParams)) == (16, 24)


def test_defaults_agree_on_both_sides(vpt):
    lib = vpt.load_library()
    p = vpt.SvgfSpatialOptions(9, 9, 9.0, 9.0, 9.0, (9, 9, 9))
    lib.vpt_default_svgf_spatial_options(C.byref(p))
    q = vpt.default_svgf_spatial_options()
    for k in FIELDS:
        assert getattr(p, k) == getattr(q, k), k
    assert tuple(getattr(p, k) for k in FIELDS) == tuple(C.c_float(d).value if isinstance(d, float) else d for d in DEFAULTS)     # (0.1 and 0.05 as float32)
    assert list(p.reserved) == list(q.reserved) == [0, 0, 0]
    lib.vpt_default_svgf_spatial_options(None)   # a NULL pointer is ignored
    assert vpt.default_svgf_spatial_options(mode=1, radius=2).radius == 2
    with pytest.raises(AttributeError):
        vpt.default_svgf_spatial_options(sigma=1)


def test_entry_points_are_declared_mirrored_and_exported(vpt):
    hdr = open(os.path.join(ROOT, "include", "vpt.h")).read()
    lib = vpt.load_library()
    for name in ENTRIES:
        assert re.search(r"\b(int|void) %s\(" % name, hdr) and name in vpt._abi.PROTOTYPES and hasattr(lib, name), name
    for m in ("set_svgf_spatial_options", "svgf_spatial_options"):
        assert hasattr(vpt.PathTracer, m)
    facade = open(os.path.join(ROOT, "vulkan-path-tracer_amd", "host", "PathTracer.h")).read()
    assert "DefaultSvgfSpatialOptions" in facade and "SetSvgfSpatialOptions" in facade


def test_null_arguments_are_refused_without_a_device(vpt):
    lib = vpt.load_library()
    o = vpt.default_svgf_spatial_options()
    assert lib.vpt_set_svgf_spatial_options(None, C.byref(o)) == -1            # VPT_ERR_INVALID_ARGUMENT
    assert lib.vpt_get_svgf_spatial_options(None, C.byref(o)) == -1
