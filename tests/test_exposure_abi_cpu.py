"""vpt_exposure_options and vpt_exposure_state: sizeof and every field offset, as gcc lays out include/vpt.h, against the ctypes mirror (the technique of
tests/test_denoise_abi_cpu.py), the defaults on both sides, and the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vpt_default_exposure_options", "vpt_set_exposure_options", "vpt_get_exposure_options", "vpt_get_exposure_state", "vpt_get_exposure_histogram",
           "vpt_exposure_reset")


def test_structs_match_the_compiled_header(vpt, tmp_path):
    a = vpt._abi
    pairs = [("vpt_exposure_options", a.ExposureOptions), ("vpt_exposure_state", a.ExposureState)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vpt.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append('printf("%%zu", sizeof(%s));' % cname)
        for fname, _ in cls._fields_:
            lines.append('printf(" %%zu", offsetof(%s, %s));' % (cname, fname))
        lines.append('printf("\\n");')
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.check_output([exe], text=True).strip().splitlines()
    want = {"vpt_exposure_options": (48, [4 * k for k in range(12)]), "vpt_exposure_state": (32, [0, 4, 8, 12, 16, 20, 24])}
    for (cname, cls), line in zip(pairs, out):
        tok = [int(t) for t in line.split()]
        assert tok[0] == C.sizeof(cls) == want[cname][0], cname
        assert [getattr(cls, f).offset for f, _ in cls._fields_] == tok[1:] == want[cname][1], cname
    assert a.EXPOSURE_BINS == vpt.EXPOSURE_BINS == 256


def test_defaults_agree_on_both_sides(vpt):
    lib = vpt.load_library()
    p = vpt._abi.ExposureOptions(*([9] * 12))
    lib.vpt_default_exposure_options(C.byref(p))
    q = vpt.default_exposure_options()
    for k, _ in vpt._abi.ExposureOptions._fields_:
        assert getattr(p, k) == getattr(q, k), k
    f = C.c_float
    assert (p.mode, p.min_log2, p.max_log2, p.low_percentile, p.high_percentile, p.key, p.compensation_log2, p.min_exposure_log2, p.max_exposure_log2,
            p.rate_up, p.rate_down, p.reserved) == (0, -10.0, 6.0, 0.5, f(0.95).value, f(0.18).value, 0.0, -8.0, 8.0, f(0.1).value, 0.25, 0)
    lib.vpt_default_exposure_options(None)   # a NULL pointer is ignored
    assert vpt.default_exposure_options(mode=1, key=0.5).key == 0.5
    with pytest.raises(AttributeError):
        vpt.default_exposure_options(speed=1.0)


def test_entry_points_are_declared_mirrored_and_exported(vpt):
    hdr = open(os.path.join(ROOT, "include", "vpt.h")).read()
    lib = vpt.load_library()
    for name in ENTRIES:
        assert re.search(r"\b(int|void) %s\(" % name, hdr) and name in vpt._abi.PROTOTYPES and hasattr(lib, name), name
    for m in ("set_exposure_options", "exposure_options", "exposure_state", "exposure_histogram", "exposure_reset"):
        assert hasattr(vpt.PathTracer, m)


def test_null_arguments_are_refused_without_a_device(vpt):
    lib = vpt.load_library()
    o = vpt.default_exposure_options()
    s = vpt.ExposureState()
    hist = (C.c_uint32 * 256)()
    assert lib.vpt_set_exposure_options(None, C.byref(o)) == -1            # VPT_ERR_INVALID_ARGUMENT
    assert lib.vpt_get_exposure_options(None, C.byref(o)) == -1
    assert lib.vpt_get_exposure_state(None, C.byref(s)) == -1
    assert lib.vpt_get_exposure_histogram(None, hist) == -1
    assert lib.vpt_exposure_reset(None) == -1
