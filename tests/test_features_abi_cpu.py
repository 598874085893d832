"""vpt_feature_buffers and vpt_pick_result: sizeof and every field offset, as gcc lays out include/vpt.h, against the ctypes mirror (the technique of
tests/test_abi.py's test_ctypes_mirror_matches_the_compiled_header), the two mode constants, and the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_feature_structs_match_the_compiled_header(vpt, tmp_path):
    a = vpt._abi
    pairs = [("vpt_feature_buffers", a.FeatureBuffers), ("vpt_pick_result", a.PickResult)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vpt.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append('printf("%s %%zu", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf(" %%zu", offsetof(%s, %s));' % (cname, fname))
        lines.append('printf("\\n");')
    lines += ['printf("modes %u %u\\n", VPT_FEATURES_CENTER, VPT_FEATURES_SAMPLE);', 'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.check_output([exe], text=True).strip().splitlines()
    for (cname, cls), line in zip(pairs, out):
        tok = line.split()
        assert tok[0] == cname and int(tok[1]) == C.sizeof(cls), (cname, tok[1], C.sizeof(cls))
        assert len(tok) == 2 + len(cls._fields_)
        for (fname, _), off in zip(cls._fields_, tok[2:]):
            assert getattr(cls, fname).offset == int(off), (cname, fname)
    assert out[2].split() == ["modes", str(a.FEATURES_CENTER), str(a.FEATURES_SAMPLE)]
    assert (C.sizeof(a.FeatureBuffers), C.sizeof(a.PickResult)) == (40, 40)
    assert (vpt.FEATURES_CENTER, vpt.FEATURES_SAMPLE) == (0, 1)


def test_entry_points_are_declared_mirrored_and_exported(vpt):
    hdr = open(os.path.join(ROOT, "include", "vpt.h")).read()
    lib = vpt.load_library()
    for name in ("vpt_render_features", "vpt_pick"):
        assert re.search(r"\bint %s\(vpt_ctx\*" % name, hdr) and name in vpt._abi.PROTOTYPES and hasattr(lib, name)


def test_null_arguments_are_refused_without_a_device(vpt):
    lib = vpt.load_library()
    fb, pr = vpt._abi.FeatureBuffers(), vpt._abi.PickResult()
    assert lib.vpt_render_features(None, 0, 0, C.byref(fb)) == -1    # VPT_ERR_INVALID_ARGUMENT
    assert lib.vpt_pick(None, 0, 0, C.byref(pr)) == -1


def test_facade_refuses_unknown_buffer_names(vpt):
    import pytest
    g = vpt.PathTracer.__new__(vpt.PathTracer)   # no context: the name check comes before any call into the library
    g.width, g.height = 4, 4
    with pytest.raises(ValueError, match="unknown feature buffers"):
        g.render_features(which=("depth", "roughness"))
