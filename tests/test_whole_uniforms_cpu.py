"""How the loop of the whole-path kernel (kernels_whole.hip k_whole) reads its arguments: vulkan-path-tracer_amd/csrc/whole_args.hpp.  The kernel's one
parameter is a WholeArgs, which it reads again from its argument segment where it uses a word; the scene and the parameters in it are read through
WholeScene<STRICT, PLAIN> and WholeParams, which hide three fields of DeviceScene and one of RenderParams behind constants.  Compiled for the host by
tests/tools/whole_uniforms_driver.cpp, on a WholeArgs in which every word differs from every other: every field the loop reads must come out of
the view as the struct's own field, for a scene with emissive meshes and for one without (no light tables: null pointers, count 0), for the four
(STRICT, PLAIN) forms and for the dispatch index a launch passes; the constants must be what the kernel used to write into its copy; and
WholeArgs must lie as a kernel's arguments of those types lie.  (There is no copy to fill: the LDS block this test was planned for lost to this
form, profiles/r14_whole_uniforms_ab.md.)  The GPU side: tests/test_gpu_whole_uniforms.py."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vulkan-path-tracer_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "tools", "whole_uniforms_driver.cpp")
COMPARISONS = 4 * 54   # per form: 19 scene fields, 4 compile-time members, 13 parameters, sky_rot's eight, the dispatch index, 9 of the layout


def compile_driver(out, extra):
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-invalid-offsetof", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC, DRIVER, "-o", out] + extra)
    return out


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = C.CDLL(compile_driver(str(tmp_path_factory.mktemp("whole_uniforms") / "libwhole_uniforms.so"), ["-shared", "-fPIC"]))
    L.wu_check.restype = C.c_int
    L.wu_check.argtypes = [C.c_int, C.c_uint32, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    return L


@pytest.mark.parametrize("emissive", [1, 0])
@pytest.mark.parametrize("dispatch_base", [0, 7, 0xfffffff0])
def test_every_word_read_through_the_views_is_the_structs_own(lib, emissive, dispatch_base):
    fields, msg = C.c_int(), C.create_string_buffer(4096)
    bad = lib.wu_check(emissive, dispatch_base, C.byref(fields), msg, 4096)
    assert bad == 0, msg.value.decode()
    assert fields.value == COMPARISONS


def test_driver_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same checks as a stand-alone program, built with -fsanitize=address,undefined."""
    exe = compile_driver(str(tmp_path / "whole_uniforms_san"), ["-g", "-DWU_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "differing 0" in r.stdout
