"""The build lists of vulkan-path-tracer_amd/_build.py against what is in csrc/: every file there is a source of the product, a source of the laboratory
library only (LAB_SOURCES) or a header, so needs_build and source_id cannot silently miss one; the per-file flag rule of the traversal-heavy kernel
files; and which files an id hashes — the product's must not move when only the laboratory's file does."""
import importlib
import os

B = importlib.import_module("vulkan-path-tracer_amd._build")


def test_every_file_in_csrc_is_on_a_build_list():
    local_headers = {h for h in B.HEADERS if os.path.dirname(h) == ""}
    listed = set(B.SOURCES) | set(B.LAB_SOURCES) | local_headers
    assert len(listed) == len(B.SOURCES) + len(B.LAB_SOURCES) + len(local_headers)   # no file on two lists
    assert set(os.listdir(B.CSRC)) == listed
    for h in set(B.HEADERS) - local_headers:   # the public headers, hashed from where they are
        assert os.path.isfile(os.path.join(B.CSRC, h)), h


def test_kernel_files_keep_the_slp_vectoriser_off():
    """Every kernels_*.hip but the post-process chain and the LUT generator is compiled without the SLP vectoriser (_build.py EXTRA_FLAGS says why)."""
    kernel_files = [f for f in B.SOURCES + B.LAB_SOURCES if f.startswith("kernels_") and f.endswith(".hip")]
    assert kernel_files
    for f in kernel_files:
        if f not in ("kernels_post.hip", "kernels_lut.hip"):
            assert "-fno-slp-vectorize" in B.EXTRA_FLAGS.get(f, []), f


def test_source_id_hashes_the_laboratory_file_for_the_laboratory_only(monkeypatch):
    product, lab = B.source_id(), B.source_id(("-DVPT_LAB=1",))
    assert product == B.source_id(("-DVPT_LAB=0",)) and product != lab
    assert B.LAB_SOURCES
    monkeypatch.setattr(B, "LAB_SOURCES", [])
    assert B.source_id() == product                   # the product's id does not depend on the laboratory's file
    assert B.source_id(("-DVPT_LAB=1",)) != lab       # the laboratory's does
