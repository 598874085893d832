"""The renders of tests/test_gpu_narrow_node.py that need the laboratory library (not a pytest): every case with the two-slot node step on and off
(VPT_LAB_NARROW_OFF: the launch flags no child word of its LDS tree, so every step is the four-wide one).  A process of its own with VPT_LAB=1; the
test compares what it leaves in the .npz file named on the command line: images by name, the statistics as one JSON string."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
vpt = importlib.import_module("vulkan-path-tracer_amd")
A = vpt._abi
assert vpt.has_lab(), "run with VPT_LAB=1"
import narrow_node_cases as N

KEEP = ("samples", "closest_rays", "shadow_rays", "primary_hits", "connect_paths", "kernel_launches", "bvh_node_bytes")
images, stats = {}, {}
for name in N.CASES:
    for off in (0, 1):
        img, st = N.render_case(vpt, name, pipeline=A.PIPELINE_WHOLE, before_render=lambda g: g.lab_set(A.LAB_NARROW_OFF, off))
        key = "%s_%s" % (name, "off" if off else "on")
        images[key] = img
        stats[key] = {k: st[k] for k in KEEP}
np.savez(sys.argv[1], stats=np.array(json.dumps(stats)), **images)
print("ok: %d images" % len(images))
