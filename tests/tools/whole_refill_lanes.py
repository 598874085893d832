"""Probe (not a pytest): on how many lanes the whole-path kernel (kernels_whole.hip k_whole) generates its camera rays.  Needs a library built with
-DVPT_DIAG_REFILL_LANES=1 in the product's place (tests/tools/build_variant.py refill_lanes -DVPT_DIAG_REFILL_LANES=1 --sources kernels_whole.hip, copied over
libvpt_hip.so as tests/tools/ab_variants.sh does): that build counts, per wave, the passes that ran launch_pixel + camera_ray and the lanes that were live in
them, and reports the two sums where a counting context reports its closest-hit node visits and triangle tests (which it does not count).
Cornell box 1920x1080 depth 8, the headline workload.  Prints one JSON line.     python tests/tools/whole_refill_lanes.py [frames]"""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
vpt = importlib.import_module("vulkan-path-tracer_amd")
frames = int(sys.argv[1]) if len(sys.argv) > 1 else 64
sc = vpt.scenes.Scene.load(os.path.join(ROOT, "tests", "golden", "cornell_box.npz"))
g = vpt.PathTracer(1920, 1080, count_traversal=True, frames_in_flight=frames)
g.set_scene(sc); g.set_params(vpt.default_params(max_depth=8, max_samples=0x7fffffff))
g.render(frames)
st = g.stats(); g.close()
passes, lanes = st["nodes_visited"], st["tris_tested"]
assert lanes == st["samples"], "not a -DVPT_DIAG_REFILL_LANES=1 build: %d generating lanes for %d samples" % (lanes, st["samples"])
print(json.dumps({"frames": frames, "samples": st["samples"], "closest_rays": st["closest_rays"], "camera_ray_passes": passes, "generating_lanes": lanes,
                  "mean_lanes_per_camera_ray_pass": round(lanes / max(passes, 1), 2)}))
