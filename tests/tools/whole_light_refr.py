"""Probe (not a pytest): how often the light-sample evaluation of the whole-path kernel (kernels_whole.hip k_whole, shade_core.hpp) runs the refraction
lobe of Bsdf::eval, on a -DVPT_DIAG_LIGHT_REFR=1 build (tests/tools/build_variant.py; copy it over the product library first).  That build reports, IN PLACE
of a counting context's visit counters: shade steps of a wave (nodes_visited), shade steps in which the lobe ran on at least one lane (tris_tested), and, of
those, the steps in which every lane that ran it has pg == 0 (shadow_nodes_visited) — the steps an evaluation without that lobe would spare (profiles/REJECTED.md, round 14).  Cornell box, 1920x1080,
depth 8.  Prints one JSON line.     python tests/tools/whole_light_refr.py [frames]"""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
vpt = importlib.import_module("vulkan-path-tracer_amd")
frames = int(sys.argv[1]) if len(sys.argv) > 1 else 4
sc = vpt.scenes.Scene.load(os.path.join(ROOT, "tests", "golden", "cornell_box.npz"))
g = vpt.PathTracer(1920, 1080, frames_in_flight=frames, pipeline=vpt._abi.PIPELINE_WHOLE, count_traversal=True)
g.set_scene(sc); g.set_params(vpt.default_params(max_depth=8, max_samples=0x7fffffff))
g.render(frames)
st = g.stats(); g.close()
steps, ran, spared = int(st["nodes_visited"]), int(st["tris_tested"]), int(st["shadow_nodes_visited"])
print(json.dumps({"scene": "cornell_box", "frames": frames, "samples": st["samples"], "shade_steps": steps, "steps_refraction_lobe_ran": ran, "steps_only_pg0_lanes_ran_it": spared,
                  "share_ran": round(ran / max(steps, 1), 4), "share_spared": round(spared / max(steps, 1), 4)}))
