"""Probe (not a pytest): the rate of whole-path batches large enough to run in PARTS (path_plan.hpp Schedule::parts: one launch of k_whole and one resolve
per part) on an LDS-resident scene other than the Cornell box, at 1920x1080, depth 8 — tests/tools/whole_scene_rate.py for batches that take more than
one launch, which that probe refuses.  For A/B runs of two library builds copied into the product's place in turn.  Prints one JSON line, with the parts a
batch ran as.     python tests/tools/whole_parts_rate.py [compact|compact_environment|chain|cornell_box] [frames per batch] [batches]"""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
vpt = importlib.import_module("vulkan-path-tracer_amd")
name = sys.argv[1] if len(sys.argv) > 1 else "chain"
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 904
batches = int(sys.argv[3]) if len(sys.argv) > 3 else 3
if name == "cornell_box":
    sc = vpt.scenes.Scene.load(os.path.join(ROOT, "tests", "golden", "cornell_box.npz"))
elif name == "chain":
    import whole_spill_scene
    sc = whole_spill_scene.chain_scene(vpt)
else:
    import material_scenes
    sc, _ = material_scenes.variant(name)
g = vpt.PathTracer(1920, 1080, frames_in_flight=frames)
g.set_scene(sc); g.set_params(vpt.default_params(max_depth=8, max_samples=0x7fffffff))
for _ in range(2):
    g.render(frames)
g.reset_stats()
t = time.perf_counter()
for _ in range(batches):
    g.render(frames)
dt = time.perf_counter() - t
st = g.stats(); g.close()
launches = st["kernel_launches"]
assert launches["primary"] % batches == 0 and launches["resolve"] == launches["primary"] and launches["bounce"] == 0, "not whole-path batches"
print(json.dumps({"scene": name, "frames_per_batch": frames, "batches": batches, "parts_per_batch": launches["primary"] // batches, "msamples_per_s": round(st["samples"] / dt / 1e6, 1),
                  "ms_per_batch": round(dt / batches * 1e3, 3), "closest_rays": st["closest_rays"], "shadow_rays": st["shadow_rays"]}))
