"""Probe (not a pytest): the rate of whole-path batches (kernels_whole.hip k_whole) on an LDS-resident scene other than the Cornell box — tests/material_scenes.py's
compact variants, whose trees are deeper, or the chain of tests/whole_spill_scene.py, whose searches overflow the kernel's six LDS stack rows — at 1920x1080, depth 8.  For A/B runs of two library builds (tests/tools/ab_variants.sh copies them into the product's
place in turn).  Prints one JSON line.     python tests/tools/whole_scene_rate.py [compact|compact_environment|chain|cornell_box] [frames per batch] [batches]"""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
vpt = importlib.import_module("vulkan-path-tracer_amd")
name = sys.argv[1] if len(sys.argv) > 1 else "compact"
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 32
batches = int(sys.argv[3]) if len(sys.argv) > 3 else 6
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
assert st["kernel_launches"]["primary"] == batches and st["kernel_launches"]["bounce"] == 0, "not whole-path batches"
print(json.dumps({"scene": name, "frames_per_batch": frames, "batches": batches, "msamples_per_s": round(st["samples"] / dt / 1e6, 1), "ms_per_batch": round(dt / batches * 1e3, 3),
                  "bvh_nodes": st["bvh_nodes"], "bvh_triangles": st["bvh_triangles"], "closest_rays": st["closest_rays"], "shadow_rays": st["shadow_rays"], "stack_spills": st["stack_spills"]}))
