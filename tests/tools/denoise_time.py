"""Probe (not a pytest): time of one vpt_denoise_device call into a torch tensor — the Cornell box at 1920 x 1080, 5 iterations, the default parameters —
as the median of 20 calls after a warm-up, each timed on the host clock from the call to the end of vpt_wait (the call only enqueues); then the same for
the guide launch alone (vpt_render_features, CENTER, depth + normal + albedo on device pointers) and for 1 and 2 iterations (the LDS-tiled kernel alone).
Next to it the least the passes must move: 32 B read + 16 B written per pixel and pass, over 8 TB/s.  For information: no threshold anywhere.
One JSON line.   python tests/tools/denoise_time.py [WxH]"""
import importlib, json, os, sys, time
import numpy as np
import torch   # (before the first context: the HIP runtime the process loads first serves both)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
vpt = importlib.import_module("vulkan-path-tracer_amd")
W, H = (int(v) for v in sys.argv[1].split("x")) if len(sys.argv) > 1 else (1920, 1080)
REPEATS, WARMUP = 20, 3
g = vpt.PathTracer(W, H)
g.set_scene(vpt.scenes.Scene.load(os.path.join(ROOT, "tests", "golden", "cornell_box.npz")))
g.set_params(vpt.default_params(max_depth=4))
g.render(4)
out_t = torch.zeros((H, W, 4), device="cuda:0")
guides = {"depth": torch.zeros((H, W), device="cuda:0"), "normal": torch.zeros((H, W, 4), device="cuda:0"), "albedo": torch.zeros((H, W, 4), device="cuda:0")}
gptr = {k: t.data_ptr() for k, t in guides.items()}


def timed(call):
    for _ in range(WARMUP):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPEATS):
        t0 = time.perf_counter(); call(); ts.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    return {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def denoise(iterations):
    dp = vpt.default_denoise_params(iterations=iterations)

    def call():
        g.denoise_device(dp, out_t.data_ptr())
        g.wait()
    return call


out = {"size": [W, H]}
for it in (5, 2, 1):
    out["denoise_%d_iterations_ms" % it] = timed(denoise(it))
out["guide_launch_ms"] = timed(lambda: g.render_features_device(vpt.FEATURES_CENTER, 0, **gptr))   # (returns after its stream synchronisation)
total, guide = out["denoise_5_iterations_ms"]["median"], out["guide_launch_ms"]["median"]
floor_ms = 5 * W * H * 48 / 8.0e12 * 1e3
out["guide_share"] = round(guide / total, 3)
out["floor_ms"] = round(floor_ms, 4)
out["ratio_to_floor"] = round(total / floor_ms, 1)
out["hit_fraction"] = round(float((guides["depth"] >= 0).float().mean().item()), 6)
g.close()
print(json.dumps(out))
