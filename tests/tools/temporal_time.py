"""Probe (not a pytest): time of one vpt_temporal_accumulate_device call into a torch tensor — the Cornell box at 1920 x 1080, the default parameters, a
camera that moves a little before every call so that the history is reprojected, not found in place — as the median of 20 calls after a warm-up, each timed
on the host clock from the call to the end of vpt_wait (the call only enqueues); then the same for the guide launch alone (vpt_render_features, CENTER,
depth + ids + normal + albedo on device pointers).  Next to it the least k_temporal must move, from the record layout: per pixel it reads the image (16 B), the
normal (16), albedo (16), ids (16), depth (4) and one previous record (16 + 16 + 4: the four taps of neighbouring pixels overlap), and writes the result
(16) and the new record (36): 156 B, over 8 TB/s.  For information: no threshold anywhere.
One JSON line.   python tests/tools/temporal_time.py [WxH]"""
import importlib, json, os, sys, time
import numpy as np
import torch   # (before the first context: the HIP runtime the process loads first serves both)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
vpt = importlib.import_module("vulkan-path-tracer_amd")
W, H = (int(v) for v in sys.argv[1].split("x")) if len(sys.argv) > 1 else (1920, 1080)
REPEATS, WARMUP = 20, 3
BYTES_PER_PIXEL = 16 + 16 + 16 + 16 + 4 + 36 + 16 + 36
sc = vpt.scenes.Scene.load(os.path.join(ROOT, "tests", "golden", "cornell_box.npz"))
g = vpt.PathTracer(W, H)
g.set_scene(sc)
g.set_params(vpt.default_params(max_depth=4))
proj_inv = sc.projection_inverse(W / H)
out_t = torch.zeros((H, W, 4), device="cuda:0")
guides = {"depth": torch.zeros((H, W), device="cuda:0"), "ids": torch.zeros((H, W, 4), dtype=torch.int32, device="cuda:0"),
          "normal": torch.zeros((H, W, 4), device="cuda:0"), "albedo": torch.zeros((H, W, 4), device="cuda:0")}
gptr = {k: t.data_ptr() for k, t in guides.items()}
step = [0]


def move_and_render():
    """Outside the timed part: a camera 0.02 units further along, one frame."""
    step[0] += 1
    v = np.array(sc.view_inverse, np.float64)
    v[:3, 3] += v[:3, 0] * 0.02 * step[0]
    g.set_camera(v.astype(np.float32), proj_inv)
    g.render(1)


def timed(call, before=None):
    ts = []
    for i in range(WARMUP + REPEATS):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter(); call(); dt = (time.perf_counter() - t0) * 1e3
        if i >= WARMUP:
            ts.append(dt)
    return {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def temporal():
    g.temporal_accumulate_device(None, out_t.data_ptr())
    g.wait()


out = {"size": [W, H]}
out["temporal_ms"] = timed(temporal, move_and_render)
out["mean_history_length"] = round(float(g.temporal_history().mean()), 2)
out["guide_launch_ms"] = timed(lambda: g.render_features_device(vpt.FEATURES_CENTER, 0, **gptr))   # (returns after its stream synchronisation)
total, guide = out["temporal_ms"]["median"], out["guide_launch_ms"]["median"]
floor_ms = W * H * BYTES_PER_PIXEL / 8.0e12 * 1e3
out["guide_share"] = round(guide / total, 3)
out["bytes_per_pixel"] = BYTES_PER_PIXEL
out["floor_ms"] = round(floor_ms, 4)
out["ratio_to_floor"] = round(total / floor_ms, 1)
out["ratio_to_floor_without_guides"] = round((total - guide) / floor_ms, 1)
out["hit_fraction"] = round(float((guides["depth"] >= 0).float().mean().item()), 6)
g.close()
print(json.dumps(out))
