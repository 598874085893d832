"""Probe (not a pytest): what vpt_temporal_options.instance_motion costs one vpt_temporal_accumulate_device call — the Cornell box at 1920 x 1080, the default
parameters, a camera that moves a little before every call (tests/tools/temporal_time.py's loop) — as the median of 20 calls after a warm-up, each timed on the
host clock from the call to the end of vpt_wait, in three settings:
  off            the option off (what temporal_time.py measures);
  on_still       the option on, no instance moved: the motion image is written (8 B per pixel more), no table;
  on_moved       the option on and the back wall moved a little before every call: the table is built on the host, uploaded, and gathered by the wall's pixels.
The move itself (vpt_set_instance_transforms: a refit) is outside the timed part.  For information: no threshold anywhere.
One JSON line.   python tests/tools/motion_time.py [WxH]"""
import importlib, json, os, sys, time
import numpy as np
import torch   # (before the first context: the HIP runtime the process loads first serves both)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
vpt = importlib.import_module("vulkan-path-tracer_amd")
W, H = (int(v) for v in sys.argv[1].split("x")) if len(sys.argv) > 1 else (1920, 1080)
REPEATS, WARMUP = 20, 3
WALL = 2
sc = vpt.scenes.Scene.load(os.path.join(ROOT, "tests", "golden", "cornell_box.npz"))
proj_inv = sc.projection_inverse(W / H)
out_t = torch.zeros((H, W, 4), device="cuda:0")


def measure(option, move_wall):
    g = vpt.PathTracer(W, H)
    g.set_scene(sc)
    g.set_params(vpt.default_params(max_depth=4))
    g.set_temporal_options(instance_motion=option)
    ts = []
    for i in range(WARMUP + REPEATS):
        v = np.array(sc.view_inverse, np.float64)
        v[:3, 3] += v[:3, 0] * 0.02 * (i + 1)
        if move_wall:
            x = np.array(sc.instances[WALL][2], np.float64)
            x[0, 3] += 0.01 * (i + 1)
            g.set_instance_transforms(WALL, [x.astype(np.float32)])
        g.set_camera(v.astype(np.float32), proj_inv)
        g.render(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.temporal_accumulate_device(None, out_t.data_ptr())
        g.wait()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= WARMUP:
            ts.append(dt)
    row = {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4), "mean_history_length": round(float(g.temporal_history().mean()), 2)}
    if option:
        row["moved_pixels"] = int((np.abs(g.temporal_motion()).max(-1) > 0.25).sum())
    g.close()
    return row


out = {"size": [W, H], "off": measure(0, False), "on_still": measure(1, False), "on_moved": measure(1, True)}
print(json.dumps(out))
