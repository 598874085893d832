"""Probe (not a pytest): what SVGF's variance costs the viewport loop — the Cornell box at 1920 x 1080, a camera that moves a little and a new seed
(vpt_set_base_seed) before every step, one frame rendered, then vpt_temporal_accumulate_device and a 5-pass vpt_denoise_device from the temporal source into
torch tensors — each call timed on the host clock from the call to the end of vpt_wait (the calls only enqueue), as the median of 20 steps after a warm-up,
once with vpt_svgf_options.variance off and once with it on.  With it on the temporal kernel reads and writes 20 B per pixel more (the moment records, the
variance image) and every a-trous pass reads its taps from memory (the tiled form of steps 1 and 2 has no variance instantiation) after a 3 x 3 prefilter of
the variance.  With "bust" also vpt_stats.bvh_build_ms of the 511 k-triangle glass bust, three times: the host builder's time (it is compiled -O2 for the library's size).
For information: no threshold anywhere.
One JSON line.   python tests/tools/svgf_time.py [WxH] [bust]"""
import importlib, json, os, sys, time
import numpy as np
import torch   # (before the first context: the HIP runtime the process loads first serves both)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
vpt = importlib.import_module("vulkan-path-tracer_amd")
W, H = (int(v) for v in sys.argv[1].split("x")) if len(sys.argv) > 1 else (1920, 1080)
REPEATS, WARMUP = 20, 3
sc = vpt.scenes.Scene.load(os.path.join(ROOT, "tests", "golden", "cornell_box.npz"))
g = vpt.PathTracer(W, H)
g.set_scene(sc)
g.set_params(vpt.default_params(max_depth=4))
g.set_denoise_source(vpt.DENOISE_SOURCE_TEMPORAL)
proj_inv = sc.projection_inverse(W / H)
out_t = torch.zeros((H, W, 4), device="cuda:0")
step = [0]


def move_reseed_and_render():
    """Outside the timed part: a camera 0.02 units further along, another seed, one frame."""
    step[0] += 1
    v = np.array(sc.view_inverse, np.float64)
    v[:3, 3] += v[:3, 0] * 0.02 * step[0]
    g.set_camera(v.astype(np.float32), proj_inv)
    g.set_base_seed(step[0])
    g.render(1)


def loop():
    """-> medians of the temporal call, the denoise call and their sum, ms."""
    tt, td = [], []
    for i in range(WARMUP + REPEATS):
        move_reseed_and_render()
        torch.cuda.synchronize()
        t0 = time.perf_counter(); g.temporal_accumulate_device(None, out_t.data_ptr()); g.wait(); t1 = time.perf_counter()
        g.denoise_device(None, out_t.data_ptr()); g.wait(); t2 = time.perf_counter()
        if i >= WARMUP:
            tt.append((t1 - t0) * 1e3); td.append((t2 - t1) * 1e3)
    stat = lambda ts: {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}
    return {"temporal_ms": stat(tt), "denoise5_ms": stat(td), "sum_of_medians_ms": round(float(np.median(tt) + np.median(td)), 4)}


out = {"size": [W, H]}
out["variance_off"] = loop()
g.set_svgf_options(variance=1)
out["variance_on"] = loop()
out["known_variance_fraction"] = round(float((g.temporal_variance() >= 0).mean()), 4)
out["mean_history_length"] = round(float(g.temporal_history().mean()), 2)
g.close()
if sys.argv[2:] == ["bust"]:
    big = vpt.scenes.glass_bust()
    ms = []
    for _ in range(3):
        b = vpt.PathTracer(64, 64)
        b.set_scene(big)
        ms.append(round(float(b.stats()["bvh_build_ms"]), 2))
        b.close()
    out["bvh_build_ms"] = {"scene": "glass_bust", "triangles": int(big.triangle_count()), "runs": ms}
print(json.dumps(out))
