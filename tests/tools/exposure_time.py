"""Probe (not a pytest): what auto-exposure costs.  The Cornell box at 1920 x 1080 and 3840 x 2160 (or the sizes given):
  frame      one vpt_postprocess_device call, host clock from the call to the end of vpt_wait, median of 20 after a warm-up, with the option off and on;
  kernels    a context made with vpt_config.profile: the time of the launches counted under VPT_K_TONEMAP per call, off and on — the difference is the two new
             launches (k_luminance_histogram + k_exposure_adapt; events around each launch, so a few microseconds of launch gap ride along) — for the
             render, for a flat image (every pixel in one bin: all 64 lanes of a wave on one LDS word) and for white noise over the whole range (every lane
             on a word of its own);
  yardstick  a plain pass over the image's bytes on the same machine: a device-to-device copy of HALF the image (it reads half and writes half: the
             traffic of one read of the whole), torch events, median of 20.
For information: no threshold anywhere.  One JSON line.   python tests/tools/exposure_time.py [WxH ...]"""
import importlib, json, os, sys, time
import numpy as np
import torch   # (before the first context: the HIP runtime the process loads first serves both)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
vpt = importlib.import_module("vulkan-path-tracer_amd")
SIZES = [tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]] or [(1920, 1080), (3840, 2160)]
REPEATS, WARMUP = 20, 3
SCENE = vpt.scenes.Scene.load(os.path.join(ROOT, "tests", "golden", "cornell_box.npz"))


def frame_ms(g):
    def call():
        g.postprocess_device()
        g.wait()
    for _ in range(WARMUP):
        call()
    ts = []
    for _ in range(REPEATS):
        t0 = time.perf_counter(); call(); ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def tonemap_ms_per_call(g):
    for _ in range(WARMUP):
        g.postprocess()
    g.reset_stats()
    for _ in range(REPEATS):
        g.postprocess()
    st = g.stats()
    return st["kernel_ms"]["tonemap"] / REPEATS, st["kernel_launches"]["tonemap"] // REPEATS


def copy_half_ms(w, h):
    src = torch.zeros(w * h * 2, device="cuda:0")      # half the image's 16 B per pixel
    dst = torch.empty_like(src)
    for _ in range(WARMUP):
        dst.copy_(src)
    ts = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); dst.copy_(src); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


out = {}
for w, h in SIZES:
    r = {}
    g = vpt.PathTracer(w, h)
    g.set_scene(SCENE); g.set_params(vpt.default_params(max_depth=4)); g.render(4)
    r["frame_off_ms"] = frame_ms(g)
    g.set_exposure_options(mode=1)
    r["frame_on_ms"] = frame_ms(g)
    image = g.radiance()
    g.close()
    rng = np.random.RandomState(1)
    noise = np.ones((h, w, 4), np.float32); noise[..., :3] = (2.0 ** rng.uniform(-10.0, 6.0, (h, w, 1))).astype(np.float32)
    flat = np.full((h, w, 4), 0.3, np.float32)
    yard = copy_half_ms(w, h)
    r["copy_half_image_ms"] = round(yard, 5)
    for name, img in (("render", image), ("flat", flat), ("noise", noise)):
        p = vpt.PathTracer(w, h, profile=True)
        p.set_radiance(img, 1)
        off, n_off = tonemap_ms_per_call(p)
        p.set_exposure_options(mode=1)
        on, n_on = tonemap_ms_per_call(p)
        p.close()
        assert (n_off, n_on) == (1, 3)
        r["meter_%s_ms" % name] = round(on - off, 5)
        r["meter_%s_over_copy" % name] = round((on - off) / yard, 2)
        r["tonemap_%s_off_ms" % name] = round(off, 5)
    out["%dx%d" % (w, h)] = r
print(json.dumps(out))
