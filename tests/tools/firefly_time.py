"""Probe (not a pytest): what the firefly filter costs vpt_temporal_accumulate.  The Cornell box at 1920 x 1080 and 3840 x 2160 (or the sizes given), one frame
rendered, a camera that stands still; every figure is vpt_temporal_accumulate_device + vpt_wait on the host clock (the call only enqueues), the median of 20
after a warm-up.
  off / on       the option off, then on with the defaults (radius 1, rank 2) and at radius 2, rank 3 — the difference is the memset of the two counters and
                 k_firefly over the whole image;
  yardstick      ONE variance-guided a-trous pass of the same size, obtained the way tests/tools/svgf_spatial_time.py obtains it: vpt_denoise_device + vpt_wait
                 from the temporal source with 2 iterations minus the same with 1;
  counts         vpt_get_firefly_state of the last call: clamped and considered pixels.
"off-only" as the first argument: only the first figure, through calls every earlier build has (for a parent / branch comparison).
For information: no threshold anywhere.  One JSON line.   python tests/tools/firefly_time.py [off-only] [WxH ...]"""
import importlib, json, os, sys, time
import numpy as np
import torch   # (before the first context: the HIP runtime the process loads first serves both)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
vpt = importlib.import_module("vulkan-path-tracer_amd")
ARGS = sys.argv[1:]
OFF_ONLY = ARGS[:1] == ["off-only"]
SIZES = [tuple(int(v) for v in a.split("x")) for a in ARGS[1 if OFF_ONLY else 0:]] or [(1920, 1080), (3840, 2160)]
REPEATS, WARMUP = 20, 3
SCENE = vpt.scenes.Scene.load(os.path.join(ROOT, "tests", "golden", "cornell_box.npz"))
stat = lambda ts: {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def timed(call):
    ts = []
    for i in range(WARMUP + REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); call(); t1 = time.perf_counter()
        if i >= WARMUP:
            ts.append((t1 - t0) * 1e3)
    return ts


out = {}
for w, h in SIZES:
    r = {}
    g = vpt.PathTracer(w, h)
    g.set_scene(SCENE); g.set_params(vpt.default_params(max_depth=4))
    g.set_svgf_options(variance=1)
    g.render(1)

    def temporal():
        g.temporal_accumulate_device(None, None); g.wait()
    r["temporal_off_ms"] = stat(timed(temporal))
    if OFF_ONLY:
        g.close()
        out["%dx%d" % (w, h)] = r
        continue
    for name, kw in (("on", dict(radius=1, rank=2)), ("on_radius2_rank3", dict(radius=2, rank=3))):
        g.set_firefly_options(mode=1, **kw)
        r["temporal_%s_ms" % name] = stat(timed(temporal))
        r["%s_added_ms" % name] = round(r["temporal_%s_ms" % name]["median"] - r["temporal_off_ms"]["median"], 4)
        s = g.firefly_state()
        r["%s_clamped" % name], r["%s_considered" % name] = int(s.clamped), int(s.considered)
    g.set_firefly_options(mode=0)
    r["temporal_off_again_ms"] = stat(timed(temporal))
    g.set_denoise_source(vpt.DENOISE_SOURCE_TEMPORAL)
    dn = {}
    for it in (1, 2):
        p = vpt.default_denoise_params(iterations=it)

        def denoise():
            g.denoise_device(p, None); g.wait()
        dn[it] = stat(timed(denoise))
    r["denoise1_ms"], r["denoise2_ms"] = dn[1], dn[2]
    r["atrous_pass_ms"] = round(dn[2]["median"] - dn[1]["median"], 4)
    for name in ("on", "on_radius2_rank3"):
        r["%s_added_over_atrous_pass" % name] = round(r["%s_added_ms" % name] / r["atrous_pass_ms"], 2)
    g.close()
    out["%dx%d" % (w, h)] = r
print(json.dumps(out))
