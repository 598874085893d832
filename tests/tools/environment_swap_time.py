"""Probe (not a pytest): what replacing the environment map of an installed scene costs through vpt_set_environment against the only route there was
before it, a second vpt_set_scene — vpt_stats.set_scene_ms / bvh_build_ms / set_environment_ms, a map of the scene's own size, three repeats each (the
minimum and all three).  Checks on the way that the swap left the two vpt_set_scene figures alone and that the image equals the one of a context that
got the new map with its scene.  One JSON line per scene.   python tests/tools/environment_swap_time.py [scenes=atrium,bust]"""
import copy, importlib, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
vpt = importlib.import_module("vulkan-path-tracer_amd")
which = sys.argv[1].split(",") if len(sys.argv) > 1 else ["atrium", "bust"]
make = {"atrium": lambda: (vpt.scenes.atrium(), 8), "bust": lambda: (vpt.scenes.glass_bust(), 32), "cornell": lambda: (vpt.scenes.Scene.load(os.path.join(ROOT, "tests", "golden", "cornell_box.npz")), 8)}
W, H, REPEATS = 640, 360, 3
for name in which:
    sc, depth = make[name]()
    eh, ew = sc.env.shape[:2]
    other = vpt.scenes.sun_sky_env(ew, eh, seed=3, sun_peak=2.0e4) if ew * eh > 1 else vpt.scenes.constant_env((0.3, 0.5, 0.9), 1, 1)
    P = vpt.default_params(max_depth=depth)
    g = vpt.PathTracer(W, H)
    g.set_scene(sc); g.set_params(P)
    st = g.stats()
    row = {"scene": name, "triangles": sc.triangle_count(), "env": [ew, eh], "env_and_alias_mb": round(ew * eh * 24 / 1e6, 1),
           "first_set_scene_ms": round(st["set_scene_ms"], 2), "first_bvh_build_ms": round(st["bvh_build_ms"], 2)}
    swaps = []
    for k in range(REPEATS):
        g.set_environment(other if k % 2 == 0 else sc.env)
        s2 = g.stats()
        assert (s2["set_scene_ms"], s2["bvh_build_ms"]) == (st["set_scene_ms"], st["bvh_build_ms"])
        swaps.append(round(s2["set_environment_ms"], 2))
    g.render(2); img = g.radiance()                      # (REPEATS is odd: `other` is installed)
    row["set_environment_ms"] = min(swaps); row["set_environment_ms_all"] = swaps
    again = copy.copy(sc); again.env = other
    scenes_ms, builds_ms = [], []
    for k in range(REPEATS):                             # the route before: the whole description again
        g.set_scene(again if k % 2 == 0 else sc); g.set_params(P)
        s3 = g.stats()
        scenes_ms.append(round(s3["set_scene_ms"], 2)); builds_ms.append(round(s3["bvh_build_ms"], 2))
    g.render(2)
    row["images_equal"] = bool(np.array_equal(g.radiance(), img))
    g.close()
    row["second_set_scene_ms"] = min(scenes_ms); row["second_set_scene_ms_all"] = scenes_ms; row["second_bvh_build_ms_all"] = builds_ms
    row["set_scene_over_set_environment"] = round(row["second_set_scene_ms"] / row["set_environment_ms"], 2)
    print(json.dumps(row), flush=True)
