"""Probe (not a pytest): what moving instances of an installed scene costs through vpt_set_instance_transforms against the only route there was before
it, a second vpt_set_scene of the moved description on the same context — the median of five one-instance moves and of five all-instance moves — and
what a refit costs in tree quality: nodes_visited / closest_rays (count_traversal) of a 4-frame 1080p render before the move, after a refit that
carries one instance across a quarter of the scene, and after a fresh vpt_set_scene of that description.  One JSON line per scene; the lines go to
profiles/set_instance_transforms.json.   python tests/tools/instance_move_time.py [scenes=atrium,bust]"""
import importlib, json, os, statistics, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import refit_moves as RM
vpt = importlib.import_module("vulkan-path-tracer_amd")
which = sys.argv[1].split(",") if len(sys.argv) > 1 else ["atrium", "bust"]
make = {"atrium": lambda: (vpt.scenes.atrium(), 8), "bust": lambda: (vpt.scenes.glass_bust(), 32), "cornell": lambda: (vpt.scenes.Scene.load(os.path.join(ROOT, "tests", "golden", "cornell_box_glass.npz")), 8)}
W, H, FRAMES, REPEATS = 1920, 1080, 4, 5
rows = []


def world_box(sc):
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for me, _, x in sc.instances:
        p = sc.meshes[me][0]["position"].astype(np.float64)
        w = (np.c_[p, np.ones(len(p))] @ np.asarray(x, np.float64).T)[:, :3]
        lo, hi = np.minimum(lo, w.min(0)), np.maximum(hi, w.max(0))
    return lo, hi


def visits(g):
    g.reset_stats(); g.reset(); g.render(FRAMES)
    st = g.stats()
    return round(st["nodes_visited"] / max(st["closest_rays"], 1), 3)


for name in which:
    sc, depth = make[name]()
    n = len(sc.instances)
    lo, hi = world_box(sc)
    sizes = [sc.triangle_count()]
    mover = max(range(n), key=lambda i: (len(sc.meshes[sc.instances[i][0]][1]) if i > 0 else -1, i)) if n > 1 else 0   # the largest instance that is not the first (the room)
    axis = int(np.argmax(hi - lo))
    step = np.zeros(3); step[axis] = 0.25 * (hi - lo)[axis]
    P = vpt.default_params(max_depth=depth)
    g = vpt.PathTracer(W, H, count_traversal=True)
    g.set_scene(sc); g.set_params(P)
    st = g.stats()
    row = {"scene": name, "triangles": sc.triangle_count(), "instances": n, "moved_instance": mover, "first_set_scene_ms": round(st["set_scene_ms"], 2), "first_bvh_build_ms": round(st["bvh_build_ms"], 2)}
    row["visits_per_ray_before"] = visits(g)
    one, every = [], []
    for k in range(REPEATS):                                # small rigid nudges that go back and forth
        w = RM.translate(*(0.01 * (k % 2 + 1) * step))
        g.set_instance_transforms(mover, [RM.moved_matrices(sc, {mover: w})[mover]])
        one.append(round(g.stats()["set_transforms_ms"], 3))
        m = RM.moved_matrices(sc, {i: w for i in range(n)})
        g.set_instance_transforms(0, [m[i] for i in range(n)])
        every.append(round(g.stats()["set_transforms_ms"], 3))
    s2 = g.stats()
    assert (s2["set_scene_ms"], s2["bvh_build_ms"]) == (st["set_scene_ms"], st["bvh_build_ms"])
    row["set_transforms_ms_one_instance"] = statistics.median(one); row["set_transforms_ms_one_instance_all"] = one
    row["set_transforms_ms_all_instances"] = statistics.median(every); row["set_transforms_ms_all_instances_all"] = every
    far = RM.moved_matrices(sc, {mover: RM.translate(*step)})
    g.set_instance_transforms(0, [np.asarray(far.get(i, sc.instances[i][2]), np.float32) for i in range(n)])
    row["visits_per_ray_after_refit"] = visits(g)
    img = g.radiance()
    moved = RM.with_matrices(sc, far)
    again = []
    for k in range(REPEATS):                                # the route before: the whole moved description again
        g.set_scene(moved); g.set_params(P)
        again.append(round(g.stats()["set_scene_ms"], 2))
    row["second_set_scene_ms"] = statistics.median(again); row["second_set_scene_ms_all"] = again
    row["visits_per_ray_after_rebuild"] = visits(g)
    row["images_equal"] = bool(np.array_equal(g.radiance(), img))     # (default flags: equal as far as two trees agree, include/vpt.h VPT_FLAG_LOCAL_HITS)
    g.close()
    row["set_scene_over_set_transforms_all"] = round(row["second_set_scene_ms"] / max(row["set_transforms_ms_all_instances"], 1e-9), 2)
    print(json.dumps(row), flush=True)
    rows.append(row)
if "--write" in sys.argv:
    with open(os.path.join(ROOT, "profiles", "set_instance_transforms.json"), "w") as f:
        f.write("\n".join(json.dumps(r) for r in rows) + "\n")
