"""The cases of tests/test_gpu_narrow_node.py, shared with the process that renders them on the laboratory library (tests/gpu_narrow_node_run.py):
the inputs of tests/test_gpu_lds_node_step.py — the Cornell box (nodes 1 and 2 are half-empty: the two-slot step runs in every closest-hit
search), the 16-sheet chain (no half-empty node: the searches pay the test and never take the step) and the compact scene under its environment (one
half-empty node; the general instantiation, which keeps the four-wide step) — the compact scene after one vpt_set_instance_transforms move of its
box and the Cornell box after a move of its back wall (tests/refit_moves.py), so that the flags come from refitted trees, and a chain of 12
sheets, whose tree (tests/test_narrow_node_cpu.py prints it: used slots 4, 4, 3, 2) has a three-slot node, which must stay unflagged, beside a
half-empty one, on the PLAIN instantiation.  Not a test module."""
import os

import refit_moves as RM
import test_gpu_lds_node_step as L
import whole_spill_scene as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("cornell", "chain", "compact_environment", "compact_moved", "cornell_moved", "chain12")
COMPACT_BOX = 6                                                                                       # tests/material_scenes.py build(compact=True)
MOVES = {"compact_moved": ("compact_environment", {COMPACT_BOX: RM.about((2.2, 3.6, -6.0), RM.rotate((0.2, 1.0, 0.1), 17.0)) @ RM.translate(-1.6, 0.0, -1.2)}),
         "cornell_moved": ("cornell", RM.CORNELL_WALL)}


def load_scene(vpt):
    return lambda name: vpt.scenes.Scene.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def case_inputs(vpt, name):
    """(scene to install, {instance: matrix} to move afterwards or None, the scene the image is of, width, height, params, frames)"""
    if name[:5] == "chain" and name[5:].isdigit():
        sc = W.chain_scene(vpt, int(name[5:]))
        return sc, None, sc, 64, 36, vpt.default_params(max_depth=4), 4
    if name not in MOVES:
        sc, w, h, p, frames = L.case_inputs(vpt, load_scene(vpt), name)
        return sc, None, sc, w, h, p, frames
    sc, w, h, p, frames = L.case_inputs(vpt, load_scene(vpt), MOVES[name][0])
    moved = RM.moved_matrices(sc, MOVES[name][1])
    return sc, moved, RM.with_matrices(sc, moved), w, h, p, frames


def render_case(vpt, name, before_render=None, **kw):
    sc, moved, _, w, h, p, frames = case_inputs(vpt, name)
    g = vpt.PathTracer(w, h, frames_in_flight=frames, **kw)
    g.set_scene(sc); g.set_params(p)
    if moved:
        for i, m in sorted(moved.items()):
            g.set_instance_transforms(i, [m])
    if before_render:
        before_render(g)
    g.render(frames)
    img, st = g.radiance(), g.stats()
    g.close()
    return img, st
