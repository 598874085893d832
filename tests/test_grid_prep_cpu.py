"""The host preparation behind vpt_add_density_grid / vpt_add_density_bricks, without a device: vulkan-path-tracer_amd/csrc/grid_prep.hpp run by
tests/tools/grid_prep_driver.cpp as api_scene.hip runs it, held to
  * the dense writing: a bricked grid's maximum, its 32,768 block maxima and every voxel read through grid_value (the function the kernels call)
    equal the equivalent dense grid's, bit for bit;
  * the oracle: both equal orc_add_density_grid's arithmetic (oracle.cpp), restated here in numpy float32;
  * indifference to what cannot matter: garbage in a partial brick's voxels outside the index box, the order the bricks come in;
  * every rejection, with its code and message;
  * AddressSanitizer / UBSan: the same driver built with -fsanitize=address,undefined, as a stand-alone program, on the same inputs.
The lookups and renders on the device: tests/test_gpu_density_bricks.py."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vulkan-path-tracer_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import density_bricks as DB   # noqa: E402

F32 = np.float32
INVALID, LIMIT = -1, -7
NO_POSITIVE = "density grid has no positive value"
GRIDS = sorted(DB.SHAPES)


def compile_driver(exe, extra=()):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math", "-march=x86-64-v3", "-D__HIP_PLATFORM_AMD__"] + list(extra) +
                          ["-I/opt/rocm/include", "-I" + CSRC, os.path.join(ROOT, "tests", "tools", "grid_prep_driver.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("grid_prep")
    return compile_driver(str(d / "grid_prep_driver")), d


def write_input(path, dims, dense, coords, values):
    dx, dy, dz = dims
    blob = [struct.pack("<5I", dx, dy, dz, 0 if dense is None else 1, len(coords))]
    if dense is not None:
        assert dense.shape == (dz, dy, dx)
        blob.append(np.ascontiguousarray(dense, F32).tobytes())
    blob += [np.ascontiguousarray(coords, np.uint32).tobytes(), np.ascontiguousarray(values, F32).tobytes()]
    open(path, "wb").write(b"".join(blob))


def run_prep(driver, dims, dense, coords, values, tag="x"):
    """-> (verdict of the dense grid, its results | None, verdict of the bricked grid, its results | None); results: max, block maxima, voxels [z, y, x] (, table)."""
    exe, d = driver
    src, dst = str(d / (tag + ".in")), str(d / (tag + ".out"))
    write_input(src, dims, dense, coords, values)
    lines = subprocess.check_output([exe, "prep", src, dst], text=True).splitlines()
    raw = open(dst, "rb").read()
    dx, dy, dz = dims
    at = [0]

    def take(dtype, n):
        a = np.frombuffer(raw, dtype, n, at[0])
        at[0] += n * np.dtype(dtype).itemsize
        return a

    def results(table):
        r = {"max": take(F32, 1)[0], "block_max": take(F32, 32768), "voxels": take(F32, dx * dy * dz).reshape(dz, dy, dx)}
        if table:
            r["table"] = take(np.uint32, int(np.prod([-(-n // 8) for n in dims])))
        return r
    dense_r = results(False) if lines[0] == "0|" else None
    brick_r = results(True) if lines[1] == "0|" else None
    assert at[0] == len(raw)
    return lines[0], dense_r, lines[1], brick_r


def oracle_maxima(grid):
    """orc_add_density_grid (oracle.cpp), restated: the maximum; per voxel (x, y, z) the raw value at storage row dy - 1 - y, raw / max clamped to
    [0, 1] in float32, into block (x * 32 / dx, y * 32 / dy, z * 32 / dz)."""
    dz, dy, dx = grid.shape
    mx = grid.max()
    dens = np.clip((grid[:, ::-1, :] / mx).astype(F32), F32(0), F32(1))
    z, y, x = np.meshgrid(np.arange(dz), np.arange(dy), np.arange(dx), indexing="ij")
    bi = (x * 32) // dx + ((y * 32) // dy) * 32 + ((z * 32) // dz) * 1024
    table = np.zeros(32768, F32)
    np.maximum.at(table, bi.reshape(-1), dens.reshape(-1))
    return mx, table


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def assert_same_grid(r, ref_max, ref_block, ref_voxels):
    assert bits(r["max"]) == bits(ref_max)
    assert np.array_equal(bits(r["block_max"]), bits(ref_block))
    assert np.array_equal(bits(r["voxels"]), bits(ref_voxels))


@pytest.fixture(scope="module")
def prepared(driver):
    """Each test grid through the driver once, dense and bricked."""
    out = {}
    for name in GRIDS:
        g = DB.thresholded_cloud(name)
        dims, coords, values = DB.bricks(g)
        out[name] = (g, dims, coords, values) + run_prep(driver, dims, g, coords, values, tag=name)
    return out


@pytest.mark.parametrize("name", GRIDS)
def test_the_test_grids_have_empty_and_active_cells(vpt, name):
    g = DB.thresholded_cloud(name)
    dims, coords, values = DB.bricks(g)
    cells = int(np.prod(DB.cell_dims(g)))
    assert cells == 150 and len(coords) == DB.ACTIVE_CELLS[name]
    assert len(coords) * 5 >= cells and (cells - len(coords)) * 3 >= cells      # at least a fifth active, at least a third empty
    assert any(n % 8 for n in g.shape)                                           # at least one partial axis
    pd, pc, pv = vpt.bricks_of(g)                                                # the package's own bricking is this one
    assert pd == dims and np.array_equal(pc, coords) and np.array_equal(bits(pv), bits(values))


@pytest.mark.parametrize("name", GRIDS)
def test_bricked_equals_dense_equals_the_oracles_arithmetic(prepared, name):
    g, dims, coords, values, dv, dr, bv, br = prepared[name]
    assert dv == "0|" and bv == "0|"
    omax, oblock = oracle_maxima(g)
    assert_same_grid(dr, omax, oblock, g)           # the dense writing == the oracle, and grid_value reads the array back
    assert_same_grid(br, omax, oblock, g)           # the bricked writing == both; uncovered voxels read 0 (they are 0 in g)
    assert_same_grid(br, dr["max"], dr["block_max"], dr["voxels"])
    assert (oblock > 0).sum() > 1000 and (oblock == 0).sum() > 1000
    # the table: the brick's ordinal in the cells given, 0xffffffff elsewhere
    cz, cy, cx = DB.cell_dims(g)
    want = np.full(cz * cy * cx, 0xffffffff, np.uint32)
    want[coords[:, 0] + coords[:, 1] * cx + coords[:, 2] * cx * cy] = np.arange(len(coords), dtype=np.uint32)
    assert np.array_equal(br["table"], want)
    empty = np.ones((cz, cy, cx), bool); empty[coords[:, 2], coords[:, 1], coords[:, 0]] = False
    ez, ey, ex = np.nonzero(empty)
    assert len(ez) == 150 - len(coords) and np.all(bits(br["voxels"][np.minimum(ez * 8, g.shape[0] - 1), np.minimum(ey * 8, g.shape[1] - 1), np.minimum(ex * 8, g.shape[2] - 1)]) == 0)   # +0.0 exactly


@pytest.mark.parametrize("name", GRIDS)
@pytest.mark.parametrize("garbage", [np.nan, 1.0e30], ids=["nan", "1e30"])
def test_garbage_outside_the_index_box_changes_nothing(driver, prepared, name, garbage):
    g, dims, coords, values, _, _, _, br = prepared[name]
    _, c2, v2 = DB.bricks(g, fill=garbage, keep_all=True)   # (the cloud's own bricks lie inside the box: every cell is given, so the partial ones are)
    outside = np.isnan(v2) if np.isnan(garbage) else v2 == F32(garbage)
    assert len(c2) == 150 and outside.any(axis=(1, 2, 3)).sum() >= 30 and outside.sum() == len(c2) * 512 - g.size
    _, _, bv, r = run_prep(driver, dims, None, c2, v2, tag="garbage_" + name)
    assert bv == "0|"
    assert_same_grid(r, br["max"], br["block_max"], br["voxels"])


@pytest.mark.parametrize("name", GRIDS)
def test_brick_order_changes_nothing(driver, prepared, name):
    g, dims, coords, values, _, _, _, br = prepared[name]
    order = np.random.default_rng(11).permutation(len(coords))
    assert not np.array_equal(order, np.arange(len(coords)))
    _, _, bv, r = run_prep(driver, dims, None, coords[order], values[order], tag="shuffled_" + name)
    assert bv == "0|"
    assert_same_grid(r, br["max"], br["block_max"], br["voxels"])
    assert np.array_equal(np.sort(r["table"]), np.sort(br["table"])) and not np.array_equal(r["table"], br["table"])


def rejected_inputs():
    """(what, dims, coords, values, code, message) of every rejection that looks at the arrays."""
    g = DB.thresholded_cloud("all_partial")
    dims, coords, values = DB.bricks(g)
    cz, cy, cx = DB.cell_dims(g)
    rows = [("a coordinate given twice", dims, np.vstack([coords, coords[3:4]]), np.concatenate([values, values[3:4]]), INVALID, "brick coordinate given twice")]
    for axis, n in enumerate((cx, cy, cz)):
        c = coords.copy(); c[0, axis] = n
        rows.append(("coordinate %d at ceil(dim / 8)" % axis, dims, c, values, INVALID, "brick coordinate outside the grid"))
    rows.append(("no bricks", dims, coords[:0], values[:0], INVALID, NO_POSITIVE))
    rows.append(("no positive value", dims, coords, -np.abs(values), INVALID, NO_POSITIVE))
    rows.append(("all zero", dims, coords, values * 0, INVALID, NO_POSITIVE))
    inside = np.zeros((8, 8, 8), F32); far = inside.copy(); far[7, 7, 7] = 1.0    # a 9^3 box's corner brick (1, 1, 1) holds voxel (8, 8, 8) at its (0, 0, 0) only
    rows.append(("positive values outside the box only", (9, 9, 9), np.array([(1, 1, 1)], np.uint32), far[None], INVALID, NO_POSITIVE))
    return rows


REJECTED = rejected_inputs()


@pytest.mark.parametrize("row", REJECTED, ids=[r[0] for r in REJECTED])
def test_every_rejection_of_the_arrays_has_its_code_and_message(driver, row):
    what, dims, coords, values, code, msg = row
    _, _, bv, r = run_prep(driver, dims, None, coords, values, tag="rej_%d" % [x[0] for x in REJECTED].index(what))
    assert bv == "%d|%s" % (code, msg) and r is None


CHECKS = [   # (what, dx, dy, dz, bricks, NULL arrays?, grids in use, code, message): in the order check_bricks reports them, no data needed
    ("zero x", 0, 8, 8, 1, False, 0, INVALID, "density grid dimension is zero"),
    ("zero y", 8, 0, 8, 1, False, 0, INVALID, "density grid dimension is zero"),
    ("zero z", 8, 8, 0, 1, False, 0, INVALID, "density grid dimension is zero"),
    ("2^26 + 1 cells", 8 * ((1 << 26) + 1), 8, 8, 1, False, 0, LIMIT, "more than 2^26 brick cells"),
    ("2^26 + 1 cells along z, partial", 1, 1, 8 * (1 << 26) + 1, 1, False, 0, LIMIT, "more than 2^26 brick cells"),
    ("a cell count that wraps 64 bits", 0xffffffff, 0xffffffff, 0xffffffff, 1, False, 0, LIMIT, "more than 2^26 brick cells"),
    ("2^26 cells", 8 << 13, 8 << 13, 1, 1, False, 0, 0, ""),
    ("a seventeenth grid", 8, 8, 8, 1, False, 16, LIMIT, "more than VPT_MAX_DENSITY_GRIDS density grids"),
    ("the sixteenth grid", 8, 8, 8, 1, False, 15, 0, ""),
    ("no bricks", 8, 8, 8, 0, False, 0, INVALID, NO_POSITIVE),
    ("no bricks, NULL arrays", 8, 8, 8, 0, True, 0, INVALID, NO_POSITIVE),
    ("2^22 + 1 bricks", 2048, 2048, 2048, (1 << 22) + 1, False, 0, LIMIT, "more than 2^22 bricks"),
    ("2^22 bricks", 2048, 2048, 2048, 1 << 22, False, 0, 0, ""),
    ("NULL arrays", 8, 8, 8, 1, True, 0, INVALID, "no brick coordinates or values"),
]


@pytest.mark.parametrize("row", CHECKS, ids=[r[0] for r in CHECKS])
def test_every_rejection_of_the_arguments_has_its_code_and_message(driver, row):
    _, dx, dy, dz, n, null, grids, code, msg = row
    out = subprocess.check_output([driver[0], "check", str(dx), str(dy), str(dz), str(n), str(int(null)), str(grids)], text=True).rstrip("\n")
    assert out == "%d|%s" % (code, msg)


def test_the_driver_is_clean_under_address_and_undefined_behaviour_sanitizers(driver, prepared, tmp_path):
    """Host code in a stand-alone program: the two grids (dense and bricked, with NaN in the partial bricks), every rejection."""
    exe = compile_driver(str(tmp_path / "grid_prep_driver_san"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    san = (exe, driver[1])
    for name in GRIDS:
        g, dims, coords, values, _, dr, _, br = prepared[name]
        _, c2, v2 = DB.bricks(g, fill=np.nan, keep_all=True)
        dv, r1, bv, r2 = run_prep(san, dims, g, c2, v2, tag="san_" + name)
        assert dv == "0|" and bv == "0|"
        assert_same_grid(r1, dr["max"], dr["block_max"], dr["voxels"])
        assert_same_grid(r2, br["max"], br["block_max"], br["voxels"])
    for i, (what, dims, coords, values, code, msg) in enumerate(REJECTED):
        assert run_prep(san, dims, None, coords, values, tag="san_rej_%d" % i)[2] == "%d|%s" % (code, msg)
    for _, dx, dy, dz, n, null, grids, code, msg in CHECKS:
        assert subprocess.check_output([exe, "check", str(dx), str(dy), str(dz), str(n), str(int(null)), str(grids)], text=True).rstrip("\n") == "%d|%s" % (code, msg)


def test_the_library_exports_the_entries(vpt):
    import ctypes as C
    lib = vpt.load_library()
    names = subprocess.check_output(["nm", "-D", vpt.library_path(lab=False)], text=True)
    for fn in ("vpt_add_density_bricks", "vpt_get_density_grid_info", "vpt_read_density_grid"):
        assert " T " + fn in names
    assert C.sizeof(vpt._abi.DensityGridInfo) == 32
    one = np.zeros(512, F32); at = np.zeros(3, np.uint32); info = vpt._abi.DensityGridInfo()
    assert lib.vpt_add_density_bricks(None, 8, 8, 8, 1, at.ctypes.data, one.ctypes.data) == INVALID
    assert lib.vpt_get_density_grid_info(None, 0, C.byref(info)) == INVALID
    assert lib.vpt_read_density_grid(None, 0, None, 0, None) == INVALID
    for m in ("add_density_bricks", "add_density_grid_sparse", "density_grid_info", "read_density_grid"):
        assert hasattr(vpt.PathTracer, m)
