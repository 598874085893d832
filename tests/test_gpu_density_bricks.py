"""Sparse density grids (vpt_add_density_bricks: a heterogeneous volume from 8x8x8 bricks, a NanoVDB tree's leaf nodes as they are) on the device.
A bricked grid is the dense grid with 0 wherever no brick lies: the device lookup (vpt_read_density_grid, the kernels' grid_value) returns the
dense array's values at every voxel of the index box and around it, and every image equals, bit for bit, the dense grid's image and the oracle's
(which is always given the dense array) — in the fused media kernel, on the media streams and through the temperature emission.  The k_finish
launch that ends small batches of the plain streams never runs for a batch with media (path_plan.hpp decide: the finisher is for Kind::Streams
and Kind::StreamsSorted, not Kind::MediaStreams), so no form below can reach it; the test of the streams form asserts that this is still so.
The host preparation, without a device: tests/test_grid_prep_cpu.py."""
import numpy as np
import pytest

import density_bricks as DB
from test_gpu_volumes import fog, glass_room, lit_env_scene

pytestmark = pytest.mark.gpu
F32 = np.float32
W, H = 128, 72


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def faces_grid():
    """The all-partial cloud with values on the three far faces of the box: its partial bricks are active, and the last voxel of every axis is not 0."""
    g = DB.thresholded_cloud("all_partial")
    rng = np.random.default_rng(3)
    g[-1, :, :] = rng.uniform(0.1, 1.0, g[-1, :, :].shape); g[:, -1, :] = rng.uniform(0.1, 1.0, g[:, -1, :].shape); g[:, :, -1] = rng.uniform(0.1, 1.0, g[:, :, -1].shape)
    return g


def lookup_grids():
    return {"y_partial": DB.thresholded_cloud("y_partial"), "all_partial": DB.thresholded_cloud("all_partial"), "faces": faces_grid()}


def probe_points(shape):
    """Every voxel of the index box, then a ring around it: per axis -1, 0, the middle, dim - 1, dim, dim + 7 in every combination."""
    dz, dy, dx = shape
    z, y, x = np.meshgrid(np.arange(dz), np.arange(dy), np.arange(dx), indexing="ij")
    box = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    ax = [np.array([-1, 0, n // 2, n - 1, n, n + 7]) for n in (dx, dy, dz)]
    rx, ry, rz = np.meshgrid(*ax, indexing="ij")
    ring = np.stack([rx, ry, rz], axis=-1).reshape(-1, 3)
    return box.astype(np.int32), ring.astype(np.int32)


def expected(grid, ijk):
    dz, dy, dx = grid.shape
    return grid[np.clip(ijk[:, 2], 0, dz - 1), np.clip(ijk[:, 1], 0, dy - 1), np.clip(ijk[:, 0], 0, dx - 1)]


@pytest.mark.parametrize("name", ["y_partial", "all_partial", "faces"])
def test_device_lookup_equals_the_dense_grid_everywhere(vpt, name):
    grid = lookup_grids()[name]
    dims, coords, values = DB.bricks(grid)
    _, call, vall = DB.bricks(grid, fill=np.nan, keep_all=True)       # every cell a brick, NaN outside the box: a partial brick's padding is never read
    g = vpt.PathTracer(16, 16)
    try:
        assert g.add_density_grid(grid) == 0 and g.add_density_bricks(dims, coords, values) == 1 and g.add_density_bricks(dims, call, vall) == 2
        assert g.add_density_grid_sparse(grid) == 3
        box, ring = probe_points(grid.shape)
        for pts in (box, ring):
            want = expected(grid, pts)
            got = [g.read_density_grid(i, pts) for i in range(4)]
            for r in got:
                assert np.array_equal(bits(r), bits(want))
        # empty cells: exactly +0.0, at their first and last voxel
        cz, cy, cx = DB.cell_dims(grid)
        empty = np.ones((cz, cy, cx), bool); empty[coords[:, 2], coords[:, 1], coords[:, 0]] = False
        ez, ey, ex = np.nonzero(empty)
        assert len(ez) == 150 - len(coords) and len(ez) >= (45 if name == "faces" else 50)   # (faces: 150 - 35 cloud cells - 70 cells on the far faces)
        lo = np.stack([ex * 8, ey * 8, ez * 8], axis=1).astype(np.int32)
        hi = np.minimum(lo + 7, np.array(dims, np.int32) - 1)
        for pts in (lo, hi):
            assert np.all(bits(g.read_density_grid(1, pts)) == 0) and np.all(bits(g.read_density_grid(3, pts)) == 0)
        # the last voxel of each axis, along the whole edge through the far corner
        dx, dy, dz = dims
        for axis, n in enumerate(dims):
            edge = np.tile(np.array([dx - 1, dy - 1, dz - 1], np.int32), (n, 1)); edge[:, axis] = np.arange(n)
            want = expected(grid, edge)
            assert np.array_equal(bits(g.read_density_grid(1, edge)), bits(want))
            if name == "faces":
                assert np.all(want > 0)
        # info
        voxels, cells = grid.size, cz * cy * cx
        d, b, a = g.density_grid_info(0), g.density_grid_info(1), g.density_grid_info(2)
        assert d["dim"] == b["dim"] == a["dim"] == dims
        assert d["brick_count"] == 0 and b["brick_count"] == len(coords) and a["brick_count"] == cells == 150
        assert d["device_bytes"] == voxels * 4 + 131072
        assert b["device_bytes"] == len(coords) * 2048 + cells * 4 + 131072 and a["device_bytes"] == cells * 2048 + cells * 4 + 131072
        if name != "faces":   # (the faces grid is two-thirds bricks: whole 2 KB bricks for its thin faces cost more than the voxels)
            assert b["device_bytes"] < d["device_bytes"]
        assert bits(d["max_density"]) == bits(b["max_density"]) == bits(a["max_density"]) == bits(grid.max())
        with pytest.raises(vpt.VptError, match="INVALID"):
            g.density_grid_info(4)
        with pytest.raises(vpt.VptError, match="INVALID"):
            g.read_density_grid(4, box[:1])
    finally:
        g.close()


def render_dense_bricked_oracle(vpt, oracle, sc, P, grid, volumes_of, frames, atmosphere=False, **gpu_kw):
    """The same volumes on the oracle (dense array), a context with the dense grid and a context with the bricked one -> (ref, dense image, its stats, bricked image, its stats)."""
    o = oracle.Oracle(sc, W, H); o.set_params(P)
    gi = o.add_density_grid(grid)
    o.set_volumes(volumes_of(gi))
    if atmosphere:
        o.set_atmosphere(vpt.atmosphere())
    o.render(frames); ref = o.radiance(); o.close()
    out = [ref]
    for bricked in (False, True):
        g = vpt.PathTracer(W, H, **gpu_kw); g.set_scene(sc); g.set_params(P)
        assert (g.add_density_grid_sparse(grid) if bricked else g.add_density_grid(grid)) == gi
        assert (g.density_grid_info(gi)["brick_count"] > 0) == bricked
        g.set_volumes(volumes_of(gi))
        if atmosphere:
            g.set_atmosphere(vpt.atmosphere())
        g.render(frames)
        out += [g.radiance(), g.stats()]; g.close()
    return out


def assert_three_way(ref, dense, dst, bricked, bst):
    assert np.array_equal(dense, ref)
    assert np.array_equal(bricked, ref)
    assert np.array_equal(bricked, dense)
    assert bst["closest_rays"] == dst["closest_rays"] and bst["shadow_rays"] == dst["shadow_rays"] and bst["samples"] == dst["samples"]
    assert float(ref[..., :3].sum()) > 0


@pytest.mark.parametrize("name", ["y_partial", "all_partial"])
def test_render_parity_fused_media_in_the_cornell_room(vpt, oracle, scenes, name):
    """VPT_PIPELINE_AUTO on a tree in LDS: the fused media kernel (k_bounce); the cloud-and-fog scene of test_heterogeneous_cloud_in_cornell."""
    grid = DB.thresholded_cloud(name)

    def vols(gi):
        return [vpt.volume(corner_min=(-3.5, -8.0, -3.0), corner_max=(3.0, -1.0, 3.5), color=(0.85, 0.85, 0.9), density=1.6, anisotropy=0.5,
                           density_data_index=gi, grid_sharpness=1.3, approximated_scattering=1, approximated_scattering_falloff=0.7), fog(vpt, density=0.05)]
    ref, dense, dst, bricked, bst = render_dense_bricked_oracle(vpt, oracle, lit_env_scene(vpt, scenes), vpt.default_params(max_depth=10), grid, vols, 4)
    assert_three_way(ref, dense, dst, bricked, bst)
    assert bst["kernel_launches"]["bounce"] > 0 and bst["kernel_launches"]["extend"] == 0


def test_render_parity_media_streams_with_the_atmosphere(vpt, oracle, scenes):
    """pipeline=2 on a tree in memory: kernels_media.hip; the scene of test_media_on_the_streams_heterogeneous_and_atmosphere.  A batch with media never
    ends in k_finish (see the module's docstring): 3 frames of 128x72x2 samples are far below the finisher's small-batch bound, and it still does not run."""
    grid = DB.thresholded_cloud("all_partial")
    P = vpt.default_params(max_depth=8, sky_altitude=-50.0, sky_azimuth=150.0, samples_per_frame=2)

    def vols(gi):
        return [vpt.volume(corner_min=(-4.0, -9.0, -4.0), corner_max=(4.0, -2.0, 4.0), color=(0.9, 0.9, 0.9), density=1.0, density_data_index=gi), fog(vpt, density=0.05)]
    ref, dense, dst, bricked, bst = render_dense_bricked_oracle(vpt, oracle, glass_room(vpt, scenes, lit=False), P, grid, vols, 3, atmosphere=True, pipeline=2)
    assert_three_way(ref, dense, dst, bricked, bst)
    assert bst["kernel_launches"]["join"] > 0 and bst["kernel_launches"]["bounce"] == 0
    assert bst["finish_paths"] == 0 and dst["finish_paths"] == 0


def test_render_parity_temperature_emission_from_a_bricked_grid(vpt, oracle, scenes):
    """has_temperature_data = 1, use_blackbody = 1: the emission reads the grid through the same lookup (test_fire_volume_temperature_emission's fire)."""
    grid = DB.thresholded_cloud("y_partial")

    def vols(gi):
        return [vpt.volume(corner_min=(-3.0, -7.0, -3.0), corner_max=(3.0, -0.5, 3.0), color=(0.2, 0.2, 0.2), density=1.2, density_data_index=gi,
                           has_temperature_data=1, use_blackbody=1, temperature_color=(1.0, 0.4, 0.1), temperature_gamma=1.7, temperature_scale=6.0,
                           emissive_color_gamma=2.2, kelvin_min=800, kelvin_max=7000)]
    ref, dense, dst, bricked, bst = render_dense_bricked_oracle(vpt, oracle, scenes("cornell_box"), vpt.default_params(max_depth=6), grid, vols, 3)
    assert_three_way(ref, dense, dst, bricked, bst)


def test_dense_and_bricked_grids_mix_clear_and_drain(vpt, oracle, scenes):
    """A dense grid at index 0 and a bricked one at index 1 in one render; vpt_clear_density_grids refused while referenced, accepted afterwards, indices
    restart at 0; a bricked grid added behind vpt_render_async frames still in flight drains them, and the next image is exact."""
    sc = lit_env_scene(vpt, scenes)
    P = vpt.default_params(max_depth=8)
    ga, gb = DB.thresholded_cloud("y_partial"), DB.thresholded_cloud("all_partial")

    def vols(ia, ib):
        return [vpt.volume(corner_min=(-4.5, -9.0, -3.0), corner_max=(-0.5, -4.0, 3.0), color=(0.85, 0.85, 0.9), density=1.6, anisotropy=0.5, density_data_index=ia, grid_sharpness=1.3),
                vpt.volume(corner_min=(0.5, -6.0, -3.0), corner_max=(4.5, -1.0, 3.0), color=(0.9, 0.8, 0.7), density=1.2, density_data_index=ib), fog(vpt, density=0.05)]
    o = oracle.Oracle(sc, W, H); o.set_params(P)
    assert o.add_density_grid(ga) == 0 and o.add_density_grid(gb) == 1
    o.set_volumes(vols(0, 1)); o.render(3); ref = o.radiance()
    g = vpt.PathTracer(W, H, frames_in_flight=2); g.set_scene(sc); g.set_params(P)
    try:
        assert g.add_density_grid(ga) == 0 and g.add_density_bricks(*DB.bricks(gb)) == 1
        g.set_volumes(vols(0, 1)); g.render(3)
        assert np.array_equal(g.radiance(), ref)
        with pytest.raises(vpt.VptError, match="INVALID"):
            g.clear_density_grids()                                       # still referenced
        before = [g.density_grid_info(i) for i in range(2)]
        with pytest.raises(vpt.VptError, match="INVALID"):
            g.add_density_bricks(DB.bricks(gb)[0], np.array([(0, 0, 0), (0, 0, 0)], np.uint32), np.ones((2, 8, 8, 8), F32))   # a rejected call ...
        assert [g.density_grid_info(i) for i in range(2)] == before          # ... leaves the list as it was
        with pytest.raises(vpt.VptError, match="INVALID"):
            g.density_grid_info(2)
        g.set_volumes([fog(vpt)]); g.clear_density_grids()
        with pytest.raises(vpt.VptError, match="INVALID"):
            g.set_volumes(vols(0, 1))                                     # no such grids any more
        g.render(2)                                                       # fog only
        g.render_async(1); g.render_async(1)                              # in flight, nobody waits
        assert g.add_density_bricks(*DB.bricks(gb)) == 0                  # indices restart; drains the two frames
        assert g.add_density_grid(ga) == 1
        assert g.stats()["samples"] == (3 + 2 + 2) * W * H                 # the two asynchronous frames were rendered, none lost
        g.set_volumes(vols(1, 0)); g.render(3)                            # the same two volumes, the grids the other way round in the list
        assert np.array_equal(g.radiance(), ref)
    finally:
        g.close(); o.close()
