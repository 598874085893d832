"""The density grids the brick tests share (tests/test_grid_prep_cpu.py, tests/test_gpu_density_bricks.py): the procedural cloud of
tests/test_oracle_volumes.py with everything below a quarter of its maximum set to 0, so that whole 8x8x8 brick cells are empty, in two shapes —
one whose y is no multiple of 8 and one where no axis is — and the bricking of such a grid restated without the package's own bricks_of."""
import numpy as np

from test_oracle_volumes import cloud_grid

SHAPES = {"y_partial": ((40, 36, 48), 2), "all_partial": ((37, 33, 43), 5)}   # [z, y, x], seed
ACTIVE_CELLS = {"y_partial": 64, "all_partial": 35}                          # of 5 x 5 x 6 = 150 brick cells each


def thresholded_cloud(name):
    shape, seed = SHAPES[name]
    g = cloud_grid(shape, seed).copy()
    g[g < g.max() / np.float32(4.0)] = 0.0
    return g


def cell_dims(grid):
    """(cells_z, cells_y, cells_x) = ceil(shape / 8)."""
    return tuple(-(-n // 8) for n in grid.shape)


def bricks(grid, fill=0.0, keep_all=False):
    """(dims (x, y, z), uint32 [n, 3] coordinates (bx, by, bz), float32 [n, 8, 8, 8] values [brick, z, y, x]) of the cells of `grid` that hold a
    non-zero voxel (keep_all: of every cell), x fastest; a partial brick's voxels outside the box hold `fill`."""
    dz, dy, dx = grid.shape
    cz, cy, cx = cell_dims(grid)
    coords, values = [], []
    for bz in range(cz):
        for by in range(cy):
            for bx in range(cx):
                part = grid[bz * 8:bz * 8 + 8, by * 8:by * 8 + 8, bx * 8:bx * 8 + 8]
                if keep_all or np.any(part != 0):
                    b = np.full((8, 8, 8), fill, np.float32)
                    b[:part.shape[0], :part.shape[1], :part.shape[2]] = part
                    coords.append((bx, by, bz)); values.append(b)
    return (dx, dy, dz), np.array(coords, np.uint32).reshape(-1, 3), np.array(values, np.float32).reshape(-1, 8, 8, 8)
