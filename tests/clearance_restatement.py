"""The clearance map (include/ndt2d_hip.h, "Clearance map"; csrc/clearance/) restated on the CPU in
numpy.  Test infrastructure only: nothing of the product is imported.  The yardstick of
tests/test_clearance_restatement.py (which pins it to a brute force, to scipy and to closed forms)
and of the GPU tests.

    obstacle  a byte that is neither 0 nor -1; with unknown_is_obstacle a byte that is not 0
    d2[y][x]  the exact squared Euclidean distance in cells to the nearest obstacle cell, uint32;
              FAR = 0xFFFFFFFF when there is none, or when a cap R > 0 is set and d2 > R * R
    min_d2    ceil((clearance / resolution)^2), the divide and the product in float64
    mask      byte 0 with d2 < min_d2 becomes 99, every other byte is kept

Everything is integer arithmetic in int64, so the restatement is exact.
"""
import math

import numpy as np

FAR = 0xFFFFFFFF
INSCRIBED = 99
_NONE = np.int64(1) << np.int64(40)        # "no obstacle in this column": its square stays below 2^63


def obstacles(grid, unknown_is_obstacle=False):
    grid = np.asarray(grid, dtype=np.int8)
    return (grid != 0) if unknown_is_obstacle else ((grid != 0) & (grid != -1))


def column_distance(obs):
    """g[y][x], int64: |y - y'| to the nearest obstacle row y' of column x, _NONE without one."""
    h, w = obs.shape
    rows = np.arange(h, dtype=np.int64)[:, None]
    up = np.maximum.accumulate(np.where(obs, rows, np.int64(-1)), axis=0)             # last obstacle row <= y
    down = np.minimum.accumulate(np.where(obs, rows, _NONE)[::-1], axis=0)[::-1]      # first obstacle row >= y
    g = np.full((h, w), _NONE, dtype=np.int64)
    g = np.where(up >= 0, np.minimum(g, rows - up), g)
    g = np.where(down < _NONE, np.minimum(g, down - rows), g)
    return g


def cap_d2(exact, max_cells=0):
    """int64 exact distances (negative: no obstacle) -> the uint32 contract."""
    out = np.where(exact < 0, np.int64(FAR), exact)
    if max_cells > 0:
        out = np.where(out > np.int64(max_cells) * np.int64(max_cells), np.int64(FAR), out)
    return out.astype(np.uint32)


def d2_separable(grid, unknown_is_obstacle=False, max_cells=0):
    """Per column the nearest obstacle, per row the minimum over ALL x' of (x - x')^2 + g^2."""
    obs = obstacles(grid, unknown_is_obstacle)
    h, w = obs.shape
    g = column_distance(obs)
    xs = np.arange(w, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2                      # [x, x']
    exact = np.empty((h, w), dtype=np.int64)
    for y in range(h):
        gy = g[y]
        cand = dx2 + np.where(gy < _NONE, gy * gy, np.int64(1) << np.int64(62))[None, :]
        best = cand.min(axis=1)
        exact[y] = np.where(best >= (np.int64(1) << np.int64(62)), np.int64(-1), best)
    return cap_d2(exact, max_cells)


def d2_brute(grid, unknown_is_obstacle=False, max_cells=0):
    """O(cells x obstacles): for small maps."""
    obs = obstacles(grid, unknown_is_obstacle)
    h, w = obs.shape
    oy, ox = np.nonzero(obs)
    if len(oy) == 0:
        return cap_d2(np.full((h, w), -1, dtype=np.int64), max_cells)
    ys, xs = np.mgrid[0:h, 0:w]
    exact = np.full((h, w), np.iinfo(np.int64).max, dtype=np.int64)
    for y, x in zip(oy.astype(np.int64), ox.astype(np.int64)):
        exact = np.minimum(exact, (ys - y) ** 2 + (xs - x) ** 2)
    return cap_d2(exact, max_cells)


def min_d2(clearance, resolution):
    """ceil(q * q), q = clearance / resolution in float64."""
    q = np.float64(clearance) / np.float64(resolution)
    return int(math.ceil(q * q))


def mask(grid, d2, threshold):
    grid = np.asarray(grid, dtype=np.int8)
    out = grid.copy()
    out[(grid == 0) & (np.asarray(d2).astype(np.int64) < int(threshold))] = INSCRIBED
    return out


def cleared_table(grid, d2, threshold, region=None):
    """The seeder's table under a clearance: the free cells with d2 >= threshold, inside the region."""
    grid = np.asarray(grid, dtype=np.int8)
    keep = (grid == 0) & (np.asarray(d2).astype(np.int64) >= int(threshold))
    if region is not None:
        x0, y0, w, h = region
        inside = np.zeros_like(keep)
        inside[y0:y0 + h, x0:x0 + w] = True
        keep &= inside
    return np.flatnonzero(keep.reshape(-1)).astype(np.uint32)


# ---- the maps of the tests ----

def random_map(height, width, seed, density):
    """Obstacles (100) at `density`, a sprinkling of unknown (-1) cells, the rest free."""
    rng = np.random.default_rng(seed)
    grid = np.zeros((height, width), dtype=np.int8)
    grid[rng.random((height, width)) < 0.1] = -1
    grid[rng.random((height, width)) < density] = 100
    return grid


SHAPES = {
    "1x1 obstacle": lambda: np.full((1, 1), 100, dtype=np.int8),
    "1x1 free": lambda: np.zeros((1, 1), dtype=np.int8),
    "1x65": lambda: random_map(1, 65, 1, 0.05),
    "65x1": lambda: random_map(65, 1, 2, 0.05),
    "7x63": lambda: random_map(7, 63, 3, 0.02),
    "7x64": lambda: random_map(7, 64, 4, 0.02),
    "5x65": lambda: random_map(5, 65, 5, 0.02),
    "9x257": lambda: random_map(9, 257, 6, 0.01),
    "1030x70": lambda: random_map(1030, 70, 7, 0.0005),
    "300x300 dense": lambda: random_map(300, 300, 8, 0.02),
    "300x300 sparse": lambda: random_map(300, 300, 9, 0.0002),
}
