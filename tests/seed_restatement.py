"""Global localisation's seeder (include/ndt2d_hip.h, "Global localisation"; csrc/seed/) restated on
the CPU in numpy, on top of noise_restatement.philox_words.  Test infrastructure only: nothing of
the product is imported.  The yardstick of tests/test_seed_restatement.py (which pins it to designed
words) and of tests/test_gpu_seed.py.

Particle `index` at (seed, step) takes block A = Philox(counter (index, step)) and block B =
Philox(counter (index, step + 1)):
    u     = ((a0 >> 5) * 2^26 + (a1 >> 6)) * 2^-53
    k     = min(F - 1, trunc(u * F));  cell = free_cells[k];  cx, cy = cell mod width, cell // width
    ux    = ((a2 >> 8) + 0.5) * 2^-24, uy from a3
    x     = origin_x + (cx + ux) * resolution   (three float64 roundings; numpy never fuses them)
    theta = -pi + (2 pi) * ((b0 >> 8) + 0.5) * 2^-24
    v     = ((b1 >> 5) * 2^26 + (b2 >> 6)) * 2^-53     the inject draw
Every step is float64 arithmetic that IEEE fixes to the bit, so the restatement is exact.
"""
import numpy as np

from noise_restatement import philox_words

PI = np.float64(np.pi)
TWO_PI = np.float64(2.0) * PI
INV53 = np.float64(2.0 ** -53)
INV24 = np.float64(2.0 ** -24)
_MASK64 = (1 << 64) - 1


def free_table(grid, region=None):
    """free_cells: the row-major indices of the cells of `grid` [h, w] (int8) that are exactly 0,
    inside region = (x0, y0, w, h) when given, ascending."""
    grid = np.asarray(grid)
    free = grid == 0
    if region is not None:
        x0, y0, w, h = region
        inside = np.zeros_like(free)
        inside[y0:y0 + h, x0:x0 + w] = True
        free = free & inside
    return np.flatnonzero(free.reshape(-1)).astype(np.uint32)


def uniform53(hi, lo):
    bits = ((np.asarray(hi, dtype=np.uint64) >> np.uint64(5)) << np.uint64(26)) + \
        (np.asarray(lo, dtype=np.uint64) >> np.uint64(6))
    return bits.astype(np.float64) * INV53        # bits < 2^53: exact; the product too


def uniform24(word):
    k = (np.asarray(word, dtype=np.uint64) >> np.uint64(8)).astype(np.float64)
    return (k + np.float64(0.5)) * INV24


def pick(u, n_free):
    """min(F - 1, (uint64)(u * F))"""
    scaled = np.asarray(u, dtype=np.float64) * np.float64(n_free)
    k = np.trunc(scaled).astype(np.uint64)
    return np.minimum(k, np.uint64(n_free - 1))


def coordinate(origin, cell, u, resolution):
    in_cells = np.asarray(cell).astype(np.float64) + u
    metres = in_cells * np.float64(resolution)
    return np.float64(origin) + metres


def heading(u):
    return -PI + TWO_PI * u


def from_words(a, b, free_cells, width, origin_x, origin_y, resolution):
    """(poses [n, 3], inject draw [n], table index k [n]) from the words of blocks A and B [n, 4]."""
    free_cells = np.asarray(free_cells, dtype=np.uint32)
    k = pick(uniform53(a[:, 0], a[:, 1]), len(free_cells))
    cell = free_cells[k.astype(np.int64)].astype(np.uint64)
    cy = cell // np.uint64(width)
    cx = cell - cy * np.uint64(width)
    x = coordinate(origin_x, cx, uniform24(a[:, 2]), resolution)
    y = coordinate(origin_y, cy, uniform24(a[:, 3]), resolution)
    theta = heading(uniform24(b[:, 0]))
    return np.stack([x, y, theta], axis=-1), uniform53(b[:, 1], b[:, 2]), k


def words(seed, step, first_index, n):
    """Blocks A and B of particles first_index .. first_index + n (the step wraps at 2^64)."""
    return philox_words(seed, step, first_index, n), philox_words(seed, (int(step) + 1) & _MASK64, first_index, n)


def sample(seed, step, first_index, n, free_cells, width, origin_x, origin_y, resolution):
    """ndt2d_seed_launch: poses [n, 3]."""
    a, b = words(seed, step, first_index, n)
    return from_words(a, b, free_cells, width, origin_x, origin_y, resolution)[0]


def inject(poses, probability, seed, step, first_index, free_cells, width, origin_x, origin_y, resolution):
    """ndt2d_seed_inject_launch: (poses after, replaced mask)."""
    poses = np.array(poses, dtype=np.float64, copy=True)
    a, b = words(seed, step, first_index, len(poses))
    fresh, v, _ = from_words(a, b, free_cells, width, origin_x, origin_y, resolution)
    take = v < np.float64(probability)
    poses[take] = fresh[take]
    return poses, take


def cell_of(p, origin, resolution):
    """int((p - origin) / resolution), the occupancy grid's own rule (reference
    src/occupancy_grid.cpp:82-83)."""
    return np.trunc((np.asarray(p, dtype=np.float64) - np.float64(origin)) / np.float64(resolution)).astype(np.int64)

