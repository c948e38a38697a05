"""Inputs for the off-grid tests (tests/test_offgrid_points.py, tests/test_gpu_offgrid_points.py).

Points that NDT::getIndex (reference src/ndt_model.cpp:203-218) cannot map to a cell -- NaN,
+-inf, 1e300, DBL_MAX, a point 2^32 cells or more from the origin -- placed first and last in a
scan, on both sides of every quarter boundary of HostNdt::add_scan and in the n % 4 tail, on
maps whose cell 0, column 0 and row 0 hold points: a point cast into column 0 / row 0 (or
wrapped mod 2^32 into an occupied cell, as the reference's conversion does on x86) changes a
grid or a score.

The expected answer for such an input is the oracle's answer for the SUBSTITUTE input: every
off-grid point replaced by the finite point (1e6, 1e6) of the scan's frame -- off the grid for
every pose a test uses, and a point whose fate the reference defines.  The off-grid rule
(include/ndt2d_hip.h) makes the two inputs give the same grid bit for bit and the same scores."""
import math
import sys

import numpy as np

NAN, INF, DMAX = float("nan"), float("inf"), sys.float_info.max
SUBSTITUTE = (1.0e6, 1.0e6)
SCAN_LENGTHS = (31, 32, 33, 720)

# (cell size, range_max) -> (n, n) cells about the map pose (0, 0): origin (-range_max, -range_max)
#   0.25 / 4.75:  39 x 39 (power-of-two cell, under 1 MiB of HostCells: the side-by-side build)
#   0.3  / 4.75:  32 x 32 (true divide, under 1 MiB)
#   0.07 / 2.0:   58 x 58 (true divide, under 1 MiB)
#   0.05 / 4.75: 191 x 191 (true divide, over 1 MiB: the sequential loop)
#   0.25 / 16.0: 129 x 129 (power-of-two cell, over 1 MiB)
MAPS = {"p2-small": (0.25, 4.75), "div-small": (0.3, 4.75), "div-fine": (0.07, 2.0),
        "div-large": (0.05, 4.75), "p2-large": (0.25, 16.0)}
HOST_CELL_BYTES = 104
SIDE_BY_SIDE_MAX_BYTES = 1 << 20


def geometry(cell, range_max):
    """The NDT addScans gives poses at (0, 0) (reference src/scan_matcher_ndt.cpp:49-74,
    src/ndt_model.cpp:121-122): (size_x, size_y, origin_x, origin_y)."""
    n = int((range_max - -range_max) / cell + 1)
    return n, n, -range_max, -range_max


def off_grid_points(cell, range_max):
    """[(x, y, k or None)] in world = scan coordinates (the scans sit at pose (0, 0, 0)).  The
    finite partner coordinate of each point lies in cell 0's column / row; k: the column (row)
    the reference's x86 conversion wraps a 2^32-cell point into."""
    sx, sy, ox, oy = geometry(cell, range_max)
    x0, y0 = ox + 0.5 * cell, oy + 0.5 * cell
    pts = [(NAN, NAN, None), (NAN, y0, None), (x0, NAN, None), (INF, y0, None), (-INF, y0, None),
           (x0, INF, None), (INF, NAN, None), (1e300, y0, None), (-1e300, y0, None), (DMAX, DMAX, None)]
    for j in (1, 2):
        for k in (0, 3):
            w = (2.0 ** 32 * j + k + 0.5) * cell
            pts.append((ox + w, y0, ("x", k)))
            pts.append((x0, oy + w, ("y", k)))
    return pts


def edge_controls(cell, range_max):
    """Finite points next to the grid's edges: the off-grid rule must leave them as they are."""
    sx, sy, ox, oy = geometry(cell, range_max)
    x0, y0 = ox + 0.5 * cell, oy + 0.5 * cell
    ex, ey = ox + sx * cell, oy + sy * cell
    return [(ox, y0), (x0, oy), (ox, oy), (np.nextafter(ox, -INF), y0), (x0, np.nextafter(oy, -INF)),
            (np.nextafter(ex, -INF), y0), (np.nextafter(ex, INF), y0),
            (x0, np.nextafter(ey, -INF)), (x0, np.nextafter(ey, INF))]


def reference_index(cell, range_max, x, y):
    """getIndex as the reference writes it, for a finite point less than 2^32 cells away
    (where it is defined): truncation toward zero."""
    sx, sy, ox, oy = geometry(cell, range_max)
    if x < ox or y < oy:
        return -1
    gx, gy = int((x - ox) / cell), int((y - oy) / cell)
    if gx >= sx or gy >= sy:
        return -1
    return gy * sx + gx


def edge_scan(cell, range_max, rng):
    """Six points in every cell of column 0 and row 0 (cell 0 gets twelve), spread over the cell
    so that each has a valid information matrix."""
    sx, sy, ox, oy = geometry(cell, range_max)
    frac = np.array([(0.2, 0.3), (0.7, 0.25), (0.5, 0.8), (0.3, 0.6), (0.8, 0.7), (0.45, 0.45)])
    out = []
    for j in range(sy):
        f = np.clip(frac + rng.uniform(-0.05, 0.05, frac.shape), 0.05, 0.95)
        out.append(np.stack([ox + f[:, 0] * cell, oy + (j + f[:, 1]) * cell], axis=1))
    for i in range(sx):
        f = np.clip(frac + rng.uniform(-0.05, 0.05, frac.shape), 0.05, 0.95)
        out.append(np.stack([ox + (i + f[:, 0]) * cell, oy + f[:, 1] * cell], axis=1))
    return np.concatenate(out)


def ring_scan(n, radius, rng):
    """n beams over the full circle hitting a ring of `radius`, a few centimetres thick."""
    ang = np.linspace(-math.pi, math.pi, n, endpoint=False)
    r = radius + 0.03 * rng.standard_normal(n)
    return np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)


def slots(n):
    """Beam positions an off-grid point is put at: first, last, k = q-1, q, q+1 at each of the
    three quarter boundaries (q = n // 4), and the n % 4 beams behind the fourth quarter."""
    q = n // 4
    s = [0, n - 1]
    for b in (q, 2 * q, 3 * q):
        s += [b - 1, b, b + 1]
    s += list(range(4 * q, n))
    return sorted({k for k in s if 0 <= k < n})


def probe_scans(cell, range_max, n, seed=0):
    """(original, substitute) lists of (pose, points[n, 2]) scans: len(off_grid_points) scans of
    n ring beams, scan s carrying point (s + i) % L at its i-th slot, so that every off-grid point
    takes every slot; the edge controls sit in the middle of the quarters."""
    rng = np.random.default_rng(seed)
    offg = off_grid_points(cell, range_max)
    ctrl = edge_controls(cell, range_max)
    sl = slots(n)
    mids = [k for k in range(n // 8, n, max(1, n // 4)) if k not in sl]
    orig, subs = [], []
    for s in range(len(offg)):
        pts = ring_scan(n, 0.6 * range_max, rng)
        for c, k in enumerate(mids):
            pts[k] = ctrl[(s + c) % len(ctrl)][:2]
        sub = pts.copy()
        for i, k in enumerate(sl):
            x, y, _ = offg[(s + i) % len(offg)]
            pts[k] = (x, y)
            sub[k] = SUBSTITUTE
        orig.append(((0.0, 0.0, 0.0), pts))
        subs.append(((0.0, 0.0, 0.0), sub))
    return orig, subs


def map_scans(name, n, seed=0):
    """(original, substitute) map of MAPS[name] built from scans of n beams: the edge scan, two
    ring scans, and the probe scans."""
    cell, range_max = MAPS[name]
    rng = np.random.default_rng(1000 + seed)
    base = [((0.0, 0.0, 0.0), edge_scan(cell, range_max, rng)),
            ((0.0, 0.0, 0.0), ring_scan(720, 0.4 * range_max, rng)),
            ((0.0, 0.0, 0.0), ring_scan(720, 0.8 * range_max, rng))]
    orig, subs = probe_scans(cell, range_max, n, seed)
    return base + orig, base + subs


def substitute(points, mask):
    """points with the rows of `mask` replaced by SUBSTITUTE."""
    out = np.array(points, dtype=np.float64, copy=True)
    out[mask] = SUBSTITUTE
    return out


def is_off_grid_value(points):
    """Rows of points holding a non-finite or beyond-1e8 coordinate (every off-grid point
    above and nothing else of these inputs)."""
    p = np.asarray(points, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(p).all(axis=1) | (np.abs(p) > 1e8).any(axis=1)
