"""numpy restatement of the wide search (include/ndt2d_hip.h, "wide search"; csrc/wide/): the bound
image in the operation order of ndt2d_wide_fn.h, the tile bounds, the order and the exact rounds.
The rounds take every candidate's exact likelihood sum from outside -- the CPU oracle's
matchScan(want_scores=True) in the CPU tests, ndt2d_starts_match's all_scores on the GPU -- so what
is restated here is the procedure, not a score."""
import math

import numpy as np

GUARD = 1.0e-9
INFLATE = 1.0 + 2.0 ** -40
FLOOR = 2.0 ** -1000
STOP = 1.0 - 2.0 ** -35
NEAR_TIE = 2.0 ** -36
FIRST_CHUNK = 64


def records(cells6):
    """cells6 rows {mean_x, mean_y, i00, i01, i11, n} -> (mx, my, h00, h01, h11, can score) with
    h = -0.5 information (exact)."""
    c = np.asarray(cells6, dtype=np.float64).reshape(-1, 6)
    return c[:, 0], c[:, 1], -0.5 * c[:, 2], -0.5 * c[:, 3], -0.5 * c[:, 4], c[:, 5] >= 5.0


def exponent_at(mx, my, h00, h01, h11, px, py):
    q0 = px - mx
    q1 = py - my
    r0 = q0 * h00 + q1 * h01
    r1 = q0 * h01 + q1 * h11
    return r0 * q0 + r1 * q1


def _take(best, v):
    v = np.where(np.isnan(v), np.inf, v)
    return np.maximum(best, v)


def box_max_exponent(mx, my, h00, h01, h11, x0, x1, y0, y1):
    """The maximum of one finite record's exponent over the rectangles [x0, x1] x [y0, y1] (arrays):
    corners, the stationary point of every edge that opens downwards, the mean when inside."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        best = _take(np.full(np.shape(x0), -np.inf), exponent_at(mx, my, h00, h01, h11, x0, y0))
        best = _take(best, exponent_at(mx, my, h00, h01, h11, x0, y1))
        best = _take(best, exponent_at(mx, my, h00, h01, h11, x1, y0))
        best = _take(best, exponent_at(mx, my, h00, h01, h11, x1, y1))
        if h00 < 0.0:
            for yc in (y0, y1):
                q1 = yc - my
                num = h01 * q1
                off = -num / h00
                xs = np.clip(mx + off, x0, x1)
                best = _take(best, exponent_at(mx, my, h00, h01, h11, xs, yc))
        if h11 < 0.0:
            for xc in (x0, x1):
                q0 = xc - mx
                num = h01 * q0
                off = -num / h11
                ys = np.clip(my + off, y0, y1)
                best = _take(best, exponent_at(mx, my, h00, h01, h11, xc, ys))
        inside = (mx >= x0) & (mx <= x1) & (my >= y0) & (my <= y1)
        return np.where(inside, np.maximum(best, 0.0), best)


def window_of(dlin, tile_steps):
    dlin = np.asarray(dlin, dtype=np.float64)
    return max(float(dlin[min(len(dlin), i + tile_steps) - 1] - dlin[i]) for i in range(0, len(dlin), tile_steps))


def geometry(size_x, size_y, cell_size, origin, window, pixels_per_tile):
    pitch = max(window, cell_size / 4.0) / float(pixels_per_tile)
    reach = window + pitch
    nx = int(math.floor((size_x * cell_size + reach) / pitch) + 2.0)
    ny = int(math.floor((size_y * cell_size + reach) / pitch) + 2.0)
    return dict(nx=nx, ny=ny, origin_x=origin[0] - (window + pitch), origin_y=origin[1] - (window + pitch), pitch=pitch,
                window=window, guard=GUARD)


def image(cells6, size_x, size_y, cell_size, origin, window, pixels_per_tile):
    """(geometry, raw, inflated): the pixel values [ny, nx] before and after the 1 + 2^-40."""
    g = geometry(size_x, size_y, cell_size, origin, window, pixels_per_tile)
    mx, my, h00, h01, h11, ok = records(cells6)
    xi = g["origin_x"] + np.arange(g["nx"], dtype=np.float64) * g["pitch"]
    yj = g["origin_y"] + np.arange(g["ny"], dtype=np.float64) * g["pitch"]
    reach = g["pitch"] + window
    bx0, bx1 = xi - GUARD, (xi + reach) + GUARD
    by0, by1 = yj - GUARD, (yj + reach) + GUARD
    # the cells a box touches along an axis: floor((lo - g - o) / c) .. floor((hi + g - o) / c)
    cx0 = np.floor(((bx0 - GUARD) - origin[0]) / cell_size)
    cx1 = np.floor(((bx1 + GUARD) - origin[0]) / cell_size)
    cy0 = np.floor(((by0 - GUARD) - origin[1]) / cell_size)
    cy1 = np.floor(((by1 + GUARD) - origin[1]) / cell_size)
    raw = np.zeros((g["ny"], g["nx"]))
    touched = np.zeros(raw.shape, dtype=bool)
    finite = np.isfinite(mx) & np.isfinite(my) & np.isfinite(h00) & np.isfinite(h01) & np.isfinite(h11)
    for cell in np.flatnonzero(ok & finite):
        cy, cx = divmod(int(cell), size_x)
        ii = np.flatnonzero((cx0 <= cx) & (cx <= cx1))
        jj = np.flatnonzero((cy0 <= cy) & (cy <= cy1))
        if len(ii) == 0 or len(jj) == 0:
            continue
        lx = origin[0] + float(cx) * cell_size - GUARD
        hx = origin[0] + float(cx + 1) * cell_size + GUARD
        ly = origin[1] + float(cy) * cell_size - GUARD
        hy = origin[1] + float(cy + 1) * cell_size + GUARD
        x0, x1 = np.maximum(lx, bx0[ii]), np.minimum(hx, bx1[ii])
        y0, y1 = np.maximum(ly, by0[jj]), np.minimum(hy, by1[jj])
        X0, Y0 = np.meshgrid(x0, y0)
        X1, Y1 = np.meshgrid(x1, y1)
        e = box_max_exponent(mx[cell], my[cell], h00[cell], h01[cell], h11[cell], X0, X1, Y0, Y1)
        with np.errstate(over="ignore"):
            v = np.exp(e)
        meets = (X0 <= X1) & (Y0 <= Y1)
        v = np.where(meets, v, 0.0)
        block = raw[np.ix_(jj, ii)]
        raw[np.ix_(jj, ii)] = np.maximum(block, v)
        touched[np.ix_(jj, ii)] |= meets
    # (the floor is added wherever the box meets a cell that can score, whatever exp() made of it)
    return g, raw, np.where(touched, raw * INFLATE + FLOOR, 0.0)


def rotated(pose, beams, theta_offset):
    """points_outer of a theta step in the searches' operation order."""
    b = np.asarray(beams, dtype=np.float64).reshape(-1, 2)
    ct, st = math.cos(pose[2] + theta_offset), math.sin(pose[2] + theta_offset)
    return b[:, 0] * ct - b[:, 1] * st + pose[0], b[:, 0] * st + b[:, 1] * ct + pose[1]


def look_up(g, data, px, py):
    with np.errstate(invalid="ignore"):
        fx = (px - g["origin_x"]) * (1.0 / g["pitch"])
        fy = (py - g["origin_y"]) * (1.0 / g["pitch"])
        on = (fx >= 0.0) & (fy >= 0.0) & (fx < g["nx"]) & (fy < g["ny"])
    i = np.where(on, fx, 0.0).astype(np.int64)
    j = np.where(on, fy, 0.0).astype(np.int64)
    return np.where(on, data[j, i], 0.0)


def tile_bounds(g, data, pose, beams, dth, dlin, tile_steps):
    """bounds[n_th, n_tiles, n_tiles]: tile (tx, ty) holds ix in [tx T, ..), iy in [ty T, ..)."""
    dlin = np.asarray(dlin, dtype=np.float64)
    corners = dlin[::tile_steps]
    n_beams = len(np.asarray(beams).reshape(-1, 2))
    slack = 1.0 + float(n_beams + 2) * 2.0 ** -51
    out = np.zeros((len(dth), len(corners), len(corners)))
    for ith, dt in enumerate(dth):
        ox, oy = rotated(pose, beams, dt)
        px = ox[None, None, :] + corners[:, None, None]
        py = oy[None, None, :] + corners[None, :, None]
        px, py = np.broadcast_arrays(px, py)
        out[ith] = look_up(g, data, px, py).sum(axis=2) * slack
    return out


def tile_maxima(sums, n_th, n_lin, tile_steps):
    """The largest exact sum inside every tile, [n_th, n_tiles, n_tiles] (NaN sums count as none)."""
    s = np.asarray(sums, dtype=np.float64).reshape(n_th, n_lin, n_lin)
    n_tiles = (n_lin + tile_steps - 1) // tile_steps
    pad = n_tiles * tile_steps - n_lin
    s = np.pad(np.where(np.isnan(s), -np.inf, s), ((0, 0), (0, pad), (0, pad)), constant_values=-np.inf)
    return s.reshape(n_th, n_tiles, tile_steps, n_tiles, tile_steps).max(axis=(2, 4))


def order(bounds):
    """Job indices by bound, descending; equal bounds in ascending job order."""
    flat = np.asarray(bounds).reshape(-1)
    return np.argsort(-flat, kind="stable")


def rounds(bounds, sums, n_th, n_lin, tile_steps, max_tiles=1 << 16):
    """The walk over the sorted jobs in chunks that double: dict(best_sum, best_index (-1: none),
    near_tie, evaluated [n_th, n_tiles, n_tiles] bool, tiles_scored).  sums: every candidate's exact
    likelihood sum (>= 0), flat in lattice order."""
    s = np.asarray(sums, dtype=np.float64).reshape(n_th, n_lin, n_lin)
    n_tiles = (n_lin + tile_steps - 1) // tile_steps
    flat = np.asarray(bounds, dtype=np.float64).reshape(-1)
    jobs = order(flat)
    evaluated = np.zeros(len(flat), dtype=bool)
    seen = np.zeros(s.shape, dtype=bool)
    best_sum, best_index = 0.0, -1
    done, chunk = 0, min(FIRST_CHUNK, max_tiles)
    while done < len(jobs):
        take = jobs[done:done + chunk]
        done += len(take)
        evaluated[take] = True
        for job in take:
            ith, t = divmod(int(job), n_tiles * n_tiles)
            tx, ty = divmod(t, n_tiles)
            seen[ith, tx * tile_steps:(tx + 1) * tile_steps, ty * tile_steps:(ty + 1) * tile_steps] = True
        # the reference's strict `<` in loop order: the largest sum, the lowest flat index among equals
        cand = np.where(seen & (s > 0.0), s, -np.inf).reshape(-1)
        k = int(np.argmax(cand))
        if cand[k] > 0.0:
            best_sum, best_index = float(cand[k]), k
        if done < len(jobs) and flat[jobs[done]] < best_sum * STOP:
            break
        chunk = min(chunk * 2, max_tiles)
    near = False
    if best_index >= 0:
        cand = np.where(seen & (s > 0.0), s, -np.inf).reshape(-1)
        close = np.abs(cand - best_sum) * 2.0 ** 36 <= np.maximum(np.abs(cand), best_sum)
        close[best_index] = False
        near = bool(np.any(close & np.isfinite(cand)))
    return dict(best_sum=best_sum, best_index=best_index, near_tie=near,
                evaluated=evaluated.reshape(n_th, n_tiles, n_tiles), tiles_scored=int(evaluated.sum()))


def subsample(points, max_beams):
    """matchScan's beams (src/scan_matcher_ndt.cpp:95-96,110)."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    n = min(int(max_beams), len(pts))
    step = len(pts) / n
    return np.ascontiguousarray([pts[int(i * step)] for i in range(n)])
