"""The Newton NDT registration's objective over the 3 x 3 cells round a point (include/ndt2d_hip.h,
"Newton NDT registration", neighbourhood 9) restated on the CPU, on top of
tests/refine_restatement.py: the same numpy arithmetic per (beam, cell) pair, libm's exp and sincos.
Test infrastructure only: the yardstick of tests/test_refine_neighbours_host.py and
tests/test_gpu_refine_neighbours.py.

Items.  With a neighbourhood of K cells (1 or 9) a job's items are (beam, neighbour) pairs,
i = K beam + j; neighbour j is (dy, dx) = (j // 3 - 1, j % 3 - 1) from the beam's own cell (j = 4 is
the own cell; K = 1 has the own cell alone).  A neighbour counts when the point is on the grid,
0 <= gx + dx < size_x and 0 <= gy + dy < size_y -- clipped on (gx, gy), not on the flat index --
and that cell can score (n >= 5).

Summation orders: "sequential" adds the items' terms in item order; "strided" adds them as the
kernel does -- thread t takes items t, t + 256, ... in order, the 64 lanes of a wave reduce over the
fixed lane network, the four waves in wave order.  For K = 1 both are refine_restatement's.
"""
import math

import numpy as np

import refine_restatement as R

CONVERGED, MAX_EVALS, STALLED, NO_OVERLAP, NOT_FINITE = R.CONVERGED, R.MAX_EVALS, R.STALLED, R.NO_OVERLAP, R.NOT_FINITE


def item_terms(grid, beams, pose, cells=9, cs=None):
    """[K N][10]: every item's ten terms at `pose`, zero rows for items that do not count; and the
    mask of the items that count."""
    assert cells in (1, 9)
    b = np.ascontiguousarray(beams, dtype=np.float64).reshape(-1, 2)
    n = len(b)
    x, y = float(pose[0]), float(pose[1])
    c, s = R.cos_sin(pose[2]) if cs is None else cs
    bx, by = np.repeat(b[:, 0], cells), np.repeat(b[:, 1], cells)
    j = np.tile(np.arange(cells), n)
    dy, dx = (j // 3 - 1, j % 3 - 1) if cells == 9 else (np.zeros_like(j), np.zeros_like(j))
    out = np.zeros((cells * n, 10))
    with np.errstate(all="ignore"):
        qx = c * bx - s * by + x
        qy = s * bx + c * by + y
        own = grid.index(qx, qy)
        gy, gx = np.divmod(np.where(own >= 0, own, 0), grid.size_x)
        nx, ny = gx + dx, gy + dy
        on = (own >= 0) & (nx >= 0) & (nx < grid.size_x) & (ny >= 0) & (ny < grid.size_y)
        rec = grid.cells[np.where(on, ny * grid.size_x + nx, 0)]
        has = on & (rec[:, 5] >= 5)
        mx, my, i00, i01, i11 = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4]
        d0, d1 = qx - mx, qy - my
        # Cell::score's exponent on h = -0.5 I, the roundings of orc_cell_score
        h00, h01, h11 = -0.5 * i00, -0.5 * i01, -0.5 * i11
        t0 = d0 * h00 + d1 * h01
        t1 = d0 * h01 + d1 * h11
        exponent = t0 * d0 + t1 * d1
        e = np.zeros(len(has))
        e[has] = [R._exp(v) for v in exponent[has].tolist()]          # libm's exp, one call per counting item
        u0 = i00 * d0 + i01 * d1
        u1 = i01 * d0 + i11 * d1
        r0, r1 = -s * bx - c * by, c * bx - s * by
        w0, w1 = -c * bx + s * by, -s * bx - c * by
        a2 = u0 * r0 + u1 * r1
        ir0 = i00 * r0 + i01 * r1
        ir1 = i01 * r0 + i11 * r1
        m22 = (r0 * ir0 + r1 * ir1) + (u0 * w0 + u1 * w1)
        cols = (e, e * u0, e * u1, e * a2, e * (-(u0 * u0) + i00), e * (-(u0 * u1) + i01), e * (-(u0 * a2) + ir0),
                e * (-(u1 * u1) + i11), e * (-(u1 * a2) + ir1), e * (-(a2 * a2) + m22))
        for k, col in enumerate(cols):
            out[:, k] = np.where(has, col, 0.0)
    return out, has


def _sequential(rows):
    """The columns of rows[n][10] added in row order (numpy's accumulate is the plain loop)."""
    if len(rows) == 0:
        return np.zeros(rows.shape[1])
    return np.add.accumulate(rows, axis=0)[-1]


def _strided(rows):
    """refine_restatement._strided on every column at once: thread t adds rows t, t + 256, ... in
    order (a thread whose rows have run out adds nothing: + 0.0 leaves a sum that is never -0.0
    as it is), the wave tree per column, the four waves in wave order."""
    trips = max(1, -(-len(rows) // R.THREADS))
    padded = np.zeros((trips * R.THREADS, rows.shape[1]))
    padded[:len(rows)] = rows
    part = np.zeros((R.THREADS, rows.shape[1]))
    for trip in padded.reshape(trips, R.THREADS, rows.shape[1]):
        part = part + trip
    out = np.zeros(rows.shape[1])
    for k in range(rows.shape[1]):
        waves = [R._wave_tree(part[w * R.WAVE:(w + 1) * R.WAVE, k]) for w in range(R.THREADS // R.WAVE)]
        out[k] = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    return out


def evaluate(grid, beams, pose, cells=9, cs=None, order="sequential"):
    """(f, g[3], H[6] as xx, xy, xt, yy, yt, tt) at `pose`, and the ten sums of |term|."""
    terms, has = item_terms(grid, beams, pose, cells, cs)
    with np.errstate(all="ignore"):
        # (an absent item adds nothing either way)
        sums = [float(v) for v in (_sequential(terms[has]) if order == "sequential" else _strided(terms))]
        counted = np.abs(terms[has])
        magnitude = np.array([float(np.sum(counted[:, k])) for k in range(10)])
    return (-sums[0], sums[1:4], sums[4:10]), magnitude


def refine(grid, beams, pose, cells=9, max_evals=32, tol_lin=1e-6, tol_ang=1e-6, order="sequential"):
    """refine_restatement.refine (the iteration is the same) on the objective of `cells` cells."""
    p = [float(v) for v in pose]
    (f, g, H), _ = evaluate(grid, beams, p, cells, None, order)
    out = {}
    evals, steps, lam = 1, 0, 0.0

    def done(status):
        out.update(pose=np.array(p), f_start=f_start, f=f, g=np.array(g), H=np.array(H), evals=evals, steps=steps,
                   status=status, lam=lam)
        return out

    f_start = f
    if f == 0.0:
        return done(NO_OVERLAP)
    if not math.isfinite(f):
        return done(NOT_FINITE)
    while evals < max_evals:
        delta = R.cholesky_solve(H, g, lam)
        while delta is None:
            lam = max(10.0 * lam, 1e-3)
            if lam > 1e12:
                return done(STALLED)
            delta = R.cholesky_solve(H, g, lam)
        if abs(delta[0]) < tol_lin and abs(delta[1]) < tol_lin and abs(delta[2]) < tol_ang:
            return done(CONVERGED)
        trial = [p[0] + delta[0], p[1] + delta[1], p[2] + delta[2]]
        (f2, g2, H2), _ = evaluate(grid, beams, trial, cells, None, order)
        evals += 1
        if f2 < f:
            p, f, g, H = trial, f2, g2, H2
            steps += 1
            lam = lam / 10.0
            if lam <= 1e-9:
                lam = 0.0
        else:
            lam = max(10.0 * lam, 1e-3)
            if lam > 1e12:
                return done(STALLED)
    return done(MAX_EVALS)


def covariance(H6):
    """H^-1 by the Cholesky of csrc/refine/ndt2d_refine_step.h (covariance()), its operation order;
    None where an entry is not finite or a pivot is not > 0."""
    if not all(math.isfinite(v) for v in H6):
        return None
    a00, a01, a02, a11, a12, a22 = (float(v) for v in H6)
    if not a00 > 0.0:
        return None
    l00 = math.sqrt(a00)
    l10 = a01 / l00
    l20 = a02 / l00
    p1 = a11 - l10 * l10
    if not p1 > 0.0:
        return None
    l11 = math.sqrt(p1)
    l21 = (a12 - l20 * l10) / l11
    p2 = (a22 - l20 * l20) - l21 * l21
    if not p2 > 0.0:
        return None
    l22 = math.sqrt(p2)
    m00, m11, m22 = 1.0 / l00, 1.0 / l11, 1.0 / l22
    m10 = -(l10 * m00) / l11
    m21 = -(l21 * m11) / l22
    m20 = -(l20 * m00 + l21 * m10) / l22
    c00 = (m00 * m00 + m10 * m10) + m20 * m20
    c01 = m10 * m11 + m20 * m21
    c02 = m20 * m22
    c11 = m11 * m11 + m21 * m21
    c12 = m21 * m22
    c22 = m22 * m22
    out = np.array([[c00, c01, c02], [c01, c11, c12], [c02, c12, c22]])
    return out if np.all(np.isfinite(out)) else None


def line_poses(start, count=300, step=(0.5e-3, 0.3e-3, 0.0)):
    """`count` poses start + k step: the line the smoothness checks walk."""
    return np.asarray(start, dtype=np.float64)[None, :] + np.arange(count)[:, None] * np.asarray(step)[None, :]


def trapezoid_defect(poses, f, g):
    """sum_k |f(p_k+1) - f(p_k) - 1/2 (g_k + g_k+1) . (p_k+1 - p_k)| along the poses: O(h^3) per
    step for a smooth f, O(jump) where f jumps.  Also the largest single step's."""
    poses, f, g = np.asarray(poses), np.asarray(f), np.asarray(g)
    dp = poses[1:] - poses[:-1]
    each = np.abs((f[1:] - f[:-1]) - 0.5 * np.sum((g[1:] + g[:-1]) * dp, axis=1))
    return float(np.sum(each)), float(np.max(each))
