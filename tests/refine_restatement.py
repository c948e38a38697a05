"""The Newton NDT registration (include/ndt2d_hip.h, "Newton NDT registration") restated on the
CPU: numpy over the oracle's cells6 records, libm's exp and sincos, every operation in the order
the contract gives.  Test infrastructure only: the yardstick of tests/test_refine_host.py (which
pins it to the oracle's scorePoints) and tests/test_gpu_refine.py.

Summation orders: "sequential" adds the beams' terms in beam order (f then has the oracle's bits);
"strided" adds them as the kernel does -- thread t takes beams t, t + 256, ... in order, the 64
lanes of a wave reduce over the fixed lane network, the four waves in wave order.
"""
import ctypes as C
import ctypes.util
import math

import numpy as np

CONVERGED, MAX_EVALS, STALLED, NO_OVERLAP, NOT_FINITE = range(5)
THREADS, WAVE = 256, 64

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sincos.restype = None
_libm.sincos.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]


def cos_sin(theta):
    """libm's sincos pair (its sine can differ from sin()'s in the last place: the oracle and the
    library ask for the pair)."""
    s, c = C.c_double(0.0), C.c_double(0.0)
    _libm.sincos(float(theta), C.byref(s), C.byref(c))
    return c.value, s.value


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


class Grid:
    """The oracle's NDT as records: cells6[ncell][6] = mean_x, mean_y, I00, I01, I11, n."""

    def __init__(self, cells6, size_x, size_y, cell_size, origin):
        self.cells = np.ascontiguousarray(cells6, dtype=np.float64).reshape(-1, 6)
        self.size_x, self.size_y = int(size_x), int(size_y)
        self.cell_size = float(cell_size)
        self.origin = (float(origin[0]), float(origin[1]))
        assert len(self.cells) == self.size_x * self.size_y

    @classmethod
    def of_oracle(cls, oracle_matcher):
        ndt = oracle_matcher.ndt
        return cls(ndt.cells6(), ndt.size_x, ndt.size_y, ndt.cell_size, ndt.origin)

    def index(self, qx, qy):
        """NDT::getIndex per point, -1 outside (the oracle's orc_ndt_get_index)."""
        with np.errstate(invalid="ignore", over="ignore"):
            fx = (qx - self.origin[0]) / self.cell_size
            fy = (qy - self.origin[1]) / self.cell_size
            inside = (qx >= self.origin[0]) & (qy >= self.origin[1]) & (fx < float(self.size_x)) & (fy < float(self.size_y))
            gx = np.where(inside, fx, 0.0).astype(np.uint32).astype(np.int64)
            gy = np.where(inside, fy, 0.0).astype(np.uint32).astype(np.int64)
        return np.where(inside, gy * self.size_x + gx, -1)


def subsample(points, max_beams):
    """src/scan_matcher_ndt.cpp:165-166,171: the points scorePoints / matchScan use."""
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    n = len(pts)
    use = min(int(max_beams), n)
    if use == 0:
        return pts[:0].copy()
    step = float(n) / float(use)
    return pts[[int(i * step) for i in range(use)]].copy()


def beam_terms(grid, beams, pose, cs=None):
    """[N][10]: each beam's ten terms {e | e a_0..2 | e (-(a_j a_k) + M_jk): xx, xy, xt, yy, yt, tt}
    at `pose`; zero rows for beams whose cell cannot score.  cs: (cos, sin) of the heading, libm's
    sincos pair if not given."""
    b = np.ascontiguousarray(beams, dtype=np.float64).reshape(-1, 2)
    x, y = float(pose[0]), float(pose[1])
    c, s = cos_sin(pose[2]) if cs is None else cs
    bx, by = b[:, 0], b[:, 1]
    out = np.zeros((len(b), 10))
    with np.errstate(all="ignore"):
        qx = c * bx - s * by + x
        qy = s * bx + c * by + y
        idx = grid.index(qx, qy)
        rec = grid.cells[np.where(idx >= 0, idx, 0)]
        has = (idx >= 0) & (rec[:, 5] >= 5)
        mx, my, i00, i01, i11 = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4]
        d0, d1 = qx - mx, qy - my
        # Cell::score's exponent on h = -0.5 I, the roundings of orc_cell_score
        h00, h01, h11 = -0.5 * i00, -0.5 * i01, -0.5 * i11
        t0 = d0 * h00 + d1 * h01
        t1 = d0 * h01 + d1 * h11
        exponent = t0 * d0 + t1 * d1
        e = np.array([_exp(v) if ok else 0.0 for v, ok in zip(exponent, has)])
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


def _sequential(column):
    total = 0.0
    for v in column:
        total += v
    return total


_LANE = np.arange(WAVE)


def _wave_tree(v):
    """wave_sum_to_last_lane: the two quad permutes, row_half_mirror, row_mirror, row_bcast15 into
    rows 1 and 3, row_bcast31 into rows 2 and 3; the sum is lane 63's."""
    v = v + v[_LANE ^ 1]
    v = v + v[_LANE ^ 2]
    v = v + v[(_LANE & ~7) | (7 - (_LANE & 7))]
    v = v + v[(_LANE & ~15) | (15 - (_LANE & 15))]
    row = _LANE >> 4
    v = v + np.where((row == 1) | (row == 3), v[np.maximum(row - 1, 0) * 16 + 15], 0.0)
    v = v + np.where(row >= 2, v[31], 0.0)
    return v[63]


def _strided(column):
    with np.errstate(all="ignore"):
        part = np.zeros(THREADS)
        for t in range(min(THREADS, len(column))):
            part[t] = _sequential(column[t::THREADS])
        waves = [_wave_tree(part[w * WAVE:(w + 1) * WAVE]) for w in range(THREADS // WAVE)]
        return ((waves[0] + waves[1]) + waves[2]) + waves[3]


def evaluate(grid, beams, pose, cs=None, order="sequential"):
    """(f, g[3], H[6] as xx, xy, xt, yy, yt, tt) at `pose`, and the ten sums of |term|."""
    terms, has = beam_terms(grid, beams, pose, cs)
    add = _sequential if order == "sequential" else _strided
    rows = terms[has] if order == "sequential" else terms   # (an absent beam adds nothing either way)
    with np.errstate(all="ignore"):
        sums = [add(rows[:, k]) for k in range(10)]
        magnitude = np.array([float(np.sum(np.abs(terms[has][:, k]))) for k in range(10)])
    return (-sums[0], sums[1:4], sums[4:10]), magnitude


def cholesky_solve(H, g, lam):
    """(H + lam diag D) delta = -g, D_j = max(|H_jj|, 1e-12); None on a pivot that is not > 0.
    The operation order of csrc/refine/ndt2d_refine_step.h."""
    d0, d1, d2 = (max(abs(H[0]), 1e-12), max(abs(H[3]), 1e-12), max(abs(H[5]), 1e-12))
    a00, a01, a02 = H[0] + lam * d0, H[1], H[2]
    a11, a12 = H[3] + lam * d1, H[4]
    a22 = H[5] + lam * d2
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
    y0 = -g[0] / l00
    y1 = (-g[1] - l10 * y0) / l11
    y2 = ((-g[2] - l20 * y0) - l21 * y1) / l22
    t2 = y2 / l22
    t1 = (y1 - l21 * t2) / l11
    t0 = ((y0 - l10 * t1) - l20 * t2) / l00
    return [t0, t1, t2]


def refine(grid, beams, pose, max_evals=32, tol_lin=1e-6, tol_ang=1e-6, order="sequential"):
    """The iteration of the contract from `pose`.  Returns dict(pose, f_start, f, g, H, evals,
    steps, status, lam)."""
    p = [float(v) for v in pose]
    (f, g, H), _ = evaluate(grid, beams, p, None, order)
    out = dict(pose=np.array(p), f_start=f, f=f, g=np.array(g), H=np.array(H), evals=1, steps=0, status=MAX_EVALS, lam=0.0)

    def done(status):
        out.update(pose=np.array(p), f=f, g=np.array(g), H=np.array(H), evals=evals, steps=steps, status=status, lam=lam)
        return out

    evals, steps, lam = 1, 0, 0.0
    if f == 0.0:
        return done(NO_OVERLAP)
    if not math.isfinite(f):
        return done(NOT_FINITE)
    while evals < max_evals:
        delta = cholesky_solve(H, g, lam)
        while delta is None:
            lam = max(10.0 * lam, 1e-3)
            if lam > 1e12:
                return done(STALLED)
            delta = cholesky_solve(H, g, lam)
        if abs(delta[0]) < tol_lin and abs(delta[1]) < tol_lin and abs(delta[2]) < tol_ang:
            return done(CONVERGED)
        trial = [p[0] + delta[0], p[1] + delta[1], p[2] + delta[2]]
        (f2, g2, H2), _ = evaluate(grid, beams, trial, None, order)
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
