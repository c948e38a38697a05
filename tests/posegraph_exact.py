"""The pose graph's contract (include/ndt2d_hip.h, "Pose graph", "Robust losses", "Marginal
covariances") restated in mpmath at 50 decimal digits: the yardstick whose own error does not grow
with the condition number of H, for the graphs of tests/posegraph_hard_cases.py on which a float64
numpy.linalg is no better than what it would judge.

Written from the header.  Nothing is shared with tests/posegraph_restatement.py or with the
product: plain Python lists of mpf values, an own Cholesky, an own inverse.  What is a double in the
contract is taken as that double, exactly (the poses, the transforms, the information matrices, and
the constant pi of Normalize, whose 2 pi is "2.0 * pi" of the double); every operation behind it --
cos and sin of the double heading, the Cholesky factor L of the double information, the products,
the sums -- is carried out in extended precision and rounded to double only when a result is handed
out.  The Newton loop takes its steps from a float64 solve of the extended-precision H (a step needs
no more than a few digits) and is held to the exact gradient: it ends at |g|_inf < 1e-30."""
import numpy as np
from mpmath import MPContext

mp = MPContext()
mp.dps = 50
mpf = mp.mpf

PI = mpf(3.141592653589793)          # the double the contract's Normalize is written with
TWO_PI = 2 * PI                      # "2.0 * pi": exact in binary
DIAG_MIN, DIAG_MAX = mpf(1e-6), mpf(1e32)
DBL_MIN = mpf(2.2250738585072014e-308)
ZERO, ONE = mpf(0), mpf(1)


def normalize(v):
    """Into [-pi, pi): v - 2pi floor((v + pi) / 2pi)."""
    return v - TWO_PI * mp.floor((v + PI) / TWO_PI)


def cholesky(a):
    """The lower factor of a symmetric positive definite matrix (lists of mpf; the lower triangle is
    read), or None where a pivot is <= 0."""
    n = len(a)
    low = [[ZERO] * n for _ in range(n)]
    for j in range(n):
        row_j = low[j]
        d = a[j][j] - mp.fdot(row_j[:j], row_j[:j])
        if not d > 0:
            return None
        root = mp.sqrt(d)
        row_j[j] = root
        for i in range(j + 1, n):
            low[i][j] = (a[i][j] - mp.fdot(low[i][:j], row_j[:j])) / root
    return low


def inverse(a):
    """The inverse of a symmetric positive definite matrix by its Cholesky factor: T = L^-1, then
    T^T T.  Lists of mpf."""
    n = len(a)
    low = cholesky(a)
    if low is None:
        raise ValueError("the matrix is not positive definite")
    t = [[ZERO] * n for _ in range(n)]              # t[c] is COLUMN c of L^-1, the rows c .. n - 1 filled
    for c in range(n):
        col = t[c]
        col[c] = ONE / low[c][c]
        for r in range(c + 1, n):
            col[r] = -mp.fdot(low[r][c:r], col[c:r]) / low[r][r]
    out = [[ZERO] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1):
            out[i][j] = out[j][i] = mp.fdot(t[i][i:], t[j][i:])
    return out


def _mat(values, rows, cols):
    flat = [mpf(float(v)) for v in np.asarray(values, dtype=np.float64).reshape(-1)]
    return [flat[r * cols:(r + 1) * cols] for r in range(rows)]


def _matmul(a, b):
    cols = list(zip(*b))
    return [[mp.fdot(row, col) for col in cols] for row in a]


def _transpose(a):
    return [list(col) for col in zip(*a)]


def to_float(a):
    """Lists of mpf (any depth) as a float64 array: the one rounding."""
    if isinstance(a, (list, tuple)):
        return np.array([to_float(v) for v in a], dtype=np.float64)
    return float(a)


def rho(kind, scale, s):
    """(rho, rho', rho'') of s = |r|^2."""
    a = mpf(float(scale))
    b = a * a
    if kind == "trivial":
        return s, ONE, ZERO
    if kind == "huber":
        if s <= b:
            return s, ONE, ZERO
        q = mp.sqrt(s)
        w = max(DBL_MIN, a / q)
        return 2 * a * q - b, w, -w / (2 * s)
    if kind == "cauchy":
        u = 1 + s / b
        w = max(DBL_MIN, 1 / u)
        return b * mp.log(u), w, -(w * w) / b
    raise ValueError(kind)


class Graph:
    """poses [n, 3]; begin, end [m]; transform [m, 3]; information [m, 3, 3]; the fixed pose; the
    weighting; the loss with its scale and the constraints it applies to (None: every one)."""

    def __init__(self, poses, begin, end, transform, information, fixed=0, weighting="reference", loss="trivial", scale=1.0, robust=None):
        if weighting not in ("reference", "information"):
            raise ValueError(weighting)
        self.poses = np.array(poses, dtype=np.float64).reshape(-1, 3)
        self.begin = [int(v) for v in begin]
        self.end = [int(v) for v in end]
        self.n, self.m = len(self.poses), len(self.begin)
        self.fixed, self.weighting = int(fixed), weighting
        self.transform = _mat(transform, self.m, 3)
        self.loss, self.scale = loss, float(scale)
        self.robust = [True] * self.m if robust is None else [bool(v) for v in np.asarray(robust).reshape(self.m)]
        self.W = []
        for c, info in enumerate(np.asarray(information, dtype=np.float64).reshape(self.m, 3, 3)):
            low = cholesky(_mat(info, 3, 3))
            if low is None:
                raise ValueError("constraint %d: its information is not symmetric positive definite" % c)
            self.W.append(low if weighting == "reference" else _transpose(low))
        self._cache = {}

    # ---- helpers ----

    def _x(self, x):
        """[n][3] mpf of doubles [n, 3] or of lists of mpf."""
        if isinstance(x, list):
            return x
        return _mat(x, self.n, 3)

    def _on(self, enabled):
        return [True] * self.m if enabled is None else [bool(v) for v in np.asarray(enabled).reshape(self.m)]

    def free_nodes(self, enabled=None):
        """The nodes that can move: with an enabled constraint, and not the fixed one."""
        on = self._on(enabled)
        touched = [False] * self.n
        for c in range(self.m):
            if on[c]:
                touched[self.begin[c]] = touched[self.end[c]] = True
        touched[self.fixed] = False
        return touched

    def index(self, enabled=None):
        """The scalar unknowns that can move, ascending."""
        return [3 * i + k for i, f in enumerate(self.free_nodes(enabled)) if f for k in range(3)]

    # ---- the terms of one constraint ----

    def _terms(self, x, c, jacobians=True):
        """(e, r, chi2, rho, rho', W A, W B, rho'') of constraint c at x."""
        a, b, t, W = x[self.begin[c]], x[self.end[c]], self.transform[c], self.W[c]
        co, si = mp.cos(a[2]), mp.sin(a[2])
        dx, dy = b[0] - a[0], b[1] - a[1]
        ex, ey = co * dx + si * dy, co * dy - si * dx
        e = [ex - t[0], ey - t[1], normalize((b[2] - a[2]) - t[2])]
        r = [mp.fdot(W[i], e) for i in range(3)]
        s = mp.fdot(r, r)
        p, w, second = rho(self.loss, self.scale, s) if self.robust[c] else (s, ONE, ZERO)
        if not jacobians:
            return e, r, s, p, w, None, None, second
        A = [[-co, -si, ey], [si, -co, -ex], [ZERO, ZERO, -ONE]]
        B = [[co, si, ZERO], [-si, co, ZERO], [ZERO, ZERO, ONE]]
        return e, r, s, p, w, _matmul(W, A), _matmul(W, B), second

    # ---- what evaluate gives ----

    def evaluate(self, x=None, enabled=None):
        """dict(e [m, 3], r [m, 3], chi2 [m], rho [m], weights [m] (rho'), cost, g [3n] (zero for a
        node that cannot move)), float64, each value rounded once."""
        x = self._x(self.poses if x is None else x)
        on = self._on(enabled)
        free = self.free_nodes(enabled)
        out = dict(e=[], r=[], chi2=[], rho=[], weights=[])
        g = [ZERO] * (3 * self.n)
        cost = ZERO
        for c in range(self.m):
            e, r, s, p, w, JA, JB, _ = self._terms(x, c)
            out["e"].append(e), out["r"].append(r), out["chi2"].append(s), out["rho"].append(p), out["weights"].append(w)
            if not on[c]:
                continue
            cost += p
            for node, J in ((self.begin[c], JA), (self.end[c], JB)):
                if free[node]:
                    for k in range(3):
                        g[3 * node + k] += w * (J[0][k] * r[0] + J[1][k] * r[1] + J[2][k] * r[2])
        out = {k: to_float(v) for k, v in out.items()}
        out.update(cost=float(cost / 2), g=to_float(g), g_exact=g)
        return out

    def gradient_norm(self, x=None, enabled=None):
        """|g|_inf over the unknowns that can move, rounded once."""
        g = self.evaluate(x, enabled)["g_exact"]
        return float(max(abs(v) for v in g)) if g else 0.0

    # ---- H and the damped system ----

    def hessian(self, x=None, enabled=None, curvature=False):
        """(H_FF as lists of mpf, the index of its unknowns): H = sum rho'_c J_c^T J_c over the
        enabled constraints, the rows and columns of the nodes that can move.  curvature=True adds the
        loss's second-order term 2 rho''_c (J_c^T r_c)(J_c^T r_c)^T, which the contract's H leaves out:
        for the Newton loop's steps only."""
        x = self._x(self.poses if x is None else x)
        on = self._on(enabled)
        index = self.index(enabled)
        at = {u: k for k, u in enumerate(index)}
        H = [[ZERO] * len(index) for _ in range(len(index))]
        for c in range(self.m):
            if not on[c]:
                continue
            _, r, _, _, w, JA, JB, second = self._terms(x, c)
            second = 2 * second if curvature else ZERO
            ends = [(self.begin[c], _transpose(JA)), (self.end[c], _transpose(JB))]
            for ni, Ji in ends:
                if 3 * ni not in at:
                    continue
                for nj, Jj in ends:
                    if 3 * nj not in at:
                        continue
                    for k in range(3):
                        row = H[at[3 * ni + k]]
                        for l in range(3):
                            row[at[3 * nj + l]] += w * mp.fdot(Ji[k], Jj[l])
                            if second:
                                row[at[3 * nj + l]] += second * mp.fdot(Ji[k], r) * mp.fdot(Jj[l], r)
        return H, index

    def system(self, x=None, enabled=None, damping=0.0, clamp=True):
        """(A = H_FF + damping clip(diag H_FF, 1e-6, 1e32), index).  clamp=False leaves the clip out:
        the matrix a solver that forgot it would invert."""
        H, index = self.hessian(x, enabled)
        d = mpf(float(damping))
        for k in range(len(H)):
            diag = H[k][k]
            if clamp:
                diag = min(max(diag, DIAG_MIN), DIAG_MAX)
            H[k][k] += d * diag
        return H, index

    def covariance(self, x=None, enabled=None, damping=0.0, clamp=True):
        """dict(sigma [len(F), len(F)] float64 (rounded once), exact (lists of mpf), index, A (float64, for
        residual checks), inverse_norm: |A^-1|_inf), cached per argument set."""
        key = ("cov", None if x is None else np.asarray(to_float(x) if isinstance(x, list) else x, dtype=np.float64).tobytes(),
               None if enabled is None else bytes(np.asarray(enabled, dtype=np.uint8)), float(damping), bool(clamp))
        if key not in self._cache:
            A, index = self.system(x, enabled, damping, clamp)
            S = inverse(A)
            norm = float(max(mp.fsum(abs(v) for v in row) for row in S)) if S else 0.0
            self._cache[key] = dict(sigma=to_float(S).reshape(len(index), len(index)), exact=S, index=index, A_exact=A,
                                    A=to_float(A).reshape(len(index), len(index)), inverse_norm=norm)
        return self._cache[key]

    def blocks(self, sigma, index):
        """[n, n, 3, 3] of a [len(F), len(F)] array over `index`: zero blocks for nodes not in F."""
        full = np.zeros((3 * self.n, 3 * self.n))
        full[np.ix_(index, index)] = sigma
        return full.reshape(self.n, 3, self.n, 3).transpose(0, 2, 1, 3)

    def defect(self, A_exact, sigma):
        """|A sigma - I|_max of a float64 sigma against the extended-precision A, rounded once."""
        n = len(A_exact)
        S = _mat(sigma, n, n)
        worst = ZERO
        cols = list(zip(*S))
        for i in range(n):
            for j in range(n):
                v = abs(mp.fdot(A_exact[i], cols[j]) - (1 if i == j else 0))
                if v > worst:
                    worst = v
        return float(worst)

    # ---- the minimiser ----

    def minimiser(self, enabled=None, start=None, max_iterations=400):
        """dict(x [n, 3] float64 (rounded once), exact (lists of mpf), gradient: the exact |g|_inf
        there, iterations, cost), cached.  Gauss-Newton on the reweighted H (under a loss with its
        second-order term, where that leaves the matrix definite) with a damping that is raised when
        neither the cost nor |g|_inf falls and dropped to zero near the minimiser; the steps come from a
        float64 solve of the extended-precision system, the test on the gradient is exact."""
        key = ("min", None if enabled is None else bytes(np.asarray(enabled, dtype=np.uint8)),
               None if start is None else np.asarray(start, dtype=np.float64).tobytes())
        if key in self._cache:
            return self._cache[key]
        x = [list(row) for row in self._x(self.poses if start is None else start)]
        index = self.index(enabled)
        lam, it = 1e-6, 0
        ev = self.evaluate(x, enabled)
        cost = self._cost_exact(x, enabled)
        while True:
            g = ev["g_exact"]
            norm = max([abs(v) for v in g] + [ZERO])
            if norm < mpf("1e-30") or not index:
                break
            if it >= max_iterations:
                raise RuntimeError("the Newton loop did not reach |g|_inf < 1e-30: %s after %d iterations" % (mp.nstr(norm, 5), it))
            it += 1
            H, _ = self.hessian(x, enabled, curvature=self.loss != "trivial")
            H64 = to_float(H).reshape(len(index), len(index))
            if self.loss != "trivial" and np.min(np.linalg.eigvalsh(H64)) <= 0.0:      # (far from the minimiser: the contract's H)
                H64 = to_float(self.hessian(x, enabled)[0]).reshape(len(index), len(index))
            g64 = np.array([float(g[u]) for u in index])
            A64 = H64 + lam * np.diag(np.clip(np.diag(H64), 1e-6, 1e32))
            step = np.linalg.solve(A64, -g64)
            trial = [list(row) for row in x]
            for k, u in enumerate(index):
                trial[u // 3][u % 3] += mpf(float(step[k]))
            trial_cost = self._cost_exact(trial, enabled)
            trial_ev = self.evaluate(trial, enabled)
            trial_norm = max(abs(v) for v in trial_ev["g_exact"])
            if trial_cost <= cost or trial_norm < norm:
                x, cost, ev = trial, trial_cost, trial_ev
                lam = 0.0 if lam < 1e-12 else lam * 0.1
            else:
                lam = max(lam * 10.0, 1e-9)
        out = dict(x=to_float(x).reshape(self.n, 3), exact=x, gradient=float(max([abs(v) for v in ev["g_exact"]] + [ZERO])),
                   iterations=it, cost=float(cost))
        self._cache[key] = out
        return out

    def _cost_exact(self, x, enabled=None):
        on = self._on(enabled)
        total = ZERO
        for c in range(self.m):
            if on[c]:
                total += self._terms(x, c, jacobians=False)[3]
        return total / 2


# ---- the derived calls ("Marginal covariances": relative, distance) ----

def relative(pose_a, pose_b, joint):
    """(transform [3], covariance [3, 3]) of pose b in pose a's frame, float64 rounded once: the predicted
    transform (R_a^T (p_b - p_a), theta_b - theta_a) and [A B] sym(joint) [A B]^T; joint [2][2][3][3]
    as lists of mpf (or a float64 array, taken exactly)."""
    t, cov = relative_exact(pose_a, pose_b, joint)
    return to_float(t), to_float(cov)


def relative_exact(pose_a, pose_b, joint):
    a, b = [mpf(float(v)) for v in pose_a], [mpf(float(v)) for v in pose_b]
    if not isinstance(joint, list):
        flat = _mat(joint, 4, 9)
        joint = [[[flat[2 * i + j][3 * r:3 * r + 3] for r in range(3)] for j in range(2)] for i in range(2)]
    co, si = mp.cos(a[2]), mp.sin(a[2])
    dx, dy = b[0] - a[0], b[1] - a[1]
    ex, ey = co * dx + si * dy, co * dy - si * dx
    T = [[-co, -si, ey, co, si, ZERO], [si, -co, -ex, -si, co, ZERO], [ZERO, ZERO, -ONE, ZERO, ZERO, ONE]]
    S = [[(joint[i // 3][j // 3][i % 3][j % 3] + joint[j // 3][i // 3][j % 3][i % 3]) / 2 for j in range(6)] for i in range(6)]
    cov = _matmul(_matmul(T, S), _transpose(T))
    return [ex, ey, b[2] - a[2]], cov


def distance(t_pred, cov_pred, t_meas, cov_meas):
    """d^2 = e^T (cov_pred + cov_meas)^-1 e, e = meas - pred with the heading through Normalize; the
    arguments lists of mpf or float64 arrays (taken exactly); float64 rounded once."""
    def as_mp(v, rows, cols):
        return v if isinstance(v, list) else _mat(v, rows, cols)
    tp, tm = as_mp(t_pred, 1, 3), as_mp(t_meas, 1, 3)
    tp, tm = (tp[0] if isinstance(tp[0], list) else tp), (tm[0] if isinstance(tm[0], list) else tm)
    cp, cm = as_mp(cov_pred, 3, 3), as_mp(cov_meas, 3, 3)
    S = [[cp[i][j] + cm[i][j] for j in range(3)] for i in range(3)]
    Si = inverse(S)
    e = [tm[0] - tp[0], tm[1] - tp[1], normalize(tm[2] - tp[2])]
    return float(mp.fdot(e, [mp.fdot(row, e) for row in Si]))
