"""The pose graph's marginal covariances (include/ndt2d_hip.h, "Marginal covariances") restated in
numpy, float64, on top of tests/posegraph_restatement.py (and, under a loss, of
tests/posegraph_robust_restatement.py, whose Problem has the reweighted H): the dense
inv(H_FF + damping clamp(diag H_FF)) placed into n x n blocks; a numpy preconditioned CG on the dense
matrix with the device's recurrences and stop rules, for iteration counts and for how far the
recurrence residual drifts from the true one; and `relative` and `distance` with every operation in
the order csrc/posegraph/ndt2d_posegraph_relative.h writes it, in Python floats (IEEE doubles, no
fused multiply-add), so that equal inputs give equal bits.  Written from the contract; nothing of
the product is imported here."""
import math

import numpy as np

import posegraph_restatement as R

DIAG_MIN, DIAG_MAX = 1e-6, 1e32
CONVERGED, CG_CAP, BREAKDOWN, NOT_FREE = range(4)


def cg_cap(n):
    return min(3 * n + 16, 8192)


class System:
    """A = H_FF + damping clamp(diag H_FF) of Problem P at x under a mask, dense, with what the
    tests measure against: Sigma = inv(A), its own defect and |inv(A)|_inf."""

    def __init__(self, P, x, enabled=None, damping=0.0):
        self.n = P.n
        self.free = P.free(enabled)                       # [3n] bools
        self.index = np.nonzero(self.free)[0]             # the scalar unknowns of F, ascending
        _, H = P.gradient_hessian(np.asarray(x, dtype=np.float64).reshape(-1, 3), enabled)
        Hf = H[np.ix_(self.free, self.free)]
        self.A = Hf + damping * np.diag(np.clip(np.diag(Hf), DIAG_MIN, DIAG_MAX))
        self._inverse = None

    def node_free(self, node):
        return bool(self.free[3 * int(node)])

    def inverse(self):
        if self._inverse is None:
            self._inverse = np.linalg.inv(self.A)
        return self._inverse

    def inverse_norm(self):
        return float(np.max(np.sum(np.abs(self.inverse()), axis=1)))

    def defect(self):
        """|A Sigma - I|_max: the dense inverse's own error, the floor of every comparison with it."""
        return float(np.max(np.abs(self.A @ self.inverse() - np.eye(len(self.A)))))

    def full(self, columns):
        """[len(F), k] over the unknowns of F -> [3n, k] with zeros elsewhere."""
        out = np.zeros((3 * self.n, columns.shape[1]))
        out[self.index] = columns
        return out

    def column(self, node):
        """Sigma[:, node] as [n, 3, 3] blocks (zero where a node is not in F, all zero if `node` is not)."""
        if not self.node_free(node):
            return np.zeros((self.n, 3, 3))
        at = np.searchsorted(self.index, 3 * int(node))
        return self.full(self.inverse()[:, at:at + 3]).reshape(self.n, 3, 3)

    def blocks(self, nodes):
        """[Q, Q, 3, 3]: block (i, j) is the rows of node q_i in the column of q_j."""
        nodes = [int(v) for v in nodes]
        cols = [self.column(q) for q in nodes]
        return np.array([[cols[j][nodes[i]] for j in range(len(nodes))] for i in range(len(nodes))])

    def true_residual(self, node, column_blocks):
        """|A x - e_j|_2 per column j of the query node, for x given as [n, 3, 3] blocks."""
        x = np.asarray(column_blocks, dtype=np.float64).reshape(3 * self.n, 3)[self.index]
        e = np.zeros((len(self.index), 3))
        if self.node_free(node):
            at = np.searchsorted(self.index, 3 * int(node))
            e[at:at + 3] = np.eye(3)
        return np.sqrt(np.sum((self.A @ x - e) ** 2, axis=0))

    # ---- the preconditioners, dense ----

    def jacobi(self):
        """inv of the 3 x 3 diagonal blocks, as one block-diagonal matrix."""
        M = np.zeros_like(self.A)
        for k in range(0, len(self.A), 3):
            M[k:k + 3, k:k + 3] = np.linalg.inv(self.A[k:k + 3, k:k + 3])
        return M

    def band(self):
        """inv of the block-tridiagonal band of A over the nodes in node order: the diagonal blocks
        and the blocks between free nodes i and i + 1."""
        node = self.index[::3] // 3
        M = np.zeros_like(self.A)
        for k in range(len(node)):
            M[3 * k:3 * k + 3, 3 * k:3 * k + 3] = self.A[3 * k:3 * k + 3, 3 * k:3 * k + 3]
            if k + 1 < len(node) and node[k + 1] == node[k] + 1:
                M[3 * k:3 * k + 3, 3 * k + 3:3 * k + 6] = self.A[3 * k:3 * k + 3, 3 * k + 3:3 * k + 6]
                M[3 * k + 3:3 * k + 6, 3 * k:3 * k + 3] = self.A[3 * k + 3:3 * k + 6, 3 * k:3 * k + 3]
        return np.linalg.inv(M)

    def pcg(self, nodes, preconditioner="jacobi", tolerance=1e-10, max_iterations=0, Minv=None):
        """The three columns of each of `nodes` (free ones) by preconditioned CG from 0 with the
        device's recurrences: alpha = r.z / p.Ap; x += alpha p; r -= alpha Ap; stop on |r|_2 <=
        tolerance after the iteration; z = M^-1 r; beta = r.z / (r.z before); p = z + beta p.  All
        columns advance together (one matrix product per iteration), each with its own alpha, beta
        and stop, frozen once stopped.  Returns dict(status, iterations, recurrence: |r|_2 of the
        recurrence, true: |A x - e|_2), each [len(nodes), 3], and x [len(F), len(nodes), 3]."""
        cap = max_iterations or cg_cap(self.n)
        if Minv is None:
            Minv = self.jacobi() if preconditioner == "jacobi" else self.band()
        nodes = [int(v) for v in nodes]
        k = 3 * len(nodes)
        E = np.zeros((len(self.A), k))
        for q, node in enumerate(nodes):
            at = np.searchsorted(self.index, 3 * node)
            E[at:at + 3, 3 * q:3 * q + 3] = np.eye(3)
        X, Rm = np.zeros_like(E), E.copy()
        Z = Minv @ Rm
        Pm, rz = Z.copy(), np.sum(Rm * Z, axis=0)
        status = np.full(k, CG_CAP)
        live = np.ones(k, dtype=bool)
        its, norm = np.zeros(k, dtype=np.int64), np.ones(k)
        it = 0
        while live.any() and it < cap:
            AP = self.A @ Pm
            pAp = np.sum(Pm * AP, axis=0)
            bad = live & ~((pAp > 0.0) & (rz > 0.0) & np.isfinite(pAp) & np.isfinite(rz))
            status[bad] = BREAKDOWN
            live &= ~bad
            alpha = np.where(live, rz / np.where(live, pAp, 1.0), 0.0)
            X[:, live] += alpha[live] * Pm[:, live]
            Rm[:, live] -= alpha[live] * AP[:, live]
            it += 1
            its[live] = it
            norm[live] = np.sqrt(np.sum(Rm[:, live] ** 2, axis=0))
            bad = live & ~np.isfinite(norm)
            status[bad] = BREAKDOWN
            done = live & ~bad & (norm <= tolerance)
            status[done] = CONVERGED
            live &= ~(bad | done)
            if not live.any():
                break
            Z[:, live] = Minv @ Rm[:, live]
            rz_new = np.sum(Rm * Z, axis=0)
            beta = np.where(live, rz_new / np.where(live, rz, 1.0), 0.0)
            Pm[:, live] = Z[:, live] + beta[live] * Pm[:, live]
            rz = np.where(live, rz_new, rz)
        true = np.sqrt(np.sum((self.A @ X - E) ** 2, axis=0))
        shape = (len(nodes), 3)
        return dict(status=status.reshape(shape), iterations=its.reshape(shape), recurrence=norm.reshape(shape), true=true.reshape(shape),
                    x=X.reshape(len(self.A), len(nodes), 3))


# ---- relative and distance (csrc/posegraph/ndt2d_posegraph_relative.h), operation by operation ----

def _jacobians(c, s, ex, ey):
    A = [[-c, -s, ey], [s, -c, -ex], [0.0, 0.0, -1.0]]
    B = [[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]]
    return A, B


def relative(c, s, pa, pb, joint):
    """(t [3], cov [3, 3]) of pose b in pose a's frame; c, s = cos, sin of pa[2]; joint [2, 2, 3, 3]."""
    c, s = float(c), float(s)
    pa, pb = [float(v) for v in pa], [float(v) for v in pb]
    J = np.asarray(joint, dtype=np.float64).reshape(2, 2, 3, 3)
    dx, dy = pb[0] - pa[0], pb[1] - pa[1]
    ex, ey = c * dx + s * dy, c * dy - s * dx
    t = np.array([ex, ey, pb[2] - pa[2]])
    A, B = _jacobians(c, s, ex, ey)
    T = [A[i] + B[i] for i in range(3)]
    S = [[0.5 * (float(J[i // 3, j // 3, i % 3, j % 3]) + float(J[j // 3, i // 3, j % 3, i % 3])) for j in range(6)] for i in range(6)]
    X = [[0.0] * 6 for _ in range(3)]
    for i in range(3):
        for k in range(6):
            v = 0.0
            for l in range(6):
                v += T[i][l] * S[l][k]
            X[i][k] = v
    cov = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            v = 0.0
            for k in range(6):
                v += X[i][k] * T[j][k]
            cov[i, j] = v
    return t, cov


def distance(t_pred, cov_pred, t_meas, cov_meas):
    """d^2 = e^T (cov_pred + cov_meas)^-1 e, or None where the sum's Cholesky fails."""
    S = np.asarray(cov_pred, dtype=np.float64).reshape(3, 3) + np.asarray(cov_meas, dtype=np.float64).reshape(3, 3)
    low = _cholesky(S)
    if low is None:
        return None
    tp, tm = [float(v) for v in t_pred], [float(v) for v in t_meas]
    e = [tm[0] - tp[0], tm[1] - tp[1], float(R.normalize(tm[2] - tp[2]))]
    y0 = e[0] / low[0][0]
    y1 = (e[1] - low[1][0] * y0) / low[1][1]
    y2 = ((e[2] - low[2][0] * y0) - low[2][1] * y1) / low[2][2]
    return (y0 * y0 + y1 * y1) + y2 * y2


def _cholesky(S):
    """cholesky_lower of csrc/posegraph/ndt2d_posegraph_fn.h in Python floats: each subtraction in turn."""
    a = [[float(v) for v in row] for row in np.asarray(S, dtype=np.float64).reshape(3, 3)]
    low = [[0.0] * 3 for _ in range(3)]
    for j in range(3):
        d = a[j][j]
        for k in range(j):
            d -= low[j][k] * low[j][k]
        if not (d > 0.0) or not math.isfinite(d):
            return None
        root = math.sqrt(d)
        low[j][j] = root
        for i in range(j + 1, 3):
            v = a[i][j]
            for k in range(j):
                v -= low[i][k] * low[j][k]
            low[i][j] = v / root
    return low


def transform_between(pa, pb):
    """(R_a^T (p_b - p_a), theta_b - theta_a) with numpy's cos and sin: for differences."""
    c, s = math.cos(pa[2]), math.sin(pa[2])
    dx, dy = pb[0] - pa[0], pb[1] - pa[1]
    return np.array([c * dx + s * dy, c * dy - s * dx, pb[2] - pa[2]])
