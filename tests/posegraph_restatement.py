"""The pose graph's contract (include/ndt2d_hip.h, "Pose graph") restated in numpy, float64: the
residual, the analytic Jacobians, the weighting, the cost, a DENSE H = J^T J, and a damped Newton
loop on np.linalg.solve that runs until |g|_inf stops decreasing.  Written from the contract, not
from the kernel: no conjugate gradients, no preconditioner, no reduction trees.  The yardstick of
tests/test_gpu_posegraph.py; nothing of the product is imported here."""
import math

import numpy as np

PI = 3.141592653589793238462643383279502884
TWO_PI = 2.0 * PI


def normalize(v):
    """Into [-pi, pi): v - 2pi floor((v + pi) / 2pi) (ceres_solver_pose.hpp:60-65)."""
    v = np.asarray(v, dtype=np.float64)
    return v - TWO_PI * np.floor((v + PI) / TWO_PI)


def cholesky_lower(information):
    """The lower factor L of one 3 x 3 (its lower triangle is read), or None where a pivot is <= 0
    or not finite."""
    a = np.asarray(information, dtype=np.float64).reshape(3, 3)
    low = np.zeros((3, 3))
    for j in range(3):
        d = a[j, j] - float(np.dot(low[j, :j], low[j, :j]))
        if not (d > 0.0) or not math.isfinite(d):
            return None
        low[j, j] = math.sqrt(d)
        for i in range(j + 1, 3):
            low[i, j] = (a[i, j] - float(np.dot(low[i, :j], low[j, :j]))) / low[j, j]
    return low


def weights(information, weighting="reference"):
    """W per constraint: L ("reference", what src/ceres_solver.cpp:132 passes) or L^T ("information")."""
    information = np.asarray(information, dtype=np.float64).reshape(-1, 3, 3)
    out = np.zeros_like(information)
    for c, info in enumerate(information):
        low = cholesky_lower(info)
        if low is None:
            raise ValueError("constraint %d: its information is not symmetric positive definite" % c)
        out[c] = low if weighting == "reference" else low.T
    if weighting not in ("reference", "information"):
        raise ValueError(weighting)
    return out


class Problem:
    """poses [n, 3]; begin, end [m]; transform [m, 3]; information [m, 3, 3]; the fixed pose."""

    def __init__(self, poses, begin, end, transform, information, fixed=0, weighting="reference"):
        self.poses = np.array(poses, dtype=np.float64).reshape(-1, 3)
        self.begin = np.array(begin, dtype=np.int64).reshape(-1)
        self.end = np.array(end, dtype=np.int64).reshape(-1)
        self.transform = np.array(transform, dtype=np.float64).reshape(-1, 3)
        self.information = np.array(information, dtype=np.float64).reshape(-1, 3, 3)
        self.fixed = int(fixed)
        self.weighting = weighting
        self.W = weights(self.information, weighting)
        self.n, self.m = len(self.poses), len(self.begin)

    def mask(self, enabled=None):
        return np.ones(self.m, dtype=bool) if enabled is None else np.asarray(enabled).reshape(self.m) != 0

    def errors(self, x):
        """e [m, 3]: (R_a^T (p_b - p_a) - t_xy, Normalize((theta_b - theta_a) - t_theta))."""
        x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
        a, b = x[self.begin], x[self.end]
        c, s = np.cos(a[:, 2]), np.sin(a[:, 2])
        dx, dy = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
        e = np.empty((self.m, 3))
        e[:, 0] = (c * dx + s * dy) - self.transform[:, 0]
        e[:, 1] = (c * dy - s * dx) - self.transform[:, 1]
        e[:, 2] = normalize((b[:, 2] - a[:, 2]) - self.transform[:, 2])
        return e

    def residuals(self, x):
        """(e, r = W e, chi2 = |r|^2), each per constraint."""
        e = self.errors(x)
        r = np.einsum("cij,cj->ci", self.W, e)
        return e, r, (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]

    def cost(self, x, enabled=None):
        return 0.5 * float(np.sum(self.residuals(x)[2][self.mask(enabled)]))

    def jacobians(self, x):
        """The unweighted blocks A = de/d(pose a), B = de/d(pose b), each [m, 3, 3]."""
        x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
        a, b = x[self.begin], x[self.end]
        c, s = np.cos(a[:, 2]), np.sin(a[:, 2])
        dx, dy = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
        ex, ey = c * dx + s * dy, c * dy - s * dx
        A = np.zeros((self.m, 3, 3))
        B = np.zeros((self.m, 3, 3))
        A[:, 0, 0], A[:, 0, 1], A[:, 0, 2] = -c, -s, ey
        A[:, 1, 0], A[:, 1, 1], A[:, 1, 2] = s, -c, -ex
        A[:, 2, 2] = -1.0
        B[:, 0, 0], B[:, 0, 1] = c, s
        B[:, 1, 0], B[:, 1, 1] = -s, c
        B[:, 2, 2] = 1.0
        return A, B

    def free(self, enabled=None):
        """The scalar unknowns that can move: every node with an enabled constraint but the fixed one."""
        on = self.mask(enabled)
        touched = np.zeros(self.n, dtype=bool)
        touched[self.begin[on]] = True
        touched[self.end[on]] = True
        touched[self.fixed] = False
        return np.repeat(touched, 3)

    def gradient_hessian(self, x, enabled=None, hessian=True):
        """g = J^T r [3n] and the dense H = J^T J [3n, 3n] over the enabled constraints (rows and
        columns of nodes that cannot move are left in; free() selects)."""
        on = self.mask(enabled)
        _, r, _ = self.residuals(x)
        A, B = self.jacobians(x)
        JA = np.einsum("cij,cjk->cik", self.W, A)
        JB = np.einsum("cij,cjk->cik", self.W, B)
        g = np.zeros((self.n, 3))
        np.add.at(g, self.begin[on], np.einsum("cji,cj->ci", JA, r)[on])
        np.add.at(g, self.end[on], np.einsum("cji,cj->ci", JB, r)[on])
        if not hessian:
            return g.reshape(-1), None
        H = np.zeros((3 * self.n, 3 * self.n))
        for c in np.nonzero(on)[0]:
            ia, ib = 3 * self.begin[c], 3 * self.end[c]
            ja, jb = JA[c], JB[c]
            H[ia:ia + 3, ia:ia + 3] += ja.T @ ja
            H[ib:ib + 3, ib:ib + 3] += jb.T @ jb
            H[ia:ia + 3, ib:ib + 3] += ja.T @ jb
            H[ib:ib + 3, ia:ia + 3] += jb.T @ ja
        return g.reshape(-1), H

    def gradient_norm(self, x, enabled=None):
        g, _ = self.gradient_hessian(x, enabled, hessian=False)
        f = self.free(enabled)
        return float(np.max(np.abs(g[f]))) if f.any() else 0.0

    def solve(self, enabled=None, max_iterations=200):
        """Damped Newton on the dense system until |g|_inf has not decreased for two iterations.
        Returns dict(x [n, 3], gradient: the smallest |g|_inf met (the floor the arithmetic bottoms
        out at), start_gradient, cost, iterations)."""
        f = self.free(enabled)
        x = self.poses.copy()
        out = dict(x=x.copy(), gradient=self.gradient_norm(x, enabled), cost=self.cost(x, enabled), iterations=0)
        out["start_gradient"] = out["gradient"]
        if not f.any() or out["gradient"] == 0.0:
            return out
        lam, stalled = 1e-9, 0
        cost = out["cost"]
        for it in range(max_iterations):
            g, H = self.gradient_hessian(x, enabled)
            Hf = H[np.ix_(f, f)]
            Hf[np.diag_indices_from(Hf)] += lam * np.maximum(np.diag(Hf), 1e-6)
            step = np.zeros(3 * self.n)
            step[f] = np.linalg.solve(Hf, -g[f])
            trial = x + step.reshape(-1, 3)
            trial_cost = self.cost(trial, enabled)
            if trial_cost <= cost * (1.0 + 1e-12) + 1e-300:
                x, cost = trial, trial_cost
                lam = max(lam * 0.1, 1e-12)
                norm = self.gradient_norm(x, enabled)
                if norm < out["gradient"]:
                    out.update(x=x.copy(), gradient=norm, cost=cost)
                    stalled = 0
                else:
                    stalled += 1
            else:
                lam *= 10.0
                stalled += 1
            out["iterations"] = it + 1
            if stalled >= 2:
                break
        return out

    def inverse_norm(self, x, enabled=None):
        """|H(x)^-1|_inf over the unknowns that can move (the largest absolute row sum)."""
        f = self.free(enabled)
        _, H = self.gradient_hessian(x, enabled)
        return float(np.max(np.sum(np.abs(np.linalg.inv(H[np.ix_(f, f)])), axis=1)))


def make_constraint(from_pose, to_pose, covariance):
    """(transform, information) as src/constraint.cpp:35-56 forms them, the inverse by numpy."""
    fx, fy, fth = (float(v) for v in from_pose)
    tx, ty, tth = (float(v) for v in to_pose)
    dx, dy = tx - fx, ty - fy
    c, s = math.cos(fth), math.sin(fth)
    return np.array([c * dx + s * dy, -s * dx + c * dy, tth - fth]), np.linalg.inv(np.asarray(covariance, dtype=np.float64))
