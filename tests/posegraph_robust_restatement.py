"""The pose graph's robust losses (include/ndt2d_hip.h, "Robust losses") restated in numpy, float64,
on top of tests/posegraph_restatement.py: rho, rho' and rho'' of Huber and Cauchy, the robust cost
F = 1/2 sum rho(s_c), its gradient g = sum rho'_c J_c^T r_c, the reweighted dense H = sum rho'_c
J_c^T J_c, a dense Levenberg-Marquardt on np.linalg.solve run to its own |g|_inf floor, and the
true Hessian of F (the reweighted term plus the rho'' term) by central differences of g.  Written
from the contract, not from the kernel; the yardstick of tests/test_gpu_posegraph_robust.py.
Nothing of the product is imported here."""
import numpy as np

import posegraph_restatement as R

DBL_MIN = 2.2250738585072014e-308
KINDS = ("trivial", "huber", "cauchy")


def rho(kind, scale, s):
    """(rho, rho', rho'') of s = |r|^2 >= 0 at the scale a, b = a^2, each shaped as s."""
    s = np.asarray(s, dtype=np.float64)
    a = float(scale)
    b = a * a
    if kind == "trivial":
        return s.copy(), np.ones_like(s), np.zeros_like(s)
    if kind == "huber":
        inlier = s <= b
        q = np.sqrt(np.where(inlier, 1.0, s))
        w = np.where(inlier, 1.0, np.maximum(DBL_MIN, a / q))
        return np.where(inlier, s, 2.0 * a * q - b), w, np.where(inlier, 0.0, -w / (2.0 * np.where(inlier, 1.0, s)))
    if kind == "cauchy":
        w = np.maximum(DBL_MIN, 1.0 / (1.0 + s / b))
        return b * np.log1p(s / b), w, -(w * w) / b
    raise ValueError(kind)


class Problem(R.Problem):
    """R.Problem under a loss: `loss` at `scale` on the constraints `robust` marks (None: every one)."""

    def __init__(self, poses, begin, end, transform, information, fixed=0, weighting="reference", loss="trivial", scale=1.0, robust=None):
        super().__init__(poses, begin, end, transform, information, fixed=fixed, weighting=weighting)
        if loss not in KINDS:
            raise ValueError(loss)
        self.loss, self.scale = loss, float(scale)
        self.robust = np.ones(self.m, dtype=bool) if robust is None else np.asarray(robust).reshape(self.m) != 0

    def rho(self, x):
        """(chi2, rho, rho', rho'') per constraint at x; a constraint the loss is not applied to has rho = s."""
        s = self.residuals(x)[2]
        p, w, c = rho(self.loss, self.scale, s)
        return s, np.where(self.robust, p, s), np.where(self.robust, w, 1.0), np.where(self.robust, c, 0.0)

    def cost(self, x, enabled=None):
        return 0.5 * float(np.sum(self.rho(x)[1][self.mask(enabled)]))

    def weights(self, x):
        return self.rho(x)[2]

    def gradient_hessian(self, x, enabled=None, hessian=True):
        """g = sum rho' J^T r [3n] and the reweighted dense H = sum rho' J^T J [3n, 3n]."""
        on = self.mask(enabled)
        _, r, _ = self.residuals(x)
        w = self.weights(x)
        A, B = self.jacobians(x)
        JA = np.einsum("cij,cjk->cik", self.W, A)
        JB = np.einsum("cij,cjk->cik", self.W, B)
        g = np.zeros((self.n, 3))
        np.add.at(g, self.begin[on], (w[:, None] * np.einsum("cji,cj->ci", JA, r))[on])
        np.add.at(g, self.end[on], (w[:, None] * np.einsum("cji,cj->ci", JB, r))[on])
        if not hessian:
            return g.reshape(-1), None
        H = np.zeros((3 * self.n, 3 * self.n))
        for c in np.nonzero(on)[0]:
            ia, ib = 3 * self.begin[c], 3 * self.end[c]
            ja, jb = JA[c], JB[c]
            H[ia:ia + 3, ia:ia + 3] += w[c] * (ja.T @ ja)
            H[ib:ib + 3, ib:ib + 3] += w[c] * (jb.T @ jb)
            H[ia:ia + 3, ib:ib + 3] += w[c] * (ja.T @ jb)
            H[ib:ib + 3, ia:ia + 3] += w[c] * (jb.T @ ja)
        return g.reshape(-1), H

    def solve(self, enabled=None, max_iterations=2000, lam0=1e-9, up=10.0, down=0.1, patience=3):
        """Dense Levenberg-Marquardt on the reweighted system from the graph's poses until |g|_inf has
        not decreased for `patience` iterations.  The damping starts at lam0, is multiplied by `up`
        on a rejected and by `down` on an accepted step.  Returns dict(x [n, 3], gradient: the
        smallest |g|_inf met, start_gradient, cost, iterations)."""
        f = self.free(enabled)
        x = self.poses.copy()
        out = dict(x=x.copy(), gradient=self.gradient_norm(x, enabled), cost=self.cost(x, enabled), iterations=0)
        out["start_gradient"] = out["gradient"]
        if not f.any() or out["gradient"] == 0.0:
            return out
        lam, stalled, cost = lam0, 0, out["cost"]
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
                lam = max(lam * down, 1e-12)
                norm = self.gradient_norm(x, enabled)
                if norm < out["gradient"]:
                    out.update(x=x.copy(), gradient=norm, cost=cost)
                    stalled = 0
                else:
                    stalled += 1
            else:
                lam *= up
                stalled += 1
            out["iterations"] = it + 1
            if stalled >= patience:
                break
        return out

    def true_hessian(self, x, enabled=None, h=1e-6):
        """The Hessian of F over the unknowns that can move: central differences of g with the
        step h, symmetrised -- the reweighted term and the rho'' term together (and the residual's
        own second derivatives, which Gauss-Newton leaves out of both)."""
        f = np.nonzero(self.free(enabled))[0]
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        H = np.zeros((len(f), len(f)))
        for col, k in enumerate(f):
            hi, lo = x.copy(), x.copy()
            hi[k] += h
            lo[k] -= h
            gh, _ = self.gradient_hessian(hi.reshape(-1, 3), enabled, hessian=False)
            gl, _ = self.gradient_hessian(lo.reshape(-1, 3), enabled, hessian=False)
            H[:, col] = (gh[f] - gl[f]) / (hi[k] - lo[k])
        return 0.5 * (H + H.T)

    def true_inverse_norm(self, x, enabled=None):
        """|H_true(x)^-1|_inf (the largest absolute row sum)."""
        return float(np.max(np.sum(np.abs(np.linalg.inv(self.true_hessian(x, enabled))), axis=1)))
