"""The direct solve's contract (include/ndt2d_hip.h, "Direct solve") restated in numpy, float64, on
tests/posegraph_restatement.py's Problem (or posegraph_robust_restatement.py's, whose cost and
reweighted H carry the loss): the solver's Levenberg-Marquardt rules with an exact linear step,
(H_FF + lambda clamp(diag H_FF)) delta = -g through a dense Cholesky (np.linalg.cholesky).  Written
from the contract, not from the kernels: no panels, no reduction trees.  The yardstick of
tests/test_gpu_posegraph_direct.py beside Problem.solve; nothing of the product is imported here."""
import math

import numpy as np

CONVERGED_GRADIENT, CONVERGED_COST, CONVERGED_STEP, MAX_ITERATIONS, FAILED = range(5)
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-4, 1e-32, 1e32
DIAG_MIN, DIAG_MAX = 1e-6, 1e32
MIN_GAIN = 1e-3
NOISE = 256.0 * 2.220446049250313e-16


def solve(P, enabled=None, max_iterations=100, gradient_tolerance=1e-10, function_tolerance=1e-6, parameter_tolerance=1e-8):
    """Returns dict(x [n, 3], status, iterations, rejected, not_positive_definite, initial_cost, cost,
    gradient: |g|_inf over the unknowns that can move at x)."""
    f = P.free(enabled)
    x = P.poses.copy()
    F = P.cost(x, enabled)
    out = dict(x=x, status=MAX_ITERATIONS, iterations=0, rejected=0, not_positive_definite=0, initial_cost=F, cost=F, gradient=0.0)
    if not math.isfinite(F):
        out["status"] = FAILED
        return out

    def linearize(at):
        g, H = P.gradient_hessian(at, enabled)
        return g[f], H[np.ix_(f, f)]

    g, H = linearize(x)
    out["gradient"] = float(np.max(np.abs(g))) if f.any() else 0.0
    if out["gradient"] <= gradient_tolerance:
        out["status"] = CONVERGED_GRADIENT
        return out
    lam, nu = LAMBDA0, 2.0
    while out["status"] == MAX_ITERATIONS and out["iterations"] < max_iterations:
        out["iterations"] += 1
        D = np.clip(np.diag(H), DIAG_MIN, DIAG_MAX)
        A = H + np.diag(lam * D)
        try:
            low = np.linalg.cholesky(A)
            failed = not np.all(np.isfinite(low))
        except np.linalg.LinAlgError:
            failed = True
        if failed:
            out["not_positive_definite"] += 1
            out["rejected"] += 1
            lam, nu = min(lam * nu, LAMBDA_MAX), nu * 2.0
            continue
        delta = np.linalg.solve(low.T, np.linalg.solve(low, -g))
        predicted = 0.5 * (lam * float(delta @ (D * delta)) - float(g @ delta))
        step, x_norm = float(np.linalg.norm(delta)), float(np.linalg.norm(x))
        if parameter_tolerance > 0.0 and step <= parameter_tolerance * (x_norm + parameter_tolerance):
            out["status"] = CONVERGED_STEP
            break
        whole = np.zeros(3 * P.n)
        whole[f] = delta
        trial = x + whole.reshape(-1, 3)
        Ft = P.cost(trial, enabled)
        dF = F - Ft
        noise = abs(dF) <= NOISE * F
        gain = dF / predicted if predicted != 0.0 else math.inf
        if math.isfinite(Ft) and predicted > 0.0 and (noise or gain > MIN_GAIN):
            x = trial
            g, H = linearize(x)
            lam *= 1.0 / 3.0 if noise else max(1.0 / 3.0, 1.0 - (2.0 * gain - 1.0) ** 3)
            lam = min(max(lam, LAMBDA_MIN), LAMBDA_MAX)
            nu = 2.0
            before, F = F, Ft
            out.update(x=x, cost=F, gradient=float(np.max(np.abs(g))))
            if out["gradient"] <= gradient_tolerance:
                out["status"] = CONVERGED_GRADIENT
            elif function_tolerance > 0.0 and abs(dF) <= function_tolerance * before:
                out["status"] = CONVERGED_COST
        else:
            out["rejected"] += 1
            lam, nu = min(lam * nu, LAMBDA_MAX), nu * 2.0
    return out
