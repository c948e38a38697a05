"""The pose graph's "chain" preconditioner (include/ndt2d_hip.h, "Pose graph") restated in numpy,
float64, on top of tests/posegraph_restatement.py's dense H: the band M of a Problem at
(x, mask, lambda) over ALL nodes in node order (a node that is not free is a segment of its own with
the identity as its block and zero couplings, which is how z = 0 there), its solve by a dense
Cholesky, a block cyclic reduction written from the contract's three sentences (not from the
header), and the solver's LM / PCG loop with either preconditioner, DESIGN.md 3.18's rules restated.
Nothing of the product is imported here."""
import numpy as np

DIAG_MIN, DIAG_MAX = 1e-6, 1e32


def damped(P, x, enabled=None, lam=1e-4):
    """(H + lambda D over all 3 n unknowns with rows and columns of nodes that are not free zeroed,
    g likewise, the free nodes [n], D = clamp(diag H) [3 n], zero where not free)."""
    g, H = P.gradient_hessian(x, enabled)
    f = P.free(enabled)
    H = np.where(f[:, None] & f[None, :], H, 0.0)
    D = np.where(f, np.clip(np.diag(H), DIAG_MIN, DIAG_MAX), 0.0)
    return H + lam * np.diag(D), np.where(f, g, 0.0), f[::3], D


def band(P, x, enabled=None, lam=1e-4):
    """M [3 n, 3 n]: the blocks (i, i) and (i, i +- 1) of H + lambda D between free nodes; the identity
    on the nodes that are not free.  The dense H's block (i, i + 1) is the sum over the enabled
    constraints joining i and i + 1, either way round, duplicates too."""
    A, _, free, _ = damped(P, x, enabled, lam)
    node = np.arange(3 * P.n) // 3
    M = np.where(np.abs(node[:, None] - node[None, :]) <= 1, A, 0.0)
    idle = np.repeat(~free, 3)
    M[idle, idle] = 1.0
    return M


def blocks(M):
    """(D [n, 3, 3], U [n, 3, 3]: the block (i, i + 1), the last zero) of a block-tridiagonal M."""
    n = M.shape[0] // 3
    D = np.array([M[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in range(n)])
    U = np.array([M[3 * i:3 * i + 3, 3 * i + 3:3 * i + 6] if i + 1 < n else np.zeros((3, 3)) for i in range(n)])
    return D, U


def dense_solve(M, r):
    """M^-1 r by a dense Cholesky (raises numpy.linalg.LinAlgError unless M is positive definite)."""
    L = np.linalg.cholesky(M)
    return np.linalg.solve(L.T, np.linalg.solve(L, r))


def cyclic_reduction(D, U, r):
    """z = M^-1 r [n, 3] by block cyclic reduction without pivoting, any n: at stride s the nodes
    whose index is an odd multiple of s are eliminated into their neighbours at +- s."""
    n = len(D)
    D, b = D.copy(), np.array(r, dtype=np.float64).reshape(n, 3).copy()
    C = U.copy()                                   # C[i]: the block (i, i + s) at the current stride
    levels, s = [], 1
    while s < n:
        odd = np.arange(s, n, 2 * s)
        inv = {int(i): np.linalg.inv(D[i]) for i in odd}
        levels.append((s, odd, inv, C.copy()))
        new = np.zeros_like(C)
        for j in range(0, n, 2 * s):
            lo, hi = j - s, j + s
            if lo >= 0:
                D[j] = D[j] - C[lo].T @ inv[lo] @ C[lo]
                b[j] = b[j] - C[lo].T @ (inv[lo] @ b[lo])
            if hi < n:
                D[j] = D[j] - C[j] @ inv[hi] @ C[j].T
                b[j] = b[j] - C[j] @ (inv[hi] @ b[hi])
                if hi + s < n:
                    new[j] = -C[j] @ inv[hi] @ C[hi]
        C, s = new, 2 * s
    z = np.zeros((n, 3))
    z[0] = np.linalg.solve(D[0], b[0])
    for s, odd, inv, C in reversed(levels):
        for i in odd:
            t = b[i] - C[i - s].T @ z[i - s]
            if i + s < n:
                t = t - C[i] @ z[i + s]
            z[i] = inv[int(i)] @ t
    return z


def pcg(A, b, apply_inverse, target, cap):
    """(delta, the residual left, iterations): the kernel's conjugate gradients from 0."""
    x, r = np.zeros_like(b), b.copy()
    z = apply_inverse(r)
    p, rz = z.copy(), float(r @ z)
    for k in range(cap):
        hp = A @ p
        php = float(p @ hp)
        if not (php > 0.0 and rz > 0.0):
            return x, r, k
        alpha = rz / php
        x = x + alpha * p
        r = r - alpha * hp
        if np.linalg.norm(r) <= target:
            return x, r, k + 1
        z = apply_inverse(r)
        rz_new = float(r @ z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, r, cap


def lm(P, preconditioner, gate, enabled=None, max_iterations=100):
    """The solver's loop with the gradient rule only.  Returns dict(x, iterations, cg_iterations,
    cg_per_iteration, converged)."""
    x = P.poses.copy()
    F = P.cost(x, enabled)
    lam, nu, g_start, total, per = 1e-4, 2.0, None, 0, []
    cap = min(3 * P.n + 16, 8192) if P.n < 8192 else 8192
    for it in range(max_iterations):
        A, g, free, Dg = damped(P, x, enabled, lam)
        if np.max(np.abs(g)) <= gate:
            return dict(x=x, iterations=it, cg_iterations=total, cg_per_iteration=per, converged=True)
        f3 = np.repeat(free, 3)
        if preconditioner == "jacobi":
            node = np.arange(3 * P.n) // 3
            J = np.where(node[:, None] == node[None, :], A, 0.0)
            J[~f3, ~f3] = 1.0
            Ji = np.linalg.inv(J)
            apply_inverse = lambda r: np.where(f3, Ji @ r, 0.0)   # noqa: E731
        else:
            D, U = blocks(band(P, x, enabled, lam))
            apply_inverse = lambda r: cyclic_reduction(D, U, r).reshape(-1)   # noqa: E731
        r0 = float(np.linalg.norm(g))
        g_start = r0 if g_start is None else g_start
        d, r, k = pcg(A, -g, apply_inverse, min(0.1, np.sqrt(r0 / g_start)) * r0, cap)
        total += k
        per.append(k)
        predicted = 0.5 * (lam * float(d @ (Dg * d)) + float(d @ r) - float(g @ d))
        trial = x + d.reshape(-1, 3)
        Ft = P.cost(trial, enabled)
        dF = F - Ft
        noise = abs(dF) <= 256.0 * 2.220446049250313e-16 * F
        gain = dF / predicted if predicted != 0.0 else 0.0
        if np.isfinite(Ft) and predicted > 0.0 and (noise or gain > 1e-3):
            x, F = trial, Ft
            t = 2.0 * gain - 1.0
            lam = min(max(lam * (1.0 / 3.0 if noise else max(1.0 / 3.0, 1.0 - t ** 3)), 1e-32), 1e32)
            nu = 2.0
        else:
            lam, nu = min(lam * nu, 1e32), 2.0 * nu
    return dict(x=x, iterations=max_iterations, cg_iterations=total, cg_per_iteration=per, converged=False)
