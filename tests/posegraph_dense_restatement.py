"""The dense covariance (include/ndt2d_hip.h, "Dense covariance") restated in numpy, float64, on top
of tests/posegraph_marginals_restatement.py's System: A = H_FF + damping clamp(diag H_FF) placed into
the 3n unknowns (a node not in F and the padding to whole panels keep the identity's rows and
columns), the blocked right-looking Cholesky without pivoting -- the diagonal block unblocked, with
the pivot ratio and the failure rule, the panel below by substitution, the trailing update of the
lower blocks -- T = L^-1 by the same panels on the identity, and the blocks of Sigma = T^T T.
Written from the contract; nothing of the product is imported here.  The order of the sums inside a
panel is numpy's, not the device's: this restates the algorithm and its error, not its bits."""
import numpy as np

BLOCK = 48
OK, NOT_POSITIVE_DEFINITE = 0, 1
EPS = np.finfo(np.float64).eps


def embed(S):
    """System S's A in the 3n unknowns, padded to whole panels: (matrix [ld, ld], d)."""
    d = 3 * S.n
    ld = -(-d // BLOCK) * BLOCK
    M = np.eye(ld)
    M[np.ix_(S.index, S.index)] = S.A
    return M, d


def factor_block(M, j0, diag, d, record):
    """The diagonal block at j0, unblocked and right-looking, in place (lower triangle)."""
    B = M[j0:j0 + BLOCK, j0:j0 + BLOCK]
    for j in range(BLOCK):
        pivot = B[j, j]
        if j0 + j < d:
            if record["status"] == OK:
                ratio = pivot / diag[j0 + j]
                if not np.isnan(ratio):
                    record["ratio"] = min(record["ratio"], ratio)
            if not (pivot > 0.0) or not np.isfinite(pivot):
                if record["status"] == OK:
                    record["first"] = j0 + j
                record["status"] = NOT_POSITIVE_DEFINITE
        with np.errstate(invalid="ignore", divide="ignore"):
            root = np.sqrt(pivot)
            B[j, j] = root
            B[j + 1:, j] = B[j + 1:, j] / root
            B[j + 1:, j + 1:] -= np.outer(B[j + 1:, j], B[j + 1:, j])


def substitute_rows(X, L):
    """X L^-T by substitution along each row, the rows in parallel."""
    for c in range(BLOCK):
        X[:, c] = (X[:, c] - X[:, :c] @ L[c, :c]) / L[c, c]


def substitute_columns(X, L):
    """L^-1 X by substitution down each column, the columns in parallel."""
    for r in range(BLOCK):
        X[r, :] = (X[r, :] - L[r, :r] @ X[:r, :]) / L[r, r]


def cholesky_inverse(M, d):
    """(T = L^-1 lower triangular, record) of the padded M by panels of BLOCK; M is overwritten by L."""
    ld = len(M)
    diag = np.diag(M).copy()
    record = dict(status=OK, first=-1, ratio=1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for j0 in range(0, ld, BLOCK):
            j1 = j0 + BLOCK
            factor_block(M, j0, diag, d, record)
            L = np.tril(M[j0:j1, j0:j1])
            if j1 < ld:
                substitute_rows(M[j1:, j0:j1], L)
                P = M[j1:, j0:j1]
                M[j1:, j1:] -= P @ P.T                    # (the device: the lower blocks only; the upper ones are never read)
        T = np.eye(ld)
        for j0 in range(0, ld, BLOCK):
            j1 = j0 + BLOCK
            substitute_columns(T[j0:j1, :j1], np.tril(M[j0:j1, j0:j1]))
            if j1 < ld:
                T[j1:, :j1] -= M[j1:, j0:j1] @ T[j0:j1, :j1]
    return T, record


def solve(S):
    """dict(sigma [len(F), len(F)] over the unknowns of F, status, first, ratio) of System S."""
    M, d = embed(S)
    T, record = cholesky_inverse(M, d)
    T = np.tril(T[:d, :d])
    if record["status"] != OK:
        sigma = np.zeros((len(S.index), len(S.index)))
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            sigma = (T.T @ T)[np.ix_(S.index, S.index)]
    return dict(sigma=sigma, status=record["status"], first=record["first"], ratio=record["ratio"])


def floor(S):
    """What |A Sigma - I|_max is measured in: the dense inverse's own defect, or, where that is below
    it (a fluke of a tiny system), the rounding of one product, eps max(|A| |Sigma_ref|)."""
    return max(S.defect(), EPS * float(np.max(np.abs(S.A) @ np.abs(S.inverse()))))


def defect_ratio(S, sigma):
    """|A sigma - I|_max / floor(S)."""
    if len(S.A) == 0:
        return 0.0
    return float(np.max(np.abs(S.A @ sigma - np.eye(len(S.A))))) / floor(S)


def singular_limit(d):
    """The pivot ratio a singular positive semidefinite matrix's last pivots stay under: Cholesky's
    backward error is about (d + 1) eps of the diagonal; 100 x that."""
    return 100.0 * (d + 1) * EPS
