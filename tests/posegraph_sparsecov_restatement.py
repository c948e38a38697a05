"""The sparse covariance (include/ndt2d_hip.h, "Sparse covariance") restated in numpy, float64, by an
algorithm that is neither the device's nor the dense inverse: no 3n x 3n matrix, no cyclic reduction.
A = H_FF + damping clamp(diag H_FF) is kept as its 3 x 3 blocks (a node not in F: the identity, no
coupling).  The separators are the ends of the graph's closure edges (|begin - end| != 1), whatever the
mask; the interior nodes between two separators are a segment, a block-tridiagonal system.  Per
segment the sequential two-sided recurrence gives the diagonal blocks of its inverse G --
    F_0 = D_0, F_k = D_k - C_{k-1}^T F_{k-1}^-1 C_{k-1};   B_last = D_last, B_k = D_k - C_k B_{k+1}^-1 C_k^T;
    G_kk = (F_k + B_k - D_k)^-1
-- and a block Thomas solve gives Z = A_ii^-1 A_is (the columns of the segment's first and last node)
and, where a pair asks for it, a block column G_.,b.  Then the dense S = A_ss - A_si Z, numpy's inverse
of it, and
    Sigma_ss = S^-1,  Sigma_is = -Z Sigma_ss,  Sigma_ii = G + Z Sigma_ss Z^T.
Written from the contract; nothing of the product is imported here.  It is the yardstick where the
dense inverse is too big; tests/test_posegraph_sparsecov_restatement.py holds it to the dense inverse
where that is not.

Also here: the designed layouts the sparse solve's device test has (the same CH.chain arguments)."""
import numpy as np

import posegraph_chain_cases as CH

DIAG_MIN, DIAG_MAX = 1e-6, 1e32


def _spread(s):
    """Closures that make exactly s separators on a chain of 70: the nodes 1, 3, 5, ... joined in a row."""
    nodes = [2 * k + 1 for k in range(s)]
    return [(nodes[k], nodes[k + 1]) for k in range(s - 1)]


# name: (the builder, the separators it has)
LAYOUTS = {
    "no_closure": (lambda: CH.chain(33, 70), 0),
    "two_poses": (lambda: CH.chain(2, 71, sigma=(0.01, 0.01, 0.005)), 0),
    "ends": (lambda: CH.chain(40, 72, closures=[(0, 39)]), 2),
    "adjacent_separators": (lambda: CH.chain(30, 73, closures=[(5, 20), (6, 21)]), 4),
    "segments_of_1_and_2": (lambda: CH.chain(30, 74, closures=[(3, 5), (5, 8), (8, 20)]), 4),
    "separator_next_to_fixed": (lambda: CH.chain(30, 75, closures=[(1, 15)], fixed=0), 2),
    "fixed_is_a_separator": (lambda: CH.chain(30, 76, closures=[(0, 15), (7, 22)], fixed=15), 4),
    "fixed_2_inside_a_segment": (lambda: CH.chain(30, 77, closures=[(0, 20)], fixed=2), 2),
    "every_node": (lambda: CH.chain(12, 78, closures=[(i, i + 2) for i in range(10)]), 12),
    "s_15": (lambda: CH.chain(70, 79, closures=_spread(15)), 15),
    "s_16": (lambda: CH.chain(70, 80, closures=_spread(16)), 16),
    "s_17": (lambda: CH.chain(70, 81, closures=_spread(17)), 17),
    "s_32": (lambda: CH.chain(70, 82, closures=_spread(32)), 32),
    "s_33": (lambda: CH.chain(70, 83, closures=_spread(33)), 33),
}


def separators(P):
    """The nodes that are an end of a closure edge of the graph, ascending."""
    far = np.abs(P.begin - P.end) != 1
    return np.unique(np.concatenate([P.begin[far], P.end[far]])).astype(np.int64)


class Sparse:
    """Sigma's blocks of Problem P (posegraph_restatement's, or the robust one's) at x under a mask."""

    def __init__(self, P, x, enabled=None, damping=0.0):
        x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
        n = self.n = P.n
        on = P.mask(enabled)
        self.free = P.free(enabled)[::3]
        rho = P.weights(x) if hasattr(P, "weights") else np.ones(P.m)
        A, B = P.jacobians(x)
        JA = np.einsum("cij,cjk->cik", P.W, A)
        JB = np.einsum("cij,cjk->cik", P.W, B)
        D = np.zeros((n, 3, 3))
        self.up = np.zeros((max(n - 1, 0), 3, 3))        # the block (i, i + 1)
        self.far = {}                                    # (i, j), i < j: the block of a closure edge
        for c in np.nonzero(on)[0]:
            a, b = int(P.begin[c]), int(P.end[c])
            D[a] += rho[c] * (JA[c].T @ JA[c])
            D[b] += rho[c] * (JB[c].T @ JB[c])
            if not (self.free[a] and self.free[b]):
                continue
            lo, hi, X = (a, b, rho[c] * (JA[c].T @ JB[c])) if a < b else (b, a, rho[c] * (JB[c].T @ JA[c]))
            if hi == lo + 1:
                self.up[lo] += X
            else:
                self.far[(lo, hi)] = self.far.get((lo, hi), np.zeros((3, 3))) + X
        for i in range(n):
            if self.free[i]:
                D[i] += damping * np.diag(np.clip(np.diag(D[i]), DIAG_MIN, DIAG_MAX))
            else:
                D[i] = np.eye(3)
        self.D = D
        self.sep = separators(P)
        self.s = len(self.sep)
        self.sep_index = {int(v): k for k, v in enumerate(self.sep)}
        is_sep = np.zeros(n, dtype=bool)
        is_sep[self.sep] = True
        # the segments: runs of interior nodes [k0, k1]
        self.segments, self.segment_of = [], np.full(n, -1, dtype=np.int64)
        i = 0
        while i < n:
            if is_sep[i]:
                i += 1
                continue
            k0 = i
            while i < n and not is_sep[i]:
                i += 1
            self.segment_of[k0:i] = len(self.segments)
            self.segments.append((k0, i - 1))
        self.G = np.zeros((n, 3, 3))                     # G_kk of the interior nodes
        self.Zl = np.zeros((n, 3, 3))
        self.Zr = np.zeros((n, 3, 3))
        S = np.zeros((3 * self.s, 3 * self.s))
        for k, v in enumerate(self.sep):
            S[3 * k:3 * k + 3, 3 * k:3 * k + 3] = D[v]
            if k + 1 < self.s and self.sep[k + 1] == v + 1:
                S[3 * k:3 * k + 3, 3 * k + 3:3 * k + 6] = self.up[v]
                S[3 * k + 3:3 * k + 6, 3 * k:3 * k + 3] = self.up[v].T
        for (lo, hi), X in self.far.items():
            a, b = self.sep_index[lo], self.sep_index[hi]
            S[3 * a:3 * a + 3, 3 * b:3 * b + 3] += X
            S[3 * b:3 * b + 3, 3 * a:3 * a + 3] += X.T
        self._forward = {}
        for seg, (k0, k1) in enumerate(self.segments):
            self._segment(seg, k0, k1, S)
        self.S = S
        self.sigma_ss = np.linalg.inv(S) if self.s else np.zeros((0, 0))

    def _thomas(self, seg, rhs):
        """The segment's block-tridiagonal solve: rhs [L, 3, k] -> [L, 3, k], with the forward pivots kept."""
        k0, k1 = self.segments[seg]
        F = self._forward[seg]
        L = k1 - k0 + 1
        y = np.array(rhs, dtype=np.float64)
        for k in range(1, L):
            y[k] = y[k] - self.up[k0 + k - 1].T @ np.linalg.solve(F[k - 1], y[k - 1])
        out = np.zeros_like(y)
        out[L - 1] = np.linalg.solve(F[L - 1], y[L - 1])
        for k in range(L - 2, -1, -1):
            out[k] = np.linalg.solve(F[k], y[k] - self.up[k0 + k] @ out[k + 1])
        return out

    def _segment(self, seg, k0, k1, S):
        L = k1 - k0 + 1
        F, B = np.zeros((L, 3, 3)), np.zeros((L, 3, 3))
        F[0] = self.D[k0]
        for k in range(1, L):
            C = self.up[k0 + k - 1]
            F[k] = self.D[k0 + k] - C.T @ np.linalg.solve(F[k - 1], C)
        B[L - 1] = self.D[k1]
        for k in range(L - 2, -1, -1):
            C = self.up[k0 + k]
            B[k] = self.D[k0 + k] - C @ np.linalg.solve(B[k + 1], C.T)
        self._forward[seg] = F
        for k in range(L):
            self.G[k0 + k] = np.linalg.inv(F[k] + B[k] - self.D[k0 + k])
        # Z: the couplings of the segment's ends to the separators before and after it
        rhs = np.zeros((L, 3, 6))
        u = self.sep_index.get(k0 - 1)
        w = self.sep_index.get(k1 + 1)
        if u is not None:
            rhs[0, :, :3] = self.up[k0 - 1].T            # A(k0, k0 - 1)
        if w is not None:
            rhs[L - 1, :, 3:] = self.up[k1]              # A(k1, k1 + 1)
        Z = self._thomas(seg, rhs)
        self.Zl[k0:k1 + 1] = Z[:, :, :3]
        self.Zr[k0:k1 + 1] = Z[:, :, 3:]
        if u is not None:
            Cl = self.up[k0 - 1].T
            S[3 * u:3 * u + 3, 3 * u:3 * u + 3] -= Cl.T @ Z[0, :, :3]
            if w is not None:
                S[3 * u:3 * u + 3, 3 * w:3 * w + 3] -= Cl.T @ Z[0, :, 3:]
        if w is not None:
            Cr = self.up[k1]
            S[3 * w:3 * w + 3, 3 * w:3 * w + 3] -= Cr.T @ Z[L - 1, :, 3:]
            if u is not None:
                S[3 * w:3 * w + 3, 3 * u:3 * u + 3] -= Cr.T @ Z[L - 1, :, :3]

    def _reach(self, node):
        """[(separator index, coefficient)]: what a node reaches Sigma_ss through."""
        node = int(node)
        if node in self.sep_index:
            return [(self.sep_index[node], np.eye(3))]
        k0, k1 = self.segments[self.segment_of[node]]
        out = []
        if k0 - 1 in self.sep_index:
            out.append((self.sep_index[k0 - 1], -self.Zl[node]))
        if k1 + 1 in self.sep_index:
            out.append((self.sep_index[k1 + 1], -self.Zr[node]))
        return out

    def _ss(self, a, b):
        return self.sigma_ss[3 * a:3 * a + 3, 3 * b:3 * b + 3]

    def block(self, a, b, columns=None):
        """Sigma's block (a, b): the rows of node a in the columns of node b; zero where either is not in F."""
        a, b = int(a), int(b)
        if not (self.free[a] and self.free[b]):
            return np.zeros((3, 3))
        out = np.zeros((3, 3))
        for u, Ca in self._reach(a):
            for w, Cb in self._reach(b):
                out += Ca @ self._ss(u, w) @ Cb.T
        seg = self.segment_of[a]
        if seg >= 0 and seg == self.segment_of[b]:
            if a == b:
                out += self.G[a]
            else:
                k0, k1 = self.segments[seg]
                if columns is None or b not in columns:
                    rhs = np.zeros((k1 - k0 + 1, 3, 3))
                    rhs[b - k0] = np.eye(3)
                    column = self._thomas(seg, rhs)
                    if columns is not None:
                        columns[b] = column
                else:
                    column = columns[b]
                out += column[a - k0]
        return out

    def diagonal(self):
        """[n, 3, 3]: every node's block."""
        return np.array([self.block(i, i) for i in range(self.n)])

    def blocks(self, pairs):
        """[P, 3, 3] for pairs [P, 2]."""
        columns = {}
        return np.array([self.block(a, b, columns) for a, b in np.asarray(pairs).reshape(-1, 2)]).reshape(-1, 3, 3)

    def whole(self):
        """Sigma [3n, 3n], zeros outside F (small graphs only)."""
        n = self.n
        columns = {}
        full = np.zeros((n, n, 3, 3))
        for a in range(n):
            for b in range(a + 1):
                full[a, b] = self.block(a, b, columns) if a != b else self.block(a, a)
                if a != b:
                    full[b, a] = full[a, b].T
        return full.transpose(0, 2, 1, 3).reshape(3 * n, 3 * n)

    def column(self, b):
        """Sigma[:, b] as [n, 3, 3] blocks."""
        columns = {}
        return np.array([self.block(a, b, columns) for a in range(self.n)])

    def product(self, X, absolute=False):
        """A X (or |A| |X|) for X [n, 3, k] by A's blocks, without a dense matrix."""
        f = np.abs if absolute else (lambda v: v)
        X = f(np.asarray(X, dtype=np.float64))
        out = np.einsum("nij,njk->nik", f(self.D), X)
        if self.n > 1:
            out[:-1] += np.einsum("nij,njk->nik", f(self.up), X[1:])
            out[1:] += np.einsum("nji,njk->nik", f(self.up), X[:-1])
        for (lo, hi), B in self.far.items():
            out[lo] += f(B) @ X[hi]
            out[hi] += f(B).T @ X[lo]
        return out
