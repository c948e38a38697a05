"""tests/posegraph_sparsecov_restatement.py against the dense inverse (tests/posegraph_marginals_restatement.py's
System) on the small graphs the device test uses: the marginals' SMALL cases and the layout edges of the
sparse solve.  The measure is the dense test's: |A Sigma - I|_max in units of the dense inverse's own floor
(tests/posegraph_dense_restatement.py's floor), and max|Sigma - Sigma_ref| <= |A^-1|_inf (gate + defect).

The restatement's own ratio to the floor, measured over these cases at damping 0 and 1e-4: at most 68.08 x
("s_16" at damping 0; RESTATEMENT_RATIO; held below to the project's margin of 100 x).  Its sequential
recurrences carry a segment's rounding from node to node, which the dense LAPACK inverse does not.  That
leaves less than a factor 4 under 100, so the device test's gate is GATE = 4 x 68.08 = 272.32 x the floor
(tests/test_gpu_posegraph_sparsecov.py)."""
import numpy as np
import pytest

import posegraph_dense_restatement as DR
import posegraph_marginals_cases as MC
import posegraph_marginals_restatement as MR
import posegraph_restatement as R
import posegraph_sparsecov_restatement as SR

RESTATEMENT_RATIO = 68.08   # the worst |A Sigma - I| / floor measured over the cases below (printed by the test)
GATE = max(100.0, 4.0 * RESTATEMENT_RATIO)   # the device test's gate, in units of the floor
DAMPINGS = (0.0, 1e-4)


def _case(name):
    if name in SR.LAYOUTS:
        P = R.Problem(**SR.LAYOUTS[name][0]())
        return P, P.poses
    return MC.case(name)


@pytest.mark.parametrize("name", MC.SMALL + tuple(SR.LAYOUTS))
def test_the_sparse_restatement_against_the_dense_inverse(name):
    P, x = _case(name)
    if name in SR.LAYOUTS:
        assert len(SR.separators(P)) == SR.LAYOUTS[name][1]
    for damping in DAMPINGS:
        S = MR.System(P, x, damping=damping)
        sparse = SR.Sparse(P, x, damping=damping)
        sigma = sparse.whole()
        held = np.ones(3 * P.n, dtype=bool)
        held[S.index] = False
        assert np.all(sigma[held] == 0.0) and np.all(sigma[:, held] == 0.0)
        inside = sigma[np.ix_(S.index, S.index)]
        ratio = DR.defect_ratio(S, inside)
        err = float(np.max(np.abs(inside - S.inverse()))) if len(S.A) else 0.0
        bound = S.inverse_norm() * (100.0 * DR.floor(S) + S.defect()) if len(S.A) else 0.0
        print("%s, damping %g: |A Sigma - I| = %.2f x the floor, |Sigma - Sigma_ref| %.2e (bound %.2e)" % (name, damping, ratio, err, bound))
        assert ratio <= 100.0, (name, damping, ratio)
        assert err <= bound, (name, damping, err, bound)
        diagonal = sparse.diagonal()
        n = P.n
        assert np.array_equal(diagonal, sigma.reshape(n, 3, n, 3).transpose(0, 2, 1, 3)[np.arange(n), np.arange(n)])
        pairs = [(0, n - 1), (n - 1, 0), (n // 2, n // 2), (n // 3, n // 2)]
        blocks = sparse.blocks(pairs)
        for q, (a, b) in enumerate(pairs):
            assert np.allclose(blocks[q], sigma[3 * a:3 * a + 3, 3 * b:3 * b + 3], rtol=0.0, atol=bound + 1e-300)


def test_masks_and_a_loss_enter_the_blocks():
    """A closure and an odometry edge switched off, and Huber on the closures, against the dense system of the
    same mask and weights."""
    import posegraph_cases as PC
    import posegraph_robust_cases as RC
    import posegraph_robust_restatement as RR
    P, x = MC.case("wrap")
    closures = np.nonzero(np.abs(P.begin - P.end) != 1)[0]
    mask = np.ones(P.m, dtype=np.uint8)
    mask[closures[1]] = 0
    mask[int(np.nonzero((P.begin == 5) & (P.end == 6))[0][0])] = 0
    S = MR.System(P, x, enabled=mask, damping=1e-4)
    inside = SR.Sparse(P, x, enabled=mask, damping=1e-4).whole()[np.ix_(S.index, S.index)]
    assert DR.defect_ratio(S, inside) <= 100.0
    g = RC.graph("loop40")[0]
    Pr = RR.Problem(loss="huber", scale=RC.SCALE, robust=RC.closures("loop40"), **g)
    assert np.min(Pr.weights(Pr.poses)) < 0.5
    S = MR.System(Pr, Pr.poses)
    inside = SR.Sparse(Pr, Pr.poses).whole()[np.ix_(S.index, S.index)]
    assert DR.defect_ratio(S, inside) <= 100.0
    assert PC is not None
