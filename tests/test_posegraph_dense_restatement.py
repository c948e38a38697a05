"""tests/posegraph_dense_restatement.py -- the blocked Cholesky, T = L^-1 and Sigma = T^T T in numpy
-- against the dense inverse of tests/posegraph_marginals_restatement.py's System, on the designed
graphs at the restatement's own solutions, each at damping 0 and 1e-4.

What is measured is the DEFECT RATIO |A Sigma - I|_max / max(System.defect(), eps max(|A| |Sigma_ref|)):
how the blocked algorithm's residual compares with numpy's own inverse's, the floor of one product's
rounding under it (on `pair` numpy's defect is 2e-17, a fluke of a 3 x 3 system).  RATIOS holds what
was measured; the device's gate (tests/test_gpu_posegraph_dense.py) is 100 x the same floor, the
project's margin over a restatement's own figure."""
import numpy as np
import pytest

import posegraph_cases as PC
import posegraph_dense_restatement as DR
import posegraph_marginals_cases as MC
import posegraph_marginals_restatement as MR
import posegraph_restatement as R

DAMPINGS = (0.0, 1e-4)
# (case, damping): (the defect ratio, the pivot ratio) as measured
RATIOS = {
    ("pair", 0.0): (0.94, 9.8e-01), ("pair", 1e-4): (1.41, 9.8e-01),
    ("square", 0.0): (0.85, 6.0e-01), ("square", 1e-4): (0.90, 6.0e-01),
    ("square_information", 0.0): (0.56, 6.0e-01), ("square_information", 1e-4): (0.56, 6.0e-01),
    ("square_fixed_2", 0.0): (0.99, 6.0e-01), ("square_fixed_2", 1e-4): (1.27, 6.0e-01),
    ("line", 0.0): (0.89, 5.0e-01), ("line", 1e-4): (1.07, 5.0e-01),
    ("wrap", 0.0): (1.30, 2.2e-01), ("wrap", 1e-4): (1.15, 2.2e-01),
    ("hub", 0.0): (3.88, 5.7e-01), ("hub", 1e-4): (3.39, 5.7e-01),
    ("n3", 0.0): (0.75, 7.2e-01), ("n3", 1e-4): (0.57, 7.2e-01),
    ("n5", 0.0): (0.99, 5.2e-01), ("n5", 1e-4): (0.63, 5.2e-01),
    ("isolated", 0.0): (1.39, 1.4e-01), ("isolated", 1e-4): (1.36, 1.4e-01),
    ("loop_1025", 0.0): (4.30, 3.3e-01), ("loop_1025", 1e-4): (5.22, 3.4e-01),
    ("chain_1025", 0.0): (11.22, 1.7e-05), ("chain_1025", 1e-4): (1.87, 7.6e-03),
}
CASES = sorted({k[0] for k in RATIOS}, key=lambda name: MC.size(name))


@pytest.mark.parametrize("name", CASES)
def test_the_blocked_algorithm_against_the_dense_inverse(name):
    for damping in DAMPINGS:
        S = MC.system(name, damping)
        got = DR.solve(S)
        ratio = DR.defect_ratio(S, got["sigma"])
        err = float(np.max(np.abs(got["sigma"] - S.inverse())))
        # Sigma - Sigma_ref = A^-1 (A Sigma - A Sigma_ref): the two residuals, each measured to within one product's rounding
        rounding = DR.EPS * float(np.max(np.abs(S.A) @ np.abs(S.inverse())))
        bound = S.inverse_norm() * (ratio * DR.floor(S) + S.defect() + 2.0 * rounding)
        want_ratio, want_pivot = RATIOS[(name, damping)]
        print("%s, damping %g: defect ratio %.2f (recorded %.2f), |Sigma - Sigma_ref| %.1e (bound %.1e), pivot ratio %.2e"
              % (name, damping, ratio, want_ratio, err, bound, got["ratio"]))
        assert got["status"] == DR.OK and got["first"] == -1
        # the recorded figure with a factor of two for another BLAS's order of sums; 100 x is the device's gate
        assert ratio <= 2.0 * want_ratio and 2.0 * want_ratio < 100.0
        assert err <= bound
        assert 0.5 * want_pivot <= got["ratio"] <= min(1.0, 2.0 * want_pivot)
        # a well-posed system is far above what a singular one's pivots stay under
        assert got["ratio"] > 1e3 * DR.singular_limit(3 * S.n)
        assert np.array_equal(got["sigma"], got["sigma"].T)


def test_line_has_its_closed_form():
    S = MC.system("line")
    sigma = DR.solve(S)["sigma"]
    n = 20
    for i in range(1, n + 1):
        want = i * (n + 1 - i) / (100.0 * (n + 1))
        assert abs(sigma[3 * (i - 1), 3 * (i - 1)] - want) <= 1e-12 * want + S.inverse_norm() * 100.0 * DR.floor(S)


def test_a_singular_system_fails_or_has_a_pivot_at_rounding_level():
    """The floating squares at damping 0: the second square's H is singular (three null directions).
    NOT_POSITIVE_DEFINITE with the first failing unknown in the floating square, or a pivot ratio
    under 100 (d + 1) eps; with damping 1e-4 the dense inverse."""
    P, x = PC.problem("floating"), PC.solution("floating")["x"]
    S = MR.System(P, x)
    got = DR.solve(S)
    print("floating, damping 0: status %d, first %d, pivot ratio %.2e (limit %.1e)" % (got["status"], got["first"], got["ratio"], DR.singular_limit(24)))
    assert got["ratio"] <= DR.singular_limit(3 * P.n)
    if got["status"] == DR.NOT_POSITIVE_DEFINITE:
        assert 12 <= got["first"] < 24 and np.all(got["sigma"] == 0.0)
    damped = MR.System(P, x, damping=1e-4)
    got = DR.solve(damped)
    assert got["status"] == DR.OK and DR.defect_ratio(damped, got["sigma"]) <= 100.0
    joined = MR.System(R.Problem(x[:4], P.begin[:4], P.end[:4], P.transform[:4], P.information[:4]), x[:4])
    assert DR.solve(joined)["status"] == DR.OK


def test_the_failure_rule_on_an_indefinite_matrix():
    M = np.eye(96)
    M[50, 50] = -2.0
    T, record = DR.cholesky_inverse(M.copy(), 96)
    assert record == dict(status=DR.NOT_POSITIVE_DEFINITE, first=50, ratio=1.0) or (record["status"], record["first"]) == (1, 50)
