"""The yardstick itself: tests/posegraph_restatement.py against central differences, a known
answer and the weighting's two costs, and every designed case's gate (tests/posegraph_cases.py)
against the floor the restatement bottoms out at.  No GPU."""
import numpy as np
import pytest

import posegraph_cases as PC
import posegraph_restatement as R


def test_normalize_is_the_formula():
    assert float(R.normalize(-R.PI)) == -R.PI and float(R.normalize(R.PI)) == -R.PI and float(R.normalize(0.0)) == 0.0
    v = np.array([3.0 * R.PI, -3.0 * R.PI, 1e6, 6.5, -2.9])
    got = R.normalize(v)
    assert np.array_equal(got, v - (2.0 * R.PI) * np.floor((v + R.PI) / (2.0 * R.PI)))
    assert np.all(np.abs(np.sin(got) - np.sin(v)) < 1e-9) and np.all((got >= -R.PI - 2.0 ** -50) & (got < R.PI))


@pytest.mark.parametrize("name", ["pair", "square", "wrap", "hub"])
def test_jacobians_against_central_differences(name):
    """Tolerance 1e-7 relative: the finite-difference error at h = 1e-6 (truncation h^2 f''' / 6 and
    rounding eps |e| / h are both far below it for residuals of a few units)."""
    P = PC.problem(name)
    x = P.poses + np.random.default_rng(3).normal(0.0, 0.01, P.poses.shape)
    A, B = P.jacobians(x)
    h = 1e-6
    for c in range(min(P.m, 40)):
        for which, node, J in (("a", P.begin[c], A[c]), ("b", P.end[c], B[c])):
            for j in range(3):
                hi, lo = x.copy(), x.copy()
                hi[node, j] += h
                lo[node, j] -= h
                numeric = (P.errors(hi)[c] - P.errors(lo)[c]) / (2.0 * h)
                assert np.all(np.abs(numeric - J[:, j]) <= 1e-7 * np.maximum(1.0, np.abs(J[:, j]))), (c, which, j)
    # the gradient is J^T r of those blocks: against differences of the cost
    g, _ = P.gradient_hessian(x, hessian=False)
    for i in (0, P.n // 2, P.n - 1):
        for j in range(3):
            hi, lo = x.copy(), x.copy()
            hi[i, j] += h
            lo[i, j] -= h
            numeric = (P.cost(hi) - P.cost(lo)) / (2.0 * h)
            assert abs(numeric - g[3 * i + j]) <= 1e-6 * max(1.0, abs(g[3 * i + j])), (i, j)


def test_the_known_answer_on_the_line():
    """n odometry constraints (1, 0, 0), one closure 0 -> n saying (n - delta, 0, 0), one diagonal
    information: x_i = i (1 - delta / (n + 1)), y = theta = 0."""
    P, ref = PC.problem("line"), PC.solution("line")
    want = PC.line_answer()
    assert ref["gradient"] <= PC.gate("line") / 10.0
    # first order: |x - x*| <= |H^-1| |g|, twice that for the remainder
    assert np.max(np.abs(ref["x"] - want)) <= 2.0 * P.inverse_norm(want) * PC.gate("line")
    assert P.gradient_norm(want) <= PC.gate("line")


def test_the_weighting_quirk():
    """With a non-diagonal information "reference" (W = L) costs e^T L^T L e and "information"
    (W = L^T) costs e^T information e: different numbers."""
    g = PC.square()
    ref, inf = R.Problem(weighting="reference", **g), R.Problem(weighting="information", **g)
    e = ref.errors(ref.poses)
    L = R.cholesky_lower(PC.INFO_FULL)
    assert np.allclose(L @ L.T, PC.INFO_FULL, rtol=1e-14, atol=0) and np.array_equal(np.triu(L, 1), np.zeros((3, 3)))
    want_ref = 0.5 * sum(float(v @ L.T @ L @ v) for v in e)
    want_inf = 0.5 * sum(float(v @ PC.INFO_FULL @ v) for v in e)
    assert abs(ref.cost(ref.poses) - want_ref) <= 1e-12 * want_ref
    assert abs(inf.cost(inf.poses) - want_inf) <= 1e-12 * want_inf
    assert abs(want_ref - want_inf) > 1e-3 * want_inf
    diag = dict(g, information=[PC.INFO_DIAGONAL] * 4)
    a, b = R.Problem(weighting="reference", **diag), R.Problem(weighting="information", **diag)
    assert a.cost(a.poses) == b.cost(b.poses)          # a diagonal L is its own transpose
    with pytest.raises(ValueError, match="constraint 2"):
        R.Problem(**dict(g, information=[PC.INFO_FULL, PC.INFO_FULL, np.zeros((3, 3)), PC.INFO_FULL]))


@pytest.mark.parametrize("name", list(PC.TABLE))
def test_the_restatement_stays_within_the_gate(name):
    """Every gate is 100 floors (rounded up) and the restatement reaches it with a factor 10 to
    spare; every gate is <= 1e-6 |g(x0)|_inf, so passing it means something."""
    P, ref, gate = PC.problem(name), PC.solution(name), PC.gate(name)
    floor = PC.TABLE[name][3]
    print("%s: n %d m %d |g(x0)| %.3e floor %.3e (table %.1e) gate %.1e cost %.6e after %d iterations" %
          (name, P.n, P.m, ref["start_gradient"], ref["gradient"], floor, gate, ref["cost"], ref["iterations"]))
    assert 100.0 * floor <= gate <= 200.0 * floor
    assert ref["gradient"] <= gate / 10.0
    assert gate <= 1e-6 * ref["start_gradient"]
    assert ref["cost"] <= P.cost(P.poses)
    assert np.array_equal(ref["x"][P.fixed], P.poses[P.fixed])


def test_the_designed_cases_are_what_they_are_for():
    sizes = {k: (PC.problem(k).n, PC.problem(k).m) for k in PC.TABLE}
    assert sizes["pair"] == (2, 1) and sizes["m_1025"][1] == 1025
    assert [sizes[k][0] for k in ("loop_1023", "loop_1024", "loop_1025")] == [1023, 1024, 1025]
    hub = PC.problem("hub")
    assert np.bincount(np.concatenate([hub.begin, hub.end]))[0] == 300
    wrap = PC.problem("wrap")
    assert wrap.poses[:, 2].max() > R.PI and wrap.poses[:, 2].min() < -R.PI
    # closures across the wrap: the raw heading difference lies a whole turn from its residual
    raw = (wrap.poses[wrap.end, 2] - wrap.poses[wrap.begin, 2]) - wrap.transform[:, 2]
    assert np.sum(np.abs(raw) > 6.0) == 4 and np.all(np.abs(wrap.errors(wrap.poses)[:, 2]) < 0.1)
    assert {PC.TABLE[k][1] for k in PC.TABLE} == {"reference", "information"}
    assert PC.problem("square_fixed_2").fixed == 2 and PC.problem("loop_1025").fixed == 512
    # the floating component: no path from poses 4..7 to the fixed pose
    f = PC.problem("floating")
    assert not np.any((f.begin < 4) != (f.end < 4))
