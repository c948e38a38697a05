"""The direct solve's restatement (tests/posegraph_direct_restatement.py) against the pose graph's own
yardstick, Problem.solve: on every designed graph of the pose-graph tests it reaches
CONVERGED_GRADIENT at the graph's gate within 200 iterations, and where the minimiser is unique it
lands within 2 |H(x*)^-1|_inf (gate + floor) of Problem.solve's.  No GPU."""
import numpy as np
import pytest

import posegraph_cases as PC
import posegraph_chain_cases as CH
import posegraph_direct_cases as DC
import posegraph_direct_restatement as DR

RULES = dict(max_iterations=200, function_tolerance=0.0, parameter_tolerance=0.0)


def _check(label, P, ref, gate, unique=True):
    got = DR.solve(P, gradient_tolerance=gate, **RULES)
    restated = P.gradient_norm(got["x"])
    print("%s: status %d after %d iterations, %d rejected, %d failed factorisations; |g| %.3e (gate %.1e); F %.12e -> %.12e"
          % (label, got["status"], got["iterations"], got["rejected"], got["not_positive_definite"], restated, gate, got["initial_cost"],
             got["cost"]))
    assert got["status"] == DR.CONVERGED_GRADIENT, (label, got["status"])
    assert restated <= gate and got["gradient"] == restated
    assert got["initial_cost"] == P.cost(P.poses) and got["cost"] == P.cost(got["x"])
    if unique:
        err, bound = float(np.max(np.abs(got["x"] - ref["x"]))), DC.bound(P, ref, gate)
        print("%s: |x - x*| %.3e (bound %.3e)" % (label, err, bound))
        assert err <= bound, (label, err, bound)
    return got


@pytest.mark.parametrize("name", list(PC.TABLE))
def test_the_table_cases_reach_their_gates(name):
    _check(name, PC.problem(name), PC.solution(name), PC.gate(name), unique=name in PC.UNIQUE)


@pytest.mark.parametrize("name", list(CH.EDGES))
def test_the_chain_edges_reach_their_gates(name):
    _check(name, CH.problem(name), CH.solution(name), CH.gate(name))


@pytest.mark.parametrize("n", DC.PANEL_CHAINS)
def test_the_chains_at_the_panel_edges_reach_their_gates(n):
    name = "chain_%d" % n
    _check(name, DC.problem(name), DC.solution(name), DC.gate(name))


def test_a_loop_with_a_hundred_closures_reaches_its_gate():
    P = DC.problem("closures_100")
    assert P.n == 200 and P.m == 299
    _check("closures_100", P, DC.solution("closures_100"), DC.gate("closures_100"))


def test_the_designed_case_rejects_steps_and_reaches_the_same_minimum():
    P = DC.problem("rejecting")
    got = _check("rejecting", P, DC.solution("rejecting"), DC.gate("rejecting"))
    assert got["rejected"] >= 1 and got["not_positive_definite"] == 0


def test_a_far_start_rejects_steps_by_a_wide_margin():
    """Steps that raise the cost several times over: rejections that no rounding decides.  The
    minimiser is the gentle start's with whole turns on some headings (posegraph_direct_cases.far_reference)."""
    P = DC.problem("rejecting_far")
    ref, gate, _ = DC.far_reference()
    rises, costs = [], []
    inner = P.cost
    P.cost = lambda x, enabled=None: costs.append(inner(x, enabled)) or costs[-1]
    try:
        got = _check("rejecting_far", P, ref, gate)
    finally:
        P.cost = inner
    costs = costs[:1 + got["iterations"]]                      # (the start's and one a trial; what _check asks afterwards is not the run's)
    best = costs[0]
    for v in costs[1:]:
        if v < best:
            best = v
        else:
            rises.append((v - best) / best)
    print("rejecting_far: trial costs above the accepted one by %s" % ["%.2g" % r for r in rises])
    assert got["rejected"] >= 3 and sum(r > 0.5 for r in rises) >= 3


def test_the_stop_rules_and_a_start_that_is_not_finite():
    P = PC.problem("square")
    assert DR.solve(P, max_iterations=1, gradient_tolerance=0.0, function_tolerance=0.0, parameter_tolerance=0.0)["iterations"] == 1
    assert DR.solve(P, max_iterations=3, gradient_tolerance=0.0, function_tolerance=0.0, parameter_tolerance=0.0)["status"] == DR.MAX_ITERATIONS
    assert DR.solve(P, gradient_tolerance=0.0, function_tolerance=1e-3, parameter_tolerance=0.0)["status"] == DR.CONVERGED_COST
    assert DR.solve(P, gradient_tolerance=0.0, function_tolerance=0.0, parameter_tolerance=1e-3)["status"] == DR.CONVERGED_STEP
    at_start = DR.solve(P, gradient_tolerance=1e3)
    assert at_start["status"] == DR.CONVERGED_GRADIENT and at_start["iterations"] == 0 and np.array_equal(at_start["x"], P.poses)
    import posegraph_restatement as R
    g = PC.square()
    g["poses"] = np.array(g["poses"])
    g["poses"][2, 0] = np.inf
    bad = DR.solve(R.Problem(**g))
    assert bad["status"] == DR.FAILED and bad["iterations"] == 0
