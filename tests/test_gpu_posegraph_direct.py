"""The direct solve on the device (ndt2d_direct_*, PoseGraph.optimize_direct) against the numpy
restatement (tests/posegraph_restatement.py's Problem and its solve; the LM loop itself restated in
tests/posegraph_direct_restatement.py) on the designed graphs of the pose-graph tests.

The assertions are tests/test_gpu_posegraph.py's test_solve_reaches_the_minimiser: the status is
CONVERGED_GRADIENT at gradient_tolerance = the graph's gate with the other rules off; |g(x_dev)|_inf
as the restatement evaluates it <= 2 x the gate; |x_dev - x*|_inf <= 2 |H(x*)^-1|_inf (gate + the
restatement's own floor).  The yardstick is the restatement, never the CG path; where the two device
paths are compared, it is by the sum of their bounds against it."""
import math

import numpy as np
import pytest

import posegraph_cases as PC
import posegraph_chain_cases as CH
import posegraph_direct_cases as DC
import posegraph_direct_restatement as DR
import posegraph_restatement as R
import posegraph_robust_cases as RC
from ndt_2d_amd import Ndt2dError, PoseGraph, ScanMatcherNDT, _capi

pytestmark = pytest.mark.gpu

RULES_OFF = dict(max_iterations=200, function_tolerance=0.0, parameter_tolerance=0.0)
GRADIENT = _capi.POSEGRAPH_CONVERGED_GRADIENT
_STATE = {}


def _matcher():
    if "m" not in _STATE:
        _STATE["m"] = ScanMatcherNDT(0)
    return _STATE["m"]


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    for pg in _STATE.pop("graphs", {}).values():
        pg.close()
    if "m" in _STATE:
        _STATE.pop("m").close()


def _new(P, max_jobs=8, switchable=None, loss=None):
    pg = PoseGraph(_matcher(), max_nodes=P.n, max_constraints=max(1, P.m), max_jobs=max_jobs)
    pg.set_weighting(P.weighting)
    if loss is not None:
        pg.set_loss(*loss)
    pg.set_graph(P.poses, begin=P.begin, end=P.end, transform=P.transform, information=P.information, fixed=P.fixed,
                 switchable=np.ones(P.m, dtype=bool) if switchable is None else switchable)
    return pg


def _graph(key, P):
    graphs = _STATE.setdefault("graphs", {})
    if key not in graphs:
        graphs[key] = _new(P)
    return graphs[key]


def _same(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert np.array_equal(a[key], b[key]), key


def _minimiser(label, P, pg, ref, gate, masks=None, enabled=None, unique=True):
    """optimize_direct at the gate against the restatement's solution ref; returns (the job, its bound)."""
    got = pg.optimize_direct(masks=masks, gradient_tolerance=gate, **RULES_OFF)[0]
    restated = P.gradient_norm(got["poses"], enabled)
    bound = DC.bound(P, ref, gate, enabled) if unique else math.inf
    err = float(np.max(np.abs(got["poses"] - ref["x"])))
    print("%s: %s after %d iterations, %d rejected, %d failed factorisations, pivot ratio %.2e; |g| device %.3e restated %.3e (gate %.1e); "
          "|x - x*| %.3e (bound %.3e); F %.12e -> %.12e"
          % (label, got["status_name"], got["iterations"], got["rejected"], got["not_positive_definite"], got["pivot_ratio"], got["gradient"],
             restated, gate, err, bound, got["initial_cost"], got["final_cost"]))
    assert got["status"] == GRADIENT
    assert restated <= 2.0 * gate
    assert err <= bound
    assert np.array_equal(got["poses"][P.fixed], P.poses[P.fixed])
    assert got["initial_cost"] == pg.evaluate(masks)[0]["cost"]                      # evaluate's F bit for bit
    assert got["rejected"] >= got["not_positive_definite"] and got["iterations"] > got["rejected"]
    assert 0.0 < got["pivot_ratio"] <= 1.0
    return got, bound


# ---- the minimiser ----

@pytest.mark.parametrize("name", PC.UNIQUE)
def test_the_table_cases_reach_the_minimiser(name):
    P = PC.problem(name)
    _minimiser(name, P, _graph(name, P), PC.solution(name), PC.gate(name))


@pytest.mark.parametrize("name", list(CH.EDGES) + ["chain_1025"])
def test_the_chain_cases_reach_the_minimiser(name):
    P = CH.problem(name)
    _minimiser(name, P, _graph(name, P), CH.solution(name), CH.gate(name))


def test_a_floating_component_reaches_the_gate():
    """A component not joined to the fixed pose has no unique minimiser (H_FF is singular, lambda D
    makes A definite): the cost and the gate only."""
    P, ref = PC.problem("floating"), PC.solution("floating")
    got, _ = _minimiser("floating", P, _graph("floating", P), ref, PC.gate("floating"), unique=False)
    assert abs(got["final_cost"] - ref["cost"]) <= 1e-12 * max(1.0, abs(ref["cost"]))


@pytest.mark.parametrize("n", DC.PANEL_CHAINS)
def test_the_panel_edges_of_the_substitution(n):
    """Chains of d = 3 n = 6 ... 195 unknowns: at -3 / 0 / +3 and +6 round one, two and three panels of
    48, and four panels -- a panel boundary, the padding, a last partial panel."""
    name = "chain_%d" % n
    P = DC.problem(name)
    pg = _new(P, max_jobs=1)
    try:
        _minimiser(name, P, pg, DC.solution(name), DC.gate(name))
    finally:
        pg.close()


def test_a_rejected_step():
    """posegraph_direct_cases' "rejecting_far": start poses 1.5 m and 1.5 rad off, whose first steps raise
    the cost up to 13 times over -- the restatement rejects 5 of its 22 steps, four of them by that
    margin.  The minimiser is posegraph_direct_cases.far_reference's.  (The designed case "rejecting",
    0.6 off, is solved beside it without the count: the restatement's 2 rejections there are trial costs
    4e-18 above F = 1.2e-4, at the level of the cost's own rounding, and the device, whose sums round
    otherwise, takes 6 iterations without one.)"""
    P = DC.problem("rejecting_far")
    ref, gate, want = DC.far_reference()
    assert want["rejected"] >= 3
    pg = _new(P, max_jobs=1)
    try:
        got, _ = _minimiser("rejecting_far", P, pg, ref, gate)
    finally:
        pg.close()
    print("rejecting_far: the restatement %d iterations, %d rejected" % (want["iterations"], want["rejected"]))
    assert got["rejected"] >= 1 and got["not_positive_definite"] == 0
    P = DC.problem("rejecting")
    pg = _new(P, max_jobs=1)
    try:
        _minimiser("rejecting", P, pg, DC.solution("rejecting"), DC.gate("rejecting"))
    finally:
        pg.close()


def test_many_closures_and_the_cg_path_beside_it():
    """200 poses, 100 closures: every constraint on, and every second closure off.  Each mask against
    the restatement for that mask; PoseGraph.optimize under "jacobi" on the same object lands within
    the sum of the two paths' bounds."""
    P = DC.problem("closures_100")
    pg = _graph("closures_100", P)
    closures = np.nonzero(np.abs(P.begin - P.end) != 1)[0]
    assert len(closures) == 100
    masks = np.ones((2, P.m), dtype=np.uint8)
    masks[1, closures[1::2]] = 0
    pg.set_preconditioner("jacobi")
    for k in range(2):
        ref, gate = DC.solution("closures_100", masks[k]), DC.gate("closures_100", masks[k])
        got, bound = _minimiser("closures_100, mask %d" % k, P, pg, ref, gate, masks=masks[k:k + 1], enabled=masks[k])
        cg = pg.optimize(masks=masks[k:k + 1], gradient_tolerance=gate, **RULES_OFF)[0]
        apart = float(np.max(np.abs(got["poses"] - cg["poses"])))
        print("closures_100, mask %d: CG %s after %d iterations, %d CG; |x_direct - x_cg| %.3e (the two bounds %.3e)"
              % (k, cg["status_name"], cg["iterations"], cg["cg_iterations"], apart, 2.0 * bound))
        assert cg["status"] == GRADIENT and apart <= 2.0 * bound
    both = pg.optimize_direct(masks=masks, gradient_tolerance=DC.gate("closures_100"), **RULES_OFF)
    assert float(np.max(np.abs(both[0]["poses"] - both[1]["poses"]))) > 1e-6          # the mask matters


# ---- the losses ----

@pytest.mark.parametrize("loss", RC.LOSSES)
def test_losses(loss):
    case, weighting = "loop40", "reference"
    P, ref, gate = RC.problem(case, loss, weighting), RC.solution(case, loss, weighting), RC.gate(case, loss, weighting)
    false = RC.graph(case)[2]
    pg = _new(P, switchable=RC.closures(case), loss=(loss, RC.SCALE))
    try:
        got = pg.optimize_direct(gradient_tolerance=gate, **RULES_OFF)[0]
        start = pg.evaluate()[0]["cost"]
    finally:
        pg.close()
    restated = P.gradient_norm(got["poses"])
    bound = 2.0 * ref["inverse_norm"] * (gate + ref["gradient"])
    err = float(np.max(np.abs(got["poses"] - ref["x"])))
    print("%s %s: %s after %d iterations, %d rejected; robust |g| restated %.3e (gate %.1e); |x - x*| %.3e (bound %.3e); rho' of the false closure %.4f"
          % (case, loss, got["status_name"], got["iterations"], got["rejected"], restated, gate, err, bound, got["weights"][false]))
    assert got["status"] == GRADIENT and restated <= 2.0 * gate and err <= bound
    assert got["initial_cost"] == start
    assert abs(got["final_cost"] - ref["cost"]) <= 1e-9 * ref["cost"]
    assert got["weights"].shape == (P.m,) and got["weights"][false] < 0.1 and np.delete(got["weights"], false).min() > 0.9
    assert np.all(np.abs(got["weights"] - P.weights(got["poses"])) <= 1e-9)


def test_trivial_is_an_object_without_a_loss():
    g = RC.graph("loop40")[0]
    P = R.Problem(**g)
    never, pg = _new(P, switchable=RC.closures("loop40")), _new(P, switchable=RC.closures("loop40"))
    try:
        want = never.optimize_direct()[0]
        pg.set_loss("huber", 0.7)
        robust = pg.optimize_direct()[0]
        assert "weights" in robust and not np.array_equal(robust["poses"], want["poses"])
        pg.set_loss("trivial")
        again = pg.optimize_direct()[0]
        assert "weights" not in again
        _same(again, want)
    finally:
        never.close()
        pg.close()


# ---- determinism ----

def _wrap_with_a_leaf():
    """posegraph_cases.wrap (24 poses, 4 closures) and a 25th pose, with a negative zero to keep,
    that hangs on one switchable constraint."""
    g = PC.wrap()
    poses = np.vstack([g["poses"], [[9.0, -9.0, -0.0]]])
    begin, end = list(g["begin"]) + [23], list(g["end"]) + [24]
    transform = np.vstack([g["transform"], [[0.3, 0.1, 0.2]]])
    return R.Problem(poses, begin, end, transform, [PC.INFO_FULL] * len(begin))


def test_determinism():
    P = _wrap_with_a_leaf()
    leaf = P.m - 1
    closures = np.nonzero(np.abs(P.begin - P.end) != 1)[0]
    assert len(closures) == 4 and P.n == 25
    gate = 4e-11                                                                      # "wrap"'s
    pg = _new(P, max_jobs=8)
    try:
        first = pg.optimize_direct(gradient_tolerance=gate, **RULES_OFF)[0]
        assert first["status"] == GRADIENT
        _same(pg.optimize_direct(gradient_tolerance=gate, **RULES_OFF)[0], first)      # the same call twice
        # five masks: all on; one closure off each, the leaf off; every closure and the leaf off (the
        # start poses are the odometry's integration: that job stops before its first iteration)
        masks = np.ones((5, P.m), dtype=np.uint8)
        for k in range(1, 4):
            masks[k, closures[k - 1]] = 0
            masks[k, leaf] = 0
        masks[4, closures] = 0
        masks[4, leaf] = 0
        five = pg.optimize_direct(masks=masks, gradient_tolerance=gate, **RULES_OFF)
        print("determinism: iterations %s" % [j["iterations"] for j in five])
        assert all(j["status"] == GRADIENT for j in five) and len({j["iterations"] for j in five}) > 1
        assert five[4]["iterations"] == 0 and np.array_equal(five[4]["poses"], P.poses)
        _same(five[0], first)
        for k in (2, 4):                                                               # a mask alone against among five
            _same(pg.optimize_direct(masks=masks[k:k + 1], gradient_tolerance=gate, **RULES_OFF)[0], five[k])
        # a workspace that holds one job a chunk against all five in one
        job_bytes = 8 * (96 * 96 + 2 * 96 + 44 * P.n + 16)                             # d = 75: two panels of 48
        for budget in (job_bytes + 8, 2 * job_bytes, 5 * job_bytes):
            chunked = pg.optimize_direct(masks=masks, workspace_bytes=budget, gradient_tolerance=gate, **RULES_OFF)
            for k in range(5):
                _same(chunked[k], five[k])
        # nodes that must not move keep their bits: the fixed node, and a node all of whose constraints are off
        for k in range(5):
            assert np.array_equal(five[k]["poses"][P.fixed], P.poses[P.fixed])
        for k in range(1, 5):
            assert np.array_equal(five[k]["poses"][24], P.poses[24]) and np.signbit(five[k]["poses"][24, 2])
        assert not np.array_equal(five[0]["poses"][24], P.poses[24])
    finally:
        pg.close()


# ---- the stop rules ----

def test_stop_rules():
    P = PC.problem("square")
    pg = _graph("square", P)
    none = dict(gradient_tolerance=0.0, function_tolerance=0.0, parameter_tolerance=0.0)
    one = pg.optimize_direct(max_iterations=1, **none)[0]
    assert one["status"] == _capi.POSEGRAPH_MAX_ITERATIONS and one["iterations"] == 1 and one["final_cost"] < one["initial_cost"]
    three = pg.optimize_direct(max_iterations=3, **none)[0]
    assert three["status"] == _capi.POSEGRAPH_MAX_ITERATIONS and three["iterations"] == 3 and three["final_cost"] <= one["final_cost"]
    zero = pg.optimize_direct(max_iterations=0, **none)[0]
    assert zero["status"] == _capi.POSEGRAPH_MAX_ITERATIONS and zero["iterations"] == 0 and np.array_equal(zero["poses"], P.poses)
    cost = pg.optimize_direct(**dict(none, function_tolerance=1e-3))[0]
    assert cost["status"] == _capi.POSEGRAPH_CONVERGED_COST and cost["iterations"] >= 1
    step = pg.optimize_direct(**dict(none, parameter_tolerance=1e-3))[0]
    assert step["status"] == _capi.POSEGRAPH_CONVERGED_STEP and step["iterations"] >= 1
    grad = pg.optimize_direct(**dict(none, gradient_tolerance=1e3))[0]
    assert grad["status"] == GRADIENT and grad["iterations"] == 0 and np.array_equal(grad["poses"], P.poses)
    assert grad["final_cost"] == grad["initial_cost"] and grad["pivot_ratio"] == 1.0
    # no constraint, one pose: nothing moves, converged
    lone = PoseGraph(_matcher(), max_nodes=2, max_constraints=1, max_jobs=1)
    try:
        lone.set_graph(np.array([[1.0, 2.0, -0.0], [3.0, 4.0, 0.5]]))
        got = lone.optimize_direct()[0]
        assert got["status"] == GRADIENT and got["iterations"] == 0 and np.array_equal(got["poses"], [[1.0, 2.0, -0.0], [3.0, 4.0, 0.5]])
        assert np.signbit(got["poses"][0, 2]) and got["initial_cost"] == 0.0
        lone.set_graph(np.array([[1.0, 2.0, 0.25]]))
        got = lone.optimize_direct()[0]
        assert got["status"] == GRADIENT and np.array_equal(got["poses"], [[1.0, 2.0, 0.25]])
    finally:
        lone.close()


# ---- refusals, a caller's stream, timing ----

def test_refusals_a_callers_stream_and_timing():
    import ctypes as C
    import torch
    P = PC.problem("square")
    fresh = PoseGraph(_matcher(), max_nodes=4, max_constraints=4, max_jobs=2)
    try:
        with pytest.raises(Ndt2dError, match="no graph") as ei:
            fresh.optimize_direct()
        assert ei.value.code == _capi.ERR_STATE
    finally:
        fresh.close()
    pg = _graph("square", P)
    want = pg.optimize_direct()[0]

    def refused(text, **kw):
        with pytest.raises(Ndt2dError, match=text) as ei:
            pg.optimize_direct(**kw)
        assert ei.value.code == _capi.ERR_INVALID

    need = 8 * (48 * 48 + 2 * 48 + 44 * 4 + 16)
    refused("needs %d bytes" % need, workspace_bytes=need - 1)
    _same(pg.optimize_direct(workspace_bytes=need)[0], want)
    refused("tolerance", gradient_tolerance=-1e-12)
    refused("tolerance", function_tolerance=math.nan)
    refused("tolerance", parameter_tolerance=math.inf)
    with pytest.raises(Ndt2dError) as ei:
        pg.optimize_direct(workspace_bytes=0)
    assert ei.value.code == _capi.ERR_INVALID
    with pytest.raises(TypeError):
        pg.optimize_direct(tolerance=1.0)
    _same(pg.optimize_direct()[0], want)                                              # (the object is made anew)
    L, d = pg._L, _capi.dptr
    z, rec = np.zeros(12), np.zeros(_capi.DIRECT_RECORD_DOUBLES)
    assert L.ndt2d_direct_solve(pg._direct, None, 1, 10, 0.0, 0.0, 0.0, None, d(rec), None) == _capi.ERR_INVALID      # NULL outputs
    assert L.ndt2d_direct_solve(pg._direct, None, 1, 10, 0.0, 0.0, 0.0, d(z), None, None) == _capi.ERR_INVALID
    assert b"null argument" in L.ndt2d_direct_last_error(pg._direct)
    assert L.ndt2d_direct_solve(pg._direct, None, 0, 10, 0.0, 0.0, 0.0, None, None, None) == _capi.OK                 # n_jobs == 0
    assert L.ndt2d_direct_solve(pg._direct, None, 1, 100, 1e-10, 1e-6, 1e-8, d(z), d(rec), None) == _capi.OK          # no chi2
    assert np.array_equal(z.reshape(4, 3), want["poses"]) and rec[0] == want["status"] and rec[1] == want["iterations"]
    # a caller's stream, timed
    m = _matcher()
    stream = torch.cuda.Stream()
    m.set_stream(stream.cuda_stream)
    try:
        got = pg.optimize_direct()[0]
        pg.set_timing(True)
        timed = pg.optimize_direct()[0]
        kernel_ms, fetch_ms = pg.direct_last_ms()
        assert kernel_ms > 0.0 and fetch_ms >= 0.0
    finally:
        pg.set_timing(False)
        m.set_stream(None)
    _same(got, want)
    _same(timed, want)
    assert C.sizeof(C.c_double) == 8


# ---- end to end ----

def test_graph_optimize_by_either_method_end_to_end():
    """The close_loops graph of tests/test_gpu_posegraph.py's end-to-end test: Graph.optimize(method=
    "direct") against method="cg", both at the restatement's gate for that graph, apart by no more
    than the sum of the two paths' bounds."""
    import test_gpu_posegraph_marginals as TM
    m = ScanMatcherNDT(0)
    try:
        graph, _ = TM._end_to_end_graph(m)
        start = [np.array(s.pose, dtype=np.float64) for s in graph.scans]
        P = R.Problem(np.array(start), [c.begin for c in graph.constraints], [c.end for c in graph.constraints],
                      [c.transform for c in graph.constraints], [c.information for c in graph.constraints])
        ref = P.solve()
        raw = 100.0 * ref["gradient"]
        digit = 10.0 ** math.floor(math.log10(raw))
        gate = math.ceil(raw / digit) * digit
        bound = DC.bound(P, ref, gate)
        found = {}
        for method in ("cg", "direct"):
            for s, pose in zip(graph.scans, start):
                s.pose = pose.copy()
            assert graph.optimize(m, method=method, gradient_tolerance=gate, **RULES_OFF) is True
            found[method] = graph.last_optimize
            after = np.array([s.pose for s in graph.scans])
            assert graph.last_optimize["status"] == GRADIENT and np.array_equal(after, graph.last_optimize["poses"])
            assert float(np.max(np.abs(after - ref["x"]))) <= bound
        apart = float(np.max(np.abs(found["cg"]["poses"] - found["direct"]["poses"])))
        print("end to end: direct %d iterations (%d rejected), CG %d iterations; apart %.3e (the two bounds %.3e)"
              % (found["direct"]["iterations"], found["direct"]["rejected"], found["cg"]["iterations"], apart, 2.0 * bound))
        assert apart <= 2.0 * bound and "rejected" in found["direct"] and "cg_iterations" in found["cg"]
        with pytest.raises(ValueError, match="method"):
            graph.optimize(m, method="sparse")
    finally:
        m.close()
