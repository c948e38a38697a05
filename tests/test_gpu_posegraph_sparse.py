"""The sparse solve on the device (ndt2d_sparse_*, PoseGraph.optimize_sparse) against the numpy
restatement (tests/posegraph_restatement.py's Problem and its dense minimiser; the LM loop restated in
tests/posegraph_direct_restatement.py) on the designed graphs of the pose-graph tests and on chains
laid out for the edges of the separator layout.

The assertions are tests/test_gpu_posegraph_direct.py's: the status is CONVERGED_GRADIENT at
gradient_tolerance = the graph's gate with the other rules off; |g(x_dev)|_inf as the restatement
evaluates it <= 2 x the gate; |x_dev - x*|_inf <= 2 |H(x*)^-1|_inf (gate + the restatement's own
floor); initial_cost is evaluate's bit for bit.  The yardstick is the restatement, never the CG path,
the direct solve or the code under test."""
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
    if "m" in _STATE:
        _STATE.pop("m").close()


def _new(P, max_jobs=1, switchable=None, loss=None):
    pg = PoseGraph(_matcher(), max_nodes=P.n, max_constraints=max(1, P.m), max_jobs=max_jobs)
    pg.set_weighting(P.weighting)
    if loss is not None:
        pg.set_loss(*loss)
    pg.set_graph(P.poses, begin=P.begin, end=P.end, transform=P.transform, information=P.information, fixed=P.fixed,
                 switchable=np.ones(P.m, dtype=bool) if switchable is None else switchable)
    return pg


def _same(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert np.array_equal(a[key], b[key]), key


def _separators(P):
    closure = np.abs(P.begin - P.end) != 1
    return len(set(P.begin[closure]) | set(P.end[closure]))


def _job_bytes(P, loss=False):
    s = _separators(P)
    ld = 48 * ((3 * s + 47) // 48)
    return 8 * (90 * (P.n - s) + ld * ld + 2 * ld + 6 * s + 41 * P.n + (P.m if loss else 0) + 17)


def _report(label, got, restated, gate, err=None, bound=None):
    print("%s: %s after %d iterations, %d rejected, %d failed factorisations, pivot ratio %.2e; |g| device %.3e restated %.3e (gate %.1e); "
          "|x - x*| %s (bound %s); F %.12e -> %.12e"
          % (label, got["status_name"], got["iterations"], got["rejected"], got["not_positive_definite"], got["pivot_ratio"], got["gradient"],
             restated, gate, "-" if err is None else "%.3e" % err, "-" if bound is None else "%.3e" % bound, got["initial_cost"],
             got["final_cost"]))


def _minimiser(label, P, pg, ref, gate, masks=None, enabled=None, unique=True):
    """optimize_sparse at the gate against the restatement's solution ref; returns (the job, its bound)."""
    got = pg.optimize_sparse(masks=masks, gradient_tolerance=gate, **RULES_OFF)[0]
    restated = P.gradient_norm(got["poses"], enabled)
    bound = DC.bound(P, ref, gate, enabled) if unique else math.inf
    err = float(np.max(np.abs(got["poses"] - ref["x"])))
    _report(label, got, restated, gate, err, bound)
    assert got["status"] == GRADIENT
    assert restated <= 2.0 * gate
    assert err <= bound
    assert np.array_equal(got["poses"][P.fixed], P.poses[P.fixed])
    assert got["initial_cost"] == pg.evaluate(masks)[0]["cost"]                      # evaluate's F bit for bit
    assert got["rejected"] >= got["not_positive_definite"] and got["iterations"] > got["rejected"]
    assert 0.0 < got["pivot_ratio"] <= 1.0
    layout = pg.sparse_layout()
    assert layout == dict(separators=_separators(P), interior=P.n - _separators(P))
    return got, bound


def _solved(label, P, ref, gate, **kw):
    pg = _new(P)
    try:
        return _minimiser(label, P, pg, ref, gate, **kw)
    finally:
        pg.close()


# ---- the minimiser on the designed graphs ----

@pytest.mark.parametrize("name", PC.UNIQUE)
def test_the_table_cases_reach_the_minimiser(name):
    """posegraph_cases' table through the new call; "hub": pose 0 an end of 299 closure edges, every
    node a separator, a dense S of 903 unknowns."""
    P = PC.problem(name)
    _solved(name, P, PC.solution(name), PC.gate(name))


@pytest.mark.parametrize("name", list(CH.EDGES))
def test_the_chain_cases_reach_the_minimiser(name):
    P = CH.problem(name)
    _solved(name, P, CH.solution(name), CH.gate(name))


# ---- the edges of the layout ----

def _spread(s):
    """Closures that make exactly s separators on a chain of 70: the nodes 1, 3, 5, ... joined in a row."""
    nodes = [2 * k + 1 for k in range(s)]
    return [(nodes[k], nodes[k + 1]) for k in range(s - 1)]


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


def _round_up(raw):
    digit = 10.0 ** math.floor(math.log10(raw))
    return math.ceil(raw / digit) * digit


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_edges_of_the_layout(name):
    """Chains of 2 to 70 poses: no closure (s = 0: no dense launch), separators at both ends, next to one
    another, next to and on the fixed node, the fixed node inside a segment, every node a separator, and
    3 s at -3 / 0 / +3 round the panel of 48 and round 96.  The gate: 100 x the restatement's floor, as
    posegraph_chain_cases'."""
    build, s = LAYOUTS[name]
    P = R.Problem(**build())
    assert _separators(P) == s
    ref = P.solve()
    gate = PC.gate("pair") if name == "two_poses" else _round_up(100.0 * ref["gradient"])
    got, _ = _solved(name, P, ref, gate)
    if s == 0:
        assert got["pivot_ratio"] == 1.0


# ---- thread ownership: 1,023, 1,024, 1,025 and 2,049 interior nodes ----

def _owned(interior):
    n = interior + 8
    return R.Problem(**CH.chain(n, 90 + interior % 7, closures=[(2, n // 2), (n // 4, n - 3), (n // 3, n // 3 + 200), (40, n - 40)]))


def _owned_gate():
    """100 x the restatement's floor on the chain of 1,025 interior nodes (computed once: its dense solve is
    this module's 2 - 3 s); the chains of 1,023 and 1,024 are the same construction two and one node
    shorter and take it as it is, the chain of 2,049 takes twice it (the floor grows with the terms of a
    node's sum, not with n: posegraph_cases' table has 3.8e-13 at 24 poses and 1.3e-12 at 1,025)."""
    if "owned" not in _STATE:
        P = _owned(1025)
        ref = P.solve()
        _STATE["owned"] = (P, ref, _round_up(100.0 * ref["gradient"]))
    return _STATE["owned"]


@pytest.mark.parametrize("interior", (1023, 1024, 1025, 2049))
def test_thread_ownership(interior):
    P1025, ref, gate = _owned_gate()
    if interior == 1025:
        _solved("owned_1025", P1025, ref, gate)
        return
    P = _owned(interior)
    assert P.n - _separators(P) == interior
    gate = 2.0 * gate if interior == 2049 else gate
    pg = _new(P)
    try:
        got = pg.optimize_sparse(gradient_tolerance=gate, **RULES_OFF)[0]
        assert pg.sparse_layout() == dict(separators=8, interior=interior)
    finally:
        pg.close()
    restated = P.gradient_norm(got["poses"])
    _report("owned_%d" % interior, got, restated, gate)
    assert got["status"] == GRADIENT and restated <= 2.0 * gate
    assert got["final_cost"] < got["initial_cost"] and np.array_equal(got["poses"][0], P.poses[0])


# ---- masks ----

def _wrap_with_a_leaf():
    """posegraph_cases.wrap (24 poses, 4 closures: 8 separators) and a 25th pose, with a negative zero to
    keep, that hangs on one switchable constraint."""
    g = PC.wrap()
    poses = np.vstack([g["poses"], [[9.0, -9.0, -0.0]]])
    begin, end = list(g["begin"]) + [23], list(g["end"]) + [24]
    transform = np.vstack([g["transform"], [[0.3, 0.1, 0.2]]])
    return R.Problem(poses, begin, end, transform, [PC.INFO_FULL] * len(begin))


def test_masks_against_the_restatement():
    """A closure off; an odometry edge off (the chain is broken there, A_ii is still definite, the rest
    hangs on the closures); both, each mask against the restatement's minimiser for that mask."""
    P = _wrap_with_a_leaf()
    closures = np.nonzero(np.abs(P.begin - P.end) != 1)[0]
    odometry = int(np.nonzero((P.begin == 5) & (P.end == 6))[0][0])
    masks = np.ones((3, P.m), dtype=np.uint8)
    masks[0, closures[1]] = 0
    masks[1, odometry] = 0
    masks[2, closures[2]] = 0
    masks[2, odometry] = 0
    pg = _new(P, max_jobs=4)
    try:
        for k in range(3):
            ref = P.solve(masks[k])
            _minimiser("wrap, mask %d" % k, P, pg, ref, _round_up(100.0 * ref["gradient"]), masks=masks[k:k + 1], enabled=masks[k])
    finally:
        pg.close()


def test_a_floating_component_reaches_the_gate():
    """A component not joined to the fixed pose has no unique minimiser (H_FF is singular, lambda D
    makes A definite): the cost and the gate only."""
    P, ref = PC.problem("floating"), PC.solution("floating")
    got, _ = _solved("floating", P, ref, PC.gate("floating"), unique=False)
    assert abs(got["final_cost"] - ref["cost"]) <= 1e-12 * max(1.0, abs(ref["cost"]))


def test_determinism():
    P = _wrap_with_a_leaf()
    leaf = P.m - 1
    closures = np.nonzero(np.abs(P.begin - P.end) != 1)[0]
    assert len(closures) == 4 and P.n == 25 and _separators(P) == 8
    gate = 4e-11                                                                      # "wrap"'s
    pg = _new(P, max_jobs=8)
    try:
        first = pg.optimize_sparse(gradient_tolerance=gate, **RULES_OFF)[0]
        assert first["status"] == GRADIENT
        _same(pg.optimize_sparse(gradient_tolerance=gate, **RULES_OFF)[0], first)      # the same call twice
        # five masks: all on; one closure off each, the leaf off; every closure and the leaf off (the
        # start poses are the odometry's integration: that job stops before its first iteration)
        masks = np.ones((5, P.m), dtype=np.uint8)
        for k in range(1, 4):
            masks[k, closures[k - 1]] = 0
            masks[k, leaf] = 0
        masks[4, closures] = 0
        masks[4, leaf] = 0
        five = pg.optimize_sparse(masks=masks, gradient_tolerance=gate, **RULES_OFF)
        print("determinism: iterations %s" % [j["iterations"] for j in five])
        assert all(j["status"] == GRADIENT for j in five) and len({j["iterations"] for j in five}) > 1
        assert five[4]["iterations"] == 0 and np.array_equal(five[4]["poses"], P.poses)
        _same(five[0], first)
        for k in (2, 4):                                                               # a mask alone against among five
            _same(pg.optimize_sparse(masks=masks[k:k + 1], gradient_tolerance=gate, **RULES_OFF)[0], five[k])
        # a workspace that holds one job a chunk, two, and all five in one
        job_bytes = _job_bytes(P)
        for budget in (job_bytes + 8, 2 * job_bytes, 5 * job_bytes):
            chunked = pg.optimize_sparse(masks=masks, workspace_bytes=budget, gradient_tolerance=gate, **RULES_OFF)
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


# ---- the losses ----

@pytest.mark.parametrize("loss", RC.LOSSES)
def test_losses(loss):
    case, weighting = "loop40", "reference"
    P, ref, gate = RC.problem(case, loss, weighting), RC.solution(case, loss, weighting), RC.gate(case, loss, weighting)
    false = RC.graph(case)[2]
    pg = _new(P, switchable=RC.closures(case), loss=(loss, RC.SCALE))
    try:
        got = pg.optimize_sparse(gradient_tolerance=gate, **RULES_OFF)[0]
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
        want = never.optimize_sparse()[0]
        pg.set_loss("huber", 0.7)
        robust = pg.optimize_sparse()[0]
        assert "weights" in robust and not np.array_equal(robust["poses"], want["poses"])
        pg.set_loss("trivial")
        again = pg.optimize_sparse()[0]
        assert "weights" not in again
        _same(again, want)
    finally:
        never.close()
        pg.close()


# ---- rejected steps ----

def test_a_rejected_step():
    """posegraph_direct_cases' "rejecting_far": start poses 1.5 m and 1.5 rad off, whose first steps raise
    the cost up to 13 times over.  At the gate the device lands on the minimiser far_reference gives.
    The number of iterations and of rejections is the restatement's (posegraph_direct_restatement.solve)
    at the same tolerances, here gradient_tolerance = 1e-6 with the other rules off: 19 iterations, 4
    rejected, each by a gain ratio below -1.  The counts are compared where every decision stands clear
    of the cost's rounding.  Run on to 1e-9, the restatement rejects a fifth step at |g|_inf = 2.1e-9 on
    dF = -5.4e-17 of F = 1.2e-4, 8 x the noise rule's 256 eps F, the sign of which is the rounding of
    its cost sum, and takes 22 iterations with 5 rejected; the device, whose sums round otherwise,
    accepts that step and takes 21 with 4 (printed, not asserted)."""
    P = DC.problem("rejecting_far")
    ref, gate, far = DC.far_reference()
    rules = dict(max_iterations=200, gradient_tolerance=1e-6, function_tolerance=0.0, parameter_tolerance=0.0)
    want = DR.solve(P, **rules)
    assert want["status"] == DR.CONVERGED_GRADIENT and want["rejected"] >= 3
    pg = _new(P)
    try:
        got, _ = _minimiser("rejecting_far", P, pg, ref, gate)
        run = pg.optimize_sparse(**rules)[0]
        on = pg.optimize_sparse(**dict(rules, gradient_tolerance=1e-9))[0]
    finally:
        pg.close()
    print("rejecting_far at 1e-6: the restatement %d iterations, %d rejected; the device %d, %d.  At 1e-9: the restatement %d, %d; the device %d, %d"
          % (want["iterations"], want["rejected"], run["iterations"], run["rejected"], far["iterations"], far["rejected"], on["iterations"],
             on["rejected"]))
    assert got["rejected"] >= 1 and got["not_positive_definite"] == 0
    assert run["status"] == GRADIENT and run["iterations"] == want["iterations"] and run["rejected"] == want["rejected"]
    assert run["not_positive_definite"] == want["not_positive_definite"] == 0


# ---- a size the direct solve cannot hold ----

def test_a_loop_of_5000_poses_with_50_closures():
    """15,000 unknowns: the direct solve's matrix would be 1.8 GB, over its default workspace, and the
    restatement's dense minimiser is out of reach -- its gradient (a gather, no dense matrix, a fraction
    of a second) is the yardstick.  The gate, 1e-9: the table's loops of 1,000 poses (the same generator)
    have 2e-10 from a floor of 1.2e-12, and the floor grows slower than n (3.8e-13 at 24 poses)."""
    P = R.Problem(**PC.loop(5000, 50, seed=21))
    gate = 1e-9
    assert _separators(P) == 100
    pg = _new(P)
    try:
        got = pg.optimize_sparse(gradient_tolerance=gate, **RULES_OFF)[0]
        assert pg.sparse_layout() == dict(separators=100, interior=4900)
        with pytest.raises(Ndt2dError, match="needs [0-9]+ bytes") as ei:
            pg.optimize_direct(gradient_tolerance=gate, **RULES_OFF)
        assert ei.value.code == _capi.ERR_INVALID
    finally:
        pg.close()
    restated = P.gradient_norm(got["poses"])
    _report("loop_5000", got, restated, gate)
    assert got["status"] == GRADIENT and restated <= 2.0 * gate
    assert got["final_cost"] < got["initial_cost"] and np.array_equal(got["poses"][0], P.poses[0])


# ---- the stop rules ----

def test_stop_rules():
    P = PC.problem("square")
    pg = _new(P)
    none = dict(gradient_tolerance=0.0, function_tolerance=0.0, parameter_tolerance=0.0)
    try:
        one = pg.optimize_sparse(max_iterations=1, **none)[0]
        assert one["status"] == _capi.POSEGRAPH_MAX_ITERATIONS and one["iterations"] == 1 and one["final_cost"] < one["initial_cost"]
        three = pg.optimize_sparse(max_iterations=3, **none)[0]
        assert three["status"] == _capi.POSEGRAPH_MAX_ITERATIONS and three["iterations"] == 3 and three["final_cost"] <= one["final_cost"]
        zero = pg.optimize_sparse(max_iterations=0, **none)[0]
        assert zero["status"] == _capi.POSEGRAPH_MAX_ITERATIONS and zero["iterations"] == 0 and np.array_equal(zero["poses"], P.poses)
        cost = pg.optimize_sparse(**dict(none, function_tolerance=1e-3))[0]
        assert cost["status"] == _capi.POSEGRAPH_CONVERGED_COST and cost["iterations"] >= 1
        step = pg.optimize_sparse(**dict(none, parameter_tolerance=1e-3))[0]
        assert step["status"] == _capi.POSEGRAPH_CONVERGED_STEP and step["iterations"] >= 1
        grad = pg.optimize_sparse(**dict(none, gradient_tolerance=1e3))[0]
        assert grad["status"] == GRADIENT and grad["iterations"] == 0 and np.array_equal(grad["poses"], P.poses)
        assert grad["final_cost"] == grad["initial_cost"] and grad["pivot_ratio"] == 1.0
    finally:
        pg.close()
    # no constraint, one pose: nothing moves, converged
    lone = PoseGraph(_matcher(), max_nodes=2, max_constraints=1, max_jobs=1)
    try:
        lone.set_graph(np.array([[1.0, 2.0, -0.0], [3.0, 4.0, 0.5]]))
        got = lone.optimize_sparse()[0]
        assert got["status"] == GRADIENT and got["iterations"] == 0 and np.array_equal(got["poses"], [[1.0, 2.0, -0.0], [3.0, 4.0, 0.5]])
        assert np.signbit(got["poses"][0, 2]) and got["initial_cost"] == 0.0
        assert lone.sparse_layout() == dict(separators=0, interior=2)
        lone.set_graph(np.array([[1.0, 2.0, 0.25]]))
        got = lone.optimize_sparse()[0]
        assert got["status"] == GRADIENT and np.array_equal(got["poses"], [[1.0, 2.0, 0.25]])
        assert lone.sparse_layout() == dict(separators=0, interior=1)
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
            fresh.optimize_sparse()
        assert ei.value.code == _capi.ERR_STATE
        with pytest.raises(Ndt2dError, match="no graph") as ei:
            fresh.sparse_layout()
        assert ei.value.code == _capi.ERR_STATE
    finally:
        fresh.close()
    pg = _new(P, max_jobs=2)
    try:
        want = pg.optimize_sparse()[0]

        def refused(text, **kw):
            with pytest.raises(Ndt2dError, match=text) as ei:
                pg.optimize_sparse(**kw)
            assert ei.value.code == _capi.ERR_INVALID

        need = _job_bytes(P)
        assert need == 8 * (90 * 2 + 48 * 48 + 96 + 12 + 164 + 17)
        refused("needs %d bytes" % need, workspace_bytes=need - 1)
        _same(pg.optimize_sparse(workspace_bytes=need)[0], want)
        refused("tolerance", gradient_tolerance=-1e-12)
        refused("tolerance", function_tolerance=math.nan)
        refused("tolerance", parameter_tolerance=math.inf)
        with pytest.raises(Ndt2dError) as ei:
            pg.optimize_sparse(workspace_bytes=0)
        assert ei.value.code == _capi.ERR_INVALID
        with pytest.raises(TypeError):
            pg.optimize_sparse(tolerance=1.0)
        _same(pg.optimize_sparse()[0], want)                                              # (the object is made anew)
        L, d = pg._L, _capi.dptr
        z, rec = np.zeros(12), np.zeros(_capi.DIRECT_RECORD_DOUBLES)
        assert L.ndt2d_sparse_solve(pg._sparse, None, 1, 10, 0.0, 0.0, 0.0, None, d(rec), None) == _capi.ERR_INVALID      # NULL outputs
        assert L.ndt2d_sparse_solve(pg._sparse, None, 1, 10, 0.0, 0.0, 0.0, d(z), None, None) == _capi.ERR_INVALID
        assert b"null argument" in L.ndt2d_sparse_last_error(pg._sparse)
        s = C.c_size_t(0)
        assert L.ndt2d_sparse_layout(pg._sparse, None, C.byref(s)) == _capi.ERR_INVALID
        assert L.ndt2d_sparse_layout(pg._sparse, C.byref(s), None) == _capi.ERR_INVALID
        assert L.ndt2d_sparse_solve(pg._sparse, None, 0, 10, 0.0, 0.0, 0.0, None, None, None) == _capi.OK                 # n_jobs == 0
        assert L.ndt2d_sparse_solve(pg._sparse, None, 1, 100, 1e-10, 1e-6, 1e-8, d(z), d(rec), None) == _capi.OK          # no chi2
        assert np.array_equal(z.reshape(4, 3), want["poses"]) and rec[0] == want["status"] and rec[1] == want["iterations"]
        # a caller's stream, timed
        m = _matcher()
        stream = torch.cuda.Stream()
        m.set_stream(stream.cuda_stream)
        try:
            got = pg.optimize_sparse()[0]
            pg.set_timing(True)
            timed = pg.optimize_sparse()[0]
            kernel_ms, fetch_ms = pg.sparse_last_ms()
            assert kernel_ms > 0.0 and fetch_ms >= 0.0
        finally:
            pg.set_timing(False)
            m.set_stream(None)
        _same(got, want)
        _same(timed, want)
    finally:
        pg.close()


# ---- end to end ----

def test_graph_optimize_end_to_end():
    """The close_loops graph of tests/test_gpu_posegraph.py's end-to-end test through Graph.optimize
    (method="schur": the name under which graph_io offers optimize_sparse) at the restatement's gate for
    that graph: within the bound of the restatement's minimiser."""
    import test_gpu_posegraph_marginals as TM
    m = ScanMatcherNDT(0)
    try:
        graph, _ = TM._end_to_end_graph(m)
        start = [np.array(s.pose, dtype=np.float64) for s in graph.scans]
        P = R.Problem(np.array(start), [c.begin for c in graph.constraints], [c.end for c in graph.constraints],
                      [c.transform for c in graph.constraints], [c.information for c in graph.constraints])
        ref = P.solve()
        gate = _round_up(100.0 * ref["gradient"])
        bound = DC.bound(P, ref, gate)
        assert graph.optimize(m, method="schur", gradient_tolerance=gate, **RULES_OFF) is True
        after = np.array([s.pose for s in graph.scans])
        got = graph.last_optimize
        err = float(np.max(np.abs(after - ref["x"])))
        print("end to end: %d poses, %d separators, %d iterations (%d rejected); |x - x*| %.3e (bound %.3e)"
              % (P.n, _separators(P), got["iterations"], got["rejected"], err, bound))
        assert got["status"] == GRADIENT and np.array_equal(after, got["poses"]) and "rejected" in got
        assert P.gradient_norm(after) <= 2.0 * gate and err <= bound
    finally:
        m.close()
