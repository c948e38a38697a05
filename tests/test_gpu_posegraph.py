"""The pose graph on the device (csrc/posegraph/, ndt_2d_amd.PoseGraph) against the numpy restatement
(tests/posegraph_restatement.py) on the designed graphs of tests/posegraph_cases.py.

The bounds.  evaluate: e_theta bit for bit; e_xy, r, chi2 and F within 1e-12 max(1, |value|), the
project's parity bound (cos and sin are the device library's).  solve, per case: the status is
CONVERGED_GRADIENT at gradient_tolerance = the case's gate with the other rules off; |g(x_dev)|_inf
as the restatement evaluates it <= 2 x the gate (the device's own evaluation of g differs from
numpy's by the rounding the gate is 100 floors above); and |x_dev - x*|_inf <= 2 |H(x*)^-1|_inf
(gate + the restatement's own final |g|_inf): to first order H (x_dev - x*) = g(x_dev) - g(x*), the
factor 2 is for the remainder.  Computed per case by the restatement, fixed nowhere."""
import math

import numpy as np
import pytest

import closure_refine_cases as CC
import posegraph_cases as PC
import posegraph_restatement as R
from ndt_2d_amd import Ndt2dError, PoseGraph, ScanMatcherNDT, _capi, close_loops, closure_constraints, graph_io, loop_closure_window, make_constraint

pytestmark = pytest.mark.gpu

PARITY = 1e-12
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


def _graph(name):
    """A PoseGraph holding the case (one per case for the module)."""
    graphs = _STATE.setdefault("graphs", {})
    if name not in graphs:
        P = PC.problem(name)
        pg = PoseGraph(_matcher(), max_nodes=P.n, max_constraints=max(1, P.m), max_jobs=8)
        pg.set_weighting(P.weighting)
        pg.set_graph(P.poses, begin=P.begin, end=P.end, transform=P.transform, information=P.information, fixed=P.fixed,
                     switchable=np.ones(P.m, dtype=bool))
        graphs[name] = pg
    return graphs[name]


def _within(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return bool(np.all(np.abs(got - want) <= PARITY * np.maximum(1.0, np.abs(want))))


def _boundary_problem():
    """Heading residuals on and round Normalize's edges: v = (theta_b - theta_a) - t_theta at -pi,
    pi, nextafter(pi, 0), +-3 pi, 1e6 and a few ordinary values."""
    vs = [-R.PI, R.PI, math.nextafter(R.PI, 0.0), 3.0 * R.PI, -3.0 * R.PI, 1e6, 0.0, 0.3, -2.9, 6.5, math.nextafter(-R.PI, 0.0)]
    poses, begin, end, transform = [[0.0, 0.0, 0.0]], [], [], []
    for k, v in enumerate(vs):
        poses.append([1.0 + k, 0.5 * k, v])
        begin.append(0)
        end.append(k + 1)
        transform.append([0.5, -0.25, 0.0])
    return R.Problem(poses, begin, end, transform, [PC.INFO_FULL] * len(vs))


@pytest.mark.parametrize("name", ["boundary", "wrap", "hub", "loop_1025"])
def test_evaluate_against_the_restatement(name):
    if name == "boundary":
        P = _boundary_problem()
        pg = PoseGraph(_matcher(), max_nodes=P.n, max_constraints=P.m, max_jobs=2)
        pg.set_graph(P.poses, begin=P.begin, end=P.end, transform=P.transform, information=P.information)
    else:
        P, pg = PC.problem(name), _graph(name)
    e, r, chi2 = P.residuals(P.poses)
    mask = np.ones((2, P.m), dtype=np.uint8)
    mask[1, ::3] = 0
    pg.switchable = np.ones(P.m, dtype=bool)
    got = pg.evaluate(mask, want_residuals=True)
    for k in range(2):
        assert np.array_equal(got[k]["e"][:, 2], e[:, 2]), np.nonzero(got[k]["e"][:, 2] != e[:, 2])
        assert _within(got[k]["e"], e) and _within(got[k]["r"], r) and _within(got[k]["chi2"], chi2)
        want = P.cost(P.poses, mask[k])
        print("%s mask %d: F %.17g (restatement %.17g)" % (name, k, got[k]["cost"], want))
        assert _within(got[k]["cost"], want)
    # (the formula's range is [-pi, pi) up to its own rounding: nextafter(pi, 0) comes out an ulp below -pi)
    assert np.all((e[:, 2] >= -R.PI - 2.0 ** -50) & (e[:, 2] < R.PI))
    if name == "boundary":
        pg.close()


@pytest.mark.parametrize("name", PC.UNIQUE)
def test_solve_reaches_the_minimiser(name):
    P, pg, gate = PC.problem(name), _graph(name), PC.gate(name)
    ref = PC.solution(name)
    got = pg.optimize(max_iterations=200, gradient_tolerance=gate, function_tolerance=0.0, parameter_tolerance=0.0)[0]
    restated = P.gradient_norm(got["poses"])
    bound = 2.0 * P.inverse_norm(ref["x"]) * (gate + ref["gradient"])
    err = float(np.max(np.abs(got["poses"] - ref["x"])))
    print("%s: %s after %d iterations, %d CG; |g| device %.3e restated %.3e (gate %.1e); |x - x*| %.3e (bound %.3e); F %.12e -> %.12e"
          % (name, got["status_name"], got["iterations"], got["cg_iterations"], got["gradient"], restated, gate, err, bound,
             got["initial_cost"], got["final_cost"]))
    assert got["status"] == _capi.POSEGRAPH_CONVERGED_GRADIENT
    assert restated <= 2.0 * gate
    assert err <= bound
    assert np.array_equal(got["poses"][P.fixed], P.poses[P.fixed])
    assert _within(got["initial_cost"], P.cost(P.poses)) and _within(got["final_cost"], P.cost(got["poses"]))
    assert _within(got["chi2_start"], P.residuals(P.poses)[2]) and _within(got["chi2"], P.residuals(got["poses"])[2])
    if name == "pair":
        a, t = P.poses[0], P.transform[0]
        c, s = math.cos(a[2]), math.sin(a[2])
        closed = np.array([a[0] + c * t[0] - s * t[1], a[1] + s * t[0] + c * t[1], a[2] + t[2]])
        assert np.max(np.abs(got["poses"][1] - closed)) <= bound and got["final_cost"] <= 1e-24
    if name == "line":
        assert np.max(np.abs(got["poses"] - PC.line_answer())) <= bound


def test_a_floating_component_reaches_the_gate():
    """A component not connected to the fixed pose has no unique minimiser: the cost and the gate only."""
    P, pg, gate = PC.problem("floating"), _graph("floating"), PC.gate("floating")
    ref = PC.solution("floating")
    got = pg.optimize(max_iterations=200, gradient_tolerance=gate, function_tolerance=0.0, parameter_tolerance=0.0)[0]
    print("floating: %s, %d iterations, F %.15e (restatement %.15e), restated |g| %.3e" %
          (got["status_name"], got["iterations"], got["final_cost"], ref["cost"], P.gradient_norm(got["poses"])))
    assert got["status"] == _capi.POSEGRAPH_CONVERGED_GRADIENT
    assert P.gradient_norm(got["poses"]) <= 2.0 * gate
    assert _within(got["final_cost"], ref["cost"])


def _masked_graph():
    """A loop whose odometry constraints are make_constraint on the start poses themselves (their
    residuals are rounding), with six switchable closures that disagree, and an isolated last pose."""
    if "masked" not in _STATE:
        g = PC.loop(60, 6, seed=21)
        poses = np.vstack([g["poses"], [[9.0, -9.0, -0.0]]])   # (the isolated pose, with a negative zero to keep)
        cons = []
        cov = np.linalg.inv(PC.INFO_FULL)
        for i in range(59):
            cons.append(make_constraint(i, i + 1, poses[i], poses[i + 1], cov))
        for c in range(59, 65):
            k = graph_io.Constraint(g["begin"][c], g["end"][c], g["transform"][c], PC.INFO_FULL, switchable=True)
            cons.append(k)
        pg = PoseGraph(_matcher(), max_nodes=len(poses), max_constraints=len(cons), max_jobs=3)   # (five masks: two chunks)
        pg.set_graph(poses, cons, fixed=0)
        _STATE["masked"] = (pg, poses, cons)
        _STATE.setdefault("graphs", {})["masked"] = pg
    return _STATE["masked"]


def test_masks_jobs_are_independent_and_repeatable():
    pg, poses, cons = _masked_graph()
    m = len(cons)
    masks = np.ones((6, m), dtype=np.uint8)
    masks[0, 59:] = 0                      # every closure off
    masks[1, 59] = 0
    masks[2, 60:63] = 0
    masks[3, 64] = 0
    masks[4, 59:62] = 0                    # (job 5 has every constraint on)
    five = pg.optimize(masks[[0, 1, 2, 3, 5]])
    off = five[0]
    print("closures off: %s, %d iterations, |g| %.3e" % (off["status_name"], off["iterations"], off["gradient"]))
    assert off["status"] == _capi.POSEGRAPH_CONVERGED_GRADIENT and off["iterations"] == 0
    assert off["poses"].tobytes() == poses.tobytes()
    alone = pg.optimize(masks[[1, 2, 5]])
    for a, b in zip(alone, [five[1], five[2], five[4]]):
        assert a["iterations"] > 0
        for key in a:
            assert np.array_equal(a[key], b[key]), key
    again = pg.optimize(masks[[0, 1, 2, 3, 5]])
    for a, b in zip(again, five):
        for key in a:
            assert np.array_equal(a[key], b[key]), key
    # a switched-off closure still gets its chi2, against the others' solution
    assert five[1]["chi2"][59] > 0.0 and not np.array_equal(five[1]["poses"], five[4]["poses"])


def test_nodes_that_must_not_move_keep_their_bits():
    pg, poses, cons = _masked_graph()
    masks = np.ones((2, len(cons)), dtype=np.uint8)
    masks[1, 61:] = 0                      # the poses behind the last enabled closure still hang on the odometry
    for got in pg.optimize(masks):
        assert got["iterations"] > 0
        assert got["poses"][-1].tobytes() == poses[-1].tobytes()      # isolated, -0.0 included
        assert got["poses"][0].tobytes() == poses[0].tobytes()        # fixed
        assert not np.array_equal(got["poses"][1:-1], poses[1:-1])
    # a node whose only constraint is switched off in the job is isolated in that job
    P = PC.problem("square")
    pg2 = PoseGraph(_matcher(), max_nodes=5, max_constraints=5, max_jobs=2)
    pg2.set_graph(np.vstack([P.poses, [[3.0, 3.0, 0.1]]]), begin=list(P.begin) + [0], end=list(P.end) + [4],
                  transform=np.vstack([P.transform, [[2.0, 2.0, 0.0]]]), information=np.vstack([P.information, [PC.INFO_FULL]]),
                  switchable=[False] * 4 + [True])
    on, off = pg2.optimize(np.array([[1, 1, 1, 1, 1], [1, 1, 1, 1, 0]], dtype=np.uint8))
    assert off["poses"][4].tobytes() == np.array([3.0, 3.0, 0.1]).tobytes() and not np.array_equal(on["poses"][4], off["poses"][4])
    pg2.close()


def test_stop_rules():
    pg = _graph("square")
    one = pg.optimize(max_iterations=1, gradient_tolerance=0.0, function_tolerance=0.0, parameter_tolerance=0.0)[0]
    assert one["status"] == _capi.POSEGRAPH_MAX_ITERATIONS and one["iterations"] == 1 and one["final_cost"] < one["initial_cost"]
    default = pg.optimize()[0]
    print("default tolerances on the square: %s after %d iterations" % (default["status_name"], default["iterations"]))
    assert default["status"] == _capi.POSEGRAPH_CONVERGED_COST
    step = pg.optimize(gradient_tolerance=0.0, function_tolerance=0.0, parameter_tolerance=1e-3)[0]
    assert step["status"] == _capi.POSEGRAPH_CONVERGED_STEP
    none = pg.optimize(max_iterations=0)[0]
    assert none["status"] == _capi.POSEGRAPH_MAX_ITERATIONS and none["iterations"] == 0
    assert np.array_equal(none["poses"], PC.problem("square").poses)


def test_degenerate_graphs_are_legal():
    pg = PoseGraph(_matcher(), max_nodes=4, max_constraints=4, max_jobs=2)
    pg.set_graph([[1.0, 2.0, 3.0]])                                   # n == 1
    got = pg.optimize()[0]
    assert got["status"] == _capi.POSEGRAPH_CONVERGED_GRADIENT and got["iterations"] == 0 and np.array_equal(got["poses"], [[1.0, 2.0, 3.0]])
    pg.set_graph([[1.0, 2.0, 3.0], [0.0, 1.0, -0.0]])                 # m == 0
    got = pg.optimize()[0]
    assert got["status"] == _capi.POSEGRAPH_CONVERGED_GRADIENT and got["poses"].tobytes() == np.array([[1.0, 2.0, 3.0], [0.0, 1.0, -0.0]]).tobytes()
    assert pg.evaluate()[0]["cost"] == 0.0
    L = pg._L
    assert L.ndt2d_posegraph_solve(pg._p, None, 0, 100, 0.0, 0.0, 0.0, None, None, None) == _capi.OK     # n_jobs == 0
    assert L.ndt2d_posegraph_evaluate(pg._p, None, 0, None, None, None) == _capi.OK
    pg.close()


def test_refusals_name_the_index_and_the_handle_stays_usable():
    import torch
    P = PC.problem("square")
    pg = PoseGraph(_matcher(), max_nodes=4, max_constraints=4, max_jobs=2)
    fresh = PoseGraph(_matcher(), max_nodes=4, max_constraints=4, max_jobs=2)
    with pytest.raises(Ndt2dError, match="no graph") as ei:
        fresh.optimize()
    assert ei.value.code == _capi.ERR_STATE
    fresh.close()
    good = dict(begin=P.begin, end=P.end, transform=P.transform, information=P.information)
    pg.set_graph(P.poses, **good)
    want = pg.optimize()[0]

    def refused(text, poses=P.poses, fixed=0, **change):
        with pytest.raises(Ndt2dError, match=text) as ei:
            pg.set_graph(poses, fixed=fixed, **dict(good, **change))
        assert ei.value.code == _capi.ERR_INVALID

    bad = P.poses.copy()
    bad[2, 1] = np.nan
    refused("pose 2 is not finite", poses=bad)
    refused("fixed pose 4 of 4", fixed=4)
    refused("constraint 1 names pose 7 of 4", end=[1, 7, 3, 0])
    refused("constraint 3 begins and ends at pose 3", end=[1, 2, 3, 3])
    t = P.transform.copy()
    t[2, 2] = np.inf
    refused("constraint 2: its transform is not finite", transform=t)
    info = P.information.copy()
    info[1, 0, 0] = np.nan
    refused("constraint 1: its information is not finite", information=info)
    info = P.information.copy()
    info[3] = 0.0                                                     # Constraint()'s default zeros
    refused("constraint 3: its information is not symmetric positive definite", information=info)
    info = P.information.copy()
    info[0] = [[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]     # symmetric, indefinite
    refused("constraint 0: its information is not symmetric positive definite", information=info)
    L = pg._L
    u32 = np.zeros(8, dtype=np.uint32)
    from ndt_2d_amd._capi import dptr
    import ctypes as C
    u32p = u32.ctypes.data_as(C.POINTER(C.c_uint32))
    five = np.zeros((5, 3))
    assert L.ndt2d_posegraph_set_graph(pg._p, dptr(five), 0, u32p, u32p, dptr(five), dptr(five), 0, 0) == _capi.ERR_INVALID
    assert b"no poses" in L.ndt2d_posegraph_last_error(pg._p)
    assert L.ndt2d_posegraph_set_graph(pg._p, dptr(five), 5, u32p, u32p, dptr(five), dptr(five), 0, 0) == _capi.ERR_INVALID
    assert b"5 poses, the capacity is 4" in L.ndt2d_posegraph_last_error(pg._p)
    many = np.tile(np.eye(3).reshape(9), (5, 1))
    assert L.ndt2d_posegraph_set_graph(pg._p, dptr(five), 4, u32p, u32p, dptr(five), dptr(many), 5, 0) == _capi.ERR_INVALID
    assert b"5 constraints, the capacity is 4" in L.ndt2d_posegraph_last_error(pg._p)
    with pytest.raises(Ndt2dError, match="weighting"):
        pg.set_weighting("sqrt")
    with pytest.raises(Ndt2dError, match="tolerance"):
        pg.optimize(gradient_tolerance=-1.0)
    with pytest.raises(ValueError, match="mask 0 switches off constraint 2, which is not switchable"):
        pg.optimize(np.array([[1, 1, 0, 1]]))
    # the graph in place is the last one accepted, and the handle works -- on a caller's stream too
    got = pg.optimize()[0]
    for key in want:
        assert np.array_equal(got[key], want[key]), key
    m = _matcher()
    stream = torch.cuda.Stream()
    m.set_stream(stream.cuda_stream)
    try:
        got = pg.optimize()[0]
        pg.set_timing(True)
        timed = pg.optimize()[0]
        kernel_ms, fetch_ms = pg.last_ms()
        assert kernel_ms > 0.0 and fetch_ms >= 0.0
    finally:
        m.set_stream(None)
    for key in want:
        assert np.array_equal(got[key], want[key]) and np.array_equal(timed[key], want[key]), key
    pg.close()


def test_end_to_end_from_close_loops_to_optimised_poses():
    """close_loops on tests/test_gpu_closure.py's synthetic world, closure_constraints on what it
    accepted, Graph.optimize: usable poses come back and the cost does not rise."""
    g = CC.graph()
    m = ScanMatcherNDT(0)
    try:
        m.initialize("posegraph", **CC.case(0.25)["params"])
        for i, pts in enumerate(g["points"]):
            assert m.storeScan(pts) == i
        rolling, limit = 8, 4
        window = lambda i: [(j, g["poses"][j]) for j in loop_closure_window(i, rolling)]      # noqa: E731
        cand_idx = [2, 4, 6, 8]
        first = [r["score"] for r in m.matchCandidates(g["guess"], g["query"], [window(i) for i in cand_idx])]
        typical = 0.5 * (sorted(first)[0] + sorted(first)[1])
        pose, accepted = close_loops(m, g["guess"], g["query"], cand_idx, g["poses"], rolling, typical, limit,
                                     scan_sizes=[len(p) for p in g["points"]], refine=dict(neighbourhood=9))
        assert accepted
        graph = graph_io.Graph(False)
        for i, (p, pts) in enumerate(zip(g["poses"], g["points"])):
            graph.scans.append(graph_io.Scan(i, p, pts))
        new = len(graph.scans)
        graph.scans.append(graph_io.Scan(new, pose, g["query"]))
        odometry = np.diag([0.01, 0.01, 0.0025])
        for i in range(new):
            to = graph.scans[i + 1].pose if i + 1 < new else g["guess"]       # the new scan's odometry says `guess`
            graph.constraints.append(make_constraint(i, i + 1, graph.scans[i].pose, to, odometry))
        closures = closure_constraints(accepted, new, g["poses"])
        assert len(closures) == len(accepted) and all(c.switchable and c.end == new for c in closures)
        graph.constraints.extend(closures)
        before = np.array([s.pose for s in graph.scans])
        assert graph.optimize(m) is True
        rec = graph.last_optimize
        print("end to end: %d closure(s), %s after %d iterations, F %.6e -> %.6e" %
              (len(closures), rec["status_name"], rec["iterations"], rec["initial_cost"], rec["final_cost"]))
        after = np.array([s.pose for s in graph.scans])
        assert rec["status"] != _capi.POSEGRAPH_FAILED and rec["final_cost"] <= rec["initial_cost"]
        assert np.all(np.isfinite(after)) and np.array_equal(after[0], before[0]) and np.array_equal(after, rec["poses"])
        assert graph_io.Graph(False).optimize(m) is False                     # no scans: the reference returns false
    finally:
        m.close()
