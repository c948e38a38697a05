"""Marginal covariances of the pose graph on the device (ndt2d_marginals_columns, PoseGraph.marginals)
against the numpy restatement (tests/posegraph_marginals_restatement.py) on the designed graphs of
the pose-graph tests, each at the restatement's own solution.

The gates, per column, both against the restatement and never against the device
(tests/posegraph_marginals_cases.py): the TRUE residual |A x_dev - e_j|_2, A restated densely, is
<= gate = tolerance + 100 x (the gap the restatement's own CG leaves between its true and its
recurrence residual), and max|Sigma_dev - Sigma_ref| <= |A^-1|_inf (gate + |A Sigma_ref - I|_max),
the first-order bound with the dense inverse's own defect as its floor.  For graphs outside the
table (masks, losses, the floating squares) the gate is formed by the same rule at run time."""
import math

import numpy as np
import pytest

import closure_refine_cases as CC
import posegraph_cases as PC
import posegraph_marginals_cases as MC
import posegraph_marginals_restatement as MR
import posegraph_restatement as R
import posegraph_robust_cases as RC
import posegraph_robust_restatement as RR
from ndt_2d_amd import (Ndt2dError, PoseGraph, ScanMatcherNDT, _capi, close_loops, closure_constraints, closure_distance, graph_io,
                        loop_closure_window, make_constraint, relative_covariance)

pytestmark = pytest.mark.gpu

TOL = MC.TOLERANCE
CHI2_3_999 = 16.27
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


def _upload(P, x, key, max_jobs=8, switchable=None):
    """A PoseGraph holding Problem P at the poses x (one per key for the module)."""
    graphs = _STATE.setdefault("graphs", {})
    if key not in graphs:
        pg = PoseGraph(_matcher(), max_nodes=P.n, max_constraints=max(1, P.m), max_jobs=max_jobs)
        pg.set_weighting(P.weighting)
        pg.set_graph(x, begin=P.begin, end=P.end, transform=P.transform, information=P.information, fixed=P.fixed,
                     switchable=np.ones(P.m, dtype=bool) if switchable is None else switchable)
        graphs[key] = pg
    return graphs[key]


def _graph(name, prec):
    P, x = MC.case(name)
    pg = _upload(P, x, name)
    pg.set_preconditioner(prec)
    return pg


def _run_time_gate(S, nodes, prec):
    """The table's rule for a system outside it: tolerance + 100 x the restatement CG's gap, rounded up."""
    free = sorted({int(q) for q in nodes if S.node_free(q)})
    got = S.pcg(free, "jacobi" if prec == "jacobi" else "band", TOL)
    assert np.all(got["status"] == MR.CONVERGED)
    return MC.round_up(TOL + 100.0 * float(np.max(np.abs(got["true"] - got["recurrence"]))))


def _check(label, S, nodes, got, gate):
    """One job's result against the dense system S: statuses, both gates per column, the blocks
    against the columns, the joint's symmetry and definiteness.  Returns the bound on a value."""
    bound = S.inverse_norm() * (gate + S.defect())
    worst_res, worst_err = 0.0, 0.0
    for i, node in enumerate(nodes):
        col = got["columns"][i]
        if S.node_free(node):
            assert got["status"][i] == _capi.MARGINALS_CONVERGED, (label, node, got["status"][i])
            assert np.all(got["residuals"][i] <= TOL) and got["cg_iterations"][i] >= 1
            res = float(np.max(S.true_residual(node, col)))
            err = float(np.max(np.abs(col - S.column(node))))
            worst_res, worst_err = max(worst_res, res), max(worst_err, err)
            assert res <= gate, (label, node, res, gate)
            assert err <= bound, (label, node, err, bound)
        else:
            assert got["status"][i] == _capi.MARGINALS_NOT_FREE, (label, node, got["status"][i])
            assert np.all(col == 0.0) and np.all(got["residuals"][i] == 0.0) and got["cg_iterations"][i] == 0
        for j, other in enumerate(nodes):
            assert np.array_equal(got["blocks"][j, i], col[other]), (label, node, other)       # block (j, i): rows of q_j in the column of q_i
    Q = len(nodes)
    joint = got["blocks"].transpose(0, 2, 1, 3).reshape(3 * Q, 3 * Q)
    assert np.max(np.abs(joint - joint.T)) <= 2.0 * bound, (label, np.max(np.abs(joint - joint.T)), bound)
    assert np.min(np.linalg.eigvalsh(0.5 * (joint + joint.T))) >= -bound
    print("%s: true residual <= %.2e (gate %.0e), |Sigma - Sigma_ref| <= %.2e (bound %.2e), %d lockstep iterations at the most"
          % (label, worst_res, gate, worst_err, bound, int(np.max(got["cg_iterations"]))))
    return bound


@pytest.mark.parametrize("prec", MC.PRECONDITIONERS)
@pytest.mark.parametrize("name", MC.SMALL)
def test_values_against_the_dense_inverse(name, prec):
    pg, S, nodes = _graph(name, prec), MC.system(name), MC.queries(name)
    got = pg.marginals(nodes, tolerance=TOL, want_columns=True)[0]
    bound = _check("%s %s" % (name, prec), S, nodes, got, MC.gate(name, prec))
    if name == "line":
        # the known answer: a grounded resistor chain (tests/test_posegraph_marginals_restatement.py);
        # the poses are the restatement's solution, line_answer() to its own error
        n = 20
        every = pg.marginals(list(range(1, n + 1)), tolerance=TOL)[0]
        for i in range(1, n + 1):
            want = i * (n + 1 - i) / (100.0 * (n + 1))
            assert abs(every["blocks"][i - 1, i - 1, 0, 0] - want) <= bound + 1e-12 * want, (i, every["blocks"][i - 1, i - 1, 0, 0], want)


@pytest.mark.parametrize("name", MC.THOUSAND)
def test_ownership_edges_on_the_thousand_pose_loops(name):
    """1,023 / 1,024 / 1,025 poses: one node a thread, and a thread's second node at 1,025."""
    S, nodes = MC.system(name), MC.queries(name)
    its = {}
    for prec in MC.PRECONDITIONERS:
        got = _graph(name, prec).marginals(nodes, tolerance=TOL, want_columns=True)[0]
        _check("%s %s" % (name, prec), S, nodes, got, MC.gate(name, prec))
        its[prec] = int(np.max(got["cg_iterations"]))
        assert its[prec] <= MR.cg_cap(MC.size(name))
    print("%s: %d iterations under \"jacobi\" (the restatement: %d), %d under \"chain\" (%d)"
          % (name, its["jacobi"], MC.GATES[(name, "jacobi")][2], its["chain"], MC.GATES[(name, "chain")][2]))
    assert its["chain"] <= its["jacobi"]


@pytest.mark.parametrize("name", MC.CHAIN)
def test_the_chains_level_edges(name):
    """The reduction's level edges, a chain cut at the fixed node, edges reversed, doubled and
    missing, an isolated node as query (NOT_FREE), and 1,025 nodes."""
    S, nodes = MC.system(name), MC.queries(name)
    got = _graph(name, "chain").marginals(nodes, tolerance=TOL, want_columns=True)[0]
    _check("%s chain" % name, S, nodes, got, MC.gate(name, "chain"))
    if name == "isolated":
        assert got["status"][nodes.index(11)] == _capi.MARGINALS_NOT_FREE


def test_lockstep_freezing_leaves_each_column_its_own_bits():
    """hub's spoke 1 under "jacobi": its three columns stop at three different iterations in the
    restatement.  Each column's residual is within the tolerance, and each is, bit for bit, what
    it is when the node is queried in another call among other nodes."""
    S, node = MC.system("hub"), MC.FREEZE_NODE
    restated = S.pcg([node], "jacobi", TOL)["iterations"][0]
    assert len(set(restated.tolist())) == 3
    pg = _graph("hub", "jacobi")
    alone = pg.marginals([node], tolerance=TOL, want_columns=True)[0]
    among = pg.marginals([7, 150, node, 299, 0], tolerance=TOL, want_columns=True)[0]
    print("hub node %d: restated iterations %s, lockstep iterations on the device %d; |r| %s"
          % (node, restated.tolist(), alone["cg_iterations"][0], alone["residuals"][0].tolist()))
    assert alone["status"][0] == _capi.MARGINALS_CONVERGED and np.all(alone["residuals"][0] <= TOL)
    assert np.array_equal(alone["columns"][0], among["columns"][2]) and np.array_equal(alone["residuals"][0], among["residuals"][2])
    assert alone["cg_iterations"][0] == among["cg_iterations"][2]
    _check("hub jacobi, node %d" % node, S, [node], alone, MC.gate("hub", "jacobi"))


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name,prec", [("hub", "jacobi"), ("loop_1025", "jacobi"), ("loop_1025", "chain")])
def test_the_two_forms_of_a_chunk_give_the_same_bits(name, prec):
    """A chunk of few pairs runs three workgroups a pair with one column each, a chunk of more
    pairs than a third of the device's compute units one workgroup a pair with its three columns in
    lockstep (include/ndt2d_hip.h).  The same queries both ways: every column, residual, iteration
    count and status array_equal; and the lockstep form's values against the dense inverse."""
    import torch
    units = torch.cuda.get_device_properties(0).multi_processor_count
    P, x = MC.case(name)
    S, few_nodes = MC.system(name), MC.queries(name)
    count = units // 3 + 20
    assert count < P.n
    nodes = sorted(set(np.linspace(0, P.n - 1, count).astype(int).tolist()) | set(few_nodes) | {MC.FREEZE_NODE})
    pg = _upload(P, x, name + "_many_jobs", max_jobs=len(nodes))
    pg.set_preconditioner(prec)
    many = pg.marginals(nodes, tolerance=TOL, want_columns=True)[0]                 # 3 x pairs > units: lockstep
    few = pg.marginals(few_nodes, tolerance=TOL, want_columns=True)[0]              # 3 x pairs <= units: a column a workgroup
    assert 3 * len(nodes) > units >= 3 * len(few_nodes)
    for i, node in enumerate(few_nodes):
        at = nodes.index(node)
        assert np.array_equal(few["columns"][i], many["columns"][at]) and np.array_equal(few["residuals"][i], many["residuals"][at]), node
        assert few["cg_iterations"][i] == many["cg_iterations"][at] and few["status"][i] == many["status"][at], node
    # The values of the lockstep form against the dense inverse, on the queries the case's gate was
    # measured for.  (Further out the gap behind the gate grows with the column: at node 157 of
    # loop_1025, 355 nodes from the fixed one, the restatement's own CG stops at a recurrence
    # residual of 9.98e-11 with a true one of 2.18e-10, and the device has 2.12e-10.)
    at = [nodes.index(q) for q in few_nodes]
    sub = dict(columns=many["columns"][at], status=many["status"][at], residuals=many["residuals"][at], cg_iterations=many["cg_iterations"][at],
               blocks=many["blocks"][np.ix_(at, at)])
    _check("%s %s, among %d queries in lockstep" % (name, prec, len(nodes)), S, few_nodes, sub, MC.gate(name, prec))
    assert np.all(many["status"][[S.node_free(q) for q in nodes]] == _capi.MARGINALS_CONVERGED)


@pytest.mark.parametrize("prec", MC.PRECONDITIONERS)
def test_determinism(prec):
    P, x = MC.case("wrap")
    pg = _graph("wrap", prec)
    eight = [5, 1, 23, 12, 7, 19, 2, 16]
    first = pg.marginals(eight, tolerance=TOL, want_columns=True)[0]
    again = pg.marginals(eight, tolerance=TOL, want_columns=True)[0]
    assert _same(first, again)                                                      # the same call twice
    alone = pg.marginals([12], tolerance=TOL, want_columns=True)[0]
    backwards = pg.marginals(eight[::-1], tolerance=TOL, want_columns=True)[0]
    for got, at in ((first, 3), (backwards, 4)):                                    # alone, among seven others, the list reversed
        assert np.array_equal(alone["columns"][0], got["columns"][at]) and np.array_equal(alone["residuals"][0], got["residuals"][at])
        assert alone["cg_iterations"][0] == got["cg_iterations"][at] and np.array_equal(alone["blocks"][0, 0], got["blocks"][at, at])
    twice = pg.marginals([12, 5, 12], tolerance=TOL, want_columns=True)[0]          # duplicates equal each other
    assert np.array_equal(twice["columns"][0], twice["columns"][2]) and np.array_equal(twice["columns"][0], alone["columns"][0])
    assert np.array_equal(twice["blocks"][0, 0], twice["blocks"][2, 2]) and np.array_equal(twice["blocks"][0, 2], twice["blocks"][0, 0])
    # chunking: the (job, query) pairs through an object of max_jobs = 2 against max_jobs = 8 -- 1 x 5, 5 x 1 and 3 x 3
    masks = np.ones((5, P.m), dtype=np.uint8)
    closures = np.nonzero(np.abs(P.begin - P.end) != 1)[0]
    for k in range(1, 5):
        masks[k, closures[k - 1]] = 0
    small = _upload(P, x, "wrap_two_jobs", max_jobs=2)
    small.set_preconditioner(prec)
    for nodes, en in (([3, 9, 12, 20, 23], None), ([12], masks), ([3, 12, 23], masks[:3])):
        a = small.marginals(nodes, masks=en, tolerance=TOL, want_columns=True)
        b = pg.marginals(nodes, masks=en, tolerance=TOL, want_columns=True)
        assert len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    # a mask alone against among five masks
    five = pg.marginals([3, 12], masks=masks, tolerance=TOL, want_columns=True)
    one = pg.marginals([3, 12], masks=masks[2:3], tolerance=TOL, want_columns=True)[0]
    assert _same(one, five[2]) and not np.array_equal(five[0]["blocks"], five[2]["blocks"])
    # poses = solve's poses_out against set_graph(those poses) with poses = None
    start = _upload(P, P.poses, "wrap_at_start")
    start.set_preconditioner(prec)
    solved = start.optimize(max_iterations=200, gradient_tolerance=PC.gate("wrap"), function_tolerance=0.0, parameter_tolerance=0.0)[0]["poses"]
    given = start.marginals(eight, poses=solved[None], tolerance=TOL, want_columns=True)[0]
    there = PoseGraph(_matcher(), max_nodes=P.n, max_constraints=P.m, max_jobs=8)
    try:
        there.set_weighting(P.weighting)
        there.set_preconditioner(prec)
        there.set_graph(solved, begin=P.begin, end=P.end, transform=P.transform, information=P.information, fixed=P.fixed)
        assert _same(given, there.marginals(eight, tolerance=TOL, want_columns=True)[0])
    finally:
        there.close()


@pytest.mark.parametrize("case", RC.CASES)
def test_masks_change_h_and_sigma(case):
    """Closures off: H changes, and so must Sigma -- each job against the restatement under its mask."""
    g = RC.graph(case)[0]
    P = R.Problem(**g)
    x = P.poses
    closures = RC.closures(case)
    pg = _upload(P, x, "masks_" + case, switchable=closures)
    pg.set_preconditioner("jacobi")
    masks = np.ones((2, P.m), dtype=np.uint8)
    masks[1, closures] = 0
    nodes = [1, P.n // 2, P.n - 1, 0]
    got = pg.marginals(nodes, masks=masks, tolerance=TOL, want_columns=True)
    bounds = []
    for k in range(2):
        S = MR.System(P, x, enabled=masks[k])
        bounds.append(_check("%s, closures %s" % (case, "off" if k else "on"), S, nodes, got[k], _run_time_gate(S, nodes, "jacobi")))
    assert np.max(np.abs(got[0]["blocks"] - got[1]["blocks"])) > bounds[0] + bounds[1]


@pytest.mark.parametrize("prec", MC.PRECONDITIONERS)
@pytest.mark.parametrize("loss", RC.LOSSES)
def test_losses_reweight_h(loss, prec):
    """Huber and Cauchy on the closures of loop40 at its start poses, where the false closure is far
    out (rho' < 1): Sigma against the restatement's reweighted H, and away from the unweighted one."""
    g = RC.graph("loop40")[0]
    closures = RC.closures("loop40")
    P = RR.Problem(loss=loss, scale=RC.SCALE, robust=closures, **g)
    x = P.poses
    assert np.min(P.weights(x)) < 0.5 and np.all(P.weights(x)[~closures] == 1.0)
    graphs = _STATE.setdefault("graphs", {})
    key = "loss_" + loss
    if key not in graphs:
        pg = PoseGraph(_matcher(), max_nodes=P.n, max_constraints=P.m, max_jobs=8)
        pg.set_loss(loss, RC.SCALE, "switchable")
        pg.set_graph(x, begin=P.begin, end=P.end, transform=P.transform, information=P.information, fixed=P.fixed, switchable=closures)
        graphs[key] = pg
    pg = graphs[key]
    pg.set_preconditioner(prec)
    nodes = [1, 20, 39, 0]
    got = pg.marginals(nodes, tolerance=TOL, want_columns=True)[0]
    S = MR.System(P, x)
    bound = _check("loop40 %s %s" % (loss, prec), S, nodes, got, _run_time_gate(S, nodes, prec))
    plain = MR.System(R.Problem(**g), x)
    assert np.max(np.abs(got["blocks"] - plain.blocks(nodes))) > bound


def test_a_floating_component_with_and_without_damping():
    """Two squares, the second not joined to the fixed pose.  A query in the joined square converges
    and matches the dense pseudo-solution of its own component (H is block diagonal over the
    components); one in the floating square is not CONVERGED at damping = 0, with everything
    returned written; at damping = 1e-4 it converges and matches the damped dense inverse."""
    P, x = PC.problem("floating"), PC.solution("floating")["x"]
    pg = _upload(P, x, "floating")
    pg.set_preconditioner("jacobi")
    nodes = [2, 5, 0]
    got = pg.marginals(nodes, tolerance=TOL, want_columns=True)[0]
    joined = MR.System(R.Problem(x[:4], P.begin[:4], P.end[:4], P.transform[:4], P.information[:4]), x[:4])
    bound = joined.inverse_norm() * (_run_time_gate(joined, [2], "jacobi") + joined.defect())
    assert got["status"][0] == _capi.MARGINALS_CONVERGED and got["status"][2] == _capi.MARGINALS_NOT_FREE
    assert np.max(np.abs(got["columns"][0][:4] - joined.column(2))) <= bound and np.all(got["columns"][0][4:] == 0.0)
    assert got["status"][1] in (_capi.MARGINALS_CG_CAP, _capi.MARGINALS_BREAKDOWN)
    assert not np.any(got["residuals"][1] <= TOL) and got["cg_iterations"][1] >= 1
    assert np.array_equal(got["blocks"][:, 1], got["columns"][1][nodes], equal_nan=True)      # what is returned is what was computed
    assert np.all(got["columns"][1][:4] == 0.0)                                      # (nothing of it reaches the other component)
    print("floating, damping 0: node 5 ends %s after %d iterations, |r| %s" % (_capi.MARGINALS_STATUS_NAMES[got["status"][1]],
                                                                              got["cg_iterations"][1], got["residuals"][1].tolist()))
    damped = pg.marginals(nodes, damping=1e-4, tolerance=TOL, want_columns=True)[0]
    S = MR.System(P, x, damping=1e-4)
    _check("floating, damping 1e-4", S, nodes, damped, _run_time_gate(S, nodes, "jacobi"))


def _end_to_end_graph(m):
    """The graph tests/test_gpu_posegraph.py's end-to-end test builds: close_loops on the synthetic
    world, closure_constraints on what it accepted, the odometry chain."""
    g = CC.graph()
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
        to = graph.scans[i + 1].pose if i + 1 < new else g["guess"]
        graph.constraints.append(make_constraint(i, i + 1, graph.scans[i].pose, to, odometry))
    graph.constraints.extend(closure_constraints(accepted, new, g["poses"]))
    return graph, odometry


def test_the_mirrors_and_the_closure_verdicts():
    # relative_covariance and closure_distance on the verdict graph, against the restatement
    P, x, (a, b), cov_meas = MC.verdict_case()
    pg = _upload(P, x, "verdict")
    pg.set_preconditioner("chain")
    S = MR.System(P, x)
    bound = S.inverse_norm() * (_run_time_gate(S, [a, b], "chain") + S.defect())
    got = pg.relative_covariance(a, b, poses=x, tolerance=TOL)
    want_t, want_cov = MR.relative(math.cos(x[a, 2]), math.sin(x[a, 2]), x[a], x[b], S.blocks([a, b]))
    assert np.all(got["status"] == _capi.MARGINALS_CONVERGED)
    assert np.all(np.abs(got["transform"] - want_t) <= 4.0 * np.spacing(np.max(np.abs(want_t))))
    # |[A B]|_inf^2 x 36 entries: the blocks' bound carried through the product
    lever = (2.0 + np.max(np.abs(want_t[:2]))) ** 2 * 36.0
    assert np.max(np.abs(got["covariance"] - want_cov)) <= lever * bound
    t, cov = relative_covariance(x[a], x[b], got["joint"])
    assert np.array_equal(t, got["transform"]) and np.array_equal(cov, got["covariance"])
    same, shifted = closure_distance(t, cov, t, cov_meas), closure_distance(t, cov, t + np.array([1.0, 0.0, 0.0]), cov_meas)
    want_shifted = MR.distance(want_t, want_cov, want_t + np.array([1.0, 0.0, 0.0]), cov_meas)
    print("verdict graph: d2 %.3e for the prediction itself, %.2f for 1 m off (the restatement: %.2f)" % (same, shifted, want_shifted))
    assert same == 0.0 and shifted > CHI2_3_999 and abs(shifted - want_shifted) <= 1e-6 * want_shifted
    # Graph.closure_distances on the close_loops -> closure_constraints graph
    m = ScanMatcherNDT(0)
    try:
        graph, odometry = _end_to_end_graph(m)
        assert graph.optimize(m, weighting="information") is True
        new = len(graph.scans) - 1
        # a closure made consistent with the graph: what the optimised poses themselves say of the
        # neighbours (new - 1, new), with the odometry's covariance; and the same shifted by 1 m in x.
        # The predicted covariance is at most the odometry constraint's own, so 1 m is >= 7 sigma.
        consistent = make_constraint(new - 1, new, graph.scans[new - 1].pose, graph.scans[new].pose, odometry)
        off = graph_io.Constraint(new - 1, new, np.array(consistent.transform) + np.array([1.0, 0.0, 0.0]), consistent.information, switchable=True)
        d2 = graph.closure_distances(m, [consistent, off, consistent])
        print("end to end: d2 %.3e for a consistent closure, %.1f for 1 m off; statuses %s" % (d2[0], d2[1], graph.last_closure_distances["status"]))
        assert np.all(graph.last_closure_distances["status"] == _capi.MARGINALS_CONVERGED)
        assert d2[0] < CHI2_3_999 < d2[1] and d2[0] == d2[2] and d2[0] <= 1e-12
        assert graph.closure_distances(m, []) == []
    finally:
        m.close()


def test_refusals_the_stop_rules_and_a_callers_stream():
    import ctypes as C
    import torch
    P, x = MC.case("square")
    fresh = PoseGraph(_matcher(), max_nodes=4, max_constraints=4, max_jobs=2)
    try:
        with pytest.raises(Ndt2dError, match="no graph") as ei:
            fresh.marginals([1])
        assert ei.value.code == _capi.ERR_STATE
    finally:
        fresh.close()
    pg = _graph("square", "jacobi")
    want = pg.marginals([1, 3], tolerance=TOL, want_columns=True)[0]

    def refused(text, nodes=(1, 3), **kw):
        with pytest.raises(Ndt2dError, match=text) as ei:
            pg.marginals(list(nodes), **kw)
        assert ei.value.code == _capi.ERR_INVALID

    refused("query 1 names node 4 of 4", nodes=(1, 4))
    bad = np.tile(x, (1, 1, 1))
    bad[0, 2, 1] = np.inf
    refused("job 0 pose 2 is not finite", poses=bad)
    refused("damping", damping=-1e-9)
    refused("damping", damping=math.nan)
    refused("tolerance", tolerance=0.0)
    refused("tolerance", tolerance=math.inf)
    L, d = pg._L, _capi.dptr
    z = np.zeros(64)
    u = np.array([1, 3], dtype=np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))
    assert L.ndt2d_marginals_columns(pg._p, None, 1, None, None, 2, 0.0, TOL, 0, d(z), None, d(z)) == _capi.ERR_INVALID       # NULL nodes
    assert L.ndt2d_marginals_columns(pg._p, None, 1, None, u, 2, 0.0, TOL, 0, None, None, d(z)) == _capi.ERR_INVALID
    assert L.ndt2d_marginals_columns(pg._p, None, 1, None, None, 0, 0.0, TOL, 0, None, None, None) == _capi.OK                # Q == 0
    assert L.ndt2d_marginals_columns(pg._p, None, 0, None, u, 2, 0.0, TOL, 0, None, None, None) == _capi.OK                   # n_jobs == 0
    with pytest.raises(ValueError, match="mask 0 switches off"):
        _upload(P, x, "square_fixed_masks", switchable=np.zeros(P.m, dtype=bool)).marginals([1], masks=np.array([[1, 1, 0, 1]]))
    assert _same(pg.marginals([1, 3], tolerance=TOL, want_columns=True)[0], want)       # the handle works as before
    # the stop rules, on loop_1023
    big = _graph("loop_1023", "jacobi")
    capped = big.marginals([500], tolerance=TOL, max_cg_iterations=3)[0]
    assert capped["status"][0] == _capi.MARGINALS_CG_CAP and capped["cg_iterations"][0] == 3 and np.all(capped["residuals"][0] > TOL)
    loose = big.marginals([500], tolerance=1.0)[0]
    assert loose["status"][0] == _capi.MARGINALS_CONVERGED and loose["cg_iterations"][0] == 1 and np.all(loose["residuals"][0] <= 1.0)
    # a caller's stream, timed
    m = _matcher()
    stream = torch.cuda.Stream()
    m.set_stream(stream.cuda_stream)
    try:
        got = pg.marginals([1, 3], tolerance=TOL, want_columns=True)[0]
        pg.set_timing(True)
        timed = pg.marginals([1, 3], tolerance=TOL, want_columns=True)[0]
        kernel_ms, fetch_ms = pg.last_ms()
        assert kernel_ms > 0.0 and fetch_ms >= 0.0
    finally:
        pg.set_timing(False)
        m.set_stream(None)
    assert _same(got, want) and _same(timed, want)
