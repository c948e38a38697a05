"""The pose graph's robust losses on the device (PoseGraph.set_loss; include/ndt2d_hip.h, "Robust
losses") against the numpy restatement (tests/posegraph_robust_restatement.py) on the designed
graphs of tests/posegraph_robust_cases.py, each with one planted false closure.

The bounds are tests/test_gpu_posegraph.py's, on the robust F and its gradient: evaluate's cost
within 1e-12 max(1, |value|), chi2 bit for bit what the trivial loss gives; solve: CONVERGED_GRADIENT
at the case's gate (100 x the restatement's own |g|_inf floor) with the other rules off, the
restated robust |g(x_dev)|_inf <= 2 gates, |x_dev - x*|_inf <= 2 |H_true(x*)^-1|_inf (gate +
|g(x*)|_inf) with H_true the true Hessian of F (the rho'' term included), final_cost within 1e-9
relative of F(x*), the weights rho' < 0.1 on the false closure and > 0.9 elsewhere (the CPU test
holds the restatement to the same), and the trivial loss on the same graph at least 3 x as far
from the ground truth: a loss cuts the false closure's pull |r| >= 10 scales to at most one scale,
and the CPU test holds the restatement to that factor too.  The 1,025-pose chain and the hub have
no dense restated solve here (the suite stays quick): their gates, 100 x the restatement's floors
as well, are held to the restatement in the CPU suite, and what is compared here is the restated
gradient, cost and weights at the device's poses."""
import numpy as np
import pytest

import closure_refine_cases as CC
import posegraph_cases as PC
import posegraph_robust_cases as RC
import posegraph_robust_restatement as RR
from ndt_2d_amd import Ndt2dError, PoseGraph, ScanMatcherNDT, _capi, close_loops, closure_constraints, graph_io, loop_closure_window, make_constraint

pytestmark = pytest.mark.gpu

PARITY = 1e-12
RULES_OFF = dict(max_iterations=200, function_tolerance=0.0, parameter_tolerance=0.0)
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


def _new(g, max_jobs=8, switchable=None, weighting="reference"):
    pg = PoseGraph(_matcher(), max_nodes=len(g["poses"]), max_constraints=max(1, len(g["begin"])), max_jobs=max_jobs)
    pg.set_weighting(weighting)
    pg.set_graph(g["poses"], begin=g["begin"], end=g["end"], transform=g["transform"], information=g["information"], fixed=g.get("fixed", 0),
                 switchable=switchable)
    return pg


def _graph(case, weighting):
    """A PoseGraph holding the case under the weighting (one per pair for the module), the closures switchable."""
    graphs = _STATE.setdefault("graphs", {})
    if (case, weighting) not in graphs:
        graphs[(case, weighting)] = _new(RC.graph(case)[0], switchable=RC.closures(case), weighting=weighting)
    pg = graphs[(case, weighting)]
    pg.set_preconditioner("jacobi")
    return pg


def _within(got, want, bound=PARITY):
    got, want = np.asarray(got), np.asarray(want)
    return bool(np.all(np.abs(got - want) <= bound * np.maximum(1.0, np.abs(want))))


def _same(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert np.array_equal(a[key], b[key]), key


def _from_truth(case, poses):
    return float(np.max(np.abs(poses[:, :2] - RC.graph(case)[1][:, :2])))


# ---- evaluate ----

@pytest.mark.parametrize("loss", RC.LOSSES)
def test_evaluate_on_either_side_of_the_scale(loss):
    """Two poses, W = I, e = (a, 0, 0): chi2 is the double a * a, which is b -- Huber's quadratic
    branch, on its edge; with the pose one ulp further chi2 > b, the other branch."""
    a = 1.345
    for x in (a, np.nextafter(a, np.inf)):
        g = dict(poses=[[0.0, 0.0, 0.0], [x, 0.0, 0.0]], begin=[0], end=[1], transform=[[0.0, 0.0, 0.0]], information=[np.eye(3)])
        pg = _new(g)
        try:
            plain = pg.evaluate(want_residuals=True)[0]
            assert plain["e"].tolist() == [[x, 0.0, 0.0]] and plain["chi2"][0] == x * x and (plain["chi2"][0] <= a * a) == (x == a)
            pg.set_loss(loss, a)
            got = pg.evaluate()[0]
            want = RR.Problem(loss=loss, scale=a, **g).cost(g["poses"])
            print("%s at chi2 = b%s: F %.17g (restatement %.17g, trivial %.17g)" % (loss, "" if x == a else " + an ulp", got["cost"], want,
                                                                                     plain["cost"]))
            assert _within(got["cost"], want)
            assert np.array_equal(got["chi2"], plain["chi2"])
            if loss == "huber" and x == a:
                assert got["cost"] == plain["cost"]                          # rho = s on the edge, the same sum
        finally:
            pg.close()


@pytest.mark.parametrize("loss", RC.LOSSES)
def test_evaluate_on_the_square_with_masks_and_a_selection(loss):
    g = PC.square()
    pg = _new(g, switchable=[True] * 4)
    try:
        masks = np.array([[1, 1, 1, 1], [1, 0, 1, 1]], dtype=np.uint8)
        plain = pg.evaluate(masks)
        for scale, on in ((0.5, "all"), (0.05, "all"), (0.5, np.array([0, 0, 1, 1], dtype=np.uint8))):
            pg.set_loss(loss, scale, on)
            assert pg.loss() == (loss, scale)
            P = RR.Problem(loss=loss, scale=scale, robust=None if isinstance(on, str) else on, **g)
            got = pg.evaluate(masks)
            for k in range(2):
                want = P.cost(P.poses, masks[k])
                print("%s scale %g on %s, mask %d: F %.17g (restatement %.17g, trivial %.17g)" % (loss, scale, on, k, got[k]["cost"], want,
                                                                                                 plain[k]["cost"]))
                assert _within(got[k]["cost"], want) and got[k]["cost"] < plain[k]["cost"]
                assert np.array_equal(got[k]["chi2"], plain[k]["chi2"])
    finally:
        pg.close()


# ---- solve with a planted false closure ----

def _trivial(case, weighting):
    """The device's solve of the case under the trivial loss (once per case and weighting)."""
    key = ("trivial", case, weighting)
    if key not in _STATE:
        pg = _graph(case, weighting)
        pg.set_loss("trivial")
        _STATE[key] = pg.optimize(gradient_tolerance=1e-9, **RULES_OFF)[0]
    return _STATE[key]


@pytest.mark.parametrize("preconditioner", ["jacobi", "chain"])
@pytest.mark.parametrize("weighting", RC.WEIGHTINGS)
@pytest.mark.parametrize("loss", RC.LOSSES)
@pytest.mark.parametrize("case", RC.CASES)
def test_solve_leaves_the_false_closure_without_pull(case, loss, weighting, preconditioner):
    P, ref, gate = RC.problem(case, loss, weighting), RC.solution(case, loss, weighting), RC.gate(case, loss, weighting)
    false = RC.graph(case)[2]
    trivial = _trivial(case, weighting)
    pg = _graph(case, weighting)
    pg.set_preconditioner(preconditioner)
    pg.set_loss(loss, RC.SCALE)
    got = pg.optimize(gradient_tolerance=gate, **RULES_OFF)[0]
    restated = P.gradient_norm(got["poses"])
    bound = 2.0 * ref["inverse_norm"] * (gate + ref["gradient"])
    err = float(np.max(np.abs(got["poses"] - ref["x"])))
    far, far_trivial = _from_truth(case, got["poses"]), _from_truth(case, trivial["poses"])
    others = np.delete(got["weights"], false)
    print("%s %s %s %s: %s after %d iterations, %d CG; |g| device %.3e restated %.3e (gate %.1e); |x - x*| %.3e (bound %.3e); F %.12e -> %.12e "
          "(restatement %.12e); rho' false %.4f others >= %.4f; from the truth %.4f, trivial %.4f"
          % (case, loss, weighting, preconditioner, got["status_name"], got["iterations"], got["cg_iterations"], got["gradient"], restated, gate,
             err, bound, got["initial_cost"], got["final_cost"], ref["cost"], got["weights"][false], others.min(), far, far_trivial))
    assert got["status"] == _capi.POSEGRAPH_CONVERGED_GRADIENT
    assert restated <= 2.0 * gate
    assert err <= bound
    assert np.array_equal(got["poses"][P.fixed], P.poses[P.fixed])
    assert abs(got["final_cost"] - ref["cost"]) <= 1e-9 * ref["cost"]
    assert _within(got["initial_cost"], P.cost(P.poses)) and _within(got["final_cost"], P.cost(got["poses"]))
    assert _within(got["chi2_start"], P.residuals(P.poses)[2]) and _within(got["chi2"], P.residuals(got["poses"])[2])
    assert got["weights"][false] < 0.1 and others.min() > 0.9
    assert _within(got["weights"], P.weights(got["poses"]), 1e-9)
    assert trivial["status"] == _capi.POSEGRAPH_CONVERGED_GRADIENT and "weights" not in trivial
    assert 3.0 * far < far_trivial


# ---- the selection ----

def test_the_loss_on_the_closures_only_is_the_restatements_with_that_selection():
    case, loss, weighting = "loop40", "cauchy", "reference"
    sel = RC.closures(case)
    P = RC.problem(case, loss, weighting, robust=sel, key="closures")
    ref, gate = RC.solution(case, loss, weighting, robust=sel, key="closures"), RC.gate(case, loss, weighting)
    everywhere = RC.solution(case, loss, weighting)
    assert ref["gradient"] <= 0.1 * gate                                     # the case's gate serves this selection too
    pg = _graph(case, weighting)
    pg.set_loss(loss, RC.SCALE, on="switchable")
    got = pg.optimize(gradient_tolerance=gate, **RULES_OFF)[0]
    bound = 2.0 * ref["inverse_norm"] * (gate + ref["gradient"])
    err = float(np.max(np.abs(got["poses"] - ref["x"])))
    apart = float(np.max(np.abs(ref["x"] - everywhere["x"])))
    print("closures only: %s, |x - x*| %.3e (bound %.3e); the two selections' minimisers are %.3e apart" % (got["status_name"], err, bound, apart))
    assert got["status"] == _capi.POSEGRAPH_CONVERGED_GRADIENT and P.gradient_norm(got["poses"]) <= 2.0 * gate and err <= bound
    assert apart > 100.0 * bound                                             # (the selection is not a matter of rounding)
    assert abs(got["final_cost"] - ref["cost"]) <= 1e-9 * ref["cost"]
    assert np.all(got["weights"][~sel] == 1.0) and np.all(got["weights"][sel] < 1.0)
    # a byte array says the same
    pg.set_loss(loss, RC.SCALE, on=sel.astype(np.uint8))
    _same(pg.optimize(gradient_tolerance=gate, **RULES_OFF)[0], got)


def test_huber_on_a_constraint_that_stays_inside_changes_nothing():
    """Huber at scale 10 (b = 100) on the first odometry constraint alone, whose chi2 is 0 at the
    start and below 4 at the end of the trivial solve (2.8 in the restatement), 25 times inside b:
    rho = s and rho' = 1 on it throughout."""
    case, weighting = "loop40", "reference"
    trivial = _trivial(case, weighting)
    assert trivial["chi2_start"][0] < 4.0 and trivial["chi2"][0] < 4.0
    pg = _graph(case, weighting)
    on = np.zeros(pg.m, dtype=np.uint8)
    on[0] = 1
    pg.set_loss("huber", 10.0, on=on)
    got = pg.optimize(gradient_tolerance=1e-9, **RULES_OFF)[0]
    print("huber on an inlier alone: |dx| %.3e, bits %s" % (float(np.max(np.abs(got["poses"] - trivial["poses"]))),
                                                             "agree" if np.array_equal(got["poses"], trivial["poses"]) else "differ"))
    assert got["status"] == trivial["status"] and np.max(np.abs(got["poses"] - trivial["poses"])) <= 1e-12
    assert np.all(got["weights"] == 1.0)


# ---- the trivial loss ----

def test_trivial_is_an_object_without_a_loss_and_a_huge_scale_agrees():
    g = RC.graph("loop40")[0]
    never, pg = _new(g, switchable=RC.closures("loop40")), _new(g, switchable=RC.closures("loop40"))
    try:
        assert never.loss() == ("trivial", 1.0)
        want = never.optimize()[0]
        pg.set_loss("huber", 0.7)
        robust = pg.optimize()[0]
        assert not np.array_equal(robust["poses"], want["poses"])
        pg.set_loss("trivial")
        assert pg.loss() == ("trivial", 0.7)                                 # ("trivial" ignores the scale: the one in place stays)
        _same(pg.optimize()[0], want)
        _same(pg.evaluate()[0], never.evaluate()[0])
        # every chi2 <= b: Huber's quadratic branch everywhere
        pg.set_loss("huber", 1e6)
        huge = pg.optimize()[0]
        assert float(np.max(want["chi2_start"])) < 1e12 and np.all(huge.pop("weights") == 1.0)
        bits = all(np.array_equal(huge[key], want[key]) for key in want)
        print("huber at scale 1e6 against no loss: |dx| %.3e, the bits %s" % (float(np.max(np.abs(huge["poses"] - want["poses"]))),
                                                                              "agree" if bits else "differ"))
        assert np.max(np.abs(huge["poses"] - want["poses"])) <= 1e-12 and huge["status"] == want["status"]
        assert _within(huge["final_cost"], want["final_cost"])
    finally:
        never.close()
        pg.close()


def test_refusals_leave_the_setting_in_place():
    g = RC.graph("square")[0]
    pg = PoseGraph(_matcher(), max_nodes=4, max_constraints=4, max_jobs=2)
    try:
        assert pg._L.ndt2d_robust_select(pg._p, None, 0) == _capi.ERR_STATE  # before set_graph
        pg.set_loss("cauchy", 2.5)
        for kind, scale in (("tukey", 1.0), ("huber", 0.0), ("huber", -1.0), ("cauchy", np.inf), ("huber", np.nan)):
            with pytest.raises(Ndt2dError) as ei:
                pg.set_loss(kind, scale)
            assert ei.value.code == _capi.ERR_INVALID
            assert pg.loss() == ("cauchy", 2.5)
        pg.set_graph(g["poses"], begin=g["begin"], end=g["end"], transform=g["transform"], information=g["information"])
        assert pg.loss() == ("cauchy", 2.5)                                  # kept across set_graph
        three = np.ones(3, dtype=np.uint8)
        assert pg._L.ndt2d_robust_select(pg._p, pg._u8(three), 3) == _capi.ERR_INVALID
        with pytest.raises(ValueError):
            pg.set_loss("cauchy", 2.5, on=three)
        with pytest.raises(ValueError):
            pg.set_loss("cauchy", 2.5, on="closures")
        # set_graph resets the C object's selection to every constraint; the Python object applies its own again
        pg.set_loss("cauchy", 2.5, on=np.array([1, 0, 0, 0], dtype=np.uint8))   # (an odometry constraint: the false closure keeps rho = s)
        one = pg.evaluate()[0]["cost"]
        pg.set_graph(g["poses"], begin=g["begin"], end=g["end"], transform=g["transform"], information=g["information"])
        assert pg.evaluate()[0]["cost"] == one
        assert pg._L.ndt2d_posegraph_set_graph(pg._p, _capi.dptr(np.ascontiguousarray(g["poses"], dtype=np.float64)), 4,
                                               np.array(g["begin"], dtype=np.uint32).ctypes.data_as(_capi.C.POINTER(_capi.C.c_uint32)),
                                               np.array(g["end"], dtype=np.uint32).ctypes.data_as(_capi.C.POINTER(_capi.C.c_uint32)),
                                               _capi.dptr(np.ascontiguousarray(g["transform"], dtype=np.float64)),
                                               _capi.dptr(np.ascontiguousarray(g["information"], dtype=np.float64)), 4, 0) == _capi.OK
        every = pg.evaluate()[0]["cost"]
        pg.set_loss("cauchy", 2.5, on="all")
        assert every == pg.evaluate()[0]["cost"] and every < one
    finally:
        pg.close()


# ---- determinism ----

def test_jobs_are_independent_of_masks_chunks_and_runs():
    case = "loop40"
    g, _, false = RC.graph(case)
    sel = RC.closures(case)
    m = len(sel)
    closures = np.nonzero(sel)[0]
    masks = np.ones((5, m), dtype=np.uint8)
    masks[0, closures[0]] = 0
    masks[1, false] = 0
    masks[2, closures[2:]] = 0
    masks[3, closures[[0, 3]]] = 0                                           # (job 4 has every constraint on)
    wide, narrow = _new(g, max_jobs=8, switchable=sel), _new(g, max_jobs=2, switchable=sel)   # (five masks: one chunk, three chunks)
    try:
        for loss, preconditioner in (("huber", "jacobi"), ("cauchy", "chain")):
            for pg in (wide, narrow):
                pg.set_loss(loss, RC.SCALE)
                pg.set_preconditioner(preconditioner)
            five = wide.optimize(masks)
            assert all(r["iterations"] > 0 for r in five) and not np.array_equal(five[1]["poses"], five[4]["poses"])
            alone = wide.optimize(masks[[2]])[0]
            _same(alone, five[2])
            chunks = narrow.optimize(masks)                                  # job 2 is the first of the second chunk, job 4 alone in the third
            for a, b in zip(chunks, five):
                _same(a, b)
            _same(narrow.optimize(masks[[1, 2]])[1], five[2])                # ... and the second job of a chunk
            for a, b in zip(wide.optimize(masks), five):
                _same(a, b)
            ev = wide.evaluate(masks)
            for a, b in zip(narrow.evaluate(masks), ev):
                _same(a, b)
            assert [r["initial_cost"] for r in five] == [e["cost"] for e in ev]   # a solve's initial_cost is evaluate's F bit for bit
    finally:
        wide.close()
        narrow.close()


# ---- strides ----

@pytest.mark.parametrize("preconditioner", ["chain", "jacobi"])
def test_a_chain_of_1025_poses_and_1026_constraints_under_huber(preconditioner):
    """tests/posegraph_robust_cases.py's chain1025: the constraint loops wrap, and the wrapped
    constraints are the closures, the last of them false."""
    P, gate = RC.stride_problem("chain1025"), RC.STRIDES["chain1025"][3]
    assert P.n == 1025 and P.m == 1026
    graphs = _STATE.setdefault("graphs", {})
    if "chain_1025" not in graphs:
        graphs["chain_1025"] = _new(RC.chain1025(), max_jobs=1)
    pg = graphs["chain_1025"]
    pg.set_preconditioner(preconditioner)
    pg.set_loss("huber", RC.SCALE)
    got = pg.optimize(gradient_tolerance=gate, **RULES_OFF)[0]
    restated = P.gradient_norm(got["poses"])
    print("1,025 poses %s: %s after %d iterations, %d CG; |g| device %.3e restated %.3e; F %.12e -> %.12e; rho' of the closures %s"
          % (preconditioner, got["status_name"], got["iterations"], got["cg_iterations"], got["gradient"], restated, got["initial_cost"],
             got["final_cost"], got["weights"][-2:]))
    assert got["status"] == _capi.POSEGRAPH_CONVERGED_GRADIENT and restated <= 2.0 * gate
    assert _within(got["initial_cost"], P.cost(P.poses)) and _within(got["final_cost"], P.cost(got["poses"]))
    assert got["weights"][-1] < 0.2 and np.min(got["weights"][:-1]) > 0.9   # (the CPU suite holds the restatement to the same)
    assert _within(got["weights"], P.weights(got["poses"]), 1e-9)
    assert np.array_equal(got["poses"][0], P.poses[0])


def test_a_hub_of_degree_300_under_cauchy():
    g = PC.hub()
    P, gate = RC.stride_problem("hub"), RC.STRIDES["hub"][3]
    pg = _new(g, max_jobs=1)
    try:
        pg.set_loss("cauchy", 0.5)
        got = pg.optimize(gradient_tolerance=gate, **RULES_OFF)[0]
        restated = P.gradient_norm(got["poses"])
        print("hub: %s after %d iterations, %d CG; |g| device %.3e restated %.3e; F %.12e -> %.12e; rho' in [%.3f, %.3f]"
              % (got["status_name"], got["iterations"], got["cg_iterations"], got["gradient"], restated, got["initial_cost"], got["final_cost"],
                 got["weights"].min(), got["weights"].max()))
        assert got["status"] == _capi.POSEGRAPH_CONVERGED_GRADIENT and restated <= 2.0 * gate
        assert _within(got["initial_cost"], P.cost(P.poses)) and _within(got["final_cost"], P.cost(got["poses"]))
        assert got["weights"].min() < 0.9 and _within(got["weights"], P.weights(got["poses"]), 1e-9)
    finally:
        pg.close()


def test_an_isolated_node_and_the_fixed_node_keep_their_bits():
    g = RC.graph("loop40")[0]
    poses = np.vstack([g["poses"], [[9.0, -9.0, -0.0]]])                      # (the isolated pose, with a negative zero to keep)
    pg = _new(dict(g, poses=poses), switchable=RC.closures("loop40"))
    try:
        for loss, preconditioner in (("huber", "jacobi"), ("cauchy", "chain")):
            pg.set_loss(loss, RC.SCALE)
            pg.set_preconditioner(preconditioner)
            got = pg.optimize()[0]
            assert got["iterations"] > 0 and not np.array_equal(got["poses"][1:-1], poses[1:-1])
            assert got["poses"][-1].tobytes() == poses[-1].tobytes() and got["poses"][0].tobytes() == poses[0].tobytes()
    finally:
        pg.close()


# ---- Graph.optimize ----

def test_graph_optimize_with_a_loss_from_close_loops_to_optimised_poses():
    """tests/test_gpu_posegraph.py's end-to-end path with loss="huber": the loss is on the closures
    close_loops accepted (loss_on="switchable"), the record has their weights."""
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
            to = graph.scans[i + 1].pose if i + 1 < new else g["guess"]
            graph.constraints.append(make_constraint(i, i + 1, graph.scans[i].pose, to, odometry))
        closures = closure_constraints(accepted, new, g["poses"])
        graph.constraints.extend(closures)
        before = np.array([s.pose for s in graph.scans])
        assert graph.optimize(m) is True
        plain = graph.last_optimize
        for s, p in zip(graph.scans, before):
            s.pose = p.copy()
        assert graph.optimize(m, loss="huber", loss_scale=1.0) is True
        rec = graph.last_optimize
        after = np.array([s.pose for s in graph.scans])
        print("end to end under huber: %d closure(s), %s after %d iterations, F %.6e -> %.6e (no loss: -> %.6e); rho' of the closures %s" %
              (len(closures), rec["status_name"], rec["iterations"], rec["initial_cost"], rec["final_cost"], plain["final_cost"],
               rec["weights"][new:]))
        assert "weights" not in plain and rec["weights"].shape == (len(graph.constraints),)
        assert np.all(rec["weights"][:new] == 1.0) and np.all((rec["weights"] > 0.0) & (rec["weights"] <= 1.0))
        assert rec["status"] != _capi.POSEGRAPH_FAILED and rec["final_cost"] <= rec["initial_cost"] <= plain["initial_cost"]
        assert np.all(np.isfinite(after)) and np.array_equal(after[0], before[0]) and np.array_equal(after, rec["poses"])
    finally:
        m.close()
