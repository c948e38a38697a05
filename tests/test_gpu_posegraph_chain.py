"""The pose graph's "chain" preconditioner on the device (ndt2d_pose_graph_set_preconditioner) against
the numpy restatement, on the designed graphs of tests/posegraph_cases.py and the reduction's edge
cases of tests/posegraph_chain_cases.py.

The bounds are tests/test_gpu_posegraph.py's: CONVERGED_GRADIENT at gradient_tolerance = the case's
gate with the other rules off, |g(x_dev)|_inf restated <= 2 gates, |x_dev - x*|_inf <=
2 |H(x*)^-1|_inf (gate + the restatement's own final |g|_inf).  The iteration counts: with "chain"
never more CG iterations than with "jacobi" on the same object and call; a quarter at most on the four
loops of a thousand poses (a floor: the restated solver gives 11 x on loop_1024); on a pure chain M is
H + lambda D and one CG iteration per LM step is exact, two are allowed."""
import numpy as np
import pytest

import closure_refine_cases as RC
import posegraph_cases as PC
import posegraph_chain_cases as CC
from ndt_2d_amd import Ndt2dError, PoseGraph, ScanMatcherNDT, _capi, close_loops, closure_constraints, graph_io, loop_closure_window, make_constraint

pytestmark = pytest.mark.gpu

PARITY = 1e-12
RULES = dict(max_iterations=200, function_tolerance=0.0, parameter_tolerance=0.0)
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


def _graph(name, P):
    """A PoseGraph holding the problem (one per name for the module), every constraint switchable."""
    graphs = _STATE.setdefault("graphs", {})
    if name not in graphs:
        pg = PoseGraph(_matcher(), max_nodes=P.n, max_constraints=max(1, P.m), max_jobs=8)
        pg.set_weighting(P.weighting)
        pg.set_graph(P.poses, begin=P.begin, end=P.end, transform=P.transform, information=P.information, fixed=P.fixed,
                     switchable=np.ones(P.m, dtype=bool))
        graphs[name] = pg
    return graphs[name]


def _within(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return bool(np.all(np.abs(got - want) <= PARITY * np.maximum(1.0, np.abs(want))))


def _both(pg, gate, masks=None):
    """(jacobi's, chain's) result of the same call on the same object."""
    out = []
    for name in ("jacobi", "chain"):
        pg.set_preconditioner(name)
        out.append(pg.optimize(masks, gradient_tolerance=gate, **RULES)[0])
    pg.set_preconditioner("jacobi")
    return out


def _against_the_restatement(name, P, got, ref, gate):
    restated = P.gradient_norm(got["poses"])
    bound = 2.0 * P.inverse_norm(ref["x"]) * (gate + ref["gradient"])
    err = float(np.max(np.abs(got["poses"] - ref["x"])))
    print("%s chain: %s after %d iterations, %d CG; |g| device %.3e restated %.3e (gate %.1e); |x - x*| %.3e (bound %.3e)"
          % (name, got["status_name"], got["iterations"], got["cg_iterations"], got["gradient"], restated, gate, err, bound))
    assert got["status"] == _capi.POSEGRAPH_CONVERGED_GRADIENT
    assert restated <= 2.0 * gate
    assert err <= bound
    assert np.array_equal(got["poses"][P.fixed], P.poses[P.fixed])
    assert _within(got["initial_cost"], P.cost(P.poses)) and _within(got["final_cost"], P.cost(got["poses"]))


def test_names_the_default_and_what_survives():
    P = PC.problem("square")
    pg = PoseGraph(_matcher(), max_nodes=4, max_constraints=4, max_jobs=2)
    assert pg.preconditioner() == "jacobi"
    for bad in ("", "Chain", "tridiagonal"):
        with pytest.raises(Ndt2dError, match="preconditioner") as ei:
            pg.set_preconditioner(bad)
        assert ei.value.code == _capi.ERR_INVALID and pg.preconditioner() == "jacobi"
    assert pg._L.ndt2d_pose_graph_set_preconditioner(pg._p, None) == _capi.ERR_INVALID
    pg.set_preconditioner("chain")
    assert pg.preconditioner() == "chain"
    pg.set_graph(P.poses, begin=P.begin, end=P.end, transform=P.transform, information=P.information)
    assert pg.preconditioner() == "chain"
    big = PC.problem("wrap")                                          # beyond the capacities: the object is made anew
    pg.set_graph(big.poses, begin=big.begin, end=big.end, transform=big.transform, information=big.information)
    assert pg.preconditioner() == "chain" and pg.optimize()[0]["status"] != _capi.POSEGRAPH_FAILED
    pg.set_preconditioner("jacobi")
    assert pg.preconditioner() == "jacobi"
    pg.close()


@pytest.mark.parametrize("name", PC.UNIQUE)
def test_chain_reaches_the_minimiser_in_no_more_cg_iterations(name):
    P, gate = PC.problem(name), PC.gate(name)
    jacobi, chain = _both(_graph(name, P), gate)
    _against_the_restatement(name, P, chain, PC.solution(name), gate)
    ratio = jacobi["cg_iterations"] / max(1, chain["cg_iterations"])
    print("%s: CG jacobi %d (%d LM), chain %d (%d LM): %.1f x" % (name, jacobi["cg_iterations"], jacobi["iterations"], chain["cg_iterations"],
                                                                  chain["iterations"], ratio))
    assert jacobi["status"] == _capi.POSEGRAPH_CONVERGED_GRADIENT
    assert chain["cg_iterations"] <= jacobi["cg_iterations"]
    if name in ("loop_1023", "loop_1024", "loop_1025", "m_1025"):
        assert 4 * chain["cg_iterations"] <= jacobi["cg_iterations"]


def test_chain_on_a_floating_component_reaches_the_gate():
    P, gate = PC.problem("floating"), PC.gate("floating")
    ref = PC.solution("floating")
    jacobi, chain = _both(_graph("floating", P), gate)
    print("floating: chain %s, %d iterations, %d CG (jacobi %d), F %.15e (restatement %.15e)" %
          (chain["status_name"], chain["iterations"], chain["cg_iterations"], jacobi["cg_iterations"], chain["final_cost"], ref["cost"]))
    assert chain["status"] == _capi.POSEGRAPH_CONVERGED_GRADIENT
    assert P.gradient_norm(chain["poses"]) <= 2.0 * gate
    assert _within(chain["final_cost"], ref["cost"])
    assert chain["cg_iterations"] <= jacobi["cg_iterations"]


def test_on_a_pure_chain_one_cg_iteration_a_step_is_enough():
    """1,025 poses, odometry only, the start poses off by N(0, [0.01, 0.01, 0.005]): M = H + lambda D."""
    name = "chain_1025"
    P, gate, ref = CC.problem(name), CC.gate(name), CC.solution(name)
    jacobi, chain = _both(_graph(name, P), gate)
    _against_the_restatement(name, P, chain, ref, gate)
    print("pure chain: chain %d CG in %d LM, jacobi %d CG in %d LM" % (chain["cg_iterations"], chain["iterations"], jacobi["cg_iterations"],
                                                                        jacobi["iterations"]))
    assert chain["iterations"] > 0 and chain["cg_iterations"] <= 2 * chain["iterations"]
    assert jacobi["cg_iterations"] >= 100


@pytest.mark.parametrize("name", list(CC.EDGES) + [CC.LARGE])
def test_the_edges_of_the_reduction(name):
    P, gate, ref = CC.problem(name), CC.gate(name), CC.solution(name)
    jacobi, chain = _both(_graph(name, P), gate)
    _against_the_restatement(name, P, chain, ref, gate)
    assert chain["cg_iterations"] <= jacobi["cg_iterations"]
    if name == "isolated":
        assert chain["poses"][11].tobytes() == P.poses[11].tobytes()


def test_a_mask_that_splits_the_chain_leaves_a_floating_half_that_stops_by_a_rule():
    name = "fixed_first"
    P = CC.problem(name)
    mask = np.ones((1, P.m), dtype=np.uint8)
    mask[0, 10] = 0                                                    # the edge (10, 11): nodes 11 .. 16 and 18 .. 20 hang on the closure (2, 17) only
    mask[0, 16] = 0                                                    # and (16, 17): nodes 11 .. 16 float
    ref = CC.solution(name, mask[0])
    gate = CC.gate(name, mask[0])
    jacobi, chain = _both(_graph(name, P), gate, mask)
    print("split: chain %s, %d iterations, %d CG (jacobi %d); F %.15e (restatement %.15e)" %
          (chain["status_name"], chain["iterations"], chain["cg_iterations"], jacobi["cg_iterations"], chain["final_cost"], ref["cost"]))
    assert chain["status"] == _capi.POSEGRAPH_CONVERGED_GRADIENT
    assert P.gradient_norm(chain["poses"], mask[0]) <= 2.0 * gate
    assert _within(chain["final_cost"], ref["cost"])
    # one cut only: the far half still hangs on the closure, the minimiser is unique
    mask[0, 16] = 1
    ref, gate = CC.solution(name, mask[0]), CC.gate(name, mask[0])
    jacobi, chain = _both(_graph(name, P), gate, mask)
    restated = P.gradient_norm(chain["poses"], mask[0])
    bound = 2.0 * P.inverse_norm(ref["x"], mask[0]) * (gate + ref["gradient"])
    err = float(np.max(np.abs(chain["poses"] - ref["x"])))
    print("cut: chain %s, %d CG (jacobi %d), |g| restated %.3e (gate %.1e), |x - x*| %.3e (bound %.3e)" %
          (chain["status_name"], chain["cg_iterations"], jacobi["cg_iterations"], restated, gate, err, bound))
    assert chain["status"] == _capi.POSEGRAPH_CONVERGED_GRADIENT and restated <= 2.0 * gate and err <= bound
    assert chain["cg_iterations"] <= jacobi["cg_iterations"]


def _masked_graph():
    """tests/test_gpu_posegraph.py's masked graph: a loop whose odometry constraints are make_constraint
    on the start poses themselves, six switchable closures that disagree, and an isolated last pose."""
    if "masked" not in _STATE:
        g = PC.loop(60, 6, seed=21)
        poses = np.vstack([g["poses"], [[9.0, -9.0, -0.0]]])
        cov = np.linalg.inv(PC.INFO_FULL)
        cons = [make_constraint(i, i + 1, poses[i], poses[i + 1], cov) for i in range(59)]
        cons += [graph_io.Constraint(g["begin"][c], g["end"][c], g["transform"][c], PC.INFO_FULL, switchable=True) for c in range(59, 65)]
        pg = PoseGraph(_matcher(), max_nodes=len(poses), max_constraints=len(cons), max_jobs=3)   # (five masks: two chunks)
        pg.set_graph(poses, cons, fixed=0)
        _STATE["masked"] = (pg, poses, cons)
        _STATE.setdefault("graphs", {})["masked"] = pg
    return _STATE["masked"]


def _same(a, b):
    for key in a:
        assert np.array_equal(a[key], b[key]), key


def test_chain_jobs_are_independent_repeatable_and_leave_jacobi_its_bits():
    pg, poses, cons = _masked_graph()
    m = len(cons)
    masks = np.ones((6, m), dtype=np.uint8)
    masks[0, 59:] = 0                      # every closure off: the start poses are the minimiser
    masks[1, 59] = 0
    masks[2, 60:63] = 0
    masks[3, 64] = 0
    before = pg.optimize(masks[[0, 1, 2, 3, 5]])                      # "jacobi"
    pg.set_preconditioner("chain")
    five = pg.optimize(masks[[0, 1, 2, 3, 5]])
    off = five[0]
    assert off["status"] == _capi.POSEGRAPH_CONVERGED_GRADIENT and off["iterations"] == 0
    assert off["poses"].tobytes() == poses.tobytes()                   # bit for bit, the -0.0 included
    alone = pg.optimize(masks[[1, 2, 5]])
    for a, b in zip(alone, [five[1], five[2], five[4]]):
        assert a["iterations"] > 0
        _same(a, b)
    for a, b in zip(pg.optimize(masks[[0, 1, 2, 3, 5]]), five):
        _same(a, b)
    for got in five[1:]:
        assert got["poses"][-1].tobytes() == poses[-1].tobytes() and got["poses"][0].tobytes() == poses[0].tobytes()
    assert any(not np.array_equal(a["poses"], b["poses"]) or a["cg_iterations"] != b["cg_iterations"] for a, b in zip(five[1:], before[1:]))
    pg.set_preconditioner("jacobi")
    for a, b in zip(pg.optimize(masks[[0, 1, 2, 3, 5]]), before):
        _same(a, b)


def test_graph_optimize_with_the_chain_end_to_end():
    """tests/test_gpu_posegraph.py's end-to-end case (close_loops -> closure_constraints -> Graph.optimize)
    with preconditioner="chain": the same minimiser as the default reaches, within the default tolerances."""
    g = RC.graph()
    m = ScanMatcherNDT(0)
    try:
        m.initialize("posegraph", **RC.case(0.25)["params"])
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

        def build():
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
            return graph

        default, chain = build(), build()
        assert default.optimize(m) is True and chain.optimize(m, preconditioner="chain") is True
        a, b = default.last_optimize, chain.last_optimize
        print("end to end: jacobi %s %d LM %d CG F %.9e; chain %s %d LM %d CG F %.9e" %
              (a["status_name"], a["iterations"], a["cg_iterations"], a["final_cost"], b["status_name"], b["iterations"], b["cg_iterations"],
               b["final_cost"]))
        after = np.array([s.pose for s in chain.scans])
        assert b["status"] != _capi.POSEGRAPH_FAILED and b["final_cost"] <= b["initial_cost"] and b["initial_cost"] == a["initial_cost"]
        assert np.all(np.isfinite(after)) and np.array_equal(after[0], g["poses"][0]) and np.array_equal(after, b["poses"])
        assert b["cg_iterations"] <= a["cg_iterations"]
        with pytest.raises(Ndt2dError, match="preconditioner"):
            build().optimize(m, preconditioner="band")
    finally:
        m.close()
