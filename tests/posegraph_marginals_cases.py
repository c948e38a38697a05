"""The cases of the marginal-covariance tests and each one's gate.

Every case is a designed graph of tests/posegraph_cases.py, tests/posegraph_chain_cases.py or
tests/posegraph_robust_cases.py, evaluated at the restatement's own solution of it.  A case's gate
on a column's TRUE residual |A x - e_j|_2 is

    gate = TOLERANCE + 100 x gap,   rounded up to one digit,

gap being what tests/posegraph_marginals_restatement.py's own preconditioned CG (float64, the
device's recurrences, tolerance TOLERANCE) leaves between the true residual and the recurrence
residual it stops on, the largest over the case's queries and columns: GATES below, the measured gap
beside each gate.  tests/test_posegraph_marginals_restatement.py measures the gaps again and holds
the table to them.  The bound on a value follows from the gate: to first order
|Sigma_dev - Sigma_ref|_max <= |A^-1|_inf (gate + |A Sigma_ref - I|_max), the dense inverse's own
defect its floor."""
import math

import numpy as np

import posegraph_cases as PC
import posegraph_chain_cases as CH
import posegraph_marginals_restatement as MR
import posegraph_restatement as R

TOLERANCE = 1e-10
PRECONDITIONERS = ("jacobi", "chain")
SMALL = ("pair", "square", "square_information", "square_fixed_2", "line", "wrap", "hub")
THOUSAND = ("loop_1023", "loop_1024", "loop_1025")
CHAIN = tuple(CH.EDGES) + ("chain_1025",)

_systems = {}


def case(name):
    """(the restatement's Problem, its solution's poses [n, 3])."""
    if name in PC.TABLE:
        return PC.problem(name), PC.solution(name)["x"]
    return CH.problem(name), CH.solution(name)["x"]


def size(name):
    """The case's number of poses (no solve)."""
    return (PC.problem(name) if name in PC.TABLE else CH.problem(name)).n


def system(name, damping=0.0):
    """The dense system of the case at its solution (built once, shared, not changed)."""
    key = (name, damping)
    if key not in _systems:
        P, x = case(name)
        _systems[key] = MR.System(P, x, damping=damping)
    return _systems[key]


def queries(name):
    """The first, the middle and the last free node, the fixed node, and what the case is for."""
    P, _ = case(name)
    free = [i for i in range(P.n) if system(name).node_free(i)]
    q = [free[0], free[len(free) // 2], free[-1], P.fixed]
    if name in THOUSAND:
        q += [v for v in (1, 1023, 1024) if v < P.n]      # a thread's last first node, its second node
    if name == "hub":
        q += [0, 17]                                      # the node gathering 300 constraints (held), a spoke
    if name == "isolated":
        q += [11]                                         # the node without a constraint
    return q


# hub's spoke whose three columns stop at three different iterations under "jacobi" (45, 49, 47 in
# the restatement; tests/test_posegraph_marginals_restatement.py holds it to that)
FREEZE_NODE = 1

_verdict = []


def verdict_case():
    """The graph of the closure verdicts: two laps of 40 poses with four closures under
    "information", at the restatement's solution; the proposed closure joins the neighbours
    (20, 21) and has the odometry's own covariance.  (Problem, x, (a, b), the closure's covariance)."""
    if not _verdict:
        P = R.Problem(weighting="information", **PC.loop(40, 4, seed=31))
        _verdict.append((P, P.solve()["x"], (20, 21), np.linalg.inv(PC.INFO_FULL)))
    return _verdict[0]


def round_up(v):
    digit = 10.0 ** math.floor(math.log10(v))
    return math.ceil(v / digit - 1e-9) * digit


def measure_gap(name, preconditioner):
    """The restatement's CG on the case's free queries: (gap, iterations [Q', 3], true residuals)."""
    S = system(name)
    nodes = sorted({q for q in queries(name) if S.node_free(q)})
    got = S.pcg(nodes, "jacobi" if preconditioner == "jacobi" else "band", TOLERANCE)
    assert np.all(got["status"] == MR.CONVERGED), (name, preconditioner, got["status"])
    return float(np.max(np.abs(got["true"] - got["recurrence"]))), got


def gate(name, preconditioner):
    return GATES[(name, preconditioner)][0]


def bound(name, preconditioner, damping=0.0):
    S = system(name, damping)
    return S.inverse_norm() * (gate(name, preconditioner) + S.defect())


# (case, preconditioner): (gate on the true residual, the gap it was set from, the CG iterations of
# the slowest column)
GATES = {
    ("pair", "jacobi"): (1e-10, 0.0e+00, 1),
    ("pair", "chain"): (1e-10, 0.0e+00, 1),
    ("square", "jacobi"): (2e-10, 6.2e-16, 7),
    ("square", "chain"): (2e-10, 2.0e-16, 1),
    ("square_information", "jacobi"): (2e-10, 4.3e-16, 7),
    ("square_information", "chain"): (2e-10, 1.7e-16, 1),
    ("square_fixed_2", "jacobi"): (2e-10, 5.1e-16, 7),
    ("square_fixed_2", "chain"): (2e-10, 7.8e-16, 7),
    ("line", "jacobi"): (2e-10, 3.0e-14, 40),
    ("line", "chain"): (2e-10, 4.4e-15, 1),
    ("wrap", "jacobi"): (2e-10, 7.1e-16, 61),
    ("wrap", "chain"): (2e-10, 3.5e-15, 19),
    ("hub", "jacobi"): (2e-10, 1.1e-16, 49),
    ("hub", "chain"): (2e-10, 1.0e-15, 7),
    ("n3", "chain"): (2e-10, 1.7e-16, 1),
    ("n4", "chain"): (2e-10, 1.6e-16, 1),
    ("n5", "chain"): (2e-10, 1.3e-15, 7),
    ("fixed_first", "chain"): (2e-10, 2.6e-15, 7),
    ("fixed_middle", "chain"): (2e-10, 3.9e-15, 7),
    ("fixed_last", "chain"): (2e-10, 1.4e-15, 7),
    ("reversed", "chain"): (2e-10, 2.2e-15, 7),
    ("doubled", "chain"): (2e-10, 6.6e-15, 7),
    ("isolated", "chain"): (2e-10, 2.1e-15, 13),
    ("chain_1025", "chain"): (6e-08, 5.4e-10, 2),
    ("loop_1023", "jacobi"): (2e-10, 7.1e-15, 1575),
    ("loop_1023", "chain"): (2e-10, 6.6e-15, 132),
    ("loop_1024", "jacobi"): (2e-10, 7.9e-15, 1581),
    ("loop_1024", "chain"): (2e-10, 3.6e-15, 128),
    ("loop_1025", "jacobi"): (2e-10, 4.8e-15, 1569),
    ("loop_1025", "chain"): (2e-10, 1.8e-15, 113),
}
