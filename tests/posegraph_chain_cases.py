"""The designed graphs of the "chain" preconditioner's tests, on top of tests/posegraph_cases.py: an
odometry chain along two laps of a circle (posegraph_cases.loop without closures) whose start poses
are perturbed -- the integration of the odometry alone is already the minimiser -- with closures,
reversed, doubled and missing neighbour edges put in by hand.  A case's gate on |g|_inf is 100 x the
floor the restatement's own solve bottoms out at on it, posegraph_cases.py's rule, taken at run time
(these graphs are not in its table)."""
import math

import numpy as np

import posegraph_cases as PC
import posegraph_restatement as R

SIGMA = (0.01, 0.01, 0.005)


def _inverse(t):
    """The transform of the reversed edge: pose a as pose b sees it."""
    return PC._relative(PC._compose([0.0, 0.0, 0.0], t), [0.0, 0.0, 0.0])


def chain(n, seed, closures=(), fixed=0, reverse=(), double=(), isolate=None, sigma=SIGMA):
    """n >= 2 poses, the n - 1 odometry edges (i, i + 1) in node order, then the closures (i, j) as
    given (their transform: the true one off by a few millimetres).  reverse: odometry edges stored
    as begin = i + 1, end = i.  double: odometry edges given a second time (appended, with noise of
    their own).  isolate: node k loses both its edges, (k - 1, k + 1) is joined instead."""
    g = PC.loop(n, 0, seed, laps=2 if n >= 8 else 1)
    rng = np.random.default_rng(1000 + seed)
    begin, end, transform = list(g["begin"]), list(g["end"]), [np.array(t) for t in g["transform"]]
    start = np.array(g["poses"])
    for i, j in closures:
        begin.append(i)
        end.append(j)
        transform.append(PC._relative(start[i], start[j]) + rng.normal(0.0, [0.004, 0.004, 0.001]))
    for e in double:
        begin.append(begin[e])
        end.append(end[e])
        transform.append(transform[e] + rng.normal(0.0, [0.004, 0.004, 0.001]))
    for e in reverse:
        begin[e], end[e], transform[e] = end[e], begin[e], _inverse(transform[e])
    if isolate is not None:
        k = isolate
        joined = PC._relative(start[k - 1], start[k + 1])
        keep = [c for c in range(len(begin)) if k not in (begin[c], end[c])]
        begin, end, transform = [begin[c] for c in keep], [end[c] for c in keep], [transform[c] for c in keep]
        begin.append(k - 1)
        end.append(k + 1)
        transform.append(joined)
    poses = start + rng.normal(0.0, sigma, start.shape)
    return dict(poses=poses, begin=begin, end=end, transform=np.array(transform), information=[PC.INFO_FULL] * len(begin), fixed=fixed)


# name: the builder.  The edges of the reduction: 2 to 5 nodes (one to three levels, a last node with
# and without a neighbour above), the fixed node at either end and in the middle (the chain is cut
# there), edges the other way round, twice, and missing.
# (Two nodes: posegraph_cases' "pair", with its gate from the table.  The restatement's solve of a
# perturbed chain of two lands on |g| = 9e-17, a fluke no gate can be set from.)
EDGES = {
    "n3": lambda: chain(3, 32, closures=[(0, 2)]),
    "n4": lambda: chain(4, 33, closures=[(0, 3)]),
    "n5": lambda: chain(5, 34, closures=[(0, 4), (1, 3)]),
    "fixed_first": lambda: chain(21, 35, closures=[(2, 17)], fixed=0),
    "fixed_middle": lambda: chain(21, 36, closures=[(2, 17)], fixed=10),
    "fixed_last": lambda: chain(21, 37, closures=[(2, 17)], fixed=20),
    "reversed": lambda: chain(21, 38, closures=[(2, 17)], reverse=[0, 1, 7, 8, 19]),
    "doubled": lambda: chain(21, 39, closures=[(2, 17)], double=[0, 9, 19]),
    "isolated": lambda: chain(21, 40, closures=[(2, 17)], isolate=11),
}
# 1,537 poses: the smallest size at which the 1,024 threads no longer own the same number of nodes
# each (two for some, one for the others), 11 levels.  The restatement's dense solves of it (4,611
# unknowns, ten Newton steps and an inverse) are most of this case's 9 s already; 2,049 poses would
# take 2.4 times that.
LARGE = "loop_1537"

_problems, _solutions = {}, {}


def problem(name):
    if name not in _problems:
        if name == LARGE:
            _problems[name] = R.Problem(**PC.loop(1537, 8, seed=5))
        elif name == "chain_1025":
            _problems[name] = R.Problem(**chain(1025, 41))
        else:
            _problems[name] = R.Problem(**EDGES[name]())
    return _problems[name]


def solution(name, enabled=None):
    """The restatement's solve (computed once per case and mask, shared, not changed)."""
    key = (name, None if enabled is None else bytes(np.asarray(enabled, dtype=np.uint8)))
    if key not in _solutions:
        _solutions[key] = problem(name).solve(enabled)
    return _solutions[key]


def gate(name, enabled=None):
    """100 x the restatement's floor, rounded up to one digit."""
    raw = 100.0 * solution(name, enabled)["gradient"]
    digit = 10.0 ** math.floor(math.log10(raw))
    return math.ceil(raw / digit) * digit
