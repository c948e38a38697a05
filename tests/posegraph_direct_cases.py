"""The graphs of the direct solve's tests beside tests/posegraph_cases.py and
tests/posegraph_chain_cases.py: bare chains at the edges of the substitution's panels of 48, a loop
with a closure at every second pose, and chains perturbed so far that steps are rejected.
A graph's gate on |g|_inf is posegraph_chain_cases.gate's rule -- 100 x the floor the restatement's
own Problem.solve bottoms out at, rounded up to one digit -- taken at run time; the chain of two
takes "pair"'s gate from posegraph_cases' table (a perturbed chain of two lands on a floor no gate
can be set from: posegraph_chain_cases.EDGES)."""
import math

import numpy as np

import posegraph_cases as PC
import posegraph_chain_cases as CH
import posegraph_direct_restatement as DR
import posegraph_restatement as R

# d = 3 n = 6 ... 195: at -3 / 0 / +3 and +6 round one, two and three panels of 48, and four panels
PANEL_CHAINS = (2, 3, 15, 16, 17, 18, 31, 32, 33, 34, 47, 48, 49, 64, 65)

_BUILD = {"closures_100": lambda: PC.loop(200, 100, seed=9),
          # start poses 0.6 m and 0.6 rad off: the first Gauss-Newton steps overshoot
          "rejecting": lambda: CH.chain(21, 61, closures=[(2, 17)], sigma=0.6)}


def _far():
    """The chain of "rejecting" from start poses 1.5 m and 1.5 rad off (the fixed pose kept): the first
    Gauss-Newton steps raise the cost several times over and are rejected by a wide margin -- not, as
    "rejecting"'s two, at the level of the cost's own rounding."""
    g = CH.chain(21, 61, closures=[(2, 17)])
    noise = np.random.default_rng(7004).normal(0.0, 1.5, np.shape(g["poses"]))
    noise[g["fixed"]] = 0.0
    return dict(g, poses=np.array(g["poses"]) + noise)


_BUILD["rejecting_far"] = _far
for _n in PANEL_CHAINS:
    _BUILD["chain_%d" % _n] = lambda n=_n: CH.chain(n, 50 + n)

_problems, _solutions = {}, {}


def problem(name):
    if name not in _problems:
        _problems[name] = R.Problem(**_BUILD[name]())
    return _problems[name]


def solution(name, enabled=None):
    """Problem.solve of the graph (computed once per graph and mask, shared, not changed)."""
    key = (name, None if enabled is None else bytes(np.asarray(enabled, dtype=np.uint8)))
    if key not in _solutions:
        _solutions[key] = problem(name).solve(enabled)
    return _solutions[key]


def far_reference():
    """The minimiser "rejecting_far" is measured against.  From so far off, headings come to rest whole
    turns away from the minimiser a gentle start finds: the same cost, other poses.  Which turns is
    read off the restatement's own run (posegraph_direct_restatement.solve from the far start); the
    reference is Problem.solve started at the gentle minimiser with those turns added.  Returns
    (solution, gate by this module's rule, the restatement's run)."""
    if "far" not in _solutions:
        far, g = problem("rejecting_far"), CH.chain(21, 61, closures=[(2, 17)])
        near = R.Problem(**g).solve()
        run = DR.solve(far, max_iterations=200, gradient_tolerance=1e-9, function_tolerance=0.0, parameter_tolerance=0.0)
        turns = np.round((run["x"][:, 2] - near["x"][:, 2]) / R.TWO_PI)
        assert turns[far.fixed] == 0.0 and np.any(turns != 0.0)
        start = near["x"].copy()
        start[:, 2] += R.TWO_PI * turns
        ref = R.Problem(**dict(g, poses=start)).solve()
        _solutions["far"] = (ref, _round_up(100.0 * ref["gradient"]), run)
    return _solutions["far"]


def _round_up(raw):
    digit = 10.0 ** math.floor(math.log10(raw))
    return math.ceil(raw / digit) * digit


def gate(name, enabled=None):
    if name == "chain_2":
        return PC.gate("pair")
    return _round_up(100.0 * solution(name, enabled)["gradient"])


def bound(P, ref, gate_value, enabled=None):
    """2 |H(x*)^-1|_inf (gate + the restatement's own floor): tests/test_gpu_posegraph.py's bound."""
    return 2.0 * P.inverse_norm(ref["x"], enabled) * (gate_value + ref["gradient"])
