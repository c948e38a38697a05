"""The designed graphs of the robust-loss tests: each has ONE planted false closure, starts from its
odometry, and has a ground truth to be near to.

  square   the unit square of tests/posegraph_cases.py: three odometry constraints that agree with
           the start poses (the ground truth) and a closure 3 -> 0 that is grossly wrong.
  loop40   two laps of 40 poses (posegraph_cases.loop): noisy odometry, four closures one lap back,
           the second of them replaced by a gross error; the ground truth is the circle the
           constraints were drawn from.

The odometry's information is 4 x the closures': a closure's pull, which a robust loss bounds at
about `SCALE` in whitened units, then leaves every odometry residual well inside the loss's
quadratic part.  SCALE = 1 (one sigma of a whitened residual); the false closures are 10 sigma and
more out.  tests/test_posegraph_robust_host.py holds these choices to what they are for, on the
restatement alone: at its minimiser rho' < 0.1 on the false closure and > 0.9 on every other
constraint, the true Hessian there is positive definite, and two damping schedules agree.

A gate on |g|_inf is 100 x the floor tests/posegraph_robust_restatement.py bottoms out at on the
case (as tests/posegraph_cases.py sets its gates), rounded up to one digit: GATES, the floors beside
them."""
import math

import numpy as np

import posegraph_cases as PC
import posegraph_robust_restatement as RR

SCALE = 1.0
LOSSES = ("huber", "cauchy")
WEIGHTINGS = ("reference", "information")
CASES = ("square", "loop40")


def square():
    g = PC.square()
    h = math.pi / 2
    transform = list(g["transform"])
    transform[3] = [2.2, 0.6, h + 0.5]                       # (the truth is (1, 0, h))
    information = [4.0 * PC.INFO_FULL] * 3 + [PC.INFO_FULL]
    truth = np.array(g["poses"], dtype=np.float64)
    return dict(g, transform=transform, information=information), truth, 3


def loop40():
    n, laps = 40, 2
    g = PC.loop(n, 4, seed=31)
    per_lap = n // laps
    step = 2.0 * math.pi / per_lap
    radius = 0.25 * per_lap / (2.0 * math.pi)
    truth = np.array([[radius * math.sin(step * i), radius * (1.0 - math.cos(step * i)), step * i] for i in range(n)])
    false = (n - 1) + 1                                      # the second closure
    transform = np.array(g["transform"])
    transform[false] += [1.5, -0.8, 0.6]
    transform[false, 2] = float(RR.R.normalize(transform[false, 2]))
    information = [4.0 * PC.INFO_FULL] * (n - 1) + [PC.INFO_FULL] * 4
    return dict(g, transform=transform, information=information), truth, false


_BUILD = {"square": square, "loop40": loop40}
_built = {}


def graph(case):
    """(the graph as posegraph_cases gives them, the ground truth [n, 3], the false closure's index)."""
    if case not in _built:
        _built[case] = _BUILD[case]()
    return _built[case]


def closures(case):
    """Which constraints are closures (what `switchable` marks)."""
    g = graph(case)[0]
    return np.array([abs(int(b) - int(e)) != 1 for b, e in zip(g["begin"], g["end"])])


# (case, loss, weighting): (gate on |g|_inf, the restatement's floor it was set from)
GATES = {
    ("square", "huber", "reference"): (5e-11, 4.4e-13),
    ("square", "cauchy", "reference"): (6e-11, 5.8e-13),
    ("square", "huber", "information"): (4e-11, 3.4e-13),
    ("square", "cauchy", "information"): (4e-11, 3.4e-13),
    ("loop40", "huber", "reference"): (3e-10, 2.7e-12),
    ("loop40", "cauchy", "reference"): (4e-10, 3.3e-12),
    ("loop40", "huber", "information"): (4e-10, 3.8e-12),
    ("loop40", "cauchy", "information"): (4e-10, 3.3e-12),
}



def chain1025():
    """1,025 poses, 1,024 odometry constraints and two closures, m = 1,026: the loops over the
    constraints wrap, and the wrapped constraints are the closures -- the last of them grossly
    wrong.  The odometry's information is 100 x the closures': a chain of 512 links gives way to a
    bounded pull 512 times as far as one link, and at 4 x the false closure would be pulled shut."""
    g = PC.loop(1025, 2, seed=41)
    transform = np.array(g["transform"])
    transform[-1] += [1.5, -0.8, 0.6]
    transform[-1, 2] = float(RR.R.normalize(transform[-1, 2]))
    return dict(g, transform=transform, information=[100.0 * PC.INFO_FULL] * 1024 + [PC.INFO_FULL] * 2)


# the two graphs of the stride tests, solved by the restatement in the CPU suite only:
# name: (builder, loss, scale, gate on |g|_inf, the restatement's floor it was set from)
STRIDES = {
    "chain1025": (chain1025, "huber", SCALE, 2e-8, 1.2e-10),
    "hub": (PC.hub, "cauchy", 0.5, 2e-10, 1.1e-12),
}


def stride_problem(name):
    k = ("stride", name)
    if k not in _problems:
        build, loss, scale = STRIDES[name][:3]
        _problems[k] = RR.Problem(loss=loss, scale=scale, **build())
    return _problems[k]


_problems, _solutions = {}, {}


def problem(case, loss, weighting, robust=None, key=None):
    """The case as a restatement Problem (built once per (case, loss, weighting, key))."""
    k = (case, loss, weighting, key)
    if k not in _problems:
        _problems[k] = RR.Problem(weighting=weighting, loss=loss, scale=SCALE, robust=robust, **graph(case)[0])
    return _problems[k]


def gate(case, loss, weighting):
    return GATES[(case, loss, weighting)][0]


def solution(case, loss, weighting, robust=None, key=None):
    """The restatement's solve (computed once, shared by the tests, not changed), with the true
    Hessian's inverse norm at it."""
    k = (case, loss, weighting, key)
    if k not in _solutions:
        P = problem(case, loss, weighting, robust, key)
        s = P.solve()
        s["inverse_norm"] = P.true_inverse_norm(s["x"])
        _solutions[k] = s
    return _solutions[k]
