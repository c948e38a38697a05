"""The designed pose graphs of the pose-graph tests, and each one's gate on |g|_inf.

A case's gate is 100 x the |g|_inf floor tests/posegraph_restatement.py itself bottoms out at on
it (its `solve`), rounded up to one digit and written into TABLE below;
tests/test_posegraph_restatement.py checks that the restatement reaches every gate with a factor of
10 to spare and that every gate is <= 1e-6 x |g(x0)|_inf, so that passing it means something.  The
floors these gates were set from are beside them.

Small on purpose: the sizes are those at which the solver takes another path -- one node a thread
and the 1,025th on a second trip (1,023 / 1,024 / 1,025 nodes), one constraint and 1,025, a node of
degree 300 (one thread's gather), headings beyond +-pi, a fixed pose that is not pose 0, both
weightings."""
import math

import numpy as np

import posegraph_restatement as R

INFO_DIAGONAL = np.diag([100.0, 100.0, 400.0])
INFO_FULL = np.array([[100.0, 10.0, 5.0], [10.0, 80.0, -8.0], [5.0, -8.0, 400.0]])


def _relative(a, b):
    """The transform b in a's frame, without wrapping the heading."""
    c, s = math.cos(a[2]), math.sin(a[2])
    dx, dy = b[0] - a[0], b[1] - a[1]
    return np.array([c * dx + s * dy, c * dy - s * dx, b[2] - a[2]])


def _compose(a, t):
    c, s = math.cos(a[2]), math.sin(a[2])
    return np.array([a[0] + c * t[0] - s * t[1], a[1] + s * t[0] + c * t[1], a[2] + t[2]])


def pair():
    """Two poses, one constraint: the optimum is p_a composed with t, the cost 0."""
    return dict(poses=[[0.3, -0.2, 0.4], [1.3, 0.2, 0.1]], begin=[0], end=[1], transform=[[1.0, 0.5, 0.3]],
                information=[INFO_FULL], fixed=0)


def line(n=20, delta=0.5):
    """n + 1 poses on the x axis, n odometry constraints (1, 0, 0), one closure 0 -> n saying
    (n - delta, 0, 0), all with one diagonal information: x_i = i (1 - delta / (n + 1))."""
    poses = [[float(i), 0.0, 0.0] for i in range(n + 1)]
    begin = list(range(n)) + [0]
    end = list(range(1, n + 1)) + [n]
    transform = [[1.0, 0.0, 0.0]] * n + [[n - delta, 0.0, 0.0]]
    return dict(poses=poses, begin=begin, end=end, transform=transform, information=[INFO_DIAGONAL] * (n + 1), fixed=0)


def line_answer(n=20, delta=0.5):
    return np.array([[i * (1.0 - delta / (n + 1)), 0.0, 0.0] for i in range(n + 1)])


def square(information=INFO_FULL, fixed=0):
    """Four poses round a unit square, three odometry constraints and a closure 3 -> 0 that
    disagrees with them."""
    h = math.pi / 2
    poses = [[0.0, 0.0, 0.0], [1.0, 0.0, h], [1.0, 1.0, 2 * h], [0.0, 1.0, 3 * h]]
    turn = [1.0, 0.0, h]
    return dict(poses=poses, begin=[0, 1, 2, 3], end=[1, 2, 3, 0], transform=[turn, turn, turn, [1.1, 0.05, h + 0.05]],
                information=[information] * 4, fixed=fixed)


def loop(n, n_closures, seed, information=INFO_FULL, fixed=0, laps=2, turn_sign=1.0, heading0=0.0):
    """n poses along `laps` laps of a circle, n - 1 noisy odometry constraints, the start poses
    their integration (so they drift), and n_closures closures from a pose of a later lap back to
    the pose one lap earlier, evenly spread.  The poses' headings run on through +-pi without
    wrapping (from heading0), while a closure's heading is in [-pi, pi) as a matcher gives it: the
    heading difference it is compared with lies a whole turn away, and Normalize has to act."""
    rng = np.random.default_rng(seed)
    per_lap = n // laps
    step = turn_sign * 2.0 * math.pi / per_lap
    radius = 0.25 * per_lap / (2.0 * math.pi)   # 0.25 m between poses
    true = np.array([[radius * math.sin(step * i), turn_sign * radius * (1.0 - math.cos(step * i)), step * i] for i in range(n)])
    true = np.array([_compose([0.0, 0.0, heading0], p) for p in true])
    begin, end, transform = [], [], []
    start = [true[0].copy()]
    for i in range(n - 1):
        t = _relative(true[i], true[i + 1]) + rng.normal(0.0, [0.004, 0.004, 0.001])
        begin.append(i)
        end.append(i + 1)
        transform.append(t)
        start.append(_compose(start[-1], t))
    later = np.linspace(per_lap, n - 1, n_closures).astype(int) if n_closures else []
    for j in later:
        i = int(j) - per_lap
        begin.append(i)
        end.append(int(j))
        t = _relative(true[i], true[int(j)]) + rng.normal(0.0, [0.002, 0.002, 0.0005])
        t[2] = float(R.normalize(t[2]))
        transform.append(t)
    return dict(poses=np.array(start), begin=begin, end=end, transform=np.array(transform),
                information=[information] * len(begin), fixed=fixed)


def wrap():
    """Headings beyond +-pi and closures across the wrap: a loop turning clockwise from a start
    heading of 4.0 (beyond pi) down to 4.0 - 4 pi (beyond -pi), whose closures' heading differences lie near -2 pi."""
    return loop(24, 4, seed=5, turn_sign=-1.0, heading0=4.0)


def hub(spokes=300, seed=11):
    """Pose 0 seen from 300 others: one node's gather of 300 constraints, plus the ring between the
    others."""
    rng = np.random.default_rng(seed)
    angles = np.linspace(0.0, 2.0 * math.pi, spokes, endpoint=False)
    true = np.vstack([[0.0, 0.0, 0.0], np.stack([3.0 * np.cos(angles), 3.0 * np.sin(angles), angles + math.pi / 2], axis=1)])
    begin, end, transform = [], [], []
    for i in range(1, spokes + 1):
        begin.append(i)
        end.append(0)
        transform.append(_relative(true[i], true[0]) + rng.normal(0.0, [0.01, 0.01, 0.003]))
    for i in range(1, spokes + 1):
        j = i % spokes + 1
        begin.append(i)
        end.append(j)
        transform.append(_relative(true[i], true[j]) + rng.normal(0.0, [0.01, 0.01, 0.003]))
    poses = true + np.vstack([[0.0, 0.0, 0.0], rng.normal(0.0, [0.03, 0.03, 0.01], (spokes, 3))])
    return dict(poses=poses, begin=begin, end=end, transform=np.array(transform), information=[INFO_FULL] * len(begin), fixed=0)


def floating():
    """Two squares, the second not connected to the fixed pose: its minimiser is not unique."""
    a, b = square(), square()
    shift = np.array([5.0, 5.0, 0.3])
    return dict(poses=np.vstack([a["poses"], np.array(b["poses"]) + shift]), begin=a["begin"] + [4 + i for i in b["begin"]],
                end=a["end"] + [4 + i for i in b["end"]], transform=a["transform"] + b["transform"], information=[INFO_FULL] * 8, fixed=0)


# name: (builder, weighting, gate on |g|_inf, the restatement's floor the gate was set from)
TABLE = {
    "pair": (pair, "reference", 3e-12, 2.0e-14),
    "line": (line, "reference", 4e-11, 3.6e-13),
    "square": (square, "reference", 4e-11, 3.4e-13),
    "square_information": (square, "information", 3e-11, 2.4e-13),
    "square_fixed_2": (lambda: square(fixed=2), "reference", 2e-11, 1.5e-13),
    "wrap": (wrap, "reference", 4e-11, 3.8e-13),
    "hub": (hub, "reference", 2e-10, 1.2e-12),
    "loop_1023": (lambda: loop(1023, 20, seed=1), "reference", 2e-10, 1.2e-12),
    "loop_1024": (lambda: loop(1024, 20, seed=2), "reference", 2e-10, 1.2e-12),
    "loop_1025": (lambda: loop(1025, 20, seed=3, fixed=512), "information", 2e-10, 1.3e-12),
    "m_1025": (lambda: loop(1000, 26, seed=4), "reference", 2e-10, 1.3e-12),
    "floating": (floating, "reference", 2e-10, 1.3e-12),
}
# the cases whose minimiser is unique (every pose connected to the fixed one)
UNIQUE = [k for k in TABLE if k != "floating"]

_problems = {}


def problem(name):
    """The case as a restatement Problem (built once)."""
    if name not in _problems:
        build, weighting = TABLE[name][0], TABLE[name][1]
        _problems[name] = R.Problem(weighting=weighting, **build())
    return _problems[name]


def gate(name):
    return TABLE[name][2]


_solutions = {}


def solution(name):
    """The restatement's solve of the case (computed once, shared by the tests, not changed)."""
    if name not in _solutions:
        _solutions[name] = problem(name).solve()
    return _solutions[name]
