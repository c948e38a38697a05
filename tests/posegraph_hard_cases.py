"""Designed pose graphs on the numbers the node really feeds the solver -- rotated anisotropic
information, map coordinates far from the origin, closures that span metres, weights orders of
magnitude apart, a diagonal of H below the damping's clamp -- and each one's gates, measured against
the extended-precision yardstick tests/posegraph_exact.py.

Every case has at most 25 poses (<= 72 unknowns: an extended-precision inverse in about a second)
and is built from posegraph_cases' loop / _compose / _relative.  Each knob is the smallest that still
reaches its regime.

The gates follow posegraph_cases.py and posegraph_marginals_cases.py: a gate is 100 x what the FLOAT64
RESTATEMENT OF THE SAME PATH leaves against the exact yardstick on that case, rounded up to one digit
(posegraph_marginals_cases.round_up), and stands in TABLE with the measured value beside it.
measure(name) measures them; tests/test_posegraph_exact.py measures every entry again and holds the
table to measured <= gate / 10.  No gate comes from the device.

    evaluate   |value - exact|_max / |exact|_max of cost, chi2, e, r and g at the start poses, of
               posegraph_restatement's Problem; never less than 2^-53, the format's own rounding.
    gradient   the exact |g|_inf at Problem.solve's solution, the floor the float64 restatement bottoms out at: the
               gate on every solver, as posegraph_cases, posegraph_chain_cases and posegraph_direct_cases set theirs.
    sigma      max|Sigma - Sigma_exact| at the double-rounded exact minimiser, at damping 0 and 1e-4, of
               "dense" (posegraph_dense_restatement), "sparse" (posegraph_sparsecov_restatement) and
               "pcg" (posegraph_marginals_restatement's System.pcg under both preconditioners, the
               larger; its tolerance is the case's cg_tolerance = round_up(100 x the dense floor) per damping --
               the default 1e-10 is below that floor on "corridor").

Two conditions hold for every case (tests/test_posegraph_exact.py asserts them):
    (a) the gradient gate <= 1e-6 x |g(x0)|_inf, the project's rule;
    (b) every sigma gate <= 1e-2 x the smallest diagonal entry of the exact Sigma it is compared on,
        so that an error of 10 %, such as a dropped clamp, cannot pass.

    derived    (DERIVED's cases) relative_covariances and closure_distance: the relative errors of the predicted
               transform, its covariance and d^2 that the restatements' own chain leaves (Sigma by the dense and by the
               sparse restatement, then posegraph_marginals_restatement's relative and distance) against the exact joint
               covariance pushed through the same formulas in extended precision."""
import math

import numpy as np

import posegraph_cases as PC
import posegraph_dense_restatement as DN
import posegraph_exact as X
import posegraph_marginals_cases as MC
import posegraph_marginals_restatement as MR
import posegraph_restatement as R
import posegraph_robust_restatement as RR
import posegraph_sparsecov_restatement as SC

DAMPINGS = (0.0, 1e-4)
PATHS = ("dense", "sparse", "pcg")
EPS53 = 2.0 ** -53
CG_CAP = 8192          # max_cg_iterations of the marginals: the solver's cap min(3 n + 16, 8192) is 88 at 24 poses
INFO_FULL = PC.INFO_FULL


def _rotation(angle, tilt=0.2):
    """A turn by `angle` about the heading axis behind a tilt about x: the anisotropy's axes lie
    across x, y and theta."""
    c, s, ct, st = math.cos(angle), math.sin(angle), math.cos(tilt), math.sin(tilt)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, ct, -st], [0.0, st, ct]])


def corridor_information(c):
    """Q(0.37 c) diag(1e6, 1e1, 1e4) Q(0.37 c)^T, symmetric bit for bit: what inverting a refine
    step's covariance gives in a corridor, turned differently for every constraint."""
    Q = _rotation(0.37 * c)
    M = Q @ np.diag([1e6, 1e1, 1e4]) @ Q.T
    return 0.5 * (M + M.T)


def corridor(seed=8, fixed=0):
    g = PC.loop(24, 4, seed=seed, fixed=fixed)
    return dict(g, information=[corridor_information(c) for c in range(len(g["begin"]))])


def mixed(seed=9):
    """Weak odometry (1e-4 x INFO_FULL) under strong closures (1e4 x INFO_FULL): eight orders of
    magnitude.  Two laps of 12 poses and a 25th; a closure from every pose of the second lap but one to
    the pose a lap earlier; the fixed pose is 11, the one no closure touches.  Every pose then hangs on
    the fixed one by weak odometry only (variances ~1e2 ... 1e3), while the strong closures tie the poses
    in pairs to 1e-6: each block of Sigma is 1e8 x what the difference of two of them is known to.  (With
    a closure at the fixed pose its partner's variance is 1e-7, 1e10 below the others', and no float64
    path can hold every block to a hundredth of THAT: condition (b).)  The start poses integrate an
    odometry biased by (4 mm, 0, 2 mrad) a step, so that the closures disagree with them by centimetres
    and |g(x0)| stands 1e6 above the gate: condition (a)."""
    g = PC.loop(25, 12, seed=seed, fixed=11)
    m_odo = 24
    assert all(11 not in (a, b) for a, b in zip(g["begin"][m_odo:], g["end"][m_odo:]))
    transform = np.array(g["transform"], dtype=np.float64)
    transform[:m_odo] += np.array([0.004, 0.0, 0.002])
    poses = [np.array(g["poses"][0], dtype=np.float64)]
    for i in range(m_odo):
        poses.append(PC._compose(poses[-1], transform[i]))
    info = [1e-4 * INFO_FULL] * m_odo + [1e4 * INFO_FULL] * (len(g["begin"]) - m_odo)
    return dict(g, poses=np.array(poses), transform=transform, information=info)


def far(seed=10):
    """The base loop from a start heading of 100 rad, moved by (5e4, -3e4) m, and every pose's heading
    whole turns away from its neighbours' (k_i x 2 pi, k_i = -6 ... 6): p_b - p_a cancels twelve digits,
    and Normalize acts on arguments of tens of radians."""
    g = PC.loop(24, 4, seed=seed, heading0=100.0)
    poses = np.array(g["poses"], dtype=np.float64)
    poses[:, 0] += 5e4
    poses[:, 1] -= 3e4
    turns = np.array([((7 * i) % 5 - 2) * 3 for i in range(len(poses))], dtype=np.float64)
    turns[0] = 0.0
    poses[:, 2] += R.TWO_PI * turns
    return dict(g, poses=poses)


def lever(seed=12, radius=25.0, n=24):
    """One lap of a circle of 25 m radius in 24 poses (6.5 m apart), four closures across the diameter
    (50 m): the lever arm ex, ey of the Jacobians is tens of metres, the theta block of H 1e3 x the xy block
    (at 20 m it is 700 x)."""
    rng = np.random.default_rng(seed)
    step = 2.0 * math.pi / n
    true = np.array([[radius * math.sin(step * i), radius * (1.0 - math.cos(step * i)), step * i] for i in range(n)])
    begin, end, transform, start = [], [], [], [true[0].copy()]
    for i in range(n - 1):
        t = PC._relative(true[i], true[i + 1]) + rng.normal(0.0, [0.004, 0.004, 0.001])
        begin.append(i), end.append(i + 1), transform.append(t)
        start.append(PC._compose(start[-1], t))
    for i in (0, 3, 6, 9):
        t = PC._relative(true[i], true[i + n // 2]) + rng.normal(0.0, [0.002, 0.002, 0.0005])
        t[2] = float(R.normalize(t[2]))
        begin.append(i), end.append(i + n // 2), transform.append(t)
    return dict(poses=np.array(start), begin=begin, end=end, transform=np.array(transform), information=[INFO_FULL] * len(begin), fixed=0)


LEAF_INFORMATION = 1e-8


def _with_leaf(g, information):
    """The graph with a 25th pose hung on pose 12 by one constraint it does not meet by centimetres."""
    poses = np.vstack([g["poses"], PC._compose(g["poses"][12], [0.5, 0.3, 0.2])])
    return dict(g, poses=poses, begin=list(g["begin"]) + [12], end=list(g["end"]) + [24],
                transform=np.vstack([g["transform"], [[0.45, 0.33, 0.25]]]), information=list(g["information"]) + [information])


def weak_leaf(seed=11, information=LEAF_INFORMATION):
    """A loop of 24 and a 25th pose hung on pose 12 by one constraint of information 1e-8 x I: the
    leaf's diagonal of H is 1e-8, below the damping's clamp 1e-6, and kappa(H) ~ 1e11.  (At 1e-9 x I the
    float64 restatements' own error on the leaf's block, ~1e9 x kappa x eps, breaks condition (b).)"""
    return _with_leaf(PC.loop(24, 4, seed=seed), information * np.eye(3))


PINCH = [1e7, 1e0, 1e3]


def pinched(seed=8):
    """The corridor with a 25th pose hung on ONE constraint of information Q diag(1e7, 1e0, 1e3) Q^T: the
    sums over differently turned constraints keep the other nodes' 3 x 3 blocks of H at kappa <= 1e4; this
    node's block is one constraint's, kappa = 1e7 -- what the preconditioners' 3 x 3 inverses must take."""
    Q = _rotation(0.37 * 5)
    M = Q @ np.diag(PINCH) @ Q.T
    return _with_leaf(corridor(seed), 0.5 * (M + M.T))


LEAF = 24
SCALE_BITS = 40


def base(seed=7):
    return PC.loop(24, 4, seed=seed)


def scaled(bits):
    """The base graph with every information x 2^bits: an exact scaling.  L scales by 2^(bits/2)
    exactly, so r does, chi2, F, g and H by 2^bits, Sigma by 2^-bits -- bit for bit."""
    g = base()
    return dict(g, information=[np.ldexp(INFO_FULL, bits)] * len(g["begin"]))


# name: (builder, weighting)
CASES = {
    "base": (base, "reference"),
    "corridor": (corridor, "reference"),
    "corridor_information": (lambda: corridor(fixed=11), "information"),
    "mixed": (mixed, "reference"),
    "mixed_information": (mixed, "information"),
    "far": (far, "reference"),
    "lever": (lever, "reference"),
    "lever_information": (lever, "information"),
    "weak_leaf": (weak_leaf, "reference"),
    "pinched": (pinched, "reference"),
    "scaled_up": (lambda: scaled(SCALE_BITS), "reference"),
    "scaled_down": (lambda: scaled(-SCALE_BITS), "reference"),
}
# the robust cases: corridor under a loss whose scale leaves 11 (Huber) and 7 (Cauchy) of the 27 constraints beyond
# it at the minimiser; below 0.015 and 0.045 the robust cost has other minima within reach of the start poses,
# and the float64 restatements end in different ones
ROBUST = {"corridor_huber": ("corridor", "huber", 0.015), "corridor_cauchy": ("corridor", "cauchy", 0.045)}

_cache = {}


def robust_start(of):
    """The start poses of a robust case: the minimiser of the same graph without a loss, each pose moved
    by a few millimetres and milliradians (the fixed one not).  From the drifted start poses of the graph
    half the constraints begin far beyond the scale, the robust cost has other minima there, and which
    one a solver lands in is not a property to pin."""
    x = minimiser(of)["x"].copy()
    rng = np.random.default_rng(77)
    noise = rng.normal(0.0, [0.003, 0.003, 0.002], x.shape)
    noise[CASES[of][0]()["fixed"]] = 0.0
    return x + noise


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def graph(name):
    """The case's dict of arrays and its weighting (and, for a robust case, loss and scale)."""
    if name in ROBUST:
        of, loss, scale = ROBUST[name]
        return dict(CASES[of][0](), weighting=CASES[of][1], loss=loss, scale=scale, poses=robust_start(of))
    return dict(CASES[name][0](), weighting=CASES[name][1])


def problem(name):
    """The float64 restatement's Problem (the robust one under a loss), built once."""
    return _once(("P", name), lambda: (RR.Problem if name in ROBUST else R.Problem)(**graph(name)))


def exact(name):
    """The extended-precision Graph, built once (it caches its own minimiser and inverses)."""
    return _once(("X", name), lambda: X.Graph(**graph(name)))


def minimiser(name):
    """posegraph_exact's minimiser of the case: dict(x float64, exact, gradient, ...)."""
    return exact(name).minimiser()


def covariance(name, damping, clamp=True):
    """The exact Sigma at the double-rounded exact minimiser."""
    return exact(name).covariance(minimiser(name)["x"], damping=damping, clamp=clamp)


def system(name, damping):
    """The float64 dense system of the case at the double-rounded exact minimiser."""
    return _once(("S", name, damping), lambda: MR.System(problem(name), minimiser(name)["x"], damping=damping))


def newton(name):
    return _once(("newton", name), lambda: problem(name).solve())


def _relative_error(got, want):
    want = np.asarray(want, dtype=np.float64)
    scale = float(np.max(np.abs(want))) if want.size else 0.0
    return float(np.max(np.abs(np.asarray(got) - want))) / scale if scale > 0.0 else 0.0


def evaluate_errors(name, got):
    """|got - exact|_max / |exact|_max per quantity of an evaluate at the start poses: got = dict(cost, chi2,
    e, r, g [3n])."""
    want = _once(("ev", name), lambda: exact(name).evaluate())
    return {k: _relative_error(got[k], want[k]) for k in ("cost", "chi2", "e", "r", "g")}


DERIVED = ("corridor", "corridor_information", "lever", "lever_information")
MEASURED_OFFSET = np.array([0.03, -0.02, 0.01 + 2.0 * math.pi])      # (the heading a whole turn away: Normalize acts)


def inverse_norm(name, x=None):
    """|H^-1|_inf at the exact minimiser (or at x), for the bound on |x_dev - x*|: of the contract's H, and under a loss
    of H with the loss's second-order term (rho'' < 0 makes the true Hessian smaller than the reweighted H)."""
    if name not in ROBUST:
        return covariance(name, 0.0)["inverse_norm"]
    H, _ = exact(name).hessian(minimiser(name)["x"] if x is None else x, curvature=True)
    return float(np.max(np.sum(np.abs(np.linalg.inv(X.to_float(H))), axis=1)))


def derived(name):
    """The derived calls' inputs and exact answers at the double-rounded exact minimiser, damping 0: per pair (a, b)
    dict(pair, transform, covariance: the exact joint covariance pushed through [A B] sym(joint) [A B]^T in extended
    precision, measured: the transform a closure would report (the prediction moved by MEASURED_OFFSET),
    covariance_measured: the predicted covariance itself, rounded, so that neither term of the sum drowns the other,
    distance: the exact d^2), every value rounded once."""
    def make():
        E, xs, C = exact(name), minimiser(name)["x"], covariance(name, 0.0)
        at = {u: k for k, u in enumerate(C["index"])}
        n, out = E.n, []

        def block(i, j):
            if 3 * i not in at or 3 * j not in at:
                return [[X.ZERO] * 3 for _ in range(3)]
            return [[C["exact"][at[3 * i + r]][at[3 * j + c]] for c in range(3)] for r in range(3)]

        for a, b in ((1, n // 2), (n - 2, n // 2 + 1), (5, 6)):
            joint = [[block(a, a), block(a, b)], [block(b, a), block(b, b)]]
            t, cov = X.relative_exact(xs[a], xs[b], joint)
            measured = X.to_float(t) + MEASURED_OFFSET
            cov_measured = X.to_float(cov)
            out.append(dict(pair=(a, b), transform=X.to_float(t), covariance=X.to_float(cov), measured=measured, covariance_measured=cov_measured,
                            distance=X.distance(t, cov, measured, cov_measured)))
        return out
    return _once(("derived", name), make)


def derived_errors(name, got):
    """got: per pair of derived(name) (transform, covariance, distance); the largest relative errors (against the
    largest entry of the exact value) over the pairs."""
    worst = dict(transform=0.0, covariance=0.0, distance=0.0)
    for want, (t, cov, d2) in zip(derived(name), got):
        worst["transform"] = max(worst["transform"], _relative_error(t, want["transform"]))
        worst["covariance"] = max(worst["covariance"], _relative_error(cov, want["covariance"]))
        worst["distance"] = max(worst["distance"], abs(d2 - want["distance"]) / want["distance"])
    return worst


def _derived_by_restatement(name):
    """The restatements' own chain: Sigma by the dense and by the sparse restatement, then posegraph_marginals_restatement's
    relative and distance; the larger error of the two."""
    P, xs, S = problem(name), minimiser(name)["x"], system(name, 0.0)
    dense = np.zeros((3 * P.n, 3 * P.n))
    dense[np.ix_(S.index, S.index)] = DN.solve(S)["sigma"]
    worst = dict(transform=EPS53, covariance=EPS53, distance=EPS53)
    for full in (dense, SC.Sparse(P, xs).whole()):
        got = []
        for want in derived(name):
            a, b = want["pair"]
            joint = np.array([[full[3 * i:3 * i + 3, 3 * j:3 * j + 3] for j in (a, b)] for i in (a, b)])
            t, cov = MR.relative(math.cos(xs[a][2]), math.sin(xs[a][2]), xs[a], xs[b], joint)
            got.append((t, cov, MR.distance(t, cov, want["measured"], want["covariance_measured"])))
        worst = {k: max(worst[k], v) for k, v in derived_errors(name, got).items()}
    return worst


def cg_tolerance(name, damping):
    return TABLE[name]["cg_tolerance"][damping][0]


def measure(name):
    """Every measured figure of the case's table entry."""
    P, E = problem(name), exact(name)
    out = {}
    e, r, chi2 = P.residuals(P.poses)
    g, H = P.gradient_hessian(P.poses)
    g = np.where(P.free(), g, 0.0)
    errors = evaluate_errors(name, dict(cost=P.cost(P.poses), chi2=chi2, e=e, r=r, g=g))
    out["evaluate"] = {k: max(v, EPS53) for k, v in errors.items()}
    out["g0"] = E.gradient_norm()
    xs = minimiser(name)["x"]
    Hx, _ = E.hessian(xs)
    out["kappa"] = float(np.linalg.cond(X.to_float(Hx)))
    out["min_diag"] = float(min(Hx[k][k] for k in range(len(Hx))))
    out["gradient"] = E.gradient_norm(newton(name)["x"])
    out["newton_distance"] = float(np.max(np.abs(newton(name)["x"] - xs)))
    out["inverse_norm"] = covariance(name, 0.0)["inverse_norm"]
    out["cg_tolerance"] = {d: DN.floor(system(name, d)) for d in DAMPINGS}
    out["sigma"], out["min_sigma"], out["cg_iterations"] = {}, {}, {}
    for damping in DAMPINGS:
        S, C = system(name, damping), covariance(name, damping)
        tolerance = MC.round_up(100.0 * out["cg_tolerance"][damping])
        assert list(S.index) == list(C["index"])
        want = C["sigma"]
        out["min_sigma"][damping] = float(np.min(np.diag(want)))
        full = SC.Sparse(P, xs, damping=damping).whole()
        nodes = sorted(set(int(u) // 3 for u in S.index))
        worst, iterations = 0.0, {}
        for pre in ("jacobi", "band"):
            cg = S.pcg(nodes, pre, tolerance, max_iterations=CG_CAP)
            assert np.all(cg["status"] == MR.CONVERGED), (name, damping, pre, cg["iterations"].max())
            worst = max(worst, float(np.max(np.abs(cg["x"].reshape(len(S.A), -1) - want))))
            iterations[pre] = int(np.max(cg["iterations"]))
        out["cg_iterations"][damping] = iterations
        if name in DERIVED and damping == 0.0:
            out["derived"] = _derived_by_restatement(name)
        out["sigma"][damping] = dict(dense=float(np.max(np.abs(DN.solve(S)["sigma"] - want))),
                                     sparse=float(np.max(np.abs(full[np.ix_(S.index, S.index)] - want))), pcg=worst)
    return out


def gates_from(measured):
    """The table entry a measurement gives: every gate 100 x its figure, rounded up to one digit."""
    up = lambda v: MC.round_up(100.0 * v)      # noqa: E731
    return dict(kappa=measured["kappa"], g0=measured["g0"], min_diag=measured["min_diag"],
                evaluate={k: (up(v), v) for k, v in measured["evaluate"].items()},
                gradient=(up(measured["gradient"]), measured["gradient"]),
                cg_tolerance={d: (up(v), v) for d, v in measured["cg_tolerance"].items()},
                sigma={d: {p: (up(v), v) for p, v in by.items()} for d, by in measured["sigma"].items()},
                min_sigma=dict(measured["min_sigma"]), cg_iterations=dict(measured["cg_iterations"]),
                **({"derived": {k: (up(v), v) for k, v in measured["derived"].items()}} if "derived" in measured else {}))


def gate(name, family, *key):
    """The gate of TABLE[name][family] (for "evaluate" by quantity, for "sigma" by damping and path)."""
    entry = TABLE[name][family]
    for k in key:
        entry = entry[k]
    return entry[0]


def format_entry(name, entry):
    """The table entry as the source text below."""
    def pair(p):
        return "(%.0e, %.1e)" % (p[0], p[1])
    lines = ["    \"%s\": dict(" % name,
             "        kappa=%.1e, g0=%.1e, min_diag=%.1e," % (entry["kappa"], entry["g0"], entry["min_diag"]),
             "        evaluate=dict(%s)," % ", ".join("%s=%s" % (k, pair(v)) for k, v in entry["evaluate"].items()),
             "        gradient=%s," % pair(entry["gradient"]),
             "        cg_tolerance={%s}," % ", ".join("%r: %s" % (d, pair(v)) for d, v in entry["cg_tolerance"].items()),
             "        sigma={%s}," % ", ".join("%r: dict(%s)" % (d, ", ".join("%s=%s" % (p, pair(v)) for p, v in by.items()))
                                               for d, by in entry["sigma"].items()),
             "        min_sigma={%s}," % ", ".join("%r: %.1e" % (d, v) for d, v in entry["min_sigma"].items()),
             "        cg_iterations={%s}%s" % (", ".join("%r: dict(jacobi=%d, band=%d)" % (d, v["jacobi"], v["band"]) for d, v in entry["cg_iterations"].items()),
                                                "," if "derived" in entry else "),")]
    if "derived" in entry:
        lines.append("        derived=dict(%s))," % ", ".join("%s=%s" % (k, pair(v)) for k, v in entry["derived"].items()))
    return "\n".join(lines)


# Per case: kappa(H) and the smallest diagonal entry of H at the minimiser, |g(x0)|_inf, and the gates,
# each as (gate, the restatement's measured figure it was set from).  min_sigma: the smallest diagonal
# entry of the exact Sigma per damping (condition (b)); cg_iterations: the restatement's CG, the slowest
# column, per preconditioner.  Written by format_entry(name, gates_from(measure(name))).
TABLE = {
    "base": dict(
        kappa=6.6e+02, g0=3.2e+00, min_diag=1.6e+02,
        evaluate=dict(cost=(2e-14, 1.1e-16), chi2=(2e-14, 1.7e-16), e=(2e-13, 1.5e-15), r=(2e-13, 1.7e-15), g=(2e-13, 1.5e-15)),
        gradient=(2e-10, 1.3e-12),
        cg_tolerance={0.0: (4e-13, 3.4e-15), 0.0001: (4e-13, 3.4e-15)},
        sigma={0.0: dict(dense=(1e-14, 9.4e-17), sparse=(8e-15, 7.6e-17), pcg=(2e-13, 1.4e-15)), 0.0001: dict(dense=(2e-14, 1.0e-16), sparse=(2e-14, 1.0e-16), pcg=(2e-13, 1.4e-15))},
        min_sigma={0.0: 2.1e-03, 0.0001: 2.1e-03},
        cg_iterations={0.0: dict(jacobi=66, band=19), 0.0001: dict(jacobi=66, band=19)}),
    "corridor": dict(
        kappa=1.1e+07, g0=3.3e+04, min_diag=4.9e+02,
        evaluate=dict(cost=(7e-14, 6.9e-16), chi2=(2e-13, 1.0e-15), e=(2e-12, 1.3e-14), r=(5e-13, 4.8e-15), g=(2e-13, 1.5e-15)),
        gradient=(2e-08, 1.0e-10),
        cg_tolerance={0.0: (1e-08, 9.9e-11), 0.0001: (3e-10, 2.8e-12)},
        sigma={0.0: dict(dense=(6e-10, 5.5e-12), sparse=(2e-10, 1.8e-12), pcg=(5e-09, 4.7e-11)), 0.0001: dict(dense=(5e-12, 4.1e-14), sparse=(5e-12, 4.2e-14), pcg=(9e-11, 8.5e-13))},
        min_sigma={0.0: 1.0e-06, 0.0001: 1.0e-06},
        cg_iterations={0.0: dict(jacobi=175, band=31), 0.0001: dict(jacobi=150, band=27)},
        derived=dict(transform=(2e-14, 1.1e-16), covariance=(2e-09, 1.1e-11), distance=(2e-09, 1.3e-11))),
    "corridor_information": dict(
        kappa=4.2e+06, g0=2.3e+04, min_diag=1.9e+04,
        evaluate=dict(cost=(2e-14, 1.3e-16), chi2=(2e-14, 1.9e-16), e=(2e-12, 1.3e-14), r=(4e-13, 3.5e-15), g=(2e-13, 1.2e-15)),
        gradient=(1e-08, 9.3e-11),
        cg_tolerance={0.0: (8e-09, 7.7e-11), 0.0001: (3e-10, 2.4e-12)},
        sigma={0.0: dict(dense=(4e-10, 3.2e-12), sparse=(4e-10, 3.5e-12), pcg=(9e-09, 8.6e-11)), 0.0001: dict(dense=(1e-12, 9.0e-15), sparse=(7e-13, 6.9e-15), pcg=(2e-10, 1.1e-12))},
        min_sigma={0.0: 1.7e-03, 0.0001: 1.8e-04},
        cg_iterations={0.0: dict(jacobi=241, band=33), 0.0001: dict(jacobi=153, band=25)},
        derived=dict(transform=(2e-14, 1.1e-16), covariance=(3e-09, 2.4e-11), distance=(5e-07, 4.3e-09))),
    "mixed": dict(
        kappa=2.9e+10, g0=1.2e+05, min_diag=1.7e-02,
        evaluate=dict(cost=(9e-14, 8.3e-16), chi2=(2e-12, 1.4e-14), e=(7e-13, 6.9e-15), r=(8e-13, 7.7e-15), g=(8e-13, 7.8e-15)),
        gradient=(4e-07, 3.8e-09),
        cg_tolerance={0.0: (1e-05, 9.6e-08), 0.0001: (3e-10, 2.3e-12)},
        sigma={0.0: dict(dense=(2e-03, 1.3e-05), sparse=(2e-03, 1.1e-05), pcg=(3e-02, 2.8e-04)), 0.0001: dict(dense=(3e-12, 2.1e-14), sparse=(3e-12, 2.1e-14), pcg=(9e-10, 8.1e-12))},
        min_sigma={0.0: 1.8e+01, 0.0001: 6.3e-04},
        cg_iterations={0.0: dict(jacobi=118, band=97), 0.0001: dict(jacobi=20, band=15)}),
    "mixed_information": dict(
        kappa=2.9e+10, g0=1.2e+05, min_diag=1.6e-02,
        evaluate=dict(cost=(7e-14, 6.3e-16), chi2=(2e-12, 1.4e-14), e=(7e-13, 6.9e-15), r=(8e-13, 7.7e-15), g=(8e-13, 7.6e-15)),
        gradient=(4e-07, 3.5e-09),
        cg_tolerance={0.0: (1e-05, 9.8e-08), 0.0001: (3e-10, 2.8e-12)},
        sigma={0.0: dict(dense=(3e-03, 2.0e-05), sparse=(2e-03, 1.7e-05), pcg=(4e-02, 3.3e-04)), 0.0001: dict(dense=(3e-12, 2.8e-14), sparse=(8e-13, 7.1e-15), pcg=(8e-10, 7.8e-12))},
        min_sigma={0.0: 1.8e+01, 0.0001: 6.2e-04},
        cg_iterations={0.0: dict(jacobi=117, band=96), 0.0001: dict(jacobi=20, band=15)}),
    "far": dict(
        kappa=6.6e+02, g0=3.4e+00, min_diag=1.6e+02,
        evaluate=dict(cost=(8e-13, 7.4e-15), chi2=(2e-12, 1.2e-14), e=(2e-11, 1.1e-13), r=(3e-11, 2.3e-13), g=(7e-11, 6.4e-13)),
        gradient=(2e-07, 1.4e-09),
        cg_tolerance={0.0: (4e-13, 3.7e-15), 0.0001: (4e-13, 3.7e-15)},
        sigma={0.0: dict(dense=(2e-14, 1.1e-16), sparse=(7e-15, 6.2e-17), pcg=(2e-13, 1.0e-15)), 0.0001: dict(dense=(2e-14, 1.0e-16), sparse=(5e-15, 4.9e-17), pcg=(2e-13, 1.0e-15))},
        min_sigma={0.0: 2.1e-03, 0.0001: 2.1e-03},
        cg_iterations={0.0: dict(jacobi=67, band=19), 0.0001: dict(jacobi=67, band=19)}),
    "lever": dict(
        kappa=4.7e+05, g0=7.3e+02, min_diag=7.8e+01,
        evaluate=dict(cost=(4e-12, 3.6e-14), chi2=(7e-12, 6.2e-14), e=(5e-12, 4.5e-14), r=(5e-12, 4.5e-14), g=(5e-12, 4.2e-14)),
        gradient=(7e-09, 6.6e-11),
        cg_tolerance={0.0: (6e-11, 5.6e-13), 0.0001: (6e-11, 5.4e-13)},
        sigma={0.0: dict(dense=(7e-13, 6.2e-15), sparse=(5e-13, 4.7e-15), pcg=(4e-13, 3.1e-15)), 0.0001: dict(dense=(2e-12, 1.1e-14), sparse=(7e-13, 6.4e-15), pcg=(5e-13, 4.6e-15))},
        min_sigma={0.0: 3.7e-05, 0.0001: 3.6e-05},
        cg_iterations={0.0: dict(jacobi=69, band=19), 0.0001: dict(jacobi=69, band=19)},
        derived=dict(transform=(2e-14, 1.7e-16), covariance=(8e-13, 7.3e-15), distance=(5e-12, 4.5e-14))),
    "lever_information": dict(
        kappa=4.7e+05, g0=7.2e+02, min_diag=7.6e+01,
        evaluate=dict(cost=(4e-12, 3.5e-14), chi2=(7e-12, 6.1e-14), e=(5e-12, 4.5e-14), r=(5e-12, 4.1e-14), g=(5e-12, 4.1e-14)),
        gradient=(2e-09, 1.9e-11),
        cg_tolerance={0.0: (6e-11, 5.7e-13), 0.0001: (6e-11, 5.5e-13)},
        sigma={0.0: dict(dense=(3e-13, 2.1e-15), sparse=(4e-13, 3.2e-15), pcg=(2e-13, 1.4e-15)), 0.0001: dict(dense=(2e-13, 1.9e-15), sparse=(5e-13, 4.2e-15), pcg=(2e-13, 1.8e-15))},
        min_sigma={0.0: 3.7e-05, 0.0001: 3.6e-05},
        cg_iterations={0.0: dict(jacobi=69, band=19), 0.0001: dict(jacobi=69, band=19)},
        derived=dict(transform=(2e-14, 1.7e-16), covariance=(4e-13, 3.2e-15), distance=(6e-12, 5.7e-14))),
    "weak_leaf": dict(
        kappa=1.9e+11, g0=2.2e+00, min_diag=1.0e-08,
        evaluate=dict(cost=(3e-13, 2.6e-15), chi2=(5e-13, 4.0e-15), e=(9e-13, 8.9e-15), r=(4e-12, 3.5e-14), g=(9e-12, 8.2e-14)),
        gradient=(5e-11, 4.3e-13),
        cg_tolerance={0.0: (4e-13, 3.4e-15), 0.0001: (4e-13, 3.4e-15)},
        sigma={0.0: dict(dense=(8e-06, 7.5e-08), sparse=(2e-06, 1.5e-08), pcg=(5e-06, 4.5e-08)), 0.0001: dict(dense=(3e-06, 3.0e-08), sparse=(2e-06, 1.5e-08), pcg=(3e-06, 3.0e-08))},
        min_sigma={0.0: 2.1e-03, 0.0001: 2.1e-03},
        cg_iterations={0.0: dict(jacobi=67, band=22), 0.0001: dict(jacobi=67, band=22)}),
    "pinched": dict(
        kappa=5.4e+07, g0=5.3e+05, min_diag=2.5e+01,
        evaluate=dict(cost=(8e-13, 7.2e-15), chi2=(8e-13, 7.5e-15), e=(9e-13, 8.9e-15), r=(5e-12, 4.9e-14), g=(7e-13, 6.1e-15)),
        gradient=(1e-08, 9.8e-11),
        cg_tolerance={0.0: (2e-08, 1.3e-10), 0.0001: (7e-10, 6.5e-12)},
        sigma={0.0: dict(dense=(7e-09, 6.6e-11), sparse=(7e-09, 6.7e-11), pcg=(7e-09, 6.8e-11)), 0.0001: dict(dense=(7e-09, 6.8e-11), sparse=(7e-09, 6.8e-11), pcg=(7e-09, 6.8e-11))},
        min_sigma={0.0: 1.0e-06, 0.0001: 1.0e-06},
        cg_iterations={0.0: dict(jacobi=193, band=41), 0.0001: dict(jacobi=153, band=35)}),
    "scaled_up": dict(
        kappa=6.6e+02, g0=3.5e+12, min_diag=1.7e+14,
        evaluate=dict(cost=(2e-14, 1.1e-16), chi2=(2e-14, 1.7e-16), e=(2e-13, 1.5e-15), r=(2e-13, 1.7e-15), g=(2e-13, 1.5e-15)),
        gradient=(2e+02, 1.4e+00),
        cg_tolerance={0.0: (4e-13, 3.4e-15), 0.0001: (4e-13, 3.4e-15)},
        sigma={0.0: dict(dense=(9e-27, 8.5e-29), sparse=(7e-27, 6.9e-29), pcg=(2e-25, 1.3e-27)), 0.0001: dict(dense=(1e-26, 9.2e-29), sparse=(1e-26, 9.2e-29), pcg=(2e-25, 1.2e-27))},
        min_sigma={0.0: 1.9e-15, 0.0001: 1.9e-15},
        cg_iterations={0.0: dict(jacobi=66, band=19), 0.0001: dict(jacobi=66, band=19)}),
    "scaled_down": dict(
        kappa=6.6e+02, g0=2.9e-12, min_diag=1.4e-10,
        evaluate=dict(cost=(2e-14, 1.1e-16), chi2=(2e-14, 1.7e-16), e=(2e-13, 1.5e-15), r=(2e-13, 1.7e-15), g=(2e-13, 1.5e-15)),
        gradient=(2e-22, 1.2e-24),
        cg_tolerance={0.0: (4e-13, 3.4e-15), 0.0001: (7e-14, 6.7e-16)},
        sigma={0.0: dict(dense=(2e-02, 1.0e-04), sparse=(9e-03, 8.4e-05), pcg=(2e-01, 1.5e-03)), 0.0001: dict(dense=(7e-04, 6.7e-06), sparse=(2e-04, 1.9e-06), pcg=(3e-02, 2.1e-04))},
        min_sigma={0.0: 2.3e+09, 0.0001: 1.2e+09},
        cg_iterations={0.0: dict(jacobi=66, band=19), 0.0001: dict(jacobi=39, band=18)}),
    "corridor_huber": dict(
        kappa=1.4e+07, g0=4.0e+01, min_diag=3.0e+02,
        evaluate=dict(cost=(3e-13, 2.5e-15), chi2=(7e-13, 6.8e-15), e=(6e-13, 5.1e-15), r=(8e-12, 7.6e-14), g=(2e-11, 1.1e-13)),
        gradient=(2e-08, 1.2e-10),
        cg_tolerance={0.0: (2e-08, 1.0e-10), 0.0001: (4e-10, 3.7e-12)},
        sigma={0.0: dict(dense=(2e-10, 2.0e-12), sparse=(6e-10, 5.5e-12), pcg=(2e-08, 1.4e-10)), 0.0001: dict(dense=(6e-12, 5.6e-14), sparse=(6e-12, 5.5e-14), pcg=(3e-10, 2.3e-12))},
        min_sigma={0.0: 2.5e-06, 0.0001: 1.7e-06},
        cg_iterations={0.0: dict(jacobi=176, band=30), 0.0001: dict(jacobi=146, band=24)}),
    "corridor_cauchy": dict(
        kappa=1.3e+07, g0=1.1e+01, min_diag=2.7e+02,
        evaluate=dict(cost=(2e-12, 1.8e-14), chi2=(7e-13, 6.8e-15), e=(6e-13, 5.1e-15), r=(8e-12, 7.6e-14), g=(1e-10, 9.3e-13)),
        gradient=(7e-09, 6.1e-11),
        cg_tolerance={0.0: (2e-08, 1.1e-10), 0.0001: (4e-10, 3.4e-12)},
        sigma={0.0: dict(dense=(4e-10, 3.6e-12), sparse=(9e-11, 8.8e-13), pcg=(2e-08, 1.4e-10)), 0.0001: dict(dense=(5e-12, 4.6e-14), sparse=(5e-12, 4.5e-14), pcg=(2e-10, 1.9e-12))},
        min_sigma={0.0: 2.5e-06, 0.0001: 1.8e-06},
        cg_iterations={0.0: dict(jacobi=184, band=33), 0.0001: dict(jacobi=151, band=28)}),
}
