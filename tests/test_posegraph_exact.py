"""tests/posegraph_exact.py (the extended-precision yardstick) against closed forms and the float64
restatement on the small cases, and the table of tests/posegraph_hard_cases.py held to what it was
measured from.

i.   pair, line and square: the exact minimiser is the closed form (pair: p_a composed with t, line:
     posegraph_cases.line_answer) to 1e-28; on the line the variance of x_i is the resistance of
     i links in parallel with n + 1 - i, each 1 / 100; the restatement's solutions have an exact
     |g|_inf within their recorded gates; evaluate and the inverse agree within the project's parity
     bound and the dense inverse's own defect.
ii.  every entry of posegraph_hard_cases.TABLE is measured again: measured <= gate / 10, the spare
     factor the project keeps, and every gate is 100 x the figure beside it, rounded up to one digit.
iii. conditions (a) and (b) of posegraph_hard_cases.py for every case."""
import math

import numpy as np
import pytest

import posegraph_cases as PC
import posegraph_exact as X
import posegraph_hard_cases as HC
import posegraph_marginals_cases as MC
import posegraph_marginals_restatement as MR

PARITY = 1e-12
ALL = list(HC.CASES) + list(HC.ROBUST)


def _graph(name):
    P = PC.problem(name)
    return P, X.Graph(P.poses, P.begin, P.end, P.transform, P.information, fixed=P.fixed, weighting=P.weighting)


def _within(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return bool(np.all(np.abs(got - want) <= PARITY * np.maximum(1.0, np.abs(want))))


def test_normalize_and_the_small_inverse():
    for v in (-X.PI, X.PI, 3 * X.PI, X.mpf(1e6), X.mpf(0), X.mpf(-2.9), X.mpf(6.5), X.mpf(75.0)):
        r = X.normalize(v)
        assert -X.PI <= r < X.PI and abs((v - r) / X.TWO_PI - X.mp.nint((v - r) / X.TWO_PI)) < X.mpf("1e-45")
    assert X.normalize(X.PI) == -X.PI and X.normalize(-X.PI) == -X.PI
    a = X._mat(PC.INFO_FULL, 3, 3)
    inv = X.inverse(a)
    unit = X._matmul(a, inv)
    assert max(abs(unit[i][j] - (1 if i == j else 0)) for i in range(3) for j in range(3)) < X.mpf("1e-45")
    assert X.cholesky(X._mat([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]], 3, 3)) is None
    with pytest.raises(ValueError, match="constraint 0"):
        X.Graph([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [0], [1], [[1.0, 0.0, 0.0]], [np.zeros((3, 3))])


@pytest.mark.parametrize("name", ["pair", "line", "square", "square_information", "square_fixed_2"])
def test_the_exact_module_against_the_restatement(name):
    P, E = _graph(name)
    # evaluate at the start poses
    e, r, chi2 = P.residuals(P.poses)
    g, _ = P.gradient_hessian(P.poses)
    want = E.evaluate()
    assert _within(e, want["e"]) and _within(r, want["r"]) and _within(chi2, want["chi2"]) and _within(P.cost(P.poses), want["cost"])
    assert _within(np.where(P.free(), g, 0.0), want["g"])
    # the restatement's solution under the exact gradient, and the two minimisers
    ref, best = PC.solution(name), E.minimiser()
    at_ref = E.gradient_norm(ref["x"])
    floor = PC.TABLE[name][3]
    bound = 2.0 * P.inverse_norm(ref["x"]) * PC.gate(name)
    err = float(np.max(np.abs(best["x"] - ref["x"])))
    print("%s: exact |g| at the restatement's solution %.2e (its own %.2e, recorded floor %.1e, gate %.0e); exact minimiser |g| %.1e after %d steps; "
          "|x - x_ref| %.2e (bound %.2e)" % (name, at_ref, ref["gradient"], floor, PC.gate(name), best["gradient"], best["iterations"], err, bound))
    assert best["gradient"] < 1e-30
    assert at_ref <= 10.0 * floor
    assert err <= bound
    # Sigma at the exact minimiser against the dense inverse, within that inverse's own defect
    for damping in (0.0, 1e-4):
        S = MR.System(P, best["x"], damping=damping)
        C = E.covariance(best["x"], damping=damping)
        assert list(S.index) == list(C["index"])
        assert np.max(np.abs(S.A - C["A"])) <= PARITY * np.max(np.abs(C["A"]))
        limit = S.inverse_norm() * (S.defect() + 100.0 * np.finfo(np.float64).eps)
        assert np.max(np.abs(S.inverse() - C["sigma"])) <= limit, (name, damping)
        assert E.defect(C["A_exact"], C["sigma"]) <= 3.0 * np.finfo(np.float64).eps * float(np.max(np.abs(S.A) @ np.abs(C["sigma"])))


def test_pair_and_line_have_their_closed_forms():
    P, E = _graph("pair")
    a, t = [X.mpf(float(v)) for v in P.poses[0]], [X.mpf(float(v)) for v in P.transform[0]]
    c, s = X.mp.cos(a[2]), X.mp.sin(a[2])
    closed = [a[0] + c * t[0] - s * t[1], a[1] + s * t[0] + c * t[1], a[2] + t[2]]
    best = E.minimiser()
    assert max(abs(best["exact"][1][k] - closed[k]) for k in range(3)) < X.mpf("1e-28") and best["cost"] < 1e-55
    n, delta = 20, 0.5
    P, E = _graph("line")
    best = E.minimiser()
    for i in range(n + 1):
        want = [i * (1 - X.mpf(delta) / (n + 1)), 0, 0]
        assert max(abs(best["exact"][i][k] - want[k]) for k in range(3)) < X.mpf("1e-28"), i
    # on the axis with every heading 0, x decouples from (y, theta): a chain of resistors of 1 / 100
    C = E.covariance(PC.line_answer())
    at = {u: k for k, u in enumerate(C["index"])}
    for i in range(1, n + 1):
        want = X.mpf(i * (n + 1 - i)) / (n + 1) / 100
        assert abs(C["exact"][at[3 * i]][at[3 * i]] - want) < X.mpf("1e-40"), i


def test_relative_and_distance_against_the_restatement():
    P, x, (a, b), cov_meas = MC.verdict_case()
    S = MR.System(P, x)
    joint = S.blocks([a, b])
    t, cov = X.relative(x[a], x[b], joint)
    t_ref, cov_ref = MR.relative(math.cos(x[a][2]), math.sin(x[a][2]), x[a], x[b], joint)
    assert _within(t, t_ref) and np.max(np.abs(cov - cov_ref)) <= PARITY * np.max(np.abs(cov_ref))
    meas = t_ref + np.array([0.01, -0.02, 0.005 + 2.0 * math.pi])
    d2, d2_ref = X.distance(t, cov, meas, cov_meas), MR.distance(t_ref, cov_ref, meas, cov_meas)
    assert abs(d2 - d2_ref) <= 1e-10 * d2_ref


@pytest.mark.parametrize("name", ALL)
def test_the_table_is_what_the_restatements_leave(name):
    entry, measured = HC.TABLE[name], HC.measure(name)
    best = HC.minimiser(name)
    assert best["gradient"] < 1e-30

    def held(label, gate_and_figure, now):
        gate, figure = gate_and_figure
        print("%s %s: gate %.0e, recorded %.1e, measured %.2e" % (name, label, gate, figure, now))
        assert now <= gate / 10.0, (name, label, now, gate)
        assert 95.0 * figure <= gate <= 210.0 * figure, (name, label, gate, figure)

    for key, pair in entry["evaluate"].items():
        held("evaluate " + key, pair, measured["evaluate"][key])
    held("gradient", entry["gradient"], measured["gradient"])
    for damping in HC.DAMPINGS:
        held("cg tolerance, damping %g" % damping, entry["cg_tolerance"][damping], measured["cg_tolerance"][damping])
        for path in HC.PATHS:
            held("sigma %s, damping %g" % (path, damping), entry["sigma"][damping][path], measured["sigma"][damping][path])
        assert 0.5 <= measured["min_sigma"][damping] / entry["min_sigma"][damping] <= 2.0
    assert ("derived" in entry) == (name in HC.DERIVED)
    for key, pair in entry.get("derived", {}).items():
        held("derived " + key, pair, measured["derived"][key])
    assert 0.1 <= measured["kappa"] / entry["kappa"] <= 10.0 and 0.5 <= measured["g0"] / entry["g0"] <= 2.0
    assert 0.5 <= measured["min_diag"] / entry["min_diag"] <= 2.0
    print("%s: kappa(H) %.1e, min diag(H) %.1e, |g(x0)| %.1e, |H^-1|_inf %.1e, CG iterations %s" %
          (name, measured["kappa"], measured["min_diag"], measured["g0"], measured["inverse_norm"], measured["cg_iterations"]))


@pytest.mark.parametrize("name", ALL)
def test_the_two_conditions(name):
    entry = HC.TABLE[name]
    # (a) the project's rule: passing the gradient gate means six digits of the start gradient are gone
    assert entry["gradient"][0] <= 1e-6 * entry["g0"], (name, entry["gradient"][0], entry["g0"])
    # (b) an error of 10 % of any variance cannot pass
    for damping in HC.DAMPINGS:
        smallest = float(np.min(np.diag(HC.covariance(name, damping)["sigma"])))
        assert 0.5 <= smallest / entry["min_sigma"][damping] <= 2.0
        for path in HC.PATHS:
            assert entry["sigma"][damping][path][0] <= 1e-2 * smallest, (name, damping, path)


def test_the_cases_reach_their_regimes():
    T = HC.TABLE
    assert T["corridor"]["kappa"] > 1e6 and T["mixed"]["kappa"] > 1e9 and T["weak_leaf"]["kappa"] > 1e10
    assert T["weak_leaf"]["min_diag"] < 1e-6 < T["corridor"]["min_diag"]              # the clamp acts on the leaf only
    assert HC.graph("corridor_information")["fixed"] != 0 and HC.graph("mixed")["fixed"] != 0
    # far: coordinates of 5e4 m, Normalize on tens of radians
    far = HC.problem("far")
    v = (far.poses[far.end, 2] - far.poses[far.begin, 2]) - far.transform[:, 2]
    assert np.max(np.abs(far.poses[:, :2])) > 3e4 and np.max(np.abs(v)) > 50.0 and np.min(far.poses[:, 2]) > 50.0
    # lever: arms of tens of metres, the theta block 1e3 x the xy block
    lever = HC.problem("lever")
    A, _ = lever.jacobians(lever.poses)
    assert np.max(np.abs(A[:, :2, 2])) > 30.0
    _, H = lever.gradient_hessian(lever.poses)
    ratios = [H[3 * i + 2, 3 * i + 2] / H[3 * i, 3 * i] for i in range(1, lever.n)]
    assert max(ratios) > 1e3
    # mixed: eight orders between the odometry's and the closures' information
    mixed = HC.graph("mixed")
    assert mixed["information"][-1][0, 0] / mixed["information"][0][0, 0] == pytest.approx(1e8)
    # pinched: one node's 3 x 3 block of H at kappa 1e7, the others' below 1e4
    P = HC.problem("pinched")
    _, H = P.gradient_hessian(P.poses)
    kappas = [np.linalg.cond(H[3 * i:3 * i + 3, 3 * i:3 * i + 3]) for i in range(1, P.n)]
    assert kappas[-1] > 5e6 and max(kappas[:-1]) < 1e4
    # the scalings are exact
    up, down, base = HC.graph("scaled_up"), HC.graph("scaled_down"), HC.base()
    assert np.array_equal(up["information"][0], PC.INFO_FULL * 2.0 ** 40) and np.array_equal(down["information"][0], PC.INFO_FULL * 2.0 ** -40)
    assert np.array_equal(up["poses"], base["poses"]) and np.array_equal(down["transform"], base["transform"])
    assert np.array_equal(HC.problem("scaled_up").W, HC.problem("base").W * 2.0 ** 20)
    assert np.array_equal(HC.problem("scaled_down").W, HC.problem("base").W * 2.0 ** -20)


def test_the_leaf_pins_the_clamp():
    """weak_leaf at damping 1e-4: the leaf's diagonal of H is 1e-8, the clamp lifts it to 1e-6 in the damping, and
    the leaf's variances are 1 / (1e-8 + 1e-4 x 1e-6) against 1 / (1e-8 + 1e-4 x 1e-8) without it: 1 % apart,
    1e4 x the gates on Sigma."""
    with_clamp = HC.covariance("weak_leaf", 1e-4)["sigma"]
    without = HC.covariance("weak_leaf", 1e-4, clamp=False)["sigma"]
    leaf = slice(len(with_clamp) - 3, len(with_clamp))
    apart = np.abs(np.diag(with_clamp)[leaf] - np.diag(without)[leaf])
    gate = max(HC.gate("weak_leaf", "sigma", 1e-4, path) for path in HC.PATHS)
    print("the leaf's variances: %s with the clamp, %s without; gate %.0e" % (np.diag(with_clamp)[leaf], np.diag(without)[leaf], gate))
    assert np.all(apart > 1e3 * gate) and np.all(apart / np.diag(with_clamp)[leaf] > 5e-3)


def test_the_robust_cases_have_constraints_on_both_sides_of_the_scale():
    for name, beyond in (("corridor_huber", 11), ("corridor_cauchy", 7)):
        scale = HC.ROBUST[name][2]
        ev = HC.exact(name).evaluate(HC.minimiser(name)["x"])
        assert int(np.sum(ev["chi2"] > scale * scale)) == beyond, name
        assert np.all(ev["weights"][ev["chi2"] > scale * scale] < (1.0 if "huber" in name else 0.5))
