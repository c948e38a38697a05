"""The marginal covariances' restatement (tests/posegraph_marginals_restatement.py) against answers
known otherwise, without a GPU: a resistor chain's closed form, `relative` against propagation
through central-difference Jacobians, `distance` against numpy, the gate table of
tests/posegraph_marginals_cases.py against the gaps measured again, the case that makes the three
columns of a node stop at different iterations, and the closure verdicts the GPU test repeats."""
import math

import numpy as np
import pytest

import posegraph_cases as PC
import posegraph_marginals_cases as MC
import posegraph_marginals_restatement as MR
import posegraph_restatement as R

CHI2_3_999 = 16.27          # the 99.9 % point of chi^2 with 3 degrees of freedom (16.266)


def test_a_known_answer_the_grounded_resistor_chain():
    """posegraph_cases.line() at line_answer(): theta = 0 and e_y' = 0 everywhere, so x decouples
    from y and theta, and its H is the Laplacian of a chain of n + 1 conductances of 100 from the
    held pose 0 through 1 .. n back to 0 (the closure).  The variance of x_i is the resistance from
    node i to ground: i / 100 in parallel with (n + 1 - i) / 100."""
    n = 20
    P = R.Problem(**PC.line(n))
    S = MR.System(P, PC.line_answer(n))
    worst = 0.0
    for i in range(1, n + 1):
        want = i * (n + 1 - i) / (100.0 * (n + 1))
        got = S.column(i)[i]
        worst = max(worst, abs(got[0, 0] - want) / want)
        assert abs(got[0, 0] - want) <= 1e-12 * want, (i, got[0, 0], want)
        assert abs(got[0, 1]) <= 1e-12 * want and abs(got[0, 2]) <= 1e-12 * want      # x is decoupled
    assert not S.node_free(0) and np.all(S.column(0) == 0.0)
    print("line: worst relative error of Sigma_xx(i, i) against i (n + 1 - i) / (100 (n + 1)): %.2e" % worst)


def test_relative_against_central_differences():
    """cov = J joint J^T with J = d(transform) / d(pose a, pose b): central differences with h = 1e-6
    have an error of 1e-12 |t'''| and a rounding of 1e-16 |t| / 1e-6 = 1e-10, so J is good to 1e-9
    and the covariance to 1e-8 relative to its size."""
    rng = np.random.default_rng(12)
    for _ in range(10):
        pa, pb = rng.normal(0.0, 2.0, 3), rng.normal(0.0, 2.0, 3)
        g = rng.normal(0.0, 0.1, (6, 6))
        six = g @ g.T + 1e-3 * np.eye(6)
        joint = six.reshape(2, 3, 2, 3).transpose(0, 2, 1, 3)
        t, cov = MR.relative(math.cos(pa[2]), math.sin(pa[2]), pa, pb, joint)
        assert np.allclose(t, MR.transform_between(pa, pb), rtol=0.0, atol=1e-15 * 8.0)
        J = np.zeros((3, 6))
        z = np.concatenate([pa, pb])
        for k in range(6):
            hi, lo = z.copy(), z.copy()
            hi[k] += 1e-6
            lo[k] -= 1e-6
            J[:, k] = (MR.transform_between(hi[:3], hi[3:]) - MR.transform_between(lo[:3], lo[3:])) / (hi[k] - lo[k])
        want = J @ six @ J.T
        assert np.max(np.abs(cov - want)) <= 1e-8 * np.max(np.abs(want)), np.max(np.abs(cov - want))
        # a held pose a: only b's block counts
        held = joint.copy()
        held[0, 0] = held[0, 1] = held[1, 0] = 0.0
        _, cov_b = MR.relative(math.cos(pa[2]), math.sin(pa[2]), pa, pb, held)
        assert np.max(np.abs(cov_b - J[:, 3:] @ six[3:, 3:] @ J[:, 3:].T)) <= 1e-8 * np.max(np.abs(want))
        # the joint is symmetrised: a skew part changes nothing
        skew = rng.normal(0.0, 1e-3, (6, 6))
        skew = (skew - skew.T).reshape(2, 3, 2, 3).transpose(0, 2, 1, 3)
        _, cov_s = MR.relative(math.cos(pa[2]), math.sin(pa[2]), pa, pb, joint + skew)
        assert np.max(np.abs(cov_s - cov)) <= 1e-15 * 64.0


def test_distance_against_numpy():
    """On the covariances of test_make_constraint_is_the_references (condition numbers of a few):
    e^T inv(S) e by numpy within 1e-12 relative."""
    rng = np.random.default_rng(8)
    for k in range(20):
        a = rng.normal(0.0, 1.0, (3, 3))
        cov = a @ a.T + 3.0 * np.eye(3)
        cov *= 10.0 ** rng.uniform(-4, 0)
        b = rng.normal(0.0, 1.0, (3, 3))
        cov2 = (b @ b.T + 3.0 * np.eye(3)) * 10.0 ** rng.uniform(-4, 0)
        tp, tm = rng.normal(0.0, 3.0, 3), rng.normal(0.0, 3.0, 3)
        if k % 2:
            tm[2] = tp[2] + 2.0 * R.PI + 0.01                               # a whole turn away: e_theta = 0.01
        e = tm - tp
        e[2] = float(R.normalize(e[2]))
        want = float(e @ np.linalg.inv(cov + cov2) @ e)
        got = MR.distance(tp, cov, tm, cov2)
        assert abs(got - want) <= 1e-12 * want, (got, want)
    assert MR.distance(tp, cov, tp, cov2) == 0.0
    assert MR.distance(tp, -cov, tm, 0.5 * cov) is None                     # the sum is not positive definite
    assert MR.distance(tp, cov * np.nan, tm, cov) is None


@pytest.mark.parametrize("name", MC.SMALL + MC.CHAIN[:-1] + ("loop_1023",))
def test_the_gates_hold_the_restatement(name):
    """The gaps measured again (the thousand-pose Jacobi runs, 18 s each, and chain_1025 are left to
    the table): each within the gate's rule, the restatement converged, its true residual inside
    the gate with a factor of 2 of room at the least."""
    for prec in MC.PRECONDITIONERS:
        if (name, prec) not in MC.GATES or (name in MC.THOUSAND and prec == "jacobi"):
            continue
        gate, raw, its = MC.GATES[(name, prec)]
        gap, got = MC.measure_gap(name, prec)
        S = MC.system(name)
        nodes = sorted({q for q in MC.queries(name) if S.node_free(q)})
        cols = np.concatenate([S.inverse()[:, np.searchsorted(S.index, 3 * q):np.searchsorted(S.index, 3 * q) + 3] for q in nodes], axis=1)
        err = float(np.max(np.abs(got["x"].reshape(len(S.A), -1) - cols)))
        print("%s %s: gap %.1e (table %.1e), gate %.0e, true residual <= %.2e, %d..%d iterations, error against the dense inverse %.2e (bound %.2e)"
              % (name, prec, gap, raw, gate, got["true"].max(), got["iterations"].min(), got["iterations"].max(), err, MC.bound(name, prec)))
        assert math.isclose(gate, MC.round_up(MC.TOLERANCE + 100.0 * raw), rel_tol=1e-12)
        assert MC.round_up(MC.TOLERANCE + 100.0 * gap) <= gate * (1.0 + 1e-12)
        assert got["true"].max() <= 0.5 * gate + MC.TOLERANCE and err <= MC.bound(name, prec)
        assert abs(int(got["iterations"].max()) - its) <= max(2, its // 20)


def test_every_gate_of_the_table_follows_the_rule():
    for (name, prec), (gate, raw, its) in MC.GATES.items():
        assert math.isclose(gate, MC.round_up(MC.TOLERANCE + 100.0 * raw), rel_tol=1e-12) and its <= MR.cg_cap(MC.size(name)), (name, prec)
    for name in MC.THOUSAND:
        assert MC.GATES[(name, "chain")][2] <= MC.GATES[(name, "jacobi")][2]


def test_the_columns_of_a_hub_spoke_stop_at_three_different_iterations():
    """What the lockstep test on the device needs: one node whose three columns freeze one by one."""
    got = MC.system("hub").pcg([MC.FREEZE_NODE], "jacobi", MC.TOLERANCE)
    its = got["iterations"][0]
    print("hub node %d: columns stop after %s iterations" % (MC.FREEZE_NODE, its.tolist()))
    assert len(set(its.tolist())) == 3 and np.all(got["status"] == MR.CONVERGED) and np.all(got["recurrence"] <= MC.TOLERANCE)


def test_closure_verdicts_on_the_restatement():
    """A closure that says what the graph says has d2 = 0 < 16.27, the 99.9 % point of chi^2 with 3
    degrees of freedom; the same closure shifted by 1 m in x has more.  Between neighbours (i, i + 1)
    the predicted covariance is at most the odometry constraint's own (more information never makes
    a covariance larger), 0.01-ish here, and the closure's own is the same: 1 m is then 7 sigma."""
    P, x, nodes, cov_meas = MC.verdict_case()
    S = MR.System(P, x)
    a, b = nodes
    t, cov = MR.relative(math.cos(x[a, 2]), math.sin(x[a, 2]), x[a], x[b], S.blocks([a, b]))
    assert np.max(np.linalg.eigvalsh(0.5 * (cov + cov.T))) <= np.max(np.linalg.eigvalsh(np.linalg.inv(PC.INFO_FULL))) * (1.0 + 1e-9)
    same = MR.distance(t, cov, t, cov_meas)
    shifted = MR.distance(t, cov, t + np.array([1.0, 0.0, 0.0]), cov_meas)
    print("verdicts: d2 %.3e for the graph's own prediction, %.1f for 1 m off" % (same, shifted))
    assert same == 0.0 and same < CHI2_3_999 < shifted
