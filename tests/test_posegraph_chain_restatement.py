"""The "chain" preconditioner's contract in numpy (tests/posegraph_chain_restatement.py), without a
GPU: the band M is positive definite for every designed case and mask, the block cyclic reduction
solves it as a dense Cholesky does, what M leaves out of H + lambda D has the rank the contract
claims, and the restated LM / PCG loop needs no more CG iterations with it than with the Jacobi
blocks -- one per LM step on a pure chain, where M is H + lambda D."""
import numpy as np
import pytest

import posegraph_cases as PC
import posegraph_chain_cases as CC
import posegraph_chain_restatement as CR
import posegraph_restatement as R

RELATIVE = 1e-10


def _closures(P):
    """The constraints whose ends are not neighbours."""
    return np.abs(P.begin - P.end) != 1


def _masks(P):
    """Every closure on; every second one off."""
    on = np.ones(P.m, dtype=np.uint8)
    half = on.copy()
    half[np.nonzero(_closures(P))[0][::2]] = 0
    return on, half


@pytest.mark.parametrize("name", list(PC.TABLE))
def test_the_band_is_positive_definite_on_every_case_and_mask(name):
    P = PC.problem(name)
    for mask in _masks(P):
        for lam in (1e-4, 1e-12):
            M = CR.band(P, P.poses, mask, lam)
            assert np.array_equal(M, M.T)
            np.linalg.cholesky(M)                       # (raises unless positive definite)


def _reduction_against_dense(P, enabled=None, lam=1e-4):
    M = CR.band(P, P.poses, enabled, lam)
    _, g, free, _ = CR.damped(P, P.poses, enabled, lam)
    rng = np.random.default_rng(7)
    worst = 0.0
    for r in (-g, np.where(np.repeat(free, 3), rng.normal(0.0, 1.0, 3 * P.n), 0.0)):
        want = CR.dense_solve(M, r)
        got = CR.cyclic_reduction(*CR.blocks(M), r).reshape(-1)
        assert np.all(got[~np.repeat(free, 3)] == 0.0)                # a node that is not free: z = 0
        scale = float(np.max(np.abs(want)))
        if scale > 0.0:
            worst = max(worst, float(np.max(np.abs(got - want))) / scale)
    return worst


def _sized(n):
    if n == 1:
        return R.Problem([[0.5, -0.5, 0.25]], [], [], np.zeros((0, 3)), np.zeros((0, 3, 3)))
    return R.Problem(**CC.chain(n, 50 + n, closures=[(0, n - 1)] if n >= 3 else ()))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 33])
def test_the_reduction_is_the_dense_solve_at_every_small_size(n):
    P = _sized(n)
    for lam in (1e-4, 1e-12):
        assert _reduction_against_dense(P, lam=lam) <= RELATIVE


def test_the_reduction_is_the_dense_solve_on_the_pure_chain_of_1025():
    assert _reduction_against_dense(CC.problem("chain_1025")) <= RELATIVE


@pytest.mark.parametrize("name", ["fixed_middle", "fixed_last", "reversed", "doubled", "isolated"])
def test_the_reduction_on_cut_reversed_and_doubled_chains(name):
    P = CC.problem(name)
    worst = _reduction_against_dense(P)
    print("%s: %.2e" % (name, worst))
    assert worst <= RELATIVE
    M = CR.band(P, P.poses)
    D, U = CR.blocks(M)
    if name == "fixed_middle":
        assert not U[9].any() and not U[10].any() and U[8].any() and U[11].any()       # the chain is cut at the fixed node
    if name == "isolated":
        assert not U[10].any() and not U[11].any() and np.array_equal(D[11], np.eye(3))
    if name == "reversed":
        assert not U[0].any() and U[1].any() and U[7].any() and U[8].any() and U[19].any()                 # begin = i + 1 still couples i and i + 1
    if name == "doubled":
        single = CR.blocks(CR.band(R.Problem(**CC.chain(21, 39, closures=[(2, 17)])), P.poses))[1]
        assert np.max(np.abs(U[9] - single[9])) > 0.1 * np.max(np.abs(single[9]))       # both copies are in the block


def test_a_switched_off_odometry_edge_cuts_the_chain():
    P = CC.problem("fixed_first")
    mask = np.ones(P.m, dtype=np.uint8)
    mask[10] = 0                                                       # the edge (10, 11)
    assert _reduction_against_dense(P, mask) <= RELATIVE
    U = CR.blocks(CR.band(P, P.poses, mask))[1]
    assert not U[10].any() and U[9].any() and U[11].any()


@pytest.mark.parametrize("name", ["square", "line", "hub"])
def test_what_the_band_leaves_out_has_rank_6_per_closure(name):
    P = PC.problem(name)
    for mask in _masks(P):
        A = CR.damped(P, P.poses, mask)[0]
        M = CR.band(P, P.poses, mask)
        f = P.free(mask)
        rest = (A - M)[np.ix_(f, f)]
        closures = int(np.sum(_closures(P) & (mask != 0)))
        rank = int(np.linalg.matrix_rank(rest, tol=1e-9 * max(1.0, float(np.max(np.abs(A))))))
        print("%s: rank %d, %d closure(s)" % (name, rank, closures))
        assert rank <= 6 * closures


@pytest.mark.parametrize("name", ["line", "square", "wrap"])
def test_the_restated_solver_needs_no_more_cg_iterations_with_the_chain(name):
    P, gate = PC.problem(name), PC.gate(name)
    jacobi, chain = CR.lm(P, "jacobi", gate), CR.lm(P, "chain", gate)
    print("%s: jacobi %d LM %d CG, chain %d LM %d CG" % (name, jacobi["iterations"], jacobi["cg_iterations"], chain["iterations"],
                                                          chain["cg_iterations"]))
    assert jacobi["converged"] and chain["converged"]
    assert chain["cg_iterations"] <= jacobi["cg_iterations"]
    assert P.gradient_norm(chain["x"]) <= 2.0 * gate


def test_on_a_pure_chain_one_cg_iteration_is_exact():
    P = R.Problem(**CC.chain(33, 60))
    gate = 100.0 * P.solve()["gradient"]
    got = CR.lm(P, "chain", gate)
    print("chain of 33: %d LM, CG per step %s" % (got["iterations"], got["cg_per_iteration"]))
    assert got["converged"] and all(k == 1 for k in got["cg_per_iteration"])
    assert CR.lm(P, "jacobi", gate)["cg_iterations"] > got["cg_iterations"]        # (not met trivially)
