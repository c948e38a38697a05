"""The dense covariance on the device (ndt2d_covariance_*, PoseGraph.covariances) against the numpy
restatement's dense system (tests/posegraph_marginals_restatement.py's System) on the designed graphs
of the pose-graph tests.

The gate, against the restatement and never against the device: with A restated densely and the
WHOLE Sigma_dev placed into F (every block (a, b), a >= b, asked as a pair, the others their
transposes -- which the contract says they are bit for bit, and test_determinism holds),
    |A Sigma_dev - I|_max <= 100 x max(System.defect(), eps max(|A| |Sigma_ref|)),
100 x being the project's margin over a restatement's own floor (the blocked algorithm restated in
numpy stays within 11.3 x: tests/test_posegraph_dense_restatement.py).  From it follows
    max|Sigma_dev - Sigma_ref| <= |A^-1|_inf (gate + defect)."""
import math

import numpy as np
import pytest

import posegraph_cases as PC
import posegraph_chain_cases as CH
import posegraph_dense_restatement as DR
import posegraph_marginals_cases as MC
import posegraph_marginals_restatement as MR
import posegraph_restatement as R
import posegraph_robust_cases as RC
import posegraph_robust_restatement as RR
from ndt_2d_amd import Ndt2dError, PoseGraph, ScanMatcherNDT, _capi, graph_io, make_constraint

pytestmark = pytest.mark.gpu

DAMPINGS = (0.0, 1e-4)
OK, NPD = _capi.COVARIANCE_OK, _capi.COVARIANCE_NOT_POSITIVE_DEFINITE
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


def _upload(P, x, key, max_jobs=8, switchable=None):
    graphs = _STATE.setdefault("graphs", {})
    if key not in graphs:
        pg = PoseGraph(_matcher(), max_nodes=P.n, max_constraints=max(1, P.m), max_jobs=max_jobs)
        pg.set_weighting(P.weighting)
        pg.set_graph(x, begin=P.begin, end=P.end, transform=P.transform, information=P.information, fixed=P.fixed,
                     switchable=np.ones(P.m, dtype=bool) if switchable is None else switchable)
        graphs[key] = pg
    return graphs[key]


def _lower(n):
    a, b = np.tril_indices(n)
    return np.stack([a, b], axis=1)


def _whole(n, got, k=0):
    """Job k's whole Sigma [3n, 3n] from the lower blocks asked as pairs (_lower(n)) and their transposes;
    the diagonal blocks must be the pairs (a, a)."""
    a, b = np.tril_indices(n)
    full = np.zeros((n, n, 3, 3))
    full[a, b] = got["pairs"][k]
    full[b, a] = got["pairs"][k].transpose(0, 2, 1)
    assert np.array_equal(full[np.arange(n), np.arange(n)], got["diagonal"][k])
    return full.transpose(0, 2, 1, 3).reshape(3 * n, 3 * n)


def _check(label, S, sigma, got, k=0):
    """Job k against the dense system S: the gate, the bound on the values, zeros outside F."""
    assert got["status"][k] == OK and got["failed"][k] == -1, (label, got["status"][k], got["failed"][k])
    held = np.ones(3 * S.n, dtype=bool)
    held[S.index] = False
    assert np.all(sigma[held] == 0.0) and np.all(sigma[:, held] == 0.0), label
    assert np.array_equal(got["diagonal"][k], got["diagonal"][k].transpose(0, 2, 1)), label
    inside = sigma[np.ix_(S.index, S.index)]
    floor = DR.floor(S)
    residual = float(np.max(np.abs(S.A @ inside - np.eye(len(S.A))))) if len(S.A) else 0.0
    err = float(np.max(np.abs(inside - S.inverse()))) if len(S.A) else 0.0
    bound = S.inverse_norm() * (100.0 * floor + S.defect()) if len(S.A) else 0.0
    print("%s: |A Sigma - I| %.2e = %.2f x the floor %.1e (gate 100 x), |Sigma - Sigma_ref| %.2e (bound %.2e), pivot ratio %.2e"
          % (label, residual, residual / floor if floor else 0.0, floor, err, bound, got["pivot_ratio"][k]))
    assert residual <= 100.0 * floor, (label, residual, floor)
    assert err <= bound, (label, err, bound)
    assert DR.singular_limit(3 * S.n) < got["pivot_ratio"][k] <= 1.0, (label, got["pivot_ratio"][k])
    return bound


VALUE_CASES = MC.SMALL + tuple(CH.EDGES) + ("chain_1025",) + MC.THOUSAND


@pytest.mark.parametrize("name", VALUE_CASES)
def test_values_against_the_dense_inverse(name):
    P, x = MC.case(name)
    pg = _upload(P, x, name)
    pairs = _lower(P.n)
    for damping in DAMPINGS:
        S = MC.system(name, damping)
        got = pg.covariances(damping=damping, pairs=pairs)
        sigma = _whole(P.n, got)
        bound = _check("%s, damping %g" % (name, damping), S, sigma, got)
        if name == "line" and damping == 0.0:
            n = 20
            for i in range(1, n + 1):          # a grounded resistor chain (tests/test_posegraph_marginals_restatement.py)
                want = i * (n + 1 - i) / (100.0 * (n + 1))
                assert abs(got["diagonal"][0, i, 0, 0] - want) <= bound + 1e-12 * want, (i, got["diagonal"][0, i, 0, 0], want)
        if name == "isolated":
            assert np.all(got["diagonal"][0, 11] == 0.0) and np.all(got["diagonal"][0, P.fixed] == 0.0)


def test_panel_edges():
    """Chains of 2 to 70 poses (d = 6 ... 210) at their start poses: one, two and four panels of 48
    and one and two of 96, each at -3 / 0 / +3 unknowns."""
    pg = PoseGraph(_matcher(), max_nodes=70, max_constraints=80, max_jobs=2)
    worst = 0.0
    try:
        for n in range(2, 71):
            P = R.Problem(**CH.chain(n, seed=n, closures=((0, n - 1),) if n > 3 else ()))
            pg.set_graph(P.poses, begin=P.begin, end=P.end, transform=P.transform, information=P.information, fixed=P.fixed)
            S = MR.System(P, P.poses)
            got = pg.covariances(pairs=_lower(n))
            assert got["status"][0] == OK, n
            inside = _whole(n, got)[np.ix_(S.index, S.index)]
            ratio = float(np.max(np.abs(S.A @ inside - np.eye(len(S.A))))) / DR.floor(S)
            worst = max(worst, ratio)
            assert ratio <= 100.0, (n, ratio)
            assert np.max(np.abs(inside - S.inverse())) <= S.inverse_norm() * (100.0 * DR.floor(S) + S.defect()), n
            assert np.all(got["diagonal"][0, 0] == 0.0)
    finally:
        pg.close()
    print("chains of 2 .. 70 poses: |A Sigma - I| at most %.2f x the floor" % worst)


def test_many_closures():
    """200 poses, 100 closures: the same launches as with none, the same gate."""
    P = R.Problem(**PC.loop(200, 100, seed=9))
    assert P.m == 299
    pg = _upload(P, P.poses, "closures_100")
    for damping in DAMPINGS:
        S = MR.System(P, P.poses, damping=damping)
        got = pg.covariances(damping=damping, pairs=_lower(P.n))
        _check("200 poses, 100 closures, damping %g" % damping, S, _whole(P.n, got), got)


@pytest.mark.parametrize("case", RC.CASES)
def test_masks_change_h_and_sigma(case):
    g = RC.graph(case)[0]
    P = R.Problem(**g)
    x = P.poses
    closures = RC.closures(case)
    pg = _upload(P, x, "masks_" + case, switchable=closures)
    masks = np.ones((2, P.m), dtype=np.uint8)
    masks[1, closures] = 0
    got = pg.covariances(masks=masks, pairs=_lower(P.n))
    bounds = [_check("%s, closures %s" % (case, "off" if k else "on"), MR.System(P, x, enabled=masks[k]), _whole(P.n, got, k), got, k)
              for k in range(2)]
    assert np.max(np.abs(got["diagonal"][0] - got["diagonal"][1])) > bounds[0] + bounds[1]


@pytest.mark.parametrize("loss", RC.LOSSES)
def test_losses_reweight_h(loss):
    """Huber and Cauchy on the closures of loop40 at its start poses, where the false closure is far
    out (rho' < 1): Sigma against the restatement's reweighted H, and away from the unweighted one."""
    g = RC.graph("loop40")[0]
    closures = RC.closures("loop40")
    P = RR.Problem(loss=loss, scale=RC.SCALE, robust=closures, **g)
    x = P.poses
    assert np.min(P.weights(x)) < 0.5 and np.all(P.weights(x)[~closures] == 1.0)
    pg = PoseGraph(_matcher(), max_nodes=P.n, max_constraints=P.m, max_jobs=8)
    try:
        pg.set_loss(loss, RC.SCALE, "switchable")
        pg.set_graph(x, begin=P.begin, end=P.end, transform=P.transform, information=P.information, fixed=P.fixed, switchable=closures)
        got = pg.covariances(pairs=_lower(P.n))
    finally:
        pg.close()
    sigma = _whole(P.n, got)
    bound = _check("loop40 %s" % loss, MR.System(P, x), sigma, got)
    plain = MR.System(R.Problem(**g), x)
    assert np.max(np.abs(sigma[np.ix_(plain.index, plain.index)] - plain.inverse())) > bound


def test_a_floating_component_with_and_without_damping():
    """Two squares, the second not joined to the fixed pose: H_FF is singular at damping 0.  Promised
    is NOT_POSITIVE_DEFINITE (zero blocks, the first failing unknown in the floating square) or OK
    with a pivot ratio under 100 (d + 1) eps -- Cholesky's backward error bounds a singular positive
    semidefinite matrix's last pivots by about (d + 1) eps of the diagonal.  The joined square alone,
    a second job of the same call (the floating square's constraints off: its nodes leave F), is OK
    and correct.  At damping 1e-4 both equal the damped dense inverse."""
    P, x = PC.problem("floating"), PC.solution("floating")["x"]
    pg = _upload(P, x, "floating")
    masks = np.ones((2, P.m), dtype=np.uint8)
    masks[1, 4:] = 0
    got = pg.covariances(masks=masks, pairs=_lower(P.n))
    print("floating, damping 0: status %d, first failing unknown %d, pivot ratio %.2e (limit %.1e)"
          % (got["status"][0], got["failed"][0], got["pivot_ratio"][0], DR.singular_limit(3 * P.n)))
    assert got["status"][0] == NPD or got["pivot_ratio"][0] <= DR.singular_limit(3 * P.n)
    if got["status"][0] == NPD:
        assert 12 <= got["failed"][0] < 24 and np.all(got["diagonal"][0] == 0.0) and np.all(got["pairs"][0] == 0.0)
    _check("the joined square beside it", MR.System(P, x, enabled=masks[1]), _whole(P.n, got, 1), got, 1)
    assert np.all(got["diagonal"][1, 4:] == 0.0)
    damped = pg.covariances(masks=masks, damping=1e-4, pairs=_lower(P.n))
    for k in range(2):
        _check("floating, damping 1e-4, job %d" % k, MR.System(P, x, enabled=masks[k], damping=1e-4), _whole(P.n, damped, k), damped, k)


@pytest.mark.parametrize("name", ("hub", "loop_1025"))
def test_agreement_with_the_cg_marginals(name):
    """The same blocks by the CG marginals: apart by no more than the sum of the two paths' bounds."""
    P, x = MC.case(name)
    pg, S, nodes = _upload(P, x, name), MC.system(name), MC.queries(name)
    pg.set_preconditioner("chain")
    cg = pg.marginals(nodes, tolerance=MC.TOLERANCE)[0]
    grid = [(a, b) for a in nodes for b in nodes]
    dense = pg.covariances(pairs=grid)
    assert dense["status"][0] == OK
    blocks = dense["pairs"][0].reshape(len(nodes), len(nodes), 3, 3)
    bound = MC.bound(name, "chain") + S.inverse_norm() * (100.0 * DR.floor(S) + S.defect())
    apart = float(np.max(np.abs(blocks - cg["blocks"])))
    print("%s: |Sigma_dense - Sigma_cg| %.2e (the two bounds: %.2e)" % (name, apart, bound))
    assert apart <= bound
    for i, a in enumerate(nodes):
        assert np.array_equal(blocks[i, i], dense["diagonal"][0, a])


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def test_determinism():
    P, x = MC.case("wrap")
    pg = _upload(P, x, "wrap")
    pairs = [(5, 1), (1, 5), (23, 23), (12, 7), (7, 12), (0, 3), (3, 0), (5, 1)]
    first = pg.covariances(pairs=pairs)
    assert _same(first, pg.covariances(pairs=pairs))                                 # the same call twice
    for u, v in ((0, 1), (3, 4), (5, 6)):                                            # (a, b) against the transpose of (b, a)
        assert np.array_equal(first["pairs"][0, u], first["pairs"][0, v].T)
    assert np.array_equal(first["pairs"][0, 0], first["pairs"][0, 7]) and np.array_equal(first["pairs"][0, 2], first["diagonal"][0, 23])
    assert np.all(first["pairs"][0, 5] == 0.0) and np.any(first["pairs"][0, 0] != 0.0)
    order = [7, 3, 0, 2, 2, 6]                                                       # another order, duplicated
    other = pg.covariances(pairs=[pairs[q] for q in order])
    assert np.array_equal(other["pairs"][0], first["pairs"][0, order]) and np.array_equal(other["diagonal"], first["diagonal"])
    none = pg.covariances()
    assert none["pairs"].shape == (1, 0, 3, 3) and np.array_equal(none["diagonal"], first["diagonal"])
    # a mask alone against among five
    masks = np.ones((5, P.m), dtype=np.uint8)
    closures = np.nonzero(np.abs(P.begin - P.end) != 1)[0]
    for k in range(1, 5):
        masks[k, closures[k - 1]] = 0
    five = pg.covariances(masks=masks, pairs=pairs, damping=1e-4)
    one = pg.covariances(masks=masks[2:3], pairs=pairs, damping=1e-4)
    assert all(np.array_equal(one[key][0], five[key][2]) for key in one) and not np.array_equal(five["diagonal"][0], five["diagonal"][2])
    # a workspace that holds one job a chunk against all five in one
    job_bytes = 8 * (2 * 96 * 96 + 96 + 3 * P.n)                                     # d = 72: two panels of 48
    assert _same(pg.covariances(masks=masks, pairs=pairs, damping=1e-4, workspace_bytes=job_bytes + 8), five)
    assert _same(pg.covariances(masks=masks, pairs=pairs, damping=1e-4, workspace_bytes=2 * job_bytes), five)
    assert _same(pg.covariances(masks=masks, pairs=pairs, damping=1e-4), five)
    # poses given against the graph's own
    assert _same(pg.covariances(pairs=pairs, poses=x[None]), first)


def test_refusals_a_small_workspace_a_callers_stream_and_timing():
    import ctypes as C
    import torch
    P, x = MC.case("square")
    fresh = PoseGraph(_matcher(), max_nodes=4, max_constraints=4, max_jobs=2)
    try:
        with pytest.raises(Ndt2dError, match="no graph") as ei:
            fresh.covariances()
        assert ei.value.code == _capi.ERR_STATE
    finally:
        fresh.close()
    pg = _upload(P, x, "square")
    want = pg.covariances(pairs=[(1, 3)])

    def refused(text, **kw):
        with pytest.raises(Ndt2dError, match=text) as ei:
            pg.covariances(**kw)
        assert ei.value.code == _capi.ERR_INVALID

    refused("pair 1 names node 4 of 4", pairs=[(1, 3), (4, 0)])
    bad = np.tile(x, (1, 1, 1))
    bad[0, 2, 1] = np.inf
    refused("job 0 pose 2 is not finite", poses=bad)
    refused("damping", damping=-1e-9)
    refused("damping", damping=math.nan)
    need = 8 * (2 * 48 * 48 + 48 + 12)
    refused("needs %d bytes" % need, workspace_bytes=need - 1)
    assert _same(pg.covariances(pairs=[(1, 3)], workspace_bytes=need), want)
    with pytest.raises(Ndt2dError) as ei:
        pg.covariances(workspace_bytes=0)
    assert ei.value.code == _capi.ERR_INVALID
    assert _same(pg.covariances(pairs=[(1, 3)]), want)                               # (the object is made anew)
    L, d = pg._L, _capi.dptr
    z, rec = np.zeros(64), np.zeros(3)
    cov = pg._cov
    u = np.array([1, 3], dtype=np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))
    assert L.ndt2d_covariance_compute(cov, None, 1, None, 0.0, None, 0, None, None, d(z)) == _capi.ERR_INVALID        # NULL outputs
    assert L.ndt2d_covariance_compute(cov, None, 1, None, 0.0, None, 0, d(z), None, None) == _capi.ERR_INVALID
    assert L.ndt2d_covariance_compute(cov, None, 1, None, 0.0, u, 1, d(z), None, d(z)) == _capi.ERR_INVALID
    assert L.ndt2d_covariance_compute(cov, None, 1, None, 0.0, None, 1, d(z), d(z), d(z)) == _capi.ERR_INVALID
    assert b"null argument" in L.ndt2d_covariance_last_error(cov)
    assert L.ndt2d_covariance_compute(cov, None, 0, None, 0.0, None, 0, None, None, None) == _capi.OK                  # n_jobs == 0
    assert L.ndt2d_covariance_compute(cov, None, 1, None, 0.0, None, 0, d(z), None, d(rec)) == _capi.OK                # no pairs
    assert np.array_equal(z[:36].reshape(4, 3, 3), want["diagonal"][0]) and rec[0] == OK and rec[1] == -1.0 and 0.0 < rec[2] <= 1.0
    with pytest.raises(ValueError, match="mask 0 switches off"):
        _upload(P, x, "square_fixed_masks", switchable=np.zeros(P.m, dtype=bool)).covariances(masks=np.array([[1, 1, 0, 1]]))
    # a caller's stream, timed
    m = _matcher()
    stream = torch.cuda.Stream()
    m.set_stream(stream.cuda_stream)
    try:
        got = pg.covariances(pairs=[(1, 3)])
        pg.set_timing(True)
        timed = pg.covariances(pairs=[(1, 3)])
        kernel_ms, fetch_ms = pg.covariance_last_ms()
        assert kernel_ms > 0.0 and fetch_ms >= 0.0
    finally:
        pg.set_timing(False)
        m.set_stream(None)
    assert _same(got, want) and _same(timed, want)


def test_relative_covariances_and_the_closure_verdicts_end_to_end():
    """PoseGraph.relative_covariances against relative_covariance over the CG marginals on the verdict
    graph; Graph.closure_distances(method="dense") against method="cg" on the close_loops graph of
    tests/test_gpu_posegraph_marginals.py: d2 = 0 for a consistent closure, 54.5 for one 1 m off."""
    import test_gpu_posegraph_marginals as TM
    P, x, (a, b), _ = MC.verdict_case()
    pg = _upload(P, x, "verdict")
    pg.set_preconditioner("chain")
    S = MR.System(P, x)
    dense = pg.relative_covariances([(a, b), (3, 30)], poses=x)
    want_t, want_cov = MR.relative(math.cos(x[a, 2]), math.sin(x[a, 2]), x[a], x[b], S.blocks([a, b]))
    lever = (2.0 + np.max(np.abs(want_t[:2]))) ** 2 * 36.0
    bound = S.inverse_norm() * (100.0 * DR.floor(S) + S.defect())
    assert dense[0]["status"] == OK and np.max(np.abs(dense[0]["covariance"] - want_cov)) <= lever * bound
    assert np.all(np.abs(dense[0]["transform"] - want_t) <= 4.0 * np.spacing(np.max(np.abs(want_t))))
    m = ScanMatcherNDT(0)
    try:
        graph, odometry = TM._end_to_end_graph(m)
        assert graph.optimize(m, weighting="information") is True
        new = len(graph.scans) - 1
        consistent = make_constraint(new - 1, new, graph.scans[new - 1].pose, graph.scans[new].pose, odometry)
        off = graph_io.Constraint(new - 1, new, np.array(consistent.transform) + np.array([1.0, 0.0, 0.0]), consistent.information, switchable=True)
        cg = graph.closure_distances(m, [consistent, off, consistent])
        d2 = graph.closure_distances(m, [consistent, off, consistent], method="dense")
        print("end to end: dense d2 %.3e and %.2f, by CG %.3e and %.2f" % (d2[0], d2[1], cg[0], cg[1]))
        assert np.all(graph.last_closure_distances["status"] == OK)
        assert d2[0] <= 1e-12 and d2[0] == d2[2] and abs(d2[1] - cg[1]) <= 1e-6 * cg[1] and TM.CHI2_3_999 < d2[1]
        with pytest.raises(ValueError, match="method"):
            graph.closure_distances(m, [consistent], method="sparse")
    finally:
        m.close()
