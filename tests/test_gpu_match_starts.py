"""Batched match from K start poses (ScanMatcherNDT.matchStarts, csrc/starts/): one scan against
the NDT in place, a full matchScan lattice around each start, in one upload, one search launch
and one read-back.

The yardstick of every test is the sequential matchScan per start on the same matcher and, for
the parity test, the CPU oracle.  Raw scores are compared bit for bit where the sequential path
runs the small-lattice search with its default plan: a lane of the batched search keeps that
search's partial sums (ndt2d_walk_fn.h, shared with the loop-closure batch)."""
import ctypes as C
import math
import time

import numpy as np
import pytest

import offgrid_cases
import oracle_lib as O
from ndt_2d_amd import Ndt2dError, ScanMatcherNDT, _capi, heading_fan, relocalize, search_offsets, synth

pytestmark = pytest.mark.gpu

WORLD = (12.0, 4.0, 0.25)
RANGE_MAX = 7.0
NO_INDEX = 2 ** 64 - 1
TOL_TIGHT = 1e-9              # tests/test_gpu_parity.py: regression bound on raw scores and the score
SMALL_LATTICE = "match/lane-per-candidate/small-lattice/"
# 5 theta steps x 7 x 7 translations (the closure tests' SMALL)
SMALL = dict(search_angular_size=0.045, search_angular_resolution=0.02,
             search_linear_size=0.065, search_linear_resolution=0.02, laser_max_beams=100)
TRUE_POSE = (2.2, -1.3, 0.4)
STARTS = np.array([(2.18, -1.27, 0.41), (2.2, -1.3, 0.4), (2.2, -1.3, 0.4 + math.pi / 2), (2.2, -1.3, 0.4 + math.pi),
                   (-6.0, 5.5, -1.0), (9.5, 9.5, 2.0), (2.18, -1.27, 0.41), (40.0, 40.0, 0.0),
                   (-11.9, -11.9, 0.7), (2.25, -1.35, 0.37), (0.0, 0.0, 0.0), (2.2, -1.3, -2.7)])
NEAR = (0, 1, 6, 9)           # the starts beside the truth: the oracle scores them -0.25 to -0.29


@pytest.fixture(scope="module")
def fixture():
    """45 map scans of 360 beams on a 7 x 7 pose lattice of pitch 3.0 (129 x 129 cells at 0.25:
    16,641 records, five times what LDS holds; 107 x 107 at 0.3) and a 720-beam query."""
    w = synth.world_of(WORLD)
    scans, index = [], 0
    for iy in range(7):
        for ix in range(7):
            x, y = (ix - 3) * 3.0, (iy - 3) * 3.0
            if not synth.pose_blocked(w, x, y):
                scans.append(((x, y, 0.0), synth.scan(w, (x, y, 0.0), 9000 + index, n_beams=360)))
            index += 1
    assert len(scans) == 45
    return dict(world=w, scans=scans, query=synth.scan(w, TRUE_POSE, 9100))


_ORACLE = {}


def _oracle(fixture, resolution):
    """The CPU oracle's matchScan per start, computed once per resolution and left unchanged."""
    if resolution not in _ORACLE:
        ref = O.ScanMatcherNDT()
        ref.initialize(**dict(SMALL, ndt_resolution=resolution, range_max=RANGE_MAX))
        ref.addScans(fixture["scans"])
        _ORACLE[resolution] = [ref.matchScan(s, fixture["query"], want_scores=True) for s in STARTS]
    return _ORACLE[resolution]


def _matcher(fixture, build_mode=None, by_id=False, **params):
    p = dict(SMALL, ndt_resolution=0.25, range_max=RANGE_MAX)
    p.update(params)
    m = ScanMatcherNDT(0)
    m.initialize("starts", **p)
    if build_mode:
        m.set_build_mode(build_mode)
    if by_id:
        ids = [m.storeScan(pts) for _, pts in fixture["scans"]]
        m.addScansById([pose for pose, _ in fixture["scans"]], ids)
    else:
        m.addScans(fixture["scans"])
    return m


def _sequential(m, starts, points, want_scores=True):
    out = []
    for s in starts:
        out.append(m.matchScan(s, points, want_scores=want_scores))
        out[-1]["variant"] = m.last_variant()
    return out


def _same_as_sequential(got, exp, exact_scores=True):
    assert got["n_candidates"] == exp["n_candidates"]
    assert got["best_index"] == exp["best_index"]
    assert np.array_equal(got["pose"], exp["pose"])
    if exact_scores:
        assert got["score"] == exp["score"] or (np.isnan(got["score"]) and np.isnan(exp["score"]))
        if got.get("scores") is not None and exp.get("scores") is not None:
            assert np.array_equal(got["scores"], exp["scores"], equal_nan=True)
    else:
        assert abs(got["score"] - exp["score"]) < TOL_TIGHT
        if got.get("scores") is not None and exp.get("scores") is not None:
            assert np.max(np.abs(got["scores"] - exp["scores"])) < TOL_TIGHT
    # the reduction order differs: the bound _check_match (tests/test_gpu_parity.py) uses
    assert np.allclose(got["covariance"], exp["covariance"], rtol=1e-9, atol=0, equal_nan=True)


def _check_all(m, got, seq, expect_bits=None):
    """Every start against its sequential call; bits where that call ran the small-lattice search.
    expect_bits: True / False asserts which of the two it was."""
    assert len(got) == len(seq)
    for k, (g, s) in enumerate(zip(got, seq)):
        small = s["variant"].startswith(SMALL_LATTICE)
        print("start %d: sequential variant %s, score %.17g batched %.17g" % (k, s["variant"], s["score"], g["score"]))
        assert s["variant"].startswith("match/"), s["variant"]
        if expect_bits is not None:
            assert small == expect_bits, (k, s["variant"])
        _same_as_sequential(g, s, exact_scores=small)


@pytest.mark.parametrize("resolution", [0.25, 0.3])
def test_parity_with_the_sequential_path_and_the_oracle(fixture, resolution):
    m = _matcher(fixture, ndt_resolution=resolution)
    assert m.grid()[1:3] == ((129, 129) if resolution == 0.25 else (107, 107))
    query = fixture["query"]
    before = m.matchScan(STARTS[0], query, want_scores=True)
    seq = _sequential(m, STARTS, query)
    assert all(s["n_candidates"] == 5 * 7 * 7 for s in seq)
    # no near tie for any start: the index comparison against the oracle means something
    assert m.adjudication_stats()[0] == 0
    got = m.matchStarts(STARTS, query, want_scores=True)
    assert m.adjudication_stats()[0] == 0
    assert m.has_ndt() == 1                                   # the NDT stays in place
    # (the variant string is asserted either way: bits where it names the small-lattice search,
    # the regression bound where it names another mapping)
    for s in seq:
        if s["variant"].startswith(SMALL_LATTICE):
            assert s["variant"].startswith(SMALL_LATTICE + ("pow2" if resolution == 0.25 else "div")), s["variant"]
    _check_all(m, got, seq)
    exp = _oracle(fixture, resolution)
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g["n_candidates"] == e["n_candidates"] == 245
        assert g["best_index"] == e["best_index"], k
        assert np.array_equal(g["pose"], e["pose"])
        assert abs(g["score"] - e["score"]) < TOL_TIGHT
        assert np.max(np.abs(g["scores"] - e["scores"])) < TOL_TIGHT
        assert np.allclose(g["covariance"], e["covariance"], rtol=1e-9, atol=0, equal_nan=True)
    # what the fixture is for: the starts beside the truth respond, the others do not
    for k, g in enumerate(got):
        if k in NEAR:
            assert -0.29 <= g["score"] <= -0.25, (k, g["score"])
        else:
            assert g["score"] > -0.023, (k, g["score"])
    # start 7 is off the map: no candidate below 0, no index, score 0, the pose untouched
    assert got[7]["best_index"] == NO_INDEX and got[7]["score"] == 0.0
    assert np.all(got[7]["scores"] == 0.0) and np.array_equal(got[7]["pose"], [0.0, 0.0, 0.0])
    # starts 0 and 6 are the same pose: identical bits
    assert got[0]["score"] == got[6]["score"] and got[0]["best_index"] == got[6]["best_index"]
    assert np.array_equal(got[0]["scores"], got[6]["scores"])
    assert np.array_equal(got[0]["covariance"], got[6]["covariance"])
    # a matchScan after the batch equals one before it
    after = m.matchScan(STARTS[0], query, want_scores=True)
    assert after["score"] == before["score"] and after["best_index"] == before["best_index"]
    assert np.array_equal(after["scores"], before["scores"]) and np.array_equal(after["pose"], before["pose"])
    assert np.array_equal(after["covariance"], before["covariance"])


def test_every_install_path(fixture):
    query = fixture["query"]
    # the 41 x 41 cfg-1 map, built on the host and installed from it: bits equal sequential
    m = ScanMatcherNDT(0)
    m.initialize("cfg1", **dict(SMALL, ndt_resolution=0.25, range_max=synth.CONFIGS[1]["range_max"]))
    m.addScans(synth.map_scans(1))
    assert m.last_build() == "build/host"
    q1 = synth.query_scan(1)[1]
    seq = _sequential(m, STARTS, q1)
    _check_all(m, m.matchStarts(STARTS, q1, want_scores=True), seq, expect_bits=True)
    # ... and the same map installed dense through ndt2d_set_grid on the matcher's context
    cells, sx, sy, ox, oy = _host_grid(synth.map_scans(1), 0.25, synth.CONFIGS[1]["range_max"])
    assert (sx, sy) == (41, 41)
    assert _capi.lib().ndt2d_set_grid(m.device_handle, _capi.dptr(cells), sx, sy, 0.25, ox, oy) == _capi.OK
    dense = m.matchStarts(STARTS, q1, want_scores=True)
    for g, s in zip(dense, seq):
        _same_as_sequential(g, s)
    # the fixture map under the host and the device build, and installed by the fused build
    for mode, by_id, name in (("host", False, "build/host"), ("device", False, "build/device"),
                              (None, True, "build/fused-small-map")):
        m = _matcher(fixture, build_mode=mode, by_id=by_id)
        assert m.last_build() == name, (mode, by_id, m.last_build())
        seq = _sequential(m, STARTS, query)
        got = m.matchStarts(STARTS, query, want_scores=True)
        _check_all(m, got, seq)
        assert got[7]["best_index"] == NO_INDEX and all(got[k]["best_index"] != NO_INDEX for k in NEAR)


def _host_grid(scans, resolution, range_max):
    from ndt_2d_amd import host_build_grid
    cells, sx, sy, ox, oy = host_build_grid(resolution, range_max, scans)
    return np.ascontiguousarray(cells, dtype=np.float64), sx, sy, ox, oy


def _starts_records(m, points, starts, slots):
    """ndt2d_starts_match on an object of its own with `slots` slots, against the grid installed in
    the matcher's context: (records, scores)."""
    L = _capi.lib()
    obj = C.c_void_p()
    assert L.ndt2d_starts_create(m.device_handle, slots, C.byref(obj)) == _capi.OK
    try:
        p = m.params
        dth = np.ascontiguousarray(search_offsets(p["search_angular_size"], p["search_angular_resolution"]))
        dlin = np.ascontiguousarray(search_offsets(p["search_linear_size"], p["search_linear_resolution"]))
        n_beams = min(int(p["laser_max_beams"]), len(points))
        step = len(points) / n_beams
        beams = np.ascontiguousarray([points[int(i * step)] for i in range(n_beams)], dtype=np.float64)
        st = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        records = np.zeros((len(st), 12))
        scores = np.zeros((len(st), len(dth) * len(dlin) * len(dlin)))
        rc = L.ndt2d_starts_match(obj, _capi.dptr(st), len(st), _capi.dptr(beams), n_beams, _capi.dptr(dth), len(dth),
                                  _capi.dptr(dlin), len(dlin), _capi.dptr(records), _capi.dptr(scores))
        if rc != _capi.OK:
            raise Ndt2dError(rc, "ndt2d_starts_match", L.ndt2d_starts_last_error(obj).decode())
        return records, scores
    finally:
        L.ndt2d_starts_destroy(obj)


def test_chunks_and_determinism(fixture):
    m = _matcher(fixture)
    query = fixture["query"]
    # K = 12 through 16 slots and through 5 (three chunks, the last of two starts)
    whole = _starts_records(m, query, STARTS, slots=16)
    chunked = _starts_records(m, query, STARTS, slots=5)
    assert np.array_equal(whole[0], chunked[0], equal_nan=True) and np.array_equal(whole[1], chunked[1])
    a = m.matchStarts(STARTS, query, want_scores=True)
    b = m.matchStarts(STARTS, query, want_scores=True)
    for x, y in zip(a, b):   # two calls: the same bits, covariance included
        assert x["score"] == y["score"] and x["best_index"] == y["best_index"]
        assert np.array_equal(x["scores"], y["scores"]) and np.array_equal(x["pose"], y["pose"])
        assert np.array_equal(x["covariance"], y["covariance"], equal_nan=True)
    # ... and the object's records are what the matcher's call turned into its results
    for k, x in enumerate(a):
        assert np.array_equal(whole[1][k], x["scores"])
        assert whole[0][k, 0] / 100 == x["score"]
        assert (NO_INDEX if whole[0][k, 1] < 0 else int(whole[0][k, 1])) == x["best_index"]
    # K = 1 equals the sequential call
    one = m.matchStarts(STARTS[9:10], query, want_scores=True)
    assert len(one) == 1
    _check_all(m, one, _sequential(m, STARTS[9:10], query))
    assert m.matchStarts(np.zeros((0, 3)), query) == []


def test_edges_one_theta_step_and_one_beam(fixture):
    m = _matcher(fixture, search_angular_size=0.01, search_angular_resolution=0.02)
    sel = STARTS[[0, 2, 7, 9]]
    got = m.matchStarts(sel, fixture["query"], want_scores=True)
    assert got[0]["n_candidates"] == 1 * 7 * 7
    _check_all(m, got, _sequential(m, sel, fixture["query"]))
    one_beam = fixture["query"][100:101]
    got = m.matchStarts(sel, one_beam, want_scores=True)
    _check_all(m, got, _sequential(m, sel, one_beam))


ONE_ENGINE = STARTS[[0, 2, 7, 9, 11]]   # five starts, [7] off the map
THREE_STEPS = dict(search_angular_size=0.025, search_angular_resolution=0.02)   # 3 x 7 x 7


@pytest.mark.parametrize("max_beams", [100, 21])   # C = 5 and C = 2 partial sums
def test_starts_are_jobs_of_one_scan(fixture, max_beams):
    """matchStarts runs on the scan tracking's engine with one scan that every job names: the
    two calls give the same bits, covariance included."""
    m = _matcher(fixture, laser_max_beams=max_beams, **THREE_STEPS)
    query = fixture["query"]
    as_starts = m.matchStarts(ONE_ENGINE, query, want_scores=True)
    as_jobs = m.matchScans(ONE_ENGINE, [query], job_scan=[0] * 5, want_scores=True)
    assert len(as_starts) == len(as_jobs) == 5 and as_starts[0]["n_candidates"] == 3 * 7 * 7
    assert as_starts[2]["best_index"] == NO_INDEX and as_starts[0]["best_index"] != NO_INDEX
    for s, j in zip(as_starts, as_jobs):
        print("score %.17g (start) %.17g (job), best index %d %d" % (s["score"], j["score"], s["best_index"], j["best_index"]))
        assert np.array_equal(s["score"], j["score"]) and s["best_index"] == j["best_index"]
        assert np.array_equal(s["pose"], j["pose"]) and np.array_equal(s["scores"], j["scores"])
        assert np.array_equal(s["covariance"], j["covariance"], equal_nan=True)


def test_starts_object_in_chunks_equals_the_scans_object(fixture):
    """ndt2d_starts_match through 2 slots (chunks of 2, 2 and 1 starts) against ndt2d_scans_match
    through 16: the same records and scores."""
    from test_gpu_match_scans import _scans_records
    m = _matcher(fixture, **THREE_STEPS)
    query = fixture["query"]
    starts = _starts_records(m, query, ONE_ENGINE, slots=2)
    jobs = _scans_records(m, ONE_ENGINE, [query], [0] * 5, slots=16)
    assert starts[0].shape == (5, 12) and starts[1].shape == (5, 3 * 7 * 7)
    assert np.array_equal(starts[0], jobs[0], equal_nan=True) and np.array_equal(starts[1], jobs[1])
    assert starts[0][0, 0] < 0.0 and starts[0][2, 0] == 0.0   # (a start beside the truth scores; the one off the map does not)


def test_edges_more_beams_than_one_staging_piece(fixture):
    """1,500 beams: the search block rotates them into LDS in two pieces of 1,024."""
    long_scan = synth.scan(fixture["world"], TRUE_POSE, 9200, n_beams=1500)
    m = _matcher(fixture, laser_max_beams=2000)
    sel = STARTS[[0, 3, 7, 9]]
    got = m.matchStarts(sel, long_scan, want_scores=True)
    _check_all(m, got, _sequential(m, sel, long_scan))


def test_edges_off_grid_and_non_finite_scan_points(fixture):
    m = _matcher(fixture)
    pts = fixture["query"].copy()
    bad = offgrid_cases.off_grid_points(0.25, RANGE_MAX)
    step = len(pts) / 100
    for i, (x, y, _) in enumerate(bad):
        pts[int((3 * i + 1) * step)] = (x, y)     # points the subsampling takes
    sel = STARTS[[0, 4, 7, 8, 9]]
    got = m.matchStarts(sel, pts, want_scores=True)
    seq = _sequential(m, sel, pts)
    for g in got:
        assert np.all(np.isfinite(g["scores"]))
    _check_all(m, got, seq)


def test_edges_no_points_and_no_ndt(fixture):
    m = _matcher(fixture)
    sel = STARTS[[0, 7]]
    none = m.matchStarts(sel, np.zeros((0, 2)), want_scores=True)
    for g, s in zip(none, _sequential(m, sel, np.zeros((0, 2)))):
        _same_as_sequential(g, s)
        assert g["n_candidates"] == 5 * 7 * 7 and g["best_index"] == NO_INDEX
    # no NDT in place: every score 0.0, everything else untouched (src/scan_matcher_ndt.cpp:80)
    m.reset()
    empty = m.matchStarts(sel, fixture["query"], want_scores=True)
    exp = m.matchScan(sel[0], fixture["query"], want_scores=True)
    for g in empty:
        assert g["score"] == 0.0 == exp["score"] and g["covariance"] is None and exp["covariance"] is None
        assert g["best_index"] == exp["best_index"] == NO_INDEX and g["n_candidates"] == exp["n_candidates"] == 0
        assert np.array_equal(g["pose"], [0.0, 0.0, 0.0]) and np.all(g["scores"] == 0.0)
    # outputs untouched, at the C boundary: what the caller put there stays
    L = _capi.lib()
    poses, covs, scores = np.full((2, 3), 7.0), np.full((2, 9), 8.0), np.full(2, 9.0)
    q = np.ascontiguousarray(fixture["query"])
    st = np.ascontiguousarray(sel)
    rc = L.ndt2d_matcher_match_starts(m._m, _capi.dptr(st), 2, _capi.dptr(q), len(q), _capi.dptr(poses), _capi.dptr(covs),
                                      _capi.dptr(scores), None, None, 0, None)
    assert rc == _capi.OK and np.all(scores == 0.0) and np.all(poses == 7.0) and np.all(covs == 8.0)


def test_edges_plugin_defaults(fixture):
    """80 theta steps x 21 x 21 translations, 100 of 720 beams, for starts 0, 2 and 7."""
    p = dict(ndt_resolution=0.25, range_max=RANGE_MAX)
    m = ScanMatcherNDT(0)
    m.initialize("defaults", **p)       # the plugin's declared defaults
    m.addScans(fixture["scans"])
    sel = STARTS[[0, 2, 7]]
    got = m.matchStarts(sel, fixture["query"], want_scores=True)
    assert got[0]["n_candidates"] == 80 * 21 * 21
    _check_all(m, got, _sequential(m, sel, fixture["query"]))
    assert got[0]["score"] < got[1]["score"] and got[2]["best_index"] == NO_INDEX


def test_near_tie_is_settled_by_the_sequential_call():
    """The construction of tests/test_gpu_near_ties.py: one beam aimed at the mean of a symmetric
    cell, translations placed symmetrically around it -- the top candidates tie."""
    cell = np.array([[2.0, 2.0], [3.0, 2.0], [1.0, 2.0], [2.0, 3.0], [2.0, 1.0],
                     [2.5, 2.5], [1.5, 1.5], [2.5, 1.5], [1.5, 2.5]])
    params = dict(ndt_resolution=4.0, range_max=8.0, laser_max_beams=100,
                  search_linear_size=0.1875, search_linear_resolution=0.125,
                  search_angular_size=0.001, search_angular_resolution=0.002)
    scan_pose = (0.0, 0.0, 0.001)
    other = (0.03, -0.02, 0.001)                    # an ordinary start beside it: no tie
    beam = np.array([[2.0, 2.0]])
    m = ScanMatcherNDT(0)
    m.initialize("ties", **params)
    m.addScans([((0.0, 0.0, 0.0), cell)])
    ref = O.ScanMatcherNDT()
    ref.initialize(**params)
    ref.addScans([((0.0, 0.0, 0.0), cell)])
    want = ref.matchScan(scan_pose, beam, want_scores=True)
    s = np.sort(want["scores"])
    assert s[0] == s[1] < 0.0
    exp_other = m.matchScan(other, beam, want_scores=True)
    before = m.adjudication_stats()[0]
    assert before == 0                              # the ordinary start is no tie
    got = m.matchStarts([scan_pose, other], beam, want_scores=True)
    assert m.adjudication_stats()[0] == before + 1   # exactly the tied start was settled
    assert got[0]["best_index"] == want["best_index"] and got[0]["score"] == want["score"]
    assert np.array_equal(got[0]["pose"], want["pose"])
    _same_as_sequential(got[1], exp_other)
    assert m.has_ndt() == 1


def test_refusals_name_the_start_and_leave_the_matcher_usable(fixture):
    m = _matcher(fixture)
    query = fixture["query"]
    seq = _sequential(m, STARTS[:3], query)
    bad = STARTS[:3].copy()
    bad[1, 1] = float("nan")
    with pytest.raises(Ndt2dError) as ei:
        m.matchStarts(bad, query)
    assert ei.value.code == _capi.ERR_INVALID and "start 1" in str(ei.value), str(ei.value)
    assert m.has_ndt() == 1
    # at object level: the same for a non-finite start (grid or not), and without a grid the code
    # ndt2d_match_launch gives without one
    with pytest.raises(Ndt2dError) as ei:
        _starts_records(m, query, bad, slots=4)
    assert ei.value.code == _capi.ERR_INVALID and "start 1" in str(ei.value), str(ei.value)
    bare = ScanMatcherNDT(0)
    bare.initialize("bare", **dict(SMALL, ndt_resolution=0.25, range_max=RANGE_MAX))
    with pytest.raises(Ndt2dError) as ei:
        _starts_records(bare, query, bad, slots=4)
    assert ei.value.code == _capi.ERR_INVALID and "start 1" in str(ei.value), str(ei.value)
    with pytest.raises(Ndt2dError) as ei:
        _starts_records(bare, query, STARTS[:3], slots=4)
    assert ei.value.code == _capi.ERR_NO_GRID
    assert _capi.lib().ndt2d_match_launch(bare.device_handle, 0, 1, None, None) == _capi.ERR_NO_GRID
    # a lattice or a beam count ndt2d_set_search / ndt2d_set_beams refuse
    L = _capi.lib()
    obj = C.c_void_p()
    assert L.ndt2d_starts_create(m.device_handle, 4, C.byref(obj)) == _capi.OK
    try:
        z = np.zeros(16)
        st = np.ascontiguousarray(STARTS[:2])
        for n_beams, n_th, n_lin in ((0, 1, 1), ((1 << 20) + 1, 1, 1), (1, 0, 1), (1, 1, 0), (1, (1 << 24) + 1, 1),
                                     (1, 1, 46341)):
            rc = L.ndt2d_starts_match(obj, _capi.dptr(st), 2, _capi.dptr(z), n_beams, _capi.dptr(z), n_th, _capi.dptr(z),
                                      n_lin, _capi.dptr(z), None)
            assert rc == _capi.ERR_INVALID, (n_beams, n_th, n_lin)
            assert b"bad argument" in L.ndt2d_starts_last_error(obj)
        assert L.ndt2d_starts_match(obj, _capi.dptr(st), 0, None, 0, None, 0, None, 0, None, None) == _capi.OK
        assert L.ndt2d_starts_create(m.device_handle, 0, C.byref(C.c_void_p())) == _capi.ERR_INVALID
        assert L.ndt2d_starts_create(m.device_handle, 4097, C.byref(C.c_void_p())) == _capi.ERR_INVALID
    finally:
        L.ndt2d_starts_destroy(obj)
    # afterwards the matcher works and gives the parity results
    _check_all(m, m.matchStarts(STARTS[:3], query, want_scores=True), seq)


def test_relocalize_end_to_end(fixture):
    m = _matcher(fixture)
    # six map-scan poses nearest the truth, each under 4 headings, plus start 1
    poses = np.array([pose for pose, _ in fixture["scans"]])
    d = np.hypot(poses[:, 0] - TRUE_POSE[0], poses[:, 1] - TRUE_POSE[1])
    nodes = poses[np.argsort(d, kind="stable")[:6]]
    seeds = np.concatenate([heading_fan(nodes, 4), STARTS[1:2]])
    assert seeds.shape == (25, 3)
    ranked = relocalize(m, fixture["query"], seeds)
    assert len(ranked) == 25 and m.has_ndt() == 1
    top = ranked[0]
    assert top["start"] == 24
    assert math.hypot(top["pose"][0] - TRUE_POSE[0], top["pose"][1] - TRUE_POSE[1]) < 0.05
    assert abs(top["pose"][2] - TRUE_POSE[2]) < 0.02
    assert np.array_equal(top["pose"], top["correction"] + seeds[24])
    # ranked by score: the seeds with a winner first, in ascending score
    scores = [r["score"] for r in ranked]
    assert all(np.isfinite(scores))
    n_win = sum(1 for r in ranked if r["score"] < 0.0)
    assert scores[:n_win] == sorted(scores[:n_win]) and all(sc == 0.0 for sc in scores[n_win:])
    # every wrong-heading seed ranks below every seed that scored under -0.2
    good = [r["start"] for r in ranked if r["score"] < -0.2]
    assert good and good[0] == 24
    wrong = [k for k in range(24) if k % 4 != 0]          # 90, 180 and 270 degrees off the truth's 0.4 rad + a node's 0
    rank_of = {r["start"]: i for i, r in enumerate(ranked)}
    assert all(rank_of[k] >= len(good) for k in wrong)
    kept = relocalize(m, fixture["query"], seeds, accept_below=-0.2)
    assert [r["start"] for r in kept] == good


def test_batched_is_not_slower_than_the_sequential_calls(fixture):
    """Plugin defaults, K = 16: sixteen search launches and fetches against one."""
    m = ScanMatcherNDT(0)
    m.initialize("defaults", ndt_resolution=0.25, range_max=RANGE_MAX)
    m.addScans(fixture["scans"])
    m.set_timing(False)
    query = fixture["query"]
    starts = np.concatenate([STARTS, STARTS[:4] + np.array([0.01, -0.01, 0.003])])
    assert len(starts) == 16

    def batched():
        m.matchStarts(starts, query)

    def sequential():
        for s in starts:
            m.matchScan(s, query)

    def median(fn, reps=20):
        fn()
        fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return float(np.median(t))

    t_seq = median(sequential)
    t_bat = median(batched)
    print("K = 16, plugin defaults: batched %.1f us, sequential %.1f us" % (t_bat * 1e6, t_seq * 1e6))
    assert t_bat < t_seq
