"""Batched scan tracking (ScanMatcherNDT.matchScans, csrc/scans/): K jobs, each a (scan, pose)
pair, against the NDT in place -- a full matchScan lattice around each job's pose with the job's
own beams -- in one upload, the search launches, one reduce launch and one read-back.

The yardstick of every test is the sequential matchScan per job on the same matcher and, for
the parity test, the CPU oracle.  Raw scores are compared bit for bit where the sequential path
runs the small-lattice search with its default plan (a lane of the batched search keeps that
search's partial sums, batch/ndt2d_walk_fn.h); elsewhere, and for the covariance throughout,
the bounds are those of tests/test_gpu_match_starts.py (_check_all / _same_as_sequential), whose
45-scan fixture and SMALL lattice are the base here."""
import ctypes as C
import math
import time

import numpy as np
import pytest

import offgrid_cases
import oracle_lib as O
from ndt_2d_amd import Ndt2dError, ScanMatcherNDT, _capi, search_offsets, synth, track_scans
from test_gpu_match_starts import (NO_INDEX, RANGE_MAX, SMALL, SMALL_LATTICE, TOL_TIGHT, _check_all, _matcher,
                                   _same_as_sequential, fixture)  # noqa: F401

pytestmark = pytest.mark.gpu

NEAR_TIE_REL = 2.0 ** -36        # the adjudication's band: a second candidate this close to the best is a near tie
# Where the parity test's query scans are taken, and how many of their 720 points each keeps.
# With laser_max_beams = 200 the searches run 1, 20, 21, 60, 100, 160 and 200 beams: C = 1, 1, 2,
# 3, 5, 8, 8 partial sums, five launches in the one chunk.  Scan 7 is named by no job.
SCAN_POSES = [(2.2, -1.3, 0.4), (-4.4, 1.6, -1.2), (1.4, 4.6, 2.0), (-1.5, -4.5, 0.9), (4.6, 1.4, -2.6),
              (-4.5, -1.6, 3.0), (7.4, -4.6, 0.2), (-7.5, 7.4, 1.1)]
SCAN_POINTS = [1, 20, 21, 60, 100, 160, 720, 720]
PARITY = dict(SMALL, laser_max_beams=200)
OFF_MAP = (40.0, 40.0, 0.0)


def _cut(points, n):
    """n of a scan's points, spread over the whole turn."""
    return np.ascontiguousarray(points[(np.arange(n) * len(points)) // n])


def _near(pose, dx, dy, dth):
    return (pose[0] + dx, pose[1] + dy, pose[2] + dth)


def _parity_case(fixture):
    """(jobs[12][3], scans[8], job_scan[12]): two jobs share scan 6 (and scans 2 .. 5 serve two
    each), job 8 is off the map, jobs 3 and 9 are identical, scan 7 is named by nobody."""
    w = fixture["world"]
    scans = [_cut(synth.scan(w, pose, 9300 + i), n) for i, (pose, n) in enumerate(zip(SCAN_POSES, SCAN_POINTS))]
    job_scan = [0, 1, 2, 3, 4, 5, 6, 6, 4, 3, 2, 5]
    offs = [(0.02, -0.01, 0.01), (-0.03, 0.02, -0.01), (0.01, 0.03, 0.015), (-0.02, -0.02, 0.005), (0.03, 0.0, -0.015),
            (0.0, -0.03, 0.01), (0.02, 0.02, -0.005), (-0.01, 0.04, 0.02), None, (-0.02, -0.02, 0.005),
            (-0.04, 0.01, -0.02), (0.03, -0.03, 0.012)]
    jobs = [OFF_MAP if o is None else _near(SCAN_POSES[s], *o) for s, o in zip(job_scan, offs)]
    return np.array(jobs), scans, job_scan


_ORACLE = {}


def _oracle(fixture, resolution):
    """The CPU oracle's matchScan per job of the parity case, computed once per resolution and
    left unchanged."""
    if resolution not in _ORACLE:
        jobs, scans, job_scan = _parity_case(fixture)
        ref = O.ScanMatcherNDT()
        ref.initialize(**dict(PARITY, ndt_resolution=resolution, range_max=RANGE_MAX))
        ref.addScans(fixture["scans"])
        _ORACLE[resolution] = [ref.matchScan(j, scans[s], want_scores=True) for j, s in zip(jobs, job_scan)]
    return _ORACLE[resolution]


def _no_near_tie(scores):
    """No second candidate within 2^-36 relative of the best (or no candidate below 0 at all)."""
    s = np.sort(np.asarray(scores))
    return not (s[0] < 0.0) or s[1] - s[0] > NEAR_TIE_REL * abs(s[0])


def _sequential_jobs(m, jobs, scans, job_scan=None, want_scores=True):
    out = []
    for k, j in enumerate(jobs):
        out.append(m.matchScan(j, scans[k if job_scan is None else job_scan[k]], want_scores=want_scores))
        out[-1]["variant"] = m.last_variant()
    return out


@pytest.mark.parametrize("resolution", [0.25, 0.3])
def test_parity_mixed_beam_counts_in_one_call(fixture, resolution):
    jobs, scans, job_scan = _parity_case(fixture)
    assert [len(s) for s in scans] == SCAN_POINTS and 7 not in job_scan and job_scan.count(6) == 2
    exp = _oracle(fixture, resolution)
    # the jobs are chosen so that the oracle shows no near tie: the index comparison means something
    for k, e in enumerate(exp):
        assert e["n_candidates"] == 245 and _no_near_tie(e["scores"]), k
    m = _matcher(fixture, ndt_resolution=resolution, laser_max_beams=200)
    assert m.grid()[1:3] == ((129, 129) if resolution == 0.25 else (107, 107))
    before = m.matchScan(jobs[6], scans[6], want_scores=True)
    seq = _sequential_jobs(m, jobs, scans, job_scan)
    assert m.adjudication_stats()[0] == 0
    got = m.matchScans(jobs, scans, job_scan=job_scan, want_scores=True)
    assert m.adjudication_stats()[0] == 0
    assert m.has_ndt() == 1                                   # the NDT stays in place
    for s in seq:
        if s["variant"].startswith(SMALL_LATTICE):
            assert s["variant"].startswith(SMALL_LATTICE + ("pow2" if resolution == 0.25 else "div")), s["variant"]
    _check_all(m, got, seq)
    for k, (g, e) in enumerate(zip(got, exp)):
        print("job %d (scan %d, %d points): oracle %.17g batched %.17g" % (k, job_scan[k], len(scans[job_scan[k]]),
                                                                          e["score"], g["score"]))
        assert g["n_candidates"] == e["n_candidates"] == 245
        assert g["best_index"] == e["best_index"], k
        assert np.array_equal(g["pose"], e["pose"])
        assert abs(g["score"] - e["score"]) < TOL_TIGHT
        assert np.max(np.abs(g["scores"] - e["scores"])) < TOL_TIGHT
        assert np.allclose(g["covariance"], e["covariance"], rtol=1e-9, atol=0, equal_nan=True)
    # job 8 is off the map: no candidate below 0, no index, score 0, the pose untouched
    assert got[8]["best_index"] == NO_INDEX and got[8]["score"] == 0.0
    assert np.all(got[8]["scores"] == 0.0) and np.array_equal(got[8]["pose"], [0.0, 0.0, 0.0])
    # ... every other job has a winner
    assert all(got[k]["best_index"] != NO_INDEX and got[k]["score"] < 0.0 for k in range(12) if k != 8)
    # jobs 3 and 9 are the same scan from the same pose: identical bits
    assert got[3]["score"] == got[9]["score"] and got[3]["best_index"] == got[9]["best_index"]
    assert np.array_equal(got[3]["scores"], got[9]["scores"])
    assert np.array_equal(got[3]["covariance"], got[9]["covariance"])
    # a matchScan after the batch equals one before it
    after = m.matchScan(jobs[6], scans[6], want_scores=True)
    assert after["score"] == before["score"] and after["best_index"] == before["best_index"]
    assert np.array_equal(after["scores"], before["scores"]) and np.array_equal(after["pose"], before["pose"])
    assert np.array_equal(after["covariance"], before["covariance"])


def _subsample(points, max_beams):
    n = min(int(max_beams), len(points))
    step = len(points) / n
    return np.ascontiguousarray([points[int(i * step)] for i in range(n)], dtype=np.float64).reshape(-1, 2)


def _scans_records(m, jobs, scans, job_scan, slots, subsampled=False):
    """ndt2d_scans_match on an object of its own with `slots` slots, against the grid installed in
    the matcher's context: (records, scores)."""
    L = _capi.lib()
    obj = C.c_void_p()
    assert L.ndt2d_scans_create(m.device_handle, slots, C.byref(obj)) == _capi.OK
    try:
        p = m.params
        dth = np.ascontiguousarray(search_offsets(p["search_angular_size"], p["search_angular_resolution"]))
        dlin = np.ascontiguousarray(search_offsets(p["search_linear_size"], p["search_linear_resolution"]))
        beams = [s if subsampled else _subsample(s, p["laser_max_beams"]) for s in scans]
        offsets = np.zeros(len(beams) + 1, dtype=np.uintp)
        offsets[1:] = np.cumsum([len(b) for b in beams])
        flat = np.ascontiguousarray(np.concatenate(beams), dtype=np.float64)
        jp = np.ascontiguousarray(jobs, dtype=np.float64).reshape(-1, 3)
        js = None if job_scan is None else np.ascontiguousarray(job_scan, dtype=np.uint32)
        records = np.zeros((len(jp), 12))
        scores = np.zeros((len(jp), len(dth) * len(dlin) * len(dlin)))
        rc = L.ndt2d_scans_match(obj, _capi.dptr(jp), None if js is None else js.ctypes.data_as(C.POINTER(C.c_uint32)),
                                 len(jp), _capi.dptr(flat), offsets.ctypes.data_as(C.POINTER(C.c_size_t)), len(beams),
                                 _capi.dptr(dth), len(dth), _capi.dptr(dlin), len(dlin), _capi.dptr(records),
                                 _capi.dptr(scores))
        if rc != _capi.OK:
            raise Ndt2dError(rc, "ndt2d_scans_match", L.ndt2d_scans_last_error(obj).decode())
        return records, scores
    finally:
        L.ndt2d_scans_destroy(obj)


def test_chunks_and_determinism(fixture):
    jobs, scans, job_scan = _parity_case(fixture)
    m = _matcher(fixture, laser_max_beams=200)
    # K = 12 through 16 slots and through 5 (three chunks, the last of two jobs; every chunk groups
    # its own jobs and uploads its own scans)
    whole = _scans_records(m, jobs, scans, job_scan, slots=16)
    chunked = _scans_records(m, jobs, scans, job_scan, slots=5)
    assert np.array_equal(whole[0], chunked[0], equal_nan=True) and np.array_equal(whole[1], chunked[1])
    a = m.matchScans(jobs, scans, job_scan=job_scan, want_scores=True)
    b = m.matchScans(jobs, scans, job_scan=job_scan, want_scores=True)
    for x, y in zip(a, b):   # two calls: the same bits, covariance included
        assert x["score"] == y["score"] and x["best_index"] == y["best_index"]
        assert np.array_equal(x["scores"], y["scores"]) and np.array_equal(x["pose"], y["pose"])
        assert np.array_equal(x["covariance"], y["covariance"], equal_nan=True)
    # ... and the object's records are what the matcher's call turned into its results
    for k, x in enumerate(a):
        n_use = min(200, len(scans[job_scan[k]]))
        assert np.array_equal(whole[1][k], x["scores"])
        assert whole[0][k, 0] / n_use == x["score"]
        assert (NO_INDEX if whole[0][k, 1] < 0 else int(whole[0][k, 1])) == x["best_index"]
    # job_scan = None: job k uses scan k
    ident = m.matchScans(jobs[:7], scans[:7], want_scores=True)
    for k in range(7):
        assert ident[k]["score"] == a[k]["score"] and np.array_equal(ident[k]["scores"], a[k]["scores"])
    # K = 1 equals the sequential call
    one = m.matchScans(jobs[4:5], scans[4:5], want_scores=True)
    assert len(one) == 1
    _check_all(m, one, _sequential_jobs(m, jobs[4:5], scans[4:5]))
    assert m.matchScans(np.zeros((0, 3)), scans) == []
    assert m.matchScans(np.zeros((0, 3)), []) == []


def _edge_case(fixture):
    """Four jobs over three 720-point scans (plus one off the map)."""
    w = fixture["world"]
    scans = [synth.scan(w, pose, 9400 + i) for i, pose in enumerate(SCAN_POSES[:3])]
    job_scan = [0, 1, 2, 1]
    jobs = np.array([_near(SCAN_POSES[0], 0.02, -0.01, 0.01), _near(SCAN_POSES[1], -0.03, 0.02, -0.01),
                     _near(SCAN_POSES[2], 0.01, 0.03, 0.015), OFF_MAP])
    return jobs, scans, job_scan


def test_edges_one_theta_step(fixture):
    jobs, scans, job_scan = _edge_case(fixture)
    m = _matcher(fixture, search_angular_size=0.01, search_angular_resolution=0.02)
    got = m.matchScans(jobs, scans, job_scan=job_scan, want_scores=True)
    assert got[0]["n_candidates"] == 1 * 7 * 7
    _check_all(m, got, _sequential_jobs(m, jobs, scans, job_scan))


def test_edges_the_lane_loop_runs_twice(fixture):
    """33 x 33 = 1,089 translations: more than the block's 1,024 lanes."""
    jobs, scans, job_scan = _edge_case(fixture)
    m = _matcher(fixture, search_linear_size=0.33, search_linear_resolution=0.02,
                 search_angular_size=0.03, search_angular_resolution=0.02)
    got = m.matchScans(jobs, scans, job_scan=job_scan, want_scores=True)
    assert got[0]["n_candidates"] == 3 * 33 * 33
    _check_all(m, got, _sequential_jobs(m, jobs, scans, job_scan))


def test_edges_the_reducers_stride_loop(fixture):
    """257 theta steps: the reducing block's 256 threads take a second record."""
    jobs, scans, job_scan = _edge_case(fixture)
    m = _matcher(fixture, search_linear_size=0.02, search_linear_resolution=0.02,
                 search_angular_size=0.257, search_angular_resolution=0.002)
    got = m.matchScans(jobs, scans, job_scan=job_scan, want_scores=True)
    assert got[0]["n_candidates"] == 257 * 2 * 2
    _check_all(m, got, _sequential_jobs(m, jobs, scans, job_scan))


def test_edges_two_staging_pieces_beside_a_short_scan(fixture):
    """1,500 beams: the search block rotates them into LDS in two pieces of 1,024 -- in the same
    call as a scan of five (another launch: C = 8 and C = 1)."""
    w = fixture["world"]
    long_scan = synth.scan(w, SCAN_POSES[0], 9500, n_beams=1500)
    short_scan = _cut(synth.scan(w, SCAN_POSES[1], 9501), 5)
    scans = [long_scan, short_scan]
    jobs = np.array([_near(SCAN_POSES[0], 0.02, -0.01, 0.01), _near(SCAN_POSES[1], -0.03, 0.02, -0.01),
                     _near(SCAN_POSES[0], -0.01, 0.02, -0.02), OFF_MAP])
    job_scan = [0, 1, 0, 1]
    m = _matcher(fixture, laser_max_beams=2000)
    got = m.matchScans(jobs, scans, job_scan=job_scan, want_scores=True)
    _check_all(m, got, _sequential_jobs(m, jobs, scans, job_scan))


def test_edges_off_grid_and_non_finite_scan_points(fixture):
    jobs, scans, job_scan = _edge_case(fixture)
    m = _matcher(fixture)
    bad = offgrid_cases.off_grid_points(0.25, RANGE_MAX)
    scans = [s.copy() for s in scans]
    step = 720 / 100
    for i, (x, y, _) in enumerate(bad):
        scans[i % 2][int((3 * (i // 2) + 1) * step)] = (x, y)     # points the subsampling takes, in scans 0 and 1
    got = m.matchScans(jobs, scans, job_scan=job_scan, want_scores=True)
    seq = _sequential_jobs(m, jobs, scans, job_scan)
    for g in got:
        assert np.all(np.isfinite(g["scores"]))
    _check_all(m, got, seq)


def test_edges_a_scan_without_points_and_no_ndt(fixture):
    jobs, scans, job_scan = _edge_case(fixture)
    m = _matcher(fixture)
    scans = [scans[0], np.zeros((0, 2)), scans[2]]
    got = m.matchScans(jobs, scans, job_scan=job_scan, want_scores=True)
    seq = _sequential_jobs(m, jobs, scans, job_scan)
    _check_all(m, got, seq)
    for k in (1, 3):                                   # the jobs of the empty scan
        assert got[k]["n_candidates"] == 5 * 7 * 7 and got[k]["best_index"] == NO_INDEX
    assert got[0]["best_index"] != NO_INDEX and got[2]["best_index"] != NO_INDEX
    # every scan empty
    none = m.matchScans(jobs[:2], [np.zeros((0, 2))] * 2, want_scores=True)
    for g, s in zip(none, _sequential_jobs(m, jobs[:2], [np.zeros((0, 2))] * 2)):
        _same_as_sequential(g, s)
    # no NDT in place: every score 0.0, everything else untouched (src/scan_matcher_ndt.cpp:80)
    m.reset()
    empty = m.matchScans(jobs, scans, job_scan=job_scan, want_scores=True)
    exp = m.matchScan(jobs[0], scans[0], want_scores=True)
    for g in empty:
        assert g["score"] == 0.0 == exp["score"] and g["covariance"] is None and exp["covariance"] is None
        assert g["best_index"] == exp["best_index"] == NO_INDEX and g["n_candidates"] == exp["n_candidates"] == 0
        assert np.array_equal(g["pose"], [0.0, 0.0, 0.0]) and np.all(g["scores"] == 0.0)
    # outputs untouched, at the C boundary: what the caller put there stays
    L = _capi.lib()
    poses, covs, scores = np.full((2, 3), 7.0), np.full((2, 9), 8.0), np.full(2, 9.0)
    q = np.ascontiguousarray(np.concatenate([scans[0], scans[2]]))
    off = np.array([0, 720, 1440], dtype=np.uintp)
    jp = np.ascontiguousarray(jobs[:2])
    rc = L.ndt2d_matcher_match_scans(m._m, _capi.dptr(jp), None, 2, _capi.dptr(q), off.ctypes.data_as(C.POINTER(C.c_size_t)),
                                     2, _capi.dptr(poses), _capi.dptr(covs), _capi.dptr(scores), None, None, 0, None)
    assert rc == _capi.OK and np.all(scores == 0.0) and np.all(poses == 7.0) and np.all(covs == 8.0)


def test_edges_plugin_defaults(fixture):
    """80 theta steps x 21 x 21 translations, 100 of 720 beams, for three jobs."""
    jobs, scans, job_scan = _edge_case(fixture)
    sel = [0, 1, 3]
    jobs, job_scan = jobs[sel], [job_scan[k] for k in sel]
    m = ScanMatcherNDT(0)
    m.initialize("defaults", ndt_resolution=0.25, range_max=RANGE_MAX)       # the plugin's declared defaults
    m.addScans(fixture["scans"])
    got = m.matchScans(jobs, scans, job_scan=job_scan, want_scores=True)
    assert got[0]["n_candidates"] == 80 * 21 * 21
    _check_all(m, got, _sequential_jobs(m, jobs, scans, job_scan))
    assert got[0]["score"] < -0.1 and got[1]["score"] < -0.1 and got[2]["best_index"] == NO_INDEX


def test_every_install_path(fixture):
    jobs, scans, job_scan = _parity_case(fixture)
    # the 41 x 41 cfg-1 map, built on the host and installed from it
    m = ScanMatcherNDT(0)
    m.initialize("cfg1", **dict(PARITY, ndt_resolution=0.25, range_max=synth.CONFIGS[1]["range_max"]))
    m.addScans(synth.map_scans(1))
    assert m.last_build() == "build/host"
    w1 = synth.world_of(1)
    scans1 = [_cut(synth.scan(w1, (0.13, -0.07, 0.031), 9600 + i), n) for i, n in enumerate((720, 21, 100))]
    jobs1 = np.array([(0.1, -0.05, 0.02), (0.15, -0.1, 0.04), (0.12, -0.08, 0.03), OFF_MAP])
    js1 = [0, 1, 2, 0]
    seq = _sequential_jobs(m, jobs1, scans1, js1)
    _check_all(m, m.matchScans(jobs1, scans1, job_scan=js1, want_scores=True), seq)
    # ... and the same map installed dense through ndt2d_set_grid on the matcher's context
    from ndt_2d_amd import host_build_grid
    cells, sx, sy, ox, oy = host_build_grid(0.25, synth.CONFIGS[1]["range_max"], synth.map_scans(1))
    cells = np.ascontiguousarray(cells, dtype=np.float64)
    assert (sx, sy) == (41, 41)
    assert _capi.lib().ndt2d_set_grid(m.device_handle, _capi.dptr(cells), sx, sy, 0.25, ox, oy) == _capi.OK
    dense = m.matchScans(jobs1, scans1, job_scan=js1, want_scores=True)
    for g, s in zip(dense, seq):
        _same_as_sequential(g, s)
    # the fixture map under the host and the device build, and installed by the fused build
    first = None
    for mode, by_id, name in (("host", False, "build/host"), ("device", False, "build/device"),
                              (None, True, "build/fused-small-map")):
        m = _matcher(fixture, build_mode=mode, by_id=by_id, laser_max_beams=200)
        assert m.last_build() == name, (mode, by_id, m.last_build())
        seq = _sequential_jobs(m, jobs, scans, job_scan)
        got = m.matchScans(jobs, scans, job_scan=job_scan, want_scores=True)
        _check_all(m, got, seq)
        assert got[8]["best_index"] == NO_INDEX and all(got[k]["best_index"] != NO_INDEX for k in range(12) if k != 8)
        # every install path gives the same results
        if first is None:
            first = got
        for g, f in zip(got, first):
            assert g["best_index"] == f["best_index"] and np.array_equal(g["pose"], f["pose"])
            assert abs(g["score"] - f["score"]) < TOL_TIGHT and np.max(np.abs(g["scores"] - f["scores"])) < TOL_TIGHT


def test_near_tie_is_settled_by_the_sequential_call():
    """The construction of tests/test_gpu_match_starts.py (tests/test_gpu_near_ties.py): one beam
    aimed at the mean of a symmetric cell, translations placed symmetrically around it -- the top
    candidates tie.  The tied job sits beside an ordinary job on a scan of its own."""
    cell = np.array([[2.0, 2.0], [3.0, 2.0], [1.0, 2.0], [2.0, 3.0], [2.0, 1.0],
                     [2.5, 2.5], [1.5, 1.5], [2.5, 1.5], [1.5, 2.5]])
    params = dict(ndt_resolution=4.0, range_max=8.0, laser_max_beams=100,
                  search_linear_size=0.1875, search_linear_resolution=0.125,
                  search_angular_size=0.001, search_angular_resolution=0.002)
    scan_pose = (0.0, 0.0, 0.001)
    other = (0.03, -0.02, 0.001)                    # an ordinary job beside it: no tie
    beam = np.array([[2.0, 2.0]])
    other_scan = np.array([[2.1, 1.8], [1.7, 2.2], [2.4, 2.3]])
    m = ScanMatcherNDT(0)
    m.initialize("ties", **params)
    m.addScans([((0.0, 0.0, 0.0), cell)])
    ref = O.ScanMatcherNDT()
    ref.initialize(**params)
    ref.addScans([((0.0, 0.0, 0.0), cell)])
    want = ref.matchScan(scan_pose, beam, want_scores=True)
    s = np.sort(want["scores"])
    assert s[0] == s[1] < 0.0
    assert _no_near_tie(ref.matchScan(other, other_scan, want_scores=True)["scores"])
    exp_other = m.matchScan(other, other_scan, want_scores=True)
    before = m.adjudication_stats()[0]
    assert before == 0                              # the ordinary job is no tie
    got = m.matchScans([scan_pose, other], [beam, other_scan], want_scores=True)
    assert m.adjudication_stats()[0] == before + 1   # exactly the tied job was settled
    assert got[0]["best_index"] == want["best_index"] and got[0]["score"] == want["score"]
    assert np.array_equal(got[0]["pose"], want["pose"])
    _same_as_sequential(got[1], exp_other)
    assert m.has_ndt() == 1


def test_refusals_name_the_job_or_scan_and_leave_the_matcher_usable(fixture):
    jobs, scans, job_scan = _edge_case(fixture)
    m = _matcher(fixture)
    seq = _sequential_jobs(m, jobs, scans, job_scan)
    bad = jobs.copy()
    bad[1, 1] = float("nan")
    with pytest.raises(Ndt2dError) as ei:
        m.matchScans(bad, scans, job_scan=job_scan)
    assert ei.value.code == _capi.ERR_INVALID and "job 1" in str(ei.value), str(ei.value)
    with pytest.raises(Ndt2dError) as ei:
        m.matchScans(jobs, scans, job_scan=[0, 1, 3, 1])
    assert ei.value.code == _capi.ERR_INVALID and "job 2" in str(ei.value), str(ei.value)
    with pytest.raises(Ndt2dError) as ei:
        m.matchScans(jobs, scans)                            # no job_scan: 3 scans, 4 jobs
    assert ei.value.code == _capi.ERR_INVALID and "n_scans" in str(ei.value), str(ei.value)
    assert m.has_ndt() == 1
    # at object level: the same, a scan without beams, offsets that decrease; without a grid the
    # code ndt2d_match_launch gives without one
    with pytest.raises(Ndt2dError) as ei:
        _scans_records(m, bad, scans, job_scan, slots=4)
    assert ei.value.code == _capi.ERR_INVALID and "job 1" in str(ei.value), str(ei.value)
    with pytest.raises(Ndt2dError) as ei:
        _scans_records(m, jobs, scans, [0, 1, 2, 3], slots=4)
    assert ei.value.code == _capi.ERR_INVALID and "job 3" in str(ei.value), str(ei.value)
    with pytest.raises(Ndt2dError) as ei:
        _scans_records(m, jobs, scans, None, slots=4)
    assert ei.value.code == _capi.ERR_INVALID and "n_scans" in str(ei.value), str(ei.value)
    with pytest.raises(Ndt2dError) as ei:
        _scans_records(m, jobs, [scans[0], scans[1], np.zeros((0, 2))], [0, 1, 0, 1], slots=4, subsampled=True)
    assert ei.value.code == _capi.ERR_INVALID and "scan 2" in str(ei.value), str(ei.value)
    bare = ScanMatcherNDT(0)
    bare.initialize("bare", **dict(SMALL, ndt_resolution=0.25, range_max=RANGE_MAX))
    with pytest.raises(Ndt2dError) as ei:
        _scans_records(bare, bad, scans, job_scan, slots=4)
    assert ei.value.code == _capi.ERR_INVALID and "job 1" in str(ei.value), str(ei.value)
    with pytest.raises(Ndt2dError) as ei:
        _scans_records(bare, jobs, scans, job_scan, slots=4)
    assert ei.value.code == _capi.ERR_NO_GRID
    assert _capi.lib().ndt2d_match_launch(bare.device_handle, 0, 1, None, None) == _capi.ERR_NO_GRID
    L = _capi.lib()
    obj = C.c_void_p()
    assert L.ndt2d_scans_create(m.device_handle, 4, C.byref(obj)) == _capi.OK
    try:
        z = np.zeros(16)
        jp = np.ascontiguousarray(jobs[:2])
        szp = C.POINTER(C.c_size_t)
        two = np.array([0, 1, 2], dtype=np.uintp)

        def call(offsets, n_th, n_lin):
            return L.ndt2d_scans_match(obj, _capi.dptr(jp), None, 2, _capi.dptr(z), offsets.ctypes.data_as(szp), 2,
                                       _capi.dptr(z), n_th, _capi.dptr(z), n_lin, _capi.dptr(z), None)
        # a lattice ndt2d_set_search refuses
        for n_th, n_lin in ((0, 1), (1, 0), ((1 << 24) + 1, 1), (1, 46341)):
            assert call(two, n_th, n_lin) == _capi.ERR_INVALID, (n_th, n_lin)
            assert b"bad argument" in L.ndt2d_scans_last_error(obj)
        # offsets that decrease, a scan of more than 2^20 beams
        assert call(np.array([0, 3, 2], dtype=np.uintp), 1, 1) == _capi.ERR_INVALID
        assert b"scan 1" in L.ndt2d_scans_last_error(obj)
        assert call(np.array([0, 1, (1 << 20) + 2], dtype=np.uintp), 1, 1) == _capi.ERR_INVALID
        assert b"scan 1" in L.ndt2d_scans_last_error(obj)
        assert call(np.array([0, 0, 2], dtype=np.uintp), 1, 1) == _capi.ERR_INVALID
        assert b"scan 0" in L.ndt2d_scans_last_error(obj)
        assert L.ndt2d_scans_match(obj, _capi.dptr(jp), None, 0, None, None, 0, None, 0, None, 0, None, None) == _capi.OK
        assert L.ndt2d_scans_create(m.device_handle, 0, C.byref(C.c_void_p())) == _capi.ERR_INVALID
        assert L.ndt2d_scans_create(m.device_handle, 4097, C.byref(C.c_void_p())) == _capi.ERR_INVALID
    finally:
        L.ndt2d_scans_destroy(obj)
    # afterwards the matcher works and gives the same results as before
    _check_all(m, m.matchScans(jobs, scans, job_scan=job_scan, want_scores=True), seq)


def test_track_scans_end_to_end(fixture):
    """Eight query scans ray-cast at known poses, each started about 3 cm and 0.01 rad off."""
    w = fixture["world"]
    scans = [synth.scan(w, pose, 9700 + i) for i, pose in enumerate(SCAN_POSES)]
    offs = [(0.02, -0.02, 0.01), (-0.02, 0.02, -0.01), (0.02, 0.02, 0.01), (-0.02, -0.02, -0.01),
            (0.03, 0.0, 0.01), (0.0, -0.03, -0.01), (-0.03, 0.0, 0.01), (0.0, 0.03, -0.01)]
    jobs = np.array([_near(p, *o) for p, o in zip(SCAN_POSES, offs)])
    m = _matcher(fixture)
    tracked = track_scans(m, jobs, scans)
    assert len(tracked) == 8 and m.has_ndt() == 1
    for k, (r, truth) in enumerate(zip(tracked, SCAN_POSES)):
        print("job %d: score %.6f pose %s truth %s" % (k, r["score"], r["pose"], truth))
        assert r["job"] == k and r["scan"] == k and r["score"] < 0.0
        assert math.hypot(r["pose"][0] - truth[0], r["pose"][1] - truth[1]) < 0.05, k
        assert abs(r["pose"][2] - truth[2]) < 0.02, k
        assert np.array_equal(r["pose"], r["correction"] + jobs[k])
        assert r["covariance"].shape == (3, 3)
    # with job_scan: the same jobs in another order over the same scans
    order = [5, 2, 7, 0, 3, 6, 1, 4]
    again = track_scans(m, jobs[order], scans, job_scan=order)
    for r, k in zip(again, order):
        assert r["scan"] == k and r["score"] == tracked[k]["score"] and np.array_equal(r["pose"], tracked[k]["pose"])


def test_batched_is_not_slower_than_the_sequential_calls(fixture):
    """Plugin defaults, K = 16 distinct 720-beam scans: sixteen uploads, search launches and
    fetches against one of each."""
    w = fixture["world"]
    m = ScanMatcherNDT(0)
    m.initialize("defaults", ndt_resolution=0.25, range_max=RANGE_MAX)
    m.addScans(fixture["scans"])
    m.set_timing(False)
    poses = [SCAN_POSES[k % 8] if k < 8 else _near(SCAN_POSES[k % 8], 0.5, 0.25, 0.3) for k in range(16)]
    scans = [synth.scan(w, pose, 9800 + k) for k, pose in enumerate(poses)]
    jobs = np.array([_near(p, 0.01, -0.01, 0.003) for p in poses])
    assert len(jobs) == 16 and all(len(s) == 720 for s in scans)

    def batched():
        m.matchScans(jobs, scans)

    def sequential():
        for j, s in zip(jobs, scans):
            m.matchScan(j, s)

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
