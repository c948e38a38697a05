"""Newton NDT registration (ScanMatcherNDT.refineScans, csrc/refine/): K (scan, pose) jobs refined
against the NDT in place in one upload, one kernel launch for the whole iteration of all jobs and
one read-back.

The yardsticks are the CPU restatement of the contract (tests/refine_restatement.py, pinned to
the oracle by tests/test_refine_host.py) and the oracle's scorePoints.  Fixture, lattice and
bounds are those of tests/test_gpu_match_starts.py.

What the checks measured on an MI355X is in the tests' docstrings and in DESIGN.md 3.13."""
import ctypes as C

import numpy as np
import pytest

import designed_grids as D
import offgrid_cases
import oracle_lib as O
import refine_cases
import refine_restatement as R
from ndt_2d_amd import Ndt2dError, ScanMatcherNDT, _capi, refine_matches, synth
from test_gpu_match_starts import RANGE_MAX, SMALL, STARTS, TOL_TIGHT, TRUE_POSE, _matcher, fixture  # noqa: F401

pytestmark = pytest.mark.gpu

OFF_MAP = (40.0, 40.0, 0.0)
EPS = 2.0 ** -53


def _check_contract(ref, points, jobs, results, max_evals=32):
    """Check 2, for every job of every test: f never increases, the returned score is the
    oracle's scorePoints at the returned pose, status and counts obey the contract."""
    assert len(results) == len(jobs)
    for k, (job, r) in enumerate(zip(jobs, results)):
        assert r["status"] in (_capi.REFINE_CONVERGED, _capi.REFINE_MAX_EVALS, _capi.REFINE_STALLED, _capi.REFINE_NO_OVERLAP,
                               _capi.REFINE_NOT_FINITE), (k, r)
        assert 1 <= r["evals"] <= max_evals and 0 <= r["steps"] <= r["evals"] - 1, (k, r)
        if r["status"] == _capi.REFINE_NOT_FINITE:
            assert not np.isfinite(r["start_score"]) and r["evals"] == 1 and np.array_equal(r["pose"], job), (k, r)
            continue
        assert r["score"] <= r["start_score"] <= 0.0, (k, r)
        assert (r["steps"] == 0) == (r["score"] == r["start_score"] and np.array_equal(r["pose"], job)), (k, r)
        want = ref.scorePoints(points, r["pose"])
        assert abs(want - r["score"]) < TOL_TIGHT, (k, want, r["score"])
        assert abs(ref.scorePoints(points, job) - r["start_score"]) < TOL_TIGHT, k
        # CONVERGED is found inside the loop, which runs while evals < max_evals
        assert r["status"] != _capi.REFINE_CONVERGED or r["evals"] < max_evals, (k, r)
        assert r["status"] != _capi.REFINE_MAX_EVALS or r["evals"] == max_evals, (k, r)
        if r["status"] == _capi.REFINE_NO_OVERLAP:
            assert r["score"] == 0.0 and r["evals"] == 1 and np.array_equal(r["pose"], job), (k, r)
            assert not r["gradient"].any() and not r["hessian"].any()
        assert np.array_equal(r["hessian"], r["hessian"].T)


def _same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["status"] == y["status"] and x["evals"] == y["evals"] and x["steps"] == y["steps"], (x, y)
        assert x["score"] == y["score"] and x["start_score"] == y["start_score"], (x, y)
        for key in ("pose", "gradient", "hessian"):
            assert np.array_equal(x[key], y[key]), (key, x, y)


def _check_terms(c, poses, results, n):
    """Check 1: each of the ten sums within (N + 64) 2^-53 sum |term_i| of the restatement, the
    magnitudes taken from the restatement; f_start / N within TOL_TIGHT of the oracle."""
    worst = 0.0
    for k, (pose, r) in enumerate(zip(poses, results)):
        (f, g, H), mag = R.evaluate(c["grid"], c["beams"], pose, order="strided")
        want = np.array([f] + list(g) + list(H)) / n
        h = r["hessian"]
        got = np.array([r["start_score"]] + list(r["gradient"]) + [h[0, 0], h[0, 1], h[0, 2], h[1, 1], h[1, 2], h[2, 2]])
        bound = (n + 64) * EPS * mag / n
        dev = np.abs(got - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(mag > 0.0, dev / (EPS * mag / n), 0.0)
        print("pose %d: f/N %.17g restated %.17g; largest deviation %.2f x 2^-53 sum|term| (bound %d)" % (
            k, got[0], want[0], float(np.max(share)), n + 64))
        worst = max(worst, float(np.max(share)))
        assert np.all(dev <= bound), (k, got, want, bound)
        assert r["evals"] == 1 and r["steps"] == 0 and np.array_equal(r["pose"], pose)
        assert r["status"] == (_capi.REFINE_NO_OVERLAP if f == 0.0 else _capi.REFINE_MAX_EVALS)
        assert r["score"] == r["start_score"]
        assert abs(r["start_score"] - c["ref"].scorePoints(c["points"], pose)) < TOL_TIGHT
    return worst


@pytest.mark.parametrize("resolution", [0.25, 0.3])
def test_terms_against_the_restatement(fixture, resolution):
    """max_evals = 1: the ten sums at the fixture's twelve starts (beside the truth, rotated away,
    off the map), power-of-two and divide indexing.  Measured on an MI355X: at most 3.0 x 2^-53
    sum |term| (bound N + 64 = 164): the restatement's strided order is the kernel's, what is left
    is the device's exp against libm's."""
    c = dict(refine_cases.case(fixture, resolution, 100), points=fixture["query"])
    m = _matcher(fixture, ndt_resolution=resolution)
    got = m.refineScans(STARTS, [fixture["query"]], job_scan=[0] * len(STARTS), max_evals=1)
    worst = _check_terms(c, STARTS, got, 100)
    print("resolution %.2f: largest deviation %.2f x 2^-53 sum |term|" % (resolution, worst))
    _check_contract(c["ref"], fixture["query"], STARTS, got, max_evals=1)
    assert sum(r["status"] == _capi.REFINE_NO_OVERLAP for r in got) >= 2          # (40, 40) and a heading turned away
    assert sum(r["start_score"] < -0.05 for r in got) >= 4


@pytest.mark.parametrize("beams", [100, 720])
@pytest.mark.parametrize("resolution", [0.25, 0.3])
def test_the_same_path_as_the_restatement(fixture, resolution, beams):
    """Twelve jobs: six starts within 10 cm of the truth and the oracle's lattice winners from
    them.  A job qualifies when three restatement runs -- sequential sums, the kernel's strided
    sums, a start nudged by 1e-13 -- agree on status and evals and on the pose to 1e-9; on a
    qualified job the device returns the same status and a pose within 100 x the spread of those
    runs (floor 1e-12).  At least 8 of the 12 qualify in every setting (9, 9, 11 and 9 do).
    Every job, qualified or not, obeys the contract.  Measured on an MI355X: every qualified job
    with the restatement's status and evaluation count, the largest deviation of a pose 1.3e-15."""
    c = refine_cases.case(fixture, resolution, beams)
    jobs = c["jobs"]
    m = _matcher(fixture, ndt_resolution=resolution, laser_max_beams=beams)
    got = m.refineScans(jobs, [fixture["query"]], job_scan=[0] * len(jobs))
    _check_contract(c["ref"], fixture["query"], jobs, got)
    qualified, worst, failures = 0, 0.0, []
    for k, (job, r) in enumerate(zip(jobs, got)):
        runs = [R.refine(c["grid"], c["beams"], job), R.refine(c["grid"], c["beams"], job, order="strided"),
                R.refine(c["grid"], c["beams"], job + 1e-13)]
        same = all(x["status"] == runs[0]["status"] and x["evals"] == runs[0]["evals"] for x in runs)
        spread = max(float(np.max(np.abs(x["pose"] - runs[0]["pose"]))) for x in runs)
        ok = same and spread <= 1e-9
        dev = float(np.max(np.abs(r["pose"] - runs[1]["pose"])))
        print("job %2d: restated status %s evals %s spread %.2e %s | device status %d evals %d steps %d deviation %.2e "
              "score %.6f -> %.6f" % (k, [x["status"] for x in runs], [x["evals"] for x in runs], spread,
                                      "qualifies" if ok else "-", r["status"], r["evals"], r["steps"], dev, r["start_score"],
                                      r["score"]))
        if not ok:
            continue
        qualified += 1
        worst = max(worst, dev)
        if r["status"] != runs[0]["status"] or not dev <= max(100.0 * spread, 1e-12):
            failures.append((k, r["status"], runs[0]["status"], dev, spread))
    print("resolution %.2f, %d beams: %d of 12 qualify, largest device deviation %.3e" % (resolution, beams, qualified, worst))
    assert qualified >= 8, qualified
    assert not failures, failures


def test_refined_poses_score_below_the_lattice_winners(fixture):
    """refine_matches on the six near starts: the oracle scores every refined pose strictly
    below the lattice winner's pose (on the CPU: -0.26 .. -0.29 -> -0.29 .. -0.50)."""
    c = refine_cases.case(fixture, 0.25, 100)
    m = _matcher(fixture)
    out = refine_matches(m, refine_cases.NEAR6, [fixture["query"]], job_scan=[0] * 6)
    assert len(out) == 6 and m.has_ndt() == 1
    for k, r in enumerate(out):
        assert r["match"]["best_index"] != _capi.NO_INDEX
        assert np.array_equal(r["start"], refine_cases.NEAR6[k] + r["match"]["pose"])
        lattice = c["ref"].scorePoints(fixture["query"], r["start"])
        refined = c["ref"].scorePoints(fixture["query"], r["pose"])
        off = np.hypot(r["pose"][0] - TRUE_POSE[0], r["pose"][1] - TRUE_POSE[1])
        off0 = np.hypot(r["start"][0] - TRUE_POSE[0], r["start"][1] - TRUE_POSE[1])
        print("start %d: lattice winner %.6f (%.1f mm from the truth) -> refined %.6f (%.1f mm), %d evals, status %d" % (
            k, lattice, off0 * 1e3, refined, off * 1e3, r["refined"]["evals"], r["refined"]["status"]))
        assert abs(lattice - r["match"]["score"]) < TOL_TIGHT and abs(lattice - r["refined"]["start_score"]) < TOL_TIGHT
        assert refined < lattice, k
        assert abs(refined - r["score"]) < TOL_TIGHT
    _check_contract(c["ref"], fixture["query"], [r["start"] for r in out], [r["refined"] for r in out])


def _refine_records(m, jobs, beams, job_scan, slots, max_evals=32, tol=1e-6):
    """ndt2d_refine_run on an object of its own with `slots` slots, against the grid installed in
    the matcher's context; beams: already subsampled."""
    L = _capi.lib()
    obj = C.c_void_p()
    assert L.ndt2d_refine_create(m.device_handle, slots, C.byref(obj)) == _capi.OK
    try:
        offsets = np.zeros(len(beams) + 1, dtype=np.uintp)
        offsets[1:] = np.cumsum([len(b) for b in beams])
        flat = np.ascontiguousarray(np.concatenate(beams), dtype=np.float64)
        jp = np.ascontiguousarray(jobs, dtype=np.float64).reshape(-1, 3)
        js = None if job_scan is None else np.ascontiguousarray(job_scan, dtype=np.uint32)
        records = np.zeros((len(jp), 18))
        rc = L.ndt2d_refine_run(obj, _capi.dptr(jp), None if js is None else js.ctypes.data_as(C.POINTER(C.c_uint32)), len(jp),
                                _capi.dptr(flat), offsets.ctypes.data_as(C.POINTER(C.c_size_t)), len(beams), max_evals, tol, tol,
                                _capi.dptr(records))
        if rc != _capi.OK:
            raise Ndt2dError(rc, "ndt2d_refine_run", L.ndt2d_refine_last_error(obj).decode())
        return records
    finally:
        L.ndt2d_refine_destroy(obj)


def _edge_case(fixture):
    """Eight jobs over four scans: jobs 0, 3 and 6 share scan 0, jobs 1 and 5 are identical, job 4
    is off the map, scan 2 is named by nobody."""
    w = fixture["world"]
    other = (-4.4, 1.6, -1.2)
    scans = [fixture["query"], synth.scan(w, other, 9901), synth.scan(w, (1.4, 4.6, 2.0), 9902),
             synth.scan(w, TRUE_POSE, 9903, n_beams=360)]
    jobs = np.array([refine_cases.NEAR6[0], (-4.43, 1.62, -1.21), refine_cases.NEAR6[2], refine_cases.NEAR6[4], OFF_MAP,
                     (-4.43, 1.62, -1.21), TRUE_POSE, refine_cases.NEAR6[5]])
    job_scan = [0, 1, 3, 0, 1, 1, 0, 3]
    return jobs, scans, job_scan


def _oracle_matcher(fixture, **params):
    ref = O.ScanMatcherNDT()
    ref.initialize(**dict(SMALL, ndt_resolution=0.25, range_max=RANGE_MAX, **params))
    ref.addScans(fixture["scans"])
    return ref


def test_edges_shared_scans_chunks_and_determinism(fixture):
    jobs, scans, job_scan = _edge_case(fixture)
    ref = refine_cases.case(fixture, 0.25, 100)["ref"]
    m = _matcher(fixture)
    before = m.matchScan(jobs[0], scans[0], want_scores=True)
    a = m.refineScans(jobs, scans, job_scan=job_scan)
    b = m.refineScans(jobs, scans, job_scan=job_scan)
    _same_bits(a, b)                                              # two calls
    _same_bits([a[1]], [a[5]])                                    # two identical jobs
    assert m.has_ndt() == 1
    for k, r in enumerate(a):
        _check_contract(ref, scans[job_scan[k]], [jobs[k]], [r])
    # off the map: nothing scores, the pose comes back bit for bit
    assert a[4]["status"] == _capi.REFINE_NO_OVERLAP and a[4]["evals"] == 1 and np.array_equal(a[4]["pose"], OFF_MAP)
    assert all(r["score"] < -0.05 and r["steps"] >= 1 for k, r in enumerate(a) if k != 4)
    # a job alone gives the bits it has among the others; job_scan = None: job k uses scan k
    for k in (0, 2, 5):
        _same_bits(m.refineScans(jobs[k:k + 1], [scans[job_scan[k]]]), [a[k]])
    _same_bits(m.refineScans(jobs[:2], scans[:2]), a[:2])
    # max_jobs = 3 with 8 jobs (three chunks, each uploading its own scans) gives the bits of one chunk
    sub = [R.subsample(s, 100) for s in scans]
    whole = _refine_records(m, jobs, sub, job_scan, slots=16)
    chunked = _refine_records(m, jobs, sub, job_scan, slots=3)
    assert np.array_equal(whole, chunked, equal_nan=True)
    # ... and the object's records are what the matcher's call turned into its results
    for k, r in enumerate(a):
        rec = whole[k]
        assert np.array_equal(rec[0:3], r["pose"]) and rec[4] / 100 == r["score"] and rec[3] / 100 == r["start_score"]
        assert np.array_equal(rec[5:8] / 100, r["gradient"]) and rec[8] / 100 == r["hessian"][0, 0]
        assert (int(rec[14]), int(rec[15]), int(rec[16])) == (r["evals"], r["steps"], r["status"])
        assert rec[17] >= 0.0 and (rec[16] != _capi.REFINE_STALLED or rec[17] > 1e12)
    # a matchScan after the calls equals one before them
    after = m.matchScan(jobs[0], scans[0], want_scores=True)
    assert after["score"] == before["score"] and after["best_index"] == before["best_index"]
    assert np.array_equal(after["scores"], before["scores"]) and np.array_equal(after["covariance"], before["covariance"])
    assert m.refineScans(np.zeros((0, 3)), scans) == [] and m.refineScans(np.zeros((0, 3)), []) == []
    # timing is there once the object is
    m.refine_set_timing(True)
    m.refineScans(jobs, scans, job_scan=job_scan)
    kernel_ms, fetch_ms = m.refine_last_ms()
    assert kernel_ms > 0.0 and fetch_ms >= 0.0
    m.refine_set_timing(False)


def test_edges_one_beam_and_more_than_one_staging_piece(fixture):
    """A scan of one beam; 1,500 beams -- past kStageBeams = 1,024, six trips of the 256 threads --
    checked term by term as well as end to end."""
    w = fixture["world"]
    long_scan = synth.scan(w, TRUE_POSE, 9910, n_beams=1500)
    assert len(long_scan) == 1500
    one_beam = fixture["query"][100:101]
    m = _matcher(fixture, laser_max_beams=2000)
    ref = _oracle_matcher(fixture, laser_max_beams=2000)
    jobs = np.array([refine_cases.NEAR6[0], refine_cases.NEAR6[1], refine_cases.NEAR6[3]])
    scans, job_scan = [long_scan, one_beam], [0, 1, 0]
    terms = m.refineScans(jobs, scans, job_scan=job_scan, max_evals=1)
    c = dict(ref=ref, grid=R.Grid.of_oracle(ref), beams=long_scan, points=long_scan)
    _check_terms(c, jobs[[0, 2]], [terms[0], terms[2]], 1500)
    c1 = dict(ref=ref, grid=c["grid"], beams=one_beam, points=one_beam)
    _check_terms(c1, jobs[1:2], terms[1:2], 1)
    got = m.refineScans(jobs, scans, job_scan=job_scan)
    for k, r in enumerate(got):
        print("job %d (%d beams): status %d evals %d steps %d score %.6f -> %.6f" % (
            k, len(scans[job_scan[k]]), r["status"], r["evals"], r["steps"], r["start_score"], r["score"]))
        _check_contract(ref, scans[job_scan[k]], [jobs[k]], [r])
    assert got[0]["score"] < got[0]["start_score"] < -0.05 and got[2]["score"] < got[2]["start_score"]


def test_edges_off_grid_and_non_finite_scan_points(fixture):
    jobs, scans, job_scan = _edge_case(fixture)
    ref = refine_cases.case(fixture, 0.25, 100)["ref"]
    m = _matcher(fixture)
    bad = offgrid_cases.off_grid_points(0.25, RANGE_MAX)
    scans = [s.copy() for s in scans]
    step = 720 / 100
    for i, (x, y, _) in enumerate(bad):
        scans[i % 2][int((3 * (i // 2) + 1) * step)] = (x, y)     # points the subsampling takes, in scans 0 and 1
    got = m.refineScans(jobs, scans, job_scan=job_scan)
    for k, r in enumerate(got):
        assert np.isfinite(r["score"]) and np.all(np.isfinite(r["pose"])) and np.all(np.isfinite(r["hessian"])), (k, r)
        _check_contract(ref, scans[job_scan[k]], [jobs[k]], [r])
    terms = m.refineScans(jobs[:2], scans[:2], max_evals=1)
    for k in range(2):
        c = dict(ref=ref, grid=R.Grid.of_oracle(ref), beams=R.subsample(scans[k], 100), points=scans[k])
        _check_terms(c, jobs[k:k + 1], terms[k:k + 1], 100)


def test_edges_a_degenerate_cell(fixture):
    """A designed grid (tests/designed_grids.py) on the matcher's context: the robot stands on a
    cell's mean, beam k ends 1.0 to the right of the mean of the k-th cell to the right, whose
    record gives it the exponent E exactly.  One row holds a NaN exponent and one an exponent of
    800 (exp = +inf): NOT_FINITE, the pose bit for bit; an ordinary row runs and obeys the contract."""
    E = np.full((8, 8), -1.0)
    E[5, :] = [-0.5, -1.5, -0.25, -2.0, -1.0, -0.75, -3.0, -0.125]
    E[3, 6] = float("nan")
    E[2, 5] = 800.0
    lat = D.Lattice(E, 4.0)
    cells6, sx, sy, cell, origin = lat.grid
    params = dict(SMALL, ndt_resolution=4.0, range_max=16.0, laser_max_beams=8)
    m = ScanMatcherNDT(0)
    m.initialize("designed", **params)
    m.addScans([((0.0, 0.0, 0.0), np.array([[1.0, 1.0]] * 5))])         # an NDT in place, then the designed records
    cells = np.ascontiguousarray(cells6, dtype=np.float64)
    assert _capi.lib().ndt2d_set_grid(m.device_handle, _capi.dptr(cells), sx, sy, cell, origin[0], origin[1]) == _capi.OK
    ref = O.ScanMatcherNDT()
    ref.initialize(**params)
    ref.setCells6(cells6, sx, sy, cell, origin)
    beams = lat.beams(4)
    h = lat.n_lin // 2
    rows = {3: _capi.REFINE_NOT_FINITE, 2: _capi.REFINE_NOT_FINITE, 5: None}
    jobs = np.array([(lat.pose[0], lat.pose[1] + cell * (gy - h), 0.0) for gy in rows])
    got = m.refineScans(jobs, [beams], job_scan=[0] * len(jobs))
    for job, r, (gy, status) in zip(jobs, got, rows.items()):
        print("row %d: status %d evals %d start %r score %r" % (gy, r["status"], r["evals"], r["start_score"], r["score"]))
        if status is not None:
            assert r["status"] == status and r["evals"] == 1 and np.array_equal(r["pose"], job)
            assert not np.isfinite(r["start_score"])
            want = ref.scorePoints(beams, job)
            assert (np.isnan(want) and np.isnan(r["score"])) or want == r["score"]
    _check_contract(ref, beams, jobs, got)
    assert got[2]["status"] != _capi.REFINE_NOT_FINITE and got[2]["start_score"] < 0.0


def test_edges_no_ndt_and_a_scan_without_points(fixture):
    jobs, scans, job_scan = _edge_case(fixture)
    ref = refine_cases.case(fixture, 0.25, 100)["ref"]
    m = _matcher(fixture)
    full = m.refineScans(jobs, scans, job_scan=job_scan)
    holed = [scans[0], np.zeros((0, 2)), scans[2], scans[3]]
    got = m.refineScans(jobs, holed, job_scan=job_scan)
    for k, r in enumerate(got):
        if job_scan[k] == 1:     # the jobs of the empty scan: nothing scores, the job keeps its pose
            assert r["status"] == _capi.REFINE_NO_OVERLAP and r["score"] == 0.0 == r["start_score"] and r["evals"] == 0
            assert np.array_equal(r["pose"], jobs[k]) and not r["gradient"].any() and not r["hessian"].any()
        else:
            _same_bits([r], [full[k]])
            _check_contract(ref, scans[job_scan[k]], [jobs[k]], [r])
    none = m.refineScans(jobs[:2], [np.zeros((0, 2))] * 2)
    assert all(r["status"] == _capi.REFINE_NO_OVERLAP and r["evals"] == 0 for r in none)
    # no NDT in place: every score 0.0, the poses are the jobs' own (src/scan_matcher_ndt.cpp:159)
    m.reset()
    assert m.has_ndt() == 0 and m.scorePoints(scans[0], jobs[0]) == 0.0
    empty = m.refineScans(jobs, scans, job_scan=job_scan)
    for k, r in enumerate(empty):
        assert r["status"] == _capi.REFINE_NO_OVERLAP and r["score"] == 0.0 == r["start_score"] and r["evals"] == 0
        assert np.array_equal(r["pose"], jobs[k])
    # ... and after the next build the call works again
    m.addScans(fixture["scans"])
    _same_bits(m.refineScans(jobs, scans, job_scan=job_scan), full)


def test_every_install_path_gives_the_same_bits(fixture):
    jobs, scans, job_scan = _edge_case(fixture)
    first = None
    for mode, by_id, name in (("host", False, "build/host"), ("device", False, "build/device"),
                              (None, True, "build/fused-small-map")):
        m = _matcher(fixture, build_mode=mode, by_id=by_id)
        assert m.last_build() == name, (mode, by_id, m.last_build())
        got = m.refineScans(jobs, scans, job_scan=job_scan)
        if first is None:
            first = got
        _same_bits(got, first)
    assert all(r["steps"] >= 1 for k, r in enumerate(first) if k != 4)


def test_refusals_name_the_job_or_scan_and_leave_the_matcher_usable(fixture):
    jobs, scans, job_scan = _edge_case(fixture)
    m = _matcher(fixture)
    good = m.refineScans(jobs, scans, job_scan=job_scan)
    bad = jobs.copy()
    bad[1, 1] = float("nan")
    for call, text in ((lambda: m.refineScans(bad, scans, job_scan=job_scan), "job 1"),
                       (lambda: m.refineScans(jobs, scans, job_scan=[0, 1, 4, 1, 0, 0, 0, 0]), "job 2"),
                       (lambda: m.refineScans(jobs, scans), "n_scans"),
                       (lambda: m.refineScans(jobs, scans, job_scan=job_scan, max_evals=0), "max_evals"),
                       (lambda: m.refineScans(jobs, scans, job_scan=job_scan, tol_lin=-1e-6), "tolerance"),
                       (lambda: m.refineScans(jobs, scans, job_scan=job_scan, tol_ang=float("nan")), "tolerance"),
                       (lambda: m.refineScans(jobs, scans, job_scan=job_scan, tol_lin=float("inf")), "tolerance")):
        with pytest.raises(Ndt2dError) as ei:
            call()
        assert ei.value.code == _capi.ERR_INVALID and text in str(ei.value), str(ei.value)
    assert m.has_ndt() == 1
    # at object level: the same, a scan without beams, offsets that decrease, too many beams; without a grid
    sub = [R.subsample(s, 100) for s in scans]
    for call, text in ((lambda: _refine_records(m, bad, sub, job_scan, 4), "job 1"),
                       (lambda: _refine_records(m, jobs, sub, [0, 1, 2, 4, 0, 0, 0, 0], 4), "job 3"),
                       (lambda: _refine_records(m, jobs, sub, None, 4), "n_scans"),
                       (lambda: _refine_records(m, jobs, [sub[0], sub[1], np.zeros((0, 2)), sub[3]], job_scan, 4), "scan 2"),
                       (lambda: _refine_records(m, jobs, sub, job_scan, 4, max_evals=0), "max_evals"),
                       (lambda: _refine_records(m, jobs, sub, job_scan, 4, tol=-1.0), "tolerance")):
        with pytest.raises(Ndt2dError) as ei:
            call()
        assert ei.value.code == _capi.ERR_INVALID and text in str(ei.value), str(ei.value)
    bare = ScanMatcherNDT(0)
    bare.initialize("bare", **dict(SMALL, ndt_resolution=0.25, range_max=RANGE_MAX))
    with pytest.raises(Ndt2dError) as ei:
        _refine_records(bare, bad, sub, job_scan, 4)
    assert ei.value.code == _capi.ERR_INVALID and "job 1" in str(ei.value), str(ei.value)
    with pytest.raises(Ndt2dError) as ei:
        _refine_records(bare, jobs, sub, job_scan, 4)
    assert ei.value.code == _capi.ERR_NO_GRID
    L = _capi.lib()
    obj = C.c_void_p()
    assert L.ndt2d_refine_create(m.device_handle, 4, C.byref(obj)) == _capi.OK
    try:
        z = np.zeros(36)
        jp = np.ascontiguousarray(jobs[:2])
        szp = C.POINTER(C.c_size_t)

        def call(offsets):
            return L.ndt2d_refine_run(obj, _capi.dptr(jp), None, 2, _capi.dptr(z), offsets.ctypes.data_as(szp), 2, 32, 1e-6, 1e-6,
                                      _capi.dptr(z))
        assert call(np.array([0, 3, 2], dtype=np.uintp)) == _capi.ERR_INVALID
        assert b"scan 1" in L.ndt2d_refine_last_error(obj)
        assert call(np.array([0, 1, (1 << 20) + 2], dtype=np.uintp)) == _capi.ERR_INVALID
        assert b"scan 1" in L.ndt2d_refine_last_error(obj)
        assert call(np.array([0, 0, 2], dtype=np.uintp)) == _capi.ERR_INVALID
        assert b"scan 0" in L.ndt2d_refine_last_error(obj)
        assert L.ndt2d_refine_run(obj, _capi.dptr(jp), None, 0, None, None, 0, 32, 1e-6, 1e-6, None) == _capi.OK
        assert L.ndt2d_refine_last_ms(obj, None, None) == _capi.ERR_STATE
        assert L.ndt2d_refine_create(m.device_handle, 0, C.byref(C.c_void_p())) == _capi.ERR_INVALID
        assert L.ndt2d_refine_create(m.device_handle, 4097, C.byref(C.c_void_p())) == _capi.ERR_INVALID
    finally:
        L.ndt2d_refine_destroy(obj)
    # afterwards the matcher works and gives the same results as before
    _same_bits(m.refineScans(jobs, scans, job_scan=job_scan), good)
