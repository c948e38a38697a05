"""Newton NDT registration over the 3 x 3 cells round a point (ndt2d_refine_set_neighbourhood,
refineScans(neighbourhood=9), csrc/refine/) and the covariance from its Hessian.

The yardstick is the CPU restatement of the 3 x 3 objective (tests/refine_neighbours_restatement.py,
pinned to the one-cell restatement and to central differences by
tests/test_refine_neighbours_host.py).  Fixture, cases and bounds are those of
tests/test_gpu_refine.py; the bound on a sum is its rule with one addition per item:
(9 N + 64) 2^-53 sum |term|.

What the checks measured on an MI355X is in the tests' docstrings and in DESIGN.md 3.13."""
import ctypes as C

import numpy as np
import pytest

import designed_grids as D
import refine_cases
import refine_neighbours_restatement as R9
import refine_restatement as R
from ndt_2d_amd import Ndt2dError, ScanMatcherNDT, _capi, synth
from test_gpu_match_starts import RANGE_MAX, SMALL, STARTS, TRUE_POSE, _matcher, fixture  # noqa: F401

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
REC = 18


def _run(m, jobs, beams, cells, slots=16, max_evals=32, tol=1e-6, job_scan=None):
    """ndt2d_refine_run on an object of its own with `slots` slots against the grid installed in
    the matcher's context; beams: the scans, already subsampled; job_scan None: every job uses scan
    0.  cells None: the neighbourhood is never set."""
    L = _capi.lib()
    obj = C.c_void_p()
    assert L.ndt2d_refine_create(m.device_handle, slots, C.byref(obj)) == _capi.OK
    try:
        if cells is not None:
            assert L.ndt2d_refine_set_neighbourhood(obj, cells) == _capi.OK
        got = C.c_uint32(0)
        assert L.ndt2d_refine_neighbourhood(obj, C.byref(got)) == _capi.OK and got.value == (cells or 1)
        offsets = np.zeros(len(beams) + 1, dtype=np.uintp)
        offsets[1:] = np.cumsum([len(b) for b in beams])
        flat = np.ascontiguousarray(np.concatenate(beams), dtype=np.float64)
        jp = np.ascontiguousarray(jobs, dtype=np.float64).reshape(-1, 3)
        js = np.ascontiguousarray([0] * len(jp) if job_scan is None else job_scan, dtype=np.uint32)
        records = np.zeros((len(jp), REC))
        rc = L.ndt2d_refine_run(obj, _capi.dptr(jp), js.ctypes.data_as(C.POINTER(C.c_uint32)), len(jp), _capi.dptr(flat),
                                offsets.ctypes.data_as(C.POINTER(C.c_size_t)), len(beams), max_evals, tol, tol, _capi.dptr(records))
        if rc != _capi.OK:
            raise Ndt2dError(rc, "ndt2d_refine_run", L.ndt2d_refine_last_error(obj).decode())
        return records
    finally:
        L.ndt2d_refine_destroy(obj)


def _check_sums(grid, beams, poses, records, columns=10, quiet=False):
    """Each of the first `columns` sums of a max_evals = 1 record within (9 N + 64) 2^-53 sum |term|
    of the strided restatement, the magnitudes taken from the restatement.  Returns the largest
    deviation in units of 2^-53 sum |term|."""
    n = len(beams)
    worst = 0.0
    for k, (pose, rec) in enumerate(zip(poses, records)):
        (f, g, H), mag = R9.evaluate(grid, beams, pose, order="strided")
        want = np.array([f] + list(g) + list(H))[:columns]
        got = np.concatenate([rec[3:4], rec[5:14]])[:columns]
        if not np.isfinite(f):
            assert int(rec[16]) == _capi.REFINE_NOT_FINITE and not np.isfinite(rec[3]), (k, rec)
            continue
        dev = np.abs(got - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(mag[:columns] > 0.0, dev / (EPS * mag[:columns]), 0.0)
        if not quiet:
            print("pose %d: f %.17g restated %.17g; largest deviation %.2f x 2^-53 sum|term| (bound %d)" % (
                k, got[0], want[0], float(np.max(share)), 9 * n + 64))
        worst = max(worst, float(np.max(share)))
        assert np.all(dev <= (9 * n + 64) * EPS * mag[:columns]), (k, got, want, mag)
        assert np.array_equal(rec[0:3], pose) and rec[4] == rec[3] and (int(rec[14]), int(rec[15])) == (1, 0)
        assert int(rec[16]) == (_capi.REFINE_NO_OVERLAP if f == 0.0 else _capi.REFINE_MAX_EVALS)
    return worst


def test_one_cell_set_explicitly_has_the_bits_of_an_object_never_set(fixture):
    """Check 1.  Also here, on a real object: 0, 5 and 10 cells are refused with a message and the
    value stays."""
    for resolution in (0.25, 0.3):
        c = refine_cases.case(fixture, resolution, 100)
        m = _matcher(fixture, ndt_resolution=resolution)
        never = _run(m, c["jobs"], [c["beams"]], None)
        one = _run(m, c["jobs"], [c["beams"]], 1)
        assert np.array_equal(never, one, equal_nan=True)
        assert np.all(never[6:, 14] >= 2) and np.all(never[6:, 4] < never[6:, 3])    # the jobs from the lattice winners did run
        # ... and the 3 x 3 objective is another one
        assert not np.array_equal(_run(m, c["jobs"], [c["beams"]], 9)[:, 3], never[:, 3])
    L = _capi.lib()
    obj = C.c_void_p()
    assert L.ndt2d_refine_create(m.device_handle, 4, C.byref(obj)) == _capi.OK
    try:
        assert L.ndt2d_refine_set_neighbourhood(obj, 9) == _capi.OK
        for cells in (0, 5, 10):
            assert L.ndt2d_refine_set_neighbourhood(obj, cells) == _capi.ERR_INVALID
            assert b"%d cells" % cells in L.ndt2d_refine_last_error(obj)
        got = C.c_uint32(0)
        assert L.ndt2d_refine_neighbourhood(obj, C.byref(got)) == _capi.OK and got.value == 9
        assert L.ndt2d_refine_neighbourhood(obj, None) == _capi.ERR_INVALID
    finally:
        L.ndt2d_refine_destroy(obj)
    for cells in (0, 5, 10):
        with pytest.raises(Ndt2dError) as ei:
            m.set_refine_neighbourhood(cells)
        assert ei.value.code == _capi.ERR_INVALID and "%d cells" % cells in str(ei.value)
    assert m.refine_neighbourhood() == 1


@pytest.mark.parametrize("resolution", [0.25, 0.3])
def test_terms_of_nine_cells_against_the_restatement(fixture, resolution):
    """Check 2.  max_evals = 1, the fixture's twelve starts (beside the truth, rotated away, off the
    map), power-of-two and divide indexing, 100 beams (900 items: four trips of the 256 threads,
    the last one partial); bound 9 N + 64 = 964 units of 2^-53 sum |term|.  Measured on an MI355X:
    at most 1.9 units at 0.25 and 0.3 units at 0.3 (the restatement's strided order is the kernel's;
    what is left is the device's exp against libm's).  With nine cells a heading turned away from the
    map still catches a neighbour (f = -9e-24 at 0.3): only the start off the map is sure to have
    no overlap."""
    c = refine_cases.case(fixture, resolution, 100)
    m = _matcher(fixture, ndt_resolution=resolution)
    records = _run(m, STARTS, [c["beams"]], 9, max_evals=1)
    worst = _check_sums(c["grid"], c["beams"], STARTS, records)
    print("resolution %.2f: largest deviation %.2f x 2^-53 sum |term|" % (resolution, worst))
    assert np.sum(records[:, 16] == _capi.REFINE_NO_OVERLAP) >= 1 and np.sum(records[:, 3] < -5.0) >= 4
    assert int(records[7, 16]) == _capi.REFINE_NO_OVERLAP and not records[7, 5:14].any()      # (40, 40): off the map
    # the one-cell objective at the same poses: the neighbours only add
    one = _run(m, STARTS, [c["beams"]], 1, max_evals=1)
    assert np.all(records[:, 3] <= one[:, 3] + 964 * EPS * np.abs(one[:, 3]))


def test_terms_of_nine_cells_on_a_long_scan(fixture):
    """Check 2, 1,500 beams once: 13,500 items, 53 trips.  Bound 13,564 units; measured on an
    MI355X: 0.73."""
    w = fixture["world"]
    long_scan = synth.scan(w, TRUE_POSE, 9910, n_beams=1500)
    assert len(long_scan) == 1500
    c = refine_cases.case(fixture, 0.25, 100)
    m = _matcher(fixture, laser_max_beams=2000)
    jobs = refine_cases.NEAR6[[0, 3]]
    records = _run(m, jobs, [long_scan], 9, max_evals=1)
    worst = _check_sums(c["grid"], long_scan, jobs, records)
    print("1,500 beams: largest deviation %.2f x 2^-53 sum |term|" % worst)
    assert np.all(records[:, 3] < -100.0)


def _designed(cell, E, shape):
    """A matcher whose context holds the designed grid of E's shape (tests/designed_grids.py), the
    restatement's view of it, and the lattice."""
    lat = D.Lattice(E, cell, shape)
    cells6, sx, sy, size, origin = lat.grid
    m = ScanMatcherNDT(0)
    m.initialize("designed", **dict(SMALL, ndt_resolution=cell, range_max=64.0, laser_max_beams=64))
    m.addScans([((0.0, 0.0, 0.0), np.array([[1.0, 1.0]] * 5))])         # an NDT in place, then the designed records
    cells = np.ascontiguousarray(cells6, dtype=np.float64)
    assert _capi.lib().ndt2d_set_grid(m.device_handle, _capi.dptr(cells), sx, sy, size, origin[0], origin[1]) == _capi.OK
    return m, R.Grid(cells6, sx, sy, size, origin), lat


def _beams_to(pose, targets):
    """Robot-frame beams whose end points at `pose` are the world points `targets`."""
    c, s = R.cos_sin(pose[2])
    d = np.asarray(targets, dtype=np.float64) - np.array(pose[:2])
    return np.column_stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]])


@pytest.mark.parametrize("cell", [4.0, 3.0])
def test_edges_of_the_grid(cell):
    """Check 3.  A grid of 3 x 2 cells in which every cell scores (isotropic records a quarter to
    one cell wide, so that every neighbour's term is far above rounding): one beam ends in each cell
    -- every point has clipped neighbours, the corners have four cells, the two middle ones six --,
    one beam ends just outside each side of the grid, one is NaN.  Power-of-two and divide indexing.
    A neighbour taken from the flat index instead of (gx, gy) would give the points in column 0 and
    column 2 cells of the next row: other items count then, with other records.  Measured on an
    MI355X: at most 1.15 units of 2^-53 sum |term| (bound 163)."""
    E = -np.array([[0.5, 0.125, 0.25], [0.0625, 1.0, 0.03125]])
    m, grid, lat = _designed(cell, E, "iso")
    ox, oy = lat.origin
    pose = (0.375, -0.25, 0.3)
    inside = [(ox + cell * (gx + fx), oy + cell * (gy + fy)) for (gy, gx), (fx, fy) in zip(
        [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)], [(0.25, 0.5), (0.5, 0.75), (0.9, 0.1), (0.05, 0.95), (0.6, 0.4), (0.75, 0.25)])]
    tiny = cell * 2.0 ** -20
    outside = [(ox - tiny, oy + 0.5 * cell), (ox + 3 * cell + tiny, oy + 1.5 * cell), (ox + 1.5 * cell, oy - tiny),
               (ox + 0.5 * cell, oy + 2 * cell + tiny)]
    beams = np.vstack([_beams_to(pose, inside + outside), [[float("nan"), 1.0]]])
    # the restatement's own view of the case: which items count
    _, has = R9.item_terms(grid, beams, pose)
    per_beam = has.reshape(len(beams), 9).sum(axis=1)
    assert list(per_beam) == [4, 6, 4, 4, 6, 4, 0, 0, 0, 0, 0]
    own = grid.index(*(np.array(inside).T))
    assert list(own) == [0, 1, 2, 3, 4, 5]
    jobs = np.array([pose, (pose[0] + 0.5, pose[1] + 0.25, pose[2] - 0.02)])
    records = _run(m, jobs, [beams], 9, max_evals=1)
    worst = _check_sums(grid, beams, jobs, records)
    print("cell %.1f: largest deviation %.2f x 2^-53 sum |term|" % (cell, worst))
    # the off-grid and NaN beams add nothing: without them the sums are the same to the same bound
    alone = _run(m, jobs, [beams[:6]], 9, max_evals=1)
    _check_sums(grid, beams[:6], jobs, alone)
    (f, g, H), mag = R9.evaluate(grid, beams, pose, order="strided")
    both = np.concatenate([records[0, 3:4], records[0, 5:14]]), np.concatenate([alone[0, 3:4], alone[0, 5:14]])
    assert np.all(np.abs(both[0] - both[1]) <= 2 * (9 * len(beams) + 64) * EPS * mag)
    # every cell's term matters: the one-cell sum is well away
    one = _run(m, jobs, [beams], 1, max_evals=1)
    assert np.all(records[:, 3] < one[:, 3] - 0.1) and np.all(np.isfinite(records))


def test_a_degenerate_neighbour():
    """Check 4.  The beam's own cell is sound, the cell to its right has a NaN exponent: NOT_FINITE
    with the 3 x 3 objective, the pose bit for bit; the one-cell objective does not see it."""
    E = np.array([[-0.5, float("nan"), -0.25], [-0.125, -1.0, -0.75]])
    m, grid, lat = _designed(4.0, E, "rank1")
    ox, oy = lat.origin
    pose = (0.375, -0.25, 0.3)
    beams = _beams_to(pose, [(ox + 2.0, oy + 2.0), (ox + 1.0, oy + 6.5)])             # cells (0, 0) and (0, 1)
    assert list(grid.index(*(_beams_to((0.0, 0.0, 0.0), [(ox + 2.0, oy + 2.0), (ox + 1.0, oy + 6.5)]).T))) == [0, 3]
    jobs = np.array([pose])
    nine = _run(m, jobs, [beams], 9)
    assert int(nine[0, 16]) == _capi.REFINE_NOT_FINITE and np.array_equal(nine[0, 0:3], pose) and np.isnan(nine[0, 3])
    assert (int(nine[0, 14]), int(nine[0, 15])) == (1, 0)
    (f, _, _), _ = R9.evaluate(grid, beams, pose)
    assert np.isnan(f)
    one = _run(m, jobs, [beams], 1)
    assert int(one[0, 16]) != _capi.REFINE_NOT_FINITE and np.isfinite(one[0, 4]) and one[0, 3] < 0.0
    # a diagonal neighbour counts as well: from cell (2, 1) the degenerate cell (1, 0) is one ...
    far = _beams_to(pose, [(ox + 10.0, oy + 6.0)])
    assert int(_run(m, jobs, [far], 9)[0, 16]) == _capi.REFINE_NOT_FINITE
    # ... and a degenerate cell two columns away, (0, 0), is none
    E2 = np.array([[float("nan"), -0.5, -0.25], [-0.125, -1.0, -0.75]])
    m2, _, _ = _designed(4.0, E2, "rank1")
    assert int(_run(m2, jobs, [far], 9, max_evals=1)[0, 16]) == _capi.REFINE_MAX_EVALS


def test_the_line_of_three_hundred_poses(fixture):
    """Check 5.  300 poses jobs[1] + k (0.5 mm, 0.3 mm, 0) as 300 jobs sharing one scan,
    max_evals = 1, 100 beams: f and g within the bound of check 2 of the restatement, the trapezoid
    defect from the device's own f and g within 1 % + 1e-9 of the restatement's (0.0482201 on an
    MI355X and restated, 7.8 with one cell; the largest deviation of a sum 2.3 units of 2^-53
    sum |term|), chunks of 3 and one chunk of 512 slots with the same records."""
    c = refine_cases.case(fixture, 0.25, 100)
    m = _matcher(fixture)
    poses = R9.line_poses(c["jobs"][1])
    records = _run(m, poses, [c["beams"]], 9, slots=512, max_evals=1)
    chunked = _run(m, poses, [c["beams"]], 9, slots=3, max_evals=1)
    assert np.array_equal(records, chunked, equal_nan=True)
    worst = _check_sums(c["grid"], c["beams"], poses, records, columns=4, quiet=True)
    f, g = [], []
    for p in poses:
        (fk, gk, _), _ = R9.evaluate(c["grid"], c["beams"], p)
        f.append(fk)
        g.append(gk)
    want, _ = R9.trapezoid_defect(poses, f, g)
    got, step = R9.trapezoid_defect(poses, records[:, 3], records[:, 5:8])
    print("line: largest deviation %.2f x 2^-53 sum |term|; defect %.6g on the device, %.6g restated (largest step %.3g)" % (
        worst, got, want, step))
    assert abs(got - want) <= 0.01 * want + 1e-9
    one = _run(m, poses, [c["beams"]], 1, slots=512, max_evals=1)
    assert R9.trapezoid_defect(poses, one[:, 3], one[:, 5:8])[0] >= 50.0 * got


TOTAL_QUALIFIED = {}


@pytest.mark.parametrize("beams", [100, 720])
@pytest.mark.parametrize("resolution", [0.25, 0.3])
def test_the_same_path_as_the_restatement_with_nine_cells(fixture, resolution, beams):
    """Check 6, tests/test_gpu_refine.py's path test on the 3 x 3 objective.  A job qualifies when
    three restatement runs -- sequential sums, the kernel's strided sums, a start nudged by 1e-13 --
    agree on status and evaluations and on the pose to 1e-9; on a qualified job the device returns
    the same status and evaluation count and a pose within 100 x the spread of those runs (floor
    1e-12).  Every job, qualified or not, never increases f, and the f / N it returns is the
    restated f9 / N at the pose it returns to 1e-9.  At least 4 of the 12 qualify in each setting
    and at least 28 of the 48 overall.  Measured on an MI355X: 9, 7, 10 and 8 qualify (34 of 48); on
    every qualified job the device returned the restatement's status and evaluation count, the
    largest deviation of a pose 1.6e-15."""
    c = refine_cases.case(fixture, resolution, beams)
    jobs, n = c["jobs"], c["n"]
    m = _matcher(fixture, ndt_resolution=resolution, laser_max_beams=beams)
    got = _run(m, jobs, [c["beams"]], 9)
    qualified, worst, failures = 0, 0.0, []
    for k, (job, rec) in enumerate(zip(jobs, got)):
        status, evals, steps = int(rec[16]), int(rec[14]), int(rec[15])
        assert rec[4] <= rec[3] < 0.0 and 1 <= evals <= 32 and steps <= evals - 1, (k, rec)
        assert status in (_capi.REFINE_CONVERGED, _capi.REFINE_MAX_EVALS, _capi.REFINE_STALLED), (k, rec)
        (f, _, _), _ = R9.evaluate(c["grid"], c["beams"], rec[0:3])
        assert abs(f / n - rec[4] / n) <= 1e-9, (k, f, rec[4])
        runs = [R9.refine(c["grid"], c["beams"], job), R9.refine(c["grid"], c["beams"], job, order="strided"),
                R9.refine(c["grid"], c["beams"], job + 1e-13)]
        same = all(x["status"] == runs[0]["status"] and x["evals"] == runs[0]["evals"] for x in runs)
        spread = max(float(np.max(np.abs(x["pose"] - runs[0]["pose"]))) for x in runs)
        ok = same and spread <= 1e-9
        dev = float(np.max(np.abs(rec[0:3] - runs[1]["pose"])))
        print("job %2d: restated status %s evals %s spread %.2e %s | device status %d evals %d steps %d deviation %.2e "
              "f/N %.6f -> %.6f" % (k, [x["status"] for x in runs], [x["evals"] for x in runs], spread,
                                    "qualifies" if ok else "-", status, evals, steps, dev, rec[3] / n, rec[4] / n))
        if not ok:
            continue
        qualified += 1
        worst = max(worst, dev)
        if status != runs[0]["status"] or evals != runs[0]["evals"] or not dev <= max(100.0 * spread, 1e-12):
            failures.append((k, status, runs[0]["status"], evals, runs[0]["evals"], dev, spread))
    print("resolution %.2f, %d beams: %d of 12 qualify, largest device deviation %.3e" % (resolution, beams, qualified, worst))
    TOTAL_QUALIFIED[(resolution, beams)] = qualified
    assert qualified >= 4, qualified
    assert not failures, failures
    if len(TOTAL_QUALIFIED) == 4:
        print("qualified overall: %d of 48 %r" % (sum(TOTAL_QUALIFIED.values()), TOTAL_QUALIFIED))
        assert sum(TOTAL_QUALIFIED.values()) >= 28, TOTAL_QUALIFIED


def _records_of(results, n):
    """refineScans' dicts as the fields of the records they were made from."""
    return [(tuple(r["pose"]), r["start_score"], r["score"], tuple(r["gradient"]), tuple(r["hessian"][np.triu_indices(3)]),
             r["evals"], r["steps"], r["status"]) for r in results]


def test_through_the_matcher(fixture):
    """Check 7.  refineScans with neighbourhood 9 has the bits of ndt2d_refine_run with 9 on the same
    subsampled beams; every CONVERGED job of (0.25, 100) has a covariance (on an MI355X: nine jobs,
    one sigma 1.5 .. 5.4 mm and 0.16 .. 0.73 mrad), equal to numpy's inverse of H N to 1e-10; back at 1
    the records are today's; every install path gives the same records at 9."""
    c = refine_cases.case(fixture, 0.25, 100)
    jobs, n = c["jobs"], c["n"]
    scans, job_scan = [fixture["query"]], [0] * len(jobs)
    m = _matcher(fixture)
    today = m.refineScans(jobs, scans, job_scan=job_scan)
    assert m.refine_neighbourhood() == 1
    m.set_refine_neighbourhood(9)
    assert m.refine_neighbourhood() == 9
    nine = m.refineScans(jobs, scans, job_scan=job_scan, neighbourhood=9)
    records = _run(m, jobs, [c["beams"]], 9)
    converged = 0
    for k, (r, rec) in enumerate(zip(nine, records)):
        assert np.array_equal(rec[0:3], r["pose"]) and rec[4] / n == r["score"] and rec[3] / n == r["start_score"], k
        assert np.array_equal(rec[5:8] / n, r["gradient"]), k
        assert np.array_equal(rec[8:14] / n, r["hessian"][np.triu_indices(3)]) and np.array_equal(r["hessian"], r["hessian"].T), k
        assert (int(rec[14]), int(rec[15]), int(rec[16])) == (r["evals"], r["steps"], r["status"]), k
        if r["status"] == _capi.REFINE_CONVERGED:
            converged += 1
            assert r["covariance"] is not None, (k, r)
            want = np.linalg.inv(r["hessian"] * n)
            assert np.all(np.abs(r["covariance"] - want) <= 1e-10 * np.abs(want)), (k, r["covariance"], want)
            assert np.array_equal(r["covariance"], r["covariance"].T)
            sigma = np.sqrt(np.diag(r["covariance"]))
            print("job %2d: %d evals, sigma %.2f mm %.2f mm %.3f mrad" % (k, r["evals"], 1e3 * sigma[0], 1e3 * sigma[1], 1e3 * sigma[2]))
        else:
            assert r["covariance"] is None or r["covariance"].shape == (3, 3)
    assert converged >= 6, converged
    # back to one cell: today's records again
    back = m.refineScans(jobs, scans, job_scan=job_scan, neighbourhood=1)
    assert m.refine_neighbourhood() == 1 and _records_of(back, n) == _records_of(today, n)
    assert _records_of(m.refineScans(jobs, scans, job_scan=job_scan), n) == _records_of(today, n)
    # every install path gives the same records at 9
    for mode, by_id, name in (("host", False, "build/host"), ("device", False, "build/device"), (None, True, "build/fused-small-map")):
        other = _matcher(fixture, build_mode=mode, by_id=by_id)
        assert other.last_build() == name, (mode, by_id, other.last_build())
        assert np.array_equal(_run(other, jobs, [c["beams"]], 9), records, equal_nan=True), name
        assert _records_of(other.refineScans(jobs, scans, job_scan=job_scan, neighbourhood=9), n) == _records_of(nine, n)
