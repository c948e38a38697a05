"""Match verification (ndt2d_verify_run, verifyScans, csrc/verify/): the kernel against the CPU
restatement (tests/verify_restatement.py, pinned to the oracle by tests/test_verify_host.py) on
the inputs of tests/verify_cases.py, which that file validates on the CPU.

The bound: classes, pierce flags and cells equal the restatement's exactly; m2 agrees to 1e-9
relative with a floor of 1e-12 absolute (the bound tests/test_gpu_parity.py holds scores to).  A
beam can change class only when its m2 lies within that tolerance of a gate, so every test but the
gate boundaries first asserts on the restatement that no m2 and no tested cell's r^T I r lies within
1e-8 relative of its gate."""
import ctypes as C
import itertools

import numpy as np
import pytest

import refine_restatement as R
import verify_cases as cases
import verify_restatement as V
from ndt_2d_amd import Ndt2dError, ScanMatcherNDT, _capi, explained_mask, relocalize

pytestmark = pytest.mark.gpu

U32P, U8P, SZP = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_size_t)
SMALL = dict(search_linear_size=0.1, search_linear_resolution=0.05, search_angular_size=0.02, search_angular_resolution=0.01)


def _installed(grid):
    """A matcher whose context holds the designed grid (as tests/test_gpu_refine_neighbours.py
    installs one): an NDT in place, then the designed records."""
    m = ScanMatcherNDT(0)
    m.initialize("designed", **dict(SMALL, ndt_resolution=grid.cell_size, range_max=64.0, laser_max_beams=64))
    m.addScans([((0.0, 0.0, 0.0), np.array([[1.0, 1.0]] * 5))])
    cells = np.ascontiguousarray(grid.cells, dtype=np.float64)
    assert _capi.lib().ndt2d_set_grid(m.device_handle, _capi.dptr(cells), grid.size_x, grid.size_y, grid.cell_size,
                                      grid.origin[0], grid.origin[1]) == _capi.OK
    return m


class Verifier:
    """An ndt2d_verify object of its own beside a matcher's context."""

    def __init__(self, m, slots=16):
        self.L = _capi.lib()
        self.obj = C.c_void_p()
        assert self.L.ndt2d_verify_create(m.device_handle, slots, C.byref(self.obj)) == _capi.OK

    def close(self):
        if self.obj:
            assert self.L.ndt2d_verify_destroy(self.obj) == _capi.OK
            self.obj = None

    def error(self):
        return self.L.ndt2d_verify_last_error(self.obj).decode()

    def run(self, jobs, scans, job_scan, want=(True, True, True)):
        """(rc, records[K, 8], classes, m2, cells[., 2]); the per-beam arrays None where not wanted."""
        jp = np.ascontiguousarray(jobs, dtype=np.float64).reshape(-1, 3)
        offsets = np.zeros(len(scans) + 1, dtype=np.uintp)
        offsets[1:] = np.cumsum([len(b) for b in scans])
        flat = np.ascontiguousarray(np.concatenate(scans), dtype=np.float64).reshape(-1, 2)
        js = None if job_scan is None else np.ascontiguousarray(job_scan, dtype=np.uint32)
        which = np.arange(len(jp)) if js is None else js
        n = int(sum(len(scans[int(s)]) for s in which if int(s) < len(scans)))
        records = np.full((len(jp), 8), 0xDEADBEEF, dtype=np.uint32)
        classes = np.full(n, 0xEE, dtype=np.uint8) if want[0] else None
        m2 = np.full(n, -7.0) if want[1] else None
        cells = np.full((n, 2), 0xABCDEF, dtype=np.uint32) if want[2] else None
        rc = self.L.ndt2d_verify_run(self.obj, _capi.dptr(jp), js.ctypes.data_as(U32P) if js is not None else None, len(jp),
                                     _capi.dptr(flat), offsets.ctypes.data_as(SZP), len(scans), records.ctypes.data_as(U32P),
                                     classes.ctypes.data_as(U8P) if want[0] else None, _capi.dptr(m2) if want[1] else None,
                                     cells.ctypes.data_as(U32P) if want[2] else None)
        return rc, records, classes, m2, cells


def _configured(m, cells=1, gate_inlier=cases.GATE_INLIER, gate_pierce=cases.GATE_PIERCE, rays=True, slots=16):
    v = Verifier(m, slots)
    assert v.L.ndt2d_verify_set_neighbourhood(v.obj, cells) == _capi.OK
    assert v.L.ndt2d_verify_set_gates(v.obj, gate_inlier, gate_pierce) == _capi.OK
    assert v.L.ndt2d_verify_set_rays(v.obj, 1 if rays else 0) == _capi.OK
    return v


def _restated(grid, jobs, scans, job_scan, exempt=False, **kw):
    """The restatement of every job, with the precondition: nothing within 1e-8 of a gate."""
    out = []
    for k, pose in enumerate(jobs):
        r = V.verify(grid, scans[k if job_scan is None else job_scan[k]], pose, **kw)
        if not exempt:
            assert V.near_gate(r, kw.get("gate_inlier", 9.0), kw.get("gate_pierce", 1.0)) == [], k
        out.append(r)
    return out


def _compare(got, want):
    """A device call's outputs against the restated jobs: records, classes, pierce flags and cells
    exactly; m2 to 1e-9 relative, floor 1e-12.  Returns the largest m2 deviation (relative)."""
    rc, records, classes, m2, cells = got
    assert rc == _capi.OK
    at, worst = 0, 0.0
    for k, w in enumerate(want):
        n = len(w["classes"])
        assert np.array_equal(records[k], w["record"]), (k, list(records[k]), list(w["record"]))
        if classes is not None:
            assert np.array_equal(classes[at:at + n] & 3, w["classes"]), k
            assert np.array_equal((classes[at:at + n] & 4) != 0, w["pierced_mask"]), k
            assert not (classes[at:at + n] & 0xF8).any()
        if cells is not None:
            assert np.array_equal(cells[at:at + n], w["cells"]), k
        if m2 is not None:
            g, e = m2[at:at + n], w["m2"]
            same = (g == e) | (np.isnan(g) & np.isnan(e))
            with np.errstate(invalid="ignore"):
                dev = np.where(same, 0.0, np.abs(g - e))
                # (a NaN m2 on both sides -- the degenerate cell -- is the same value: no bound is formed from it)
                assert np.all(same | (dev <= np.maximum(1e-9 * np.abs(e), 1e-12))), (k, g[~same], e[~same])
                rel = np.where(same | ~np.isfinite(e) | (e == 0.0), 0.0, dev / np.abs(e))
            worst = max(worst, float(np.max(rel)) if n else 0.0)
        at += n
    for arr in (classes, m2, cells):
        assert arr is None or len(arr) == at
    return worst


@pytest.mark.parametrize("which", ["pow2", "divide"])
@pytest.mark.parametrize("cells", [1, 9])
def test_designed_grids_against_the_restatement(which, cells):
    """The designed grids (8 x 8 cells of 0.5: power-of-two indexing; 7 x 13 of 0.75: divide): rays
    in every octant and on every half axis with a tested cell at distance 2 from the end and an
    untested one at distance 1, rays of 0 .. 3 cells and down the long columns, the robot's own cell
    scoring, a ray along gx = 0, a robot off the grid, ends off the grid, NaN and infinite beams, a
    degenerate cell; a straight and a turned pose.  Everything equals the restatement.  Measured on
    an MI355X: m2 bit for bit the restatement's in all four cases (largest deviation 0.0)."""
    d = cases.designed(which)
    poses, scans, job_scan = d.jobs()
    m = _installed(d.grid)
    v = _configured(m, cells)
    try:
        want = _restated(d.grid, poses, scans, job_scan, neighbourhood=cells)
        worst = _compare(v.run(poses, scans, job_scan), want)
        print("%s, %d cells: records %s; largest m2 deviation %.2e relative" % (
            which, cells, [[int(x) for x in w["record"]] for w in want], worst))
        assert want[3]["record"][6] == 0 and want[0]["record"][5] > 0            # off the grid: no walk; pierced rays elsewhere
        # rays off: the classes stand, nothing is walked or pierced
        assert v.L.ndt2d_verify_set_rays(v.obj, 0) == _capi.OK
        off = _restated(d.grid, poses, scans, job_scan, neighbourhood=cells, rays=False)
        _compare(v.run(poses, scans, job_scan), off)
        assert all(w["record"][5] == 0 and w["record"][6] == 0 for w in off)
        assert all(np.array_equal(a["classes"], b["classes"]) for a, b in zip(off, want))
    finally:
        v.close()


def test_gate_boundaries():
    """The one test where a value sits on a gate, exactly: identity information and offsets that
    make m2 = 4.0 and r^T I r = 4.0.  A gate of 4.0 takes the value, nextafter(4.0, 0) does not."""
    grid, pose, beams = cases.boundary_grid()
    m = _installed(grid)
    below = float(np.nextafter(4.0, 0.0))
    for gate, cls in ((4.0, V.INLIER), (below, V.OUTLIER)):
        v = _configured(m, 1, gate_inlier=gate)
        try:
            got = v.run([pose], [beams[:1]], [0])
            _compare(got, _restated(grid, [pose], [beams[:1]], [0], exempt=True, gate_inlier=gate))
            assert got[3][0] == 4.0 and got[2][0] & 3 == cls
        finally:
            v.close()
    for gate, pierced in ((4.0, True), (below, False)):
        v = _configured(m, 1, gate_pierce=gate)
        try:
            got = v.run([pose], [beams[1:]], [0])
            _compare(got, _restated(grid, [pose], [beams[1:]], [0], exempt=True, gate_pierce=gate))
            assert bool(got[2][0] & 4) == pierced and int(got[1][0, 5]) == int(pierced)
            assert int(got[4][0, 1]) == (4 * 8 + 2 if pierced else V.NO_CELL)
        finally:
            v.close()


def test_a_tie_goes_to_the_lower_neighbour_and_the_clip_is_on_gx_gy():
    for make in (cases.tie_grid, cases.wrap_grid):
        grid, pose, beams = make()
        m = _installed(grid)
        for cells in (9, 1):
            v = _configured(m, cells)
            try:
                _compare(v.run([pose], [beams], [0]), _restated(grid, [pose], [beams], [0], neighbourhood=cells))
            finally:
                v.close()
    grid, pose, beams = cases.tie_grid()
    m = _installed(grid)                        # (kept: the object is destroyed before its context)
    v = _configured(m, 9)
    try:
        got = v.run([pose], [beams], [0])
        assert int(got[4][0, 0]) == 4 and got[3][0] == 2.0                      # neighbour j = 3, not j = 5
    finally:
        v.close()


@pytest.fixture(scope="module")
def scene():
    s = cases.scenario()
    m = ScanMatcherNDT(0)
    m.initialize("verify", **s["params"])
    m.addScans(s["scans"])
    return dict(s, m=m)


def test_scan_lengths_chunks_shared_and_unnamed_scans(scene):
    """Scans of 1, 63, 64, 65, 255, 256 and 257 beams (the thread stride and the wave boundaries),
    each at the true and at a wrong pose; 1, 2 and 5 jobs with max_jobs = 2 against one chunk: the
    outputs are array_equal whole; a scan shared by three jobs; a scan no job names."""
    grid, q, m = scene["grid"], scene["query"], scene["m"]
    lengths = (1, 63, 64, 65, 255, 256, 257)
    scans = [q[i:i + n] for i, n in enumerate(lengths)]
    jobs = np.vstack([scene["jobs"][0]] * len(lengths) + [scene["jobs"][1]] * len(lengths))
    job_scan = list(range(len(lengths))) * 2
    for cells in (1, 9):
        v = _configured(m, cells, slots=64)
        try:
            _compare(v.run(jobs, scans, job_scan), _restated(grid, jobs, scans, job_scan, neighbourhood=cells))
        finally:
            v.close()
    # a scan shared by three jobs, a scan no job names (scan 1), job_scan NULL; chunks of two
    shared = [q[:257], q[100:165], q[300:364]]
    poses5 = np.vstack([scene["jobs"], scene["jobs"][:2] + 0.01])
    whole, chunked = _configured(m, 9, slots=16), _configured(m, 9, slots=2)
    try:
        for n_jobs in (1, 2, 5):
            js = [0, 2, 0, 0, 2][:n_jobs]
            a = whole.run(poses5[:n_jobs], shared, js)
            b = chunked.run(poses5[:n_jobs], shared, js)
            for x, y in zip(a[1:], b[1:]):
                assert np.array_equal(x, y, equal_nan=True)
            _compare(a, _restated(grid, poses5[:n_jobs], shared, js, neighbourhood=9))
        a = whole.run(poses5[:3], shared, None)                                   # job k uses scan k
        _compare(a, _restated(grid, poses5[:3], shared, None, neighbourhood=9))
        # per-beam outputs NULL and non-NULL in every combination: the records are the same
        full = whole.run(poses5, shared, [0, 2, 0, 0, 2])
        for want in itertools.product((False, True), repeat=3):
            part = chunked.run(poses5, shared, [0, 2, 0, 0, 2], want=want)
            assert part[0] == _capi.OK and np.array_equal(part[1], full[1])
            for x, y in zip(part[2:], full[2:]):
                assert x is None or np.array_equal(x, y, equal_nan=True)
    finally:
        whole.close()
        chunked.close()


def test_scenarios_on_cfg1(scene):
    """cfg-1's map and 720-beam query through verifyScans: the true pose, + 1 m in x, + 0.3 rad.
    The counts equal the restatement's, which holds the conditions (>= 90 % inliers and <= 2 %
    pierced at the true pose, >= 10 % pierced at each wrong pose: tests/test_verify_host.py).  Then
    the pillars: the map has them, the query's world does not; every piercing cell lies within one
    cell of a pillar."""
    m, grid, q = scene["m"], scene["grid"], scene["query"]
    want = _restated(grid, scene["jobs"], [q], [0, 0, 0], neighbourhood=9)
    got = m.verifyScans(scene["jobs"], [q], job_scan=[0, 0, 0], want_beams=True)         # laser_max_beams = 720: every beam
    for g, w in zip(got, want):
        r = w["record"]
        assert (g["n_beams"], g["off"], g["unseen"], g["outlier"], g["inlier"], g["pierced"], g["walked"]) == tuple(int(x) for x in r[:7])
        assert np.array_equal(g["classes"], w["classes"]) and np.array_equal(g["pierced_mask"], w["pierced_mask"])
        assert np.array_equal(g["cells"], w["cells"])
        assert np.allclose(g["m2"], w["m2"], rtol=1e-9, atol=1e-12)
    print("true pose %s, + 1 m %s, + 0.3 rad %s" % tuple({k: g[k] for k in ("inlier", "outlier", "unseen", "pierced")} for g in got))
    assert got[0]["inlier"] >= 648 and got[0]["pierced"] <= 14 and got[1]["pierced"] >= 72 and got[2]["pierced"] >= 72
    assert m.verify_parameters() == dict(neighbourhood=9, gate_inlier=9.0, gate_pierce=1.0, rays=True)
    # max_beams: the subsampling rule of matchScan; 0: every point
    sub = m.verifyScans(scene["jobs"][:1], [q], max_beams=100, want_beams=True)[0]
    w100 = _restated(grid, scene["jobs"][:1], [R.subsample(q, 100)], [0], neighbourhood=9)[0]
    assert sub["n_beams"] == 100 and np.array_equal(sub["classes"], w100["classes"]) and np.array_equal(sub["cells"], w100["cells"])
    every = m.verifyScans(scene["jobs"][:1], [q[:300]], max_beams=0, neighbourhood=1)[0]
    assert every["n_beams"] == 300 and every["walked"] == 300
    # a scan without points: zeros; the other job is not disturbed
    mixed = m.verifyScans(scene["jobs"][:2], [np.zeros((0, 2)), q], job_scan=[0, 1], want_beams=True)
    assert all(mixed[0][key] == 0 for key in ("n_beams", "off", "unseen", "outlier", "inlier", "pierced", "walked"))
    assert len(mixed[0]["classes"]) == 0 and mixed[1]["pierced"] == got[1]["pierced"] and len(mixed[1]["classes"]) == 720
    # the pillars
    p = cases.pillar_scenario()
    wantp = _restated(grid, p["jobs"], [p["query"]], [0], neighbourhood=9)[0]
    gotp = m.verifyScans(p["jobs"], [p["query"]], want_beams=True)[0]
    assert gotp["pierced"] == int(wantp["record"][5]) >= 1 and np.array_equal(gotp["cells"], wantp["cells"])
    assert np.array_equal(gotp["classes"], wantp["classes"]) and np.array_equal(gotp["pierced_mask"], wantp["pierced_mask"])
    assert all(cases.near_a_pillar(grid, c) for c in gotp["cells"][gotp["pierced_mask"], 1])
    keep = explained_mask(gotp)
    assert keep.sum() == int(np.sum((wantp["classes"] != V.OUTLIER) & ~wantp["pierced_mask"])) and not keep[gotp["pierced_mask"]].any()


def test_a_verification_between_two_matches_changes_neither(scene):
    """matchScan before and after verifyScans: the same scores, pose and covariance; the NDT stays
    in place; relocalize(verify=None) returns what it returned before, and with a dict the ranked
    starts gain the counts verifyScans gives at their poses."""
    m, q = scene["m"], scene["query"]
    guess = np.zeros(3)
    before = m.matchScan(guess, q, want_scores=True)
    starts = np.vstack([scene["true_pose"] + (0.02, -0.01, 0.005), scene["true_pose"] + (1.0, 0.0, 0.0)])
    plain_before = relocalize(m, q, starts)
    m.verifyScans(scene["jobs"], [q], job_scan=[0, 0, 0], want_beams=True)
    m.verifyScans(scene["jobs"][:1], [q], neighbourhood=1, rays=False)
    after = m.matchScan(guess, q, want_scores=True)
    assert m.has_ndt()
    assert np.array_equal(before["scores"], after["scores"]) and before["score"] == after["score"]
    assert np.array_equal(before["pose"], after["pose"]) and np.array_equal(before["covariance"], after["covariance"])
    assert before["best_index"] == after["best_index"]
    plain_after = relocalize(m, q, starts, verify=None)
    checked = relocalize(m, q, starts, verify=dict(neighbourhood=9))
    assert len(plain_before) == len(plain_after) == len(checked) == 2
    for a, b, c in zip(plain_before, plain_after, checked):
        assert sorted(a) == sorted(b) and sorted(c) == sorted(list(a) + ["verify"])
        for key in a:
            assert np.array_equal(a[key], b[key]) and np.array_equal(a[key], c[key]), key
        alone = m.verifyScans([c["pose"]], [q])[0]
        assert c["verify"] == alone
    assert checked[0]["verify"]["pierced"] < checked[1]["verify"]["pierced"]


def test_setters_getters_and_refusals(scene):
    m, q = scene["m"], scene["query"]
    v = Verifier(m, 4)
    L = v.L
    try:
        cells, rays = C.c_uint32(0), C.c_int(-1)
        gi, gp = C.c_double(0.0), C.c_double(0.0)
        assert L.ndt2d_verify_neighbourhood(v.obj, C.byref(cells)) == _capi.OK and cells.value == 1       # this layer's default
        assert L.ndt2d_verify_gates(v.obj, C.byref(gi), C.byref(gp)) == _capi.OK and (gi.value, gp.value) == (9.0, 1.0)
        assert L.ndt2d_verify_rays(v.obj, C.byref(rays)) == _capi.OK and rays.value == 1
        assert L.ndt2d_verify_set_neighbourhood(v.obj, 9) == _capi.OK
        assert L.ndt2d_verify_set_gates(v.obj, 6.5, 0.25) == _capi.OK
        assert L.ndt2d_verify_set_rays(v.obj, 0) == _capi.OK
        for bad in (0, 5, 10):
            assert L.ndt2d_verify_set_neighbourhood(v.obj, bad) == _capi.ERR_INVALID and "%d cells" % bad in v.error()
        for a, b in ((-1.0, 1.0), (1.0, -1e-300), (np.inf, 1.0), (1.0, np.nan), (np.nan, np.nan)):
            assert L.ndt2d_verify_set_gates(v.obj, a, b) == _capi.ERR_INVALID and "gate" in v.error()
        for bad in (2, -1):
            assert L.ndt2d_verify_set_rays(v.obj, bad) == _capi.ERR_INVALID and "0 or 1" in v.error()
        assert L.ndt2d_verify_neighbourhood(v.obj, C.byref(cells)) == _capi.OK and cells.value == 9      # the values stay
        assert L.ndt2d_verify_gates(v.obj, C.byref(gi), C.byref(gp)) == _capi.OK and (gi.value, gp.value) == (6.5, 0.25)
        assert L.ndt2d_verify_rays(v.obj, C.byref(rays)) == _capi.OK and rays.value == 0
        assert L.ndt2d_verify_set_gates(v.obj, 0.0, 0.0) == _capi.OK                                      # zero is a gate
        # what the registration refuses about jobs and scans, before anything is launched
        ok = scene["jobs"][:2]
        rc, records, _, _, _ = v.run([ok[0], (np.nan, 0.0, 0.0)], [q[:10]], [0, 0])
        assert rc == _capi.ERR_INVALID and "job 1" in v.error() and np.all(records == 0xDEADBEEF)
        assert v.run(ok, [q[:10]], [0, 1])[0] == _capi.ERR_INVALID and "job 1" in v.error()
        assert v.run(ok, [q[:10], q[:0]], [0, 0])[0] == _capi.ERR_INVALID and "scan 1" in v.error()
        assert v.run(ok, [q[:10]], None)[0] == _capi.ERR_INVALID and "n_scans" in v.error()
        assert v.run(np.zeros((0, 3)), [q[:10]], None)[0] == _capi.OK                                    # no jobs: nothing done
        assert L.ndt2d_verify_last_ms(v.obj, None, None) == _capi.ERR_STATE
        assert L.ndt2d_verify_set_timing(v.obj, 1) == _capi.OK
        assert v.run(ok, [q[:10]], [0, 0])[0] == _capi.OK
        k_ms, f_ms = C.c_float(-1.0), C.c_float(-1.0)
        assert L.ndt2d_verify_last_ms(v.obj, C.byref(k_ms), C.byref(f_ms)) == _capi.OK and k_ms.value >= 0.0 and f_ms.value >= 0.0
    finally:
        v.close()
    assert L.ndt2d_verify_create(m.device_handle, 0, C.byref(C.c_void_p())) == _capi.ERR_INVALID
    assert L.ndt2d_verify_create(m.device_handle, 4097, C.byref(C.c_void_p())) == _capi.ERR_INVALID
    # no grid in the context
    bare = ScanMatcherNDT(0)
    bare.initialize("bare", **scene["params"])
    vb = Verifier(bare, 4)
    try:
        assert vb.run(scene["jobs"][:1], [q[:10]], [0])[0] == _capi.ERR_NO_GRID and "no grid" in vb.error()
    finally:
        vb.close()
    with pytest.raises(Ndt2dError) as ei:
        bare.verifyScans(scene["jobs"][:1], [q])
    assert ei.value.code == _capi.ERR_NO_GRID
    # the matcher layer: its default is nine cells; refusals leave the values
    fresh = ScanMatcherNDT(0)
    fresh.initialize("fresh", **scene["params"])
    assert fresh.verify_parameters() == dict(neighbourhood=9, gate_inlier=9.0, gate_pierce=1.0, rays=True)
    fresh.set_verify(neighbourhood=1, gate_inlier=4.0, rays=False)
    for kw in (dict(neighbourhood=3), dict(gate_inlier=-1.0), dict(gate_pierce=float("inf"))):
        with pytest.raises(Ndt2dError) as ei:
            fresh.set_verify(**kw)
        assert ei.value.code == _capi.ERR_INVALID
    assert fresh.verify_parameters() == dict(neighbourhood=1, gate_inlier=4.0, gate_pierce=1.0, rays=False)
    with pytest.raises(Ndt2dError) as ei:
        m.verifyScans([(np.inf, 0.0, 0.0)], [q])
    assert ei.value.code == _capi.ERR_INVALID and "job 0" in str(ei.value)
    with pytest.raises(Ndt2dError):
        fresh.verify_set_timing(True)                                              # no verifyScans yet on `fresh`: no object
    m.verifyScans(scene["jobs"][:1], [q])
    m.verify_set_timing(True)
    m.verifyScans(scene["jobs"], [q], job_scan=[0, 0, 0])
    kernel_ms, fetch_ms = m.verify_last_ms()
    assert kernel_ms >= 0.0 and fetch_ms >= 0.0
    m.verify_set_timing(False)
