"""Newton NDT registration on each loop-closure candidate's own map (ScanMatcherNDT.refineCandidates,
ndt2d_closure_refine, csrc/closure/): the candidates' maps are built in the closure's slots and the
refinement's kernel runs on them, a block per job, in one launch.

The yardstick is the sequential path on the same matcher -- reset(), addScansById(candidate),
refineScans([job], [query]) -- bit for bit, with no tolerance: the closure build makes the fused
build's grid and the kernel has one text for both map sources.  The CPU restatements
(tests/refine_restatement.py, tests/refine_neighbours_restatement.py) over the oracle's build of each
candidate bound the sums themselves.  Cases: tests/closure_refine_cases.py."""
import ctypes as C

import numpy as np
import pytest

import closure_refine_cases as CC
import offgrid_cases
import refine_neighbours_restatement as R9
import refine_restatement as R
from ndt_2d_amd import Ndt2dError, ScanMatcherNDT, _capi, close_loops, loop_closure_window

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
REC = 18
KEYS = ("pose", "score", "start_score", "gradient", "hessian", "status", "evals", "steps")
_MATCHERS = {}


def _matcher(resolution):
    """A matcher with the graph's ten scans stored under their indices and the designed scan of
    this resolution behind them; one per resolution for the module."""
    if resolution not in _MATCHERS:
        c = CC.case(resolution)
        m = ScanMatcherNDT(0)
        m.initialize("closure_refine", **c["params"])
        for i, pts in enumerate(CC.graph()["points"]):
            assert m.storeScan(pts) == i
        assert m.storeScan(c["designed_scan"]) == CC.DESIGNED_ID
        _MATCHERS[resolution] = m
    return _MATCHERS[resolution]


@pytest.fixture(scope="module", autouse=True)
def _close_matchers():
    yield
    for m in _MATCHERS.values():
        m.close()
    _MATCHERS.clear()


def _sequential(m, cand, job, query, cells, **kw):
    m.reset()
    m.addScansById([p for _, p in cand], [i for i, _ in cand])
    return m.refineScans([job], [query], neighbourhood=cells, **kw)[0]


def _same(got, want, where=None):
    for key in KEYS:
        assert np.array_equal(got[key], want[key], equal_nan=True), (where, key, got[key], want[key])
    assert (got["covariance"] is None) == (want["covariance"] is None), (where, got["covariance"], want["covariance"])
    if got["covariance"] is not None:
        assert np.array_equal(got["covariance"], want["covariance"]), where


def _all_jobs(c):
    """Every slot of the case from both its starts: (jobs, scans, candidates, job_candidate, job_scan);
    scan 0 is the graph's query, scan 1 the designed one."""
    jobs, jc, js = [], [], []
    for k, s in enumerate(c["slots"]):
        for start in s["starts"]:
            jobs.append(start)
            jc.append(k)
            js.append(1 if k == len(c["slots"]) - 1 else 0)
    return np.array(jobs), [c["slots"][0]["query"], c["slots"][-1]["query"]], [s["candidate"] for s in c["slots"]], jc, js


@pytest.mark.parametrize("cells", [1, 9])
@pytest.mark.parametrize("resolution", CC.RESOLUTIONS)
def test_the_bits_of_the_sequential_path(resolution, cells):
    """The main test: reset(); addScansById(c); refineScans([job], [query]) and refineCandidates give
    array_equal pose, score, start score, gradient, Hessian, status and evaluation counts, covariances
    both present and equal or both absent -- for every candidate (tests/test_gpu_closure.py's three, the two of wider
    grids, the designed one with beams in column 0, in the last row and beside cells of n < 5) from
    both starts, in ONE call of twelve jobs over six slots of four grid sizes."""
    c = CC.case(resolution)
    m = _matcher(resolution)
    jobs, scans, cands, jc, js = _all_jobs(c)
    want = [_sequential(m, cands[k], job, scans[s], cells) for job, k, s in zip(jobs, jc, js)]
    m.reset()
    got = m.refineCandidates(jobs, scans, cands, job_candidate=jc, job_scan=js, neighbourhood=cells)
    assert len(got) == len(want) == 12 and m.has_ndt() is False
    for k, (g, w) in enumerate(zip(got, want)):
        _same(g, w, (resolution, cells, k))
    # the jobs did run: every one evaluated, most of them stepped and ended lower than they began
    assert all(g["evals"] >= 1 for g in got) and sum(g["steps"] >= 1 and g["score"] < g["start_score"] for g in got) >= 6
    assert sum(g["covariance"] is not None for g in got) >= (4 if cells == 9 else 1)
    # job k on candidate k, no job_candidate: the first start of every slot
    first = m.refineCandidates(jobs[0::2], scans, cands, job_scan=js[0::2], neighbourhood=cells)
    for k, g in enumerate(first):
        _same(g, want[2 * k], (resolution, cells, "job k on candidate k", k))


def _sums(r, n):
    h = r["hessian"]
    return np.array([r["start_score"]] + list(r["gradient"]) + [h[0, 0], h[0, 1], h[0, 2], h[1, 1], h[1, 2], h[2, 2]])


@pytest.mark.parametrize("cells", [1, 9])
@pytest.mark.parametrize("resolution", CC.RESOLUTIONS)
def test_sums_against_the_cpu_restatements(resolution, cells):
    """max_evals = 1: the ten sums at the starts, on the slots' maps, within the project's bounds of
    2^-53 sum |term| -- (N + 64) units for one cell (tests/test_gpu_refine.py), (9 N + 64) for 3 x 3
    (tests/test_gpu_refine_neighbours.py) -- of the strided restatement over the ORACLE's build of
    each candidate.  Measured on an MI355X: at most 1.6 units with one cell (bound 164) and 2.9 with
    3 x 3 (bound 964); the designed slot's sums come out exact."""
    c = CC.case(resolution)
    m = _matcher(resolution)
    jobs, scans, cands, jc, js = _all_jobs(c)
    got = m.refineCandidates(jobs, scans, cands, job_candidate=jc, job_scan=js, max_evals=1, neighbourhood=cells)
    worst = 0.0
    for k, (job, slot, r) in enumerate(zip(jobs, jc, got)):
        s = c["slots"][slot]
        n = len(s["beams"])
        if cells == 1:
            (f, g, H), mag = R.evaluate(s["grid"], s["beams"], job, order="strided")
        else:
            (f, g, H), mag = R9.evaluate(s["grid"], s["beams"], job, order="strided")
        units = (n if cells == 1 else 9 * n) + 64
        want = np.array([f] + list(g) + list(H)) / n
        dev = np.abs(_sums(r, n) - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(mag > 0.0, dev / (EPS * mag / n), 0.0)
        print("res %.2f cells %d job %2d (slot %d): f/N %.17g restated %.17g; largest deviation %.2f x 2^-53 sum|term| (bound %d)" % (
            resolution, cells, k, slot, r["start_score"], want[0], float(np.max(share)), units))
        worst = max(worst, float(np.max(share)))
        assert f < 0.0 and np.all(dev <= units * EPS * mag / n), (k, _sums(r, n), want)
        assert r["evals"] == 1 and r["steps"] == 0 and np.array_equal(r["pose"], job) and r["status"] == _capi.REFINE_MAX_EVALS
    print("resolution %.2f, %d cells: largest deviation %.2f x 2^-53 sum |term|" % (resolution, cells, worst))


def _closure_refine(m, c, cands, jobs, beams, job_scan, job_candidate, slots, cells, max_evals=32):
    """ndt2d_closure_refine on a store and a closure object of their own (`slots` slots) on the
    matcher's context; beams: the scans, already subsampled.  Returns the records."""
    L = _capi.lib()
    h = m.device_handle
    store, closure = C.c_void_p(), C.c_void_p()
    assert L.ndt2d_scanstore_create(h, 1 << 16, 64, C.byref(store)) == _capi.OK
    try:
        for pts in list(CC.graph()["points"]) + [c["designed_scan"]]:
            p = np.ascontiguousarray(pts, dtype=np.float64)
            assert L.ndt2d_scanstore_append(store, _capi.dptr(p), len(p), None) == _capi.OK
        assert L.ndt2d_closure_create(h, store, slots, C.byref(closure)) == _capi.OK
        try:
            assert L.ndt2d_closure_set_neighbourhood(closure, 5) == _capi.ERR_INVALID
            assert b"5 cells" in L.ndt2d_closure_last_error(closure)
            assert L.ndt2d_closure_set_neighbourhood(closure, cells) == _capi.OK
            out = C.c_uint32(0)
            assert L.ndt2d_closure_neighbourhood(closure, C.byref(out)) == _capi.OK and out.value == cells
            szp = lambda a: a.ctypes.data_as(C.POINTER(C.c_size_t))      # noqa: E731
            u32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))     # noqa: E731
            offsets = np.zeros(len(cands) + 1, dtype=np.uintp)
            offsets[1:] = np.cumsum([len(k) for k in cands])
            ids = np.ascontiguousarray([i for k in cands for i, _ in k], dtype=np.uintp)
            poses = np.ascontiguousarray([q for k in cands for _, q in k], dtype=np.float64)
            boff = np.zeros(len(beams) + 1, dtype=np.uintp)
            boff[1:] = np.cumsum([len(b) for b in beams])
            flat = np.ascontiguousarray(np.concatenate(beams), dtype=np.float64)
            jp = np.ascontiguousarray(jobs, dtype=np.float64).reshape(-1, 3)
            js = np.ascontiguousarray(job_scan, dtype=np.uint32)
            jc = np.ascontiguousarray(job_candidate, dtype=np.uint32)
            records = np.zeros((len(jp), REC))
            p = c["params"]
            rc = L.ndt2d_closure_refine(closure, len(cands), szp(offsets), szp(ids), _capi.dptr(poses), p["ndt_resolution"],
                                        p["range_max"], _capi.dptr(jp), u32p(js), u32p(jc), len(jp), _capi.dptr(flat), szp(boff),
                                        len(beams), max_evals, 1e-6, 1e-6, _capi.dptr(records))
            if rc != _capi.OK:
                raise Ndt2dError(rc, "ndt2d_closure_refine", L.ndt2d_closure_last_error(closure).decode())
            return records
        finally:
            L.ndt2d_closure_destroy(closure)
    finally:
        L.ndt2d_scanstore_destroy(store)


def test_a_job_depends_on_nothing_but_itself():
    """Six jobs over three candidates, job_candidate = [0, 0, 1, 2, 2, 1], two distinct scans: each
    job alone and all together give the same records, and so do two calls.  Through the C entry
    points a closure of 2 slots with 5 candidates equals one of 8 slots; through the matcher 17
    candidates -- two chunks of its 16 slots -- equal the same jobs run singly."""
    c = CC.case(0.25)
    m = _matcher(0.25)
    g = CC.graph()
    cands = [s["candidate"] for s in c["slots"][:3]]
    scans = [g["query"], g["points"][7]]
    jc, js = [0, 0, 1, 2, 2, 1], [0, 1, 0, 1, 0, 0]
    jobs = np.array([c["slots"][0]["starts"][0], g["poses"][7] + (0.02, -0.01, 0.01), c["slots"][1]["starts"][1],
                     g["poses"][7] + (-0.03, 0.02, -0.01), c["slots"][2]["starts"][0], c["slots"][1]["starts"][0]])
    for cells in (1, 9):
        together = m.refineCandidates(jobs, scans, cands, job_candidate=jc, job_scan=js, neighbourhood=cells)
        again = m.refineCandidates(jobs, scans, cands, job_candidate=jc, job_scan=js, neighbourhood=cells)
        assert sum(r["steps"] >= 1 for r in together) >= 4
        for k in range(6):
            _same(again[k], together[k], ("again", cells, k))
            alone = m.refineCandidates([jobs[k]], [scans[js[k]]], [cands[jc[k]]], neighbourhood=cells)[0]
            _same(alone, together[k], ("alone", cells, k))
    # 2 slots with 5 candidates (chunks of 2, 2 and 1) against 8 slots; the jobs name the candidates out of order
    cands5 = [s["candidate"] for s in c["slots"][:5]]
    beams = [R.subsample(g["query"], CC.BEAMS), R.subsample(g["points"][7], CC.BEAMS)]
    jobs8 = np.array([c["slots"][k]["starts"][i] for k, i in ((4, 0), (0, 1), (3, 0), (1, 0), (2, 1), (0, 0), (4, 1), (2, 0))])
    jc8, js8 = [4, 0, 3, 1, 2, 0, 4, 2], [0] * 8
    for cells in (1, 9):
        two = _closure_refine(m, c, cands5, jobs8, beams, js8, jc8, 2, cells)
        eight = _closure_refine(m, c, cands5, jobs8, beams, js8, jc8, 8, cells)
        assert np.array_equal(two, eight, equal_nan=True) and np.all(two[:, 14] >= 2)
        # ... and they are the records behind the matcher's results
        via = m.refineCandidates(jobs8, [g["query"]], cands5, job_candidate=jc8, job_scan=js8, neighbourhood=cells)
        for k, r in enumerate(via):
            assert np.array_equal(r["pose"], two[k, 0:3]) and r["score"] == two[k, 4] / CC.BEAMS and r["status"] == int(two[k, 16])
    # 17 candidates through the matcher's 16 slots
    cands17 = [[(i, g["poses"][i])] for i in range(10)] + [[(i, g["poses"][i]), (i + 1, g["poses"][i + 1])] for i in range(7)]
    jobs17 = np.array([g["guess"] + (0.001 * k, -0.001 * k, 0.0005 * k) for k in range(17)])
    got = m.refineCandidates(jobs17, [g["query"]], cands17, job_scan=[0] * 17, neighbourhood=9)
    for k in range(17):
        _same(m.refineCandidates([jobs17[k]], [g["query"]], [cands17[k]], neighbourhood=9)[0], got[k], ("17", k))
    assert sum(r["steps"] >= 1 for r in got) >= 10


def test_edges():
    c = CC.case(0.25)
    m = _matcher(0.25)
    g = CC.graph()
    cand = c["slots"][0]["candidate"]
    start = c["slots"][0]["starts"][0]
    # a candidate the scan does not reach: its scan's pose is 40 m away
    far = [(4, g["poses"][4] + (40.0, 40.0, 0.0))]
    for cells in (1, 9):
        r = m.refineCandidates([start, start], [g["query"]], [far, cand], job_scan=[0, 0], neighbourhood=cells)
        assert r[0]["status"] == _capi.REFINE_NO_OVERLAP and np.array_equal(r[0]["pose"], start) and r[0]["score"] == 0.0
        assert r[0]["evals"] == 1 and r[0]["steps"] == 0 and not r[0]["gradient"].any() and r[0]["covariance"] is None
        _same(r[0], _sequential(m, far, start, g["query"], cells), ("far", cells))
        assert r[1]["steps"] >= 1
    # a query carrying NaN / +-inf / 1e300 / 2^32-cell beams at the off-grid tests' positions
    query = R.subsample(g["query"], CC.BEAMS)
    offg = offgrid_cases.off_grid_points(0.25, CC.RANGE_MAX)
    for i, k in enumerate(offgrid_cases.slots(len(query))):
        query[k] = offg[i % len(offg)][:2]
    assert np.sum(offgrid_cases.is_off_grid_value(query)) >= 10
    for resolution in CC.RESOLUTIONS:
        mr, cr = _matcher(resolution), CC.case(resolution)
        for cells in (1, 9):
            for slot in (cr["slots"][0], cr["slots"][3]):
                got = mr.refineCandidates([slot["starts"][0]], [query], [slot["candidate"]], neighbourhood=cells)[0]
                _same(got, _sequential(mr, slot["candidate"], slot["starts"][0], query, cells), ("off-grid", resolution, cells))
                assert got["evals"] >= 2 and np.isfinite(got["score"]) and got["score"] < 0.0
    # a scan without points: NO_OVERLAP, score 0.0, the job's own pose, nothing evaluated
    r = m.refineCandidates([start, start], [np.zeros((0, 2)), g["query"]], [cand], job_candidate=[0, 0], job_scan=[0, 1])
    assert r[0]["status"] == _capi.REFINE_NO_OVERLAP and r[0]["score"] == 0.0 and r[0]["evals"] == 0
    assert np.array_equal(r[0]["pose"], start) and r[1]["steps"] >= 1
    # cells of n < 5 beside scoring ones, beams in column 0 and in the last row, at 3 x 3: the designed slot
    d = c["slots"][-1]
    for s in d["starts"]:
        got = m.refineCandidates([s], [d["query"]], [d["candidate"]], neighbourhood=9)[0]
        _same(got, _sequential(m, d["candidate"], s, d["query"], 9), "designed")
        assert got["evals"] >= 2 and got["score"] < -0.5


def test_the_ndt_in_place_is_not_touched():
    c = CC.case(0.3)
    m = _matcher(0.3)
    g = CC.graph()
    other = c["slots"][1]["candidate"]
    m.reset()
    m.addScansById([p for _, p in other], [i for i, _ in other])
    before = m.grid()
    score = m.scorePoints(g["query"], g["guess"])
    assert m.has_ndt() is True
    jobs, scans, cands, jc, js = _all_jobs(c)
    got = m.refineCandidates(jobs, scans, cands, job_candidate=jc, job_scan=js, neighbourhood=9)
    assert m.has_ndt() is True
    after = m.grid()
    assert np.array_equal(before[0], after[0], equal_nan=True) and before[1:] == after[1:]
    assert m.scorePoints(g["query"], g["guess"]) == score
    # ... and refineScans still refines against it: the call left the installed map's path alone
    here = m.refineScans([jobs[2]], [scans[0]], neighbourhood=9)[0]
    _same(here, got[2], "in place")
    # no NDT before: none after
    m.reset()
    m.refineCandidates(jobs[:2], scans, cands, job_candidate=jc[:2], job_scan=js[:2])
    assert m.has_ndt() is False


def test_refusals_name_the_offender_and_launch_nothing():
    c = CC.case(0.25)
    m = _matcher(0.25)
    g = CC.graph()
    cands = [s["candidate"] for s in c["slots"][:3]]
    jobs = np.array([c["slots"][k]["starts"][0] for k in range(3)])
    m.reset()
    m.addScansById([g["poses"][4]], [4])
    before = m.grid()
    L = _capi.lib()
    m.refineCandidates(jobs[:1], [g["query"]], cands[:1])       # (the matcher's closure object is made by its first call)
    closure = L.ndt2d_matcher_closure(m._m)
    assert closure
    L.ndt2d_closure_set_timing(C.c_void_p(closure), 1)

    def refused(what, *words, **kw):
        with pytest.raises(Ndt2dError) as ei:
            m.refineCandidates(**kw)
        assert ei.value.code == _capi.ERR_INVALID, what
        for w in words:
            assert w in str(ei.value), (what, w, str(ei.value))
        # nothing was launched: no timed chunk since timing was switched on
        a, b = C.c_float(0), C.c_float(0)
        assert L.ndt2d_closure_last_ms(C.c_void_p(closure), C.byref(a), C.byref(b)) == _capi.ERR_STATE, what

    try:
        base = dict(jobs=jobs, scans=[g["query"]], candidates=cands, job_scan=[0, 0, 0])
        refused("job_candidate", "job 1", "candidate 7 of 3", **dict(base, job_candidate=[0, 7, 2]))
        refused("job_scan", "job 2", "scan 3 of 1", **dict(base, job_scan=[0, 0, 3]))
        refused("no job_candidate", "n_candidates must equal n_jobs", **dict(base, candidates=cands[:2]))
        wide = [(0, g["poses"][0]), (1, g["poses"][1] + (500.0, 0.0, 0.0))]          # 2,039 x 39 = 79,521 cells
        refused("fused limits", "candidate 1", "fused build's limits", **dict(base, candidates=[cands[0], wide, cands[2]]))
        refused("unknown id", "candidate 2", "unknown scan id 99", **dict(base, candidates=[cands[0], cands[1], [(99, g["poses"][0])]]))
        refused("pose", "job 0", "not finite", **dict(base, jobs=np.array([[np.nan, 0, 0], jobs[1], jobs[2]])))
        refused("max_evals", "max_evals", **dict(base, max_evals=0))
        refused("tolerance", "tolerance", **dict(base, tol_lin=-1.0))
        # a refused call leaves the caller's output arrays as they were: the C entry point, a candidate
        # the closure does not take, sentinels in every output
        offsets = np.array([0, 1], dtype=np.uintp)
        ids = np.array([99], dtype=np.uintp)
        pts = np.ascontiguousarray(g["query"], dtype=np.float64)
        poff = np.array([0, len(pts)], dtype=np.uintp)
        szp = lambda a: a.ctypes.data_as(C.POINTER(C.c_size_t))      # noqa: E731
        outs = [np.full(n, -7.0) for n in (3, 1, 1, 3, 9)]
        status, evals = np.full(1, -7, dtype=np.int32), np.full(2, 7, dtype=np.uint32)
        rc = L.ndt2d_matcher_refine_candidates(
            m._m, szp(offsets), szp(ids), _capi.dptr(np.zeros(3)), 1, _capi.dptr(jobs[0].copy()), None, None, 1, _capi.dptr(pts),
            szp(poff), 1, 32, 1e-6, 1e-6, *[_capi.dptr(o) for o in outs], status.ctypes.data_as(C.POINTER(C.c_int32)),
            evals.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert rc == _capi.ERR_INVALID and all(np.all(o == -7.0) for o in outs) and status[0] == -7 and np.all(evals == 7)
        # the NDT in place is what it was, and a good call behind the refusals is timed and right
        after = m.grid()
        assert m.has_ndt() is True and np.array_equal(before[0], after[0], equal_nan=True)
        got = m.refineCandidates(**base)
        a, b = C.c_float(0), C.c_float(0)
        assert L.ndt2d_closure_last_ms(C.c_void_p(closure), C.byref(a), C.byref(b)) == _capi.OK and a.value > 0 and b.value > 0
        print("three jobs on three candidates: build %.1f us, refinement %.1f us" % (1e3 * a.value, 1e3 * b.value))
        for k in range(3):
            _same(got[k], _sequential(m, cands[k], jobs[k], g["query"], 1), ("after the refusals", k))
    finally:
        L.ndt2d_closure_set_timing(C.c_void_p(closure), 0)


def test_close_loops_with_refinement_is_the_composed_walk():
    """close_loops(refine=dict(neighbourhood=9)) on tests/test_gpu_closure.py's walk equals the walk
    composed from matchCandidates plus the sequential refinement of the accepted candidate, bit for
    bit; every accepted entry's refined pose scores no higher under the 3 x 3 objective than its start."""
    m = _matcher(0.25)
    g = CC.graph()
    rolling, limit = 8, 4
    guess, pts = g["guess"], g["query"]
    window = lambda i: [(j, g["poses"][j]) for j in loop_closure_window(i, rolling)]      # noqa: E731
    cand_idx = [2, 4, 6, 8]
    first = [r["score"] for r in m.matchCandidates(guess, pts, [window(i) for i in cand_idx])]
    worst = int(np.argmax(first))
    order = [worst] + [k for k in range(len(cand_idx)) if k != worst]
    cand_idx = [cand_idx[k] for k in order]
    first = [first[k] for k in order]
    assert first[1] < first[0]
    typical = 0.5 * (first[0] + first[1])

    pose, todo, want = guess.copy(), list(cand_idx), []
    while todo:
        results = m.matchCandidates(pose, pts, [window(i) for i in todo])
        rest = []
        for k, (i, res) in enumerate(zip(todo, results)):
            if np.isfinite(res["score"]) and res["score"] < typical:
                lattice = res["pose"] + pose
                r = _sequential(m, window(i), lattice, pts, 9)
                ok = r["status"] in (_capi.REFINE_CONVERGED, _capi.REFINE_MAX_EVALS) and r["score"] <= r["start_score"]
                want.append((i, res["score"], lattice.copy(), r))
                pose = r["pose"].copy() if ok else lattice
                rest = todo[k + 1:]
                break
        todo = rest
    assert want and want[0][0] == cand_idx[1]

    got_pose, accepted = close_loops(m, guess, pts, cand_idx, g["poses"], rolling, typical, limit,
                                     scan_sizes=[len(p) for p in g["points"]], refine=dict(neighbourhood=9))
    assert [a["candidate"] for a in accepted] == [w[0] for w in want]
    for a, (i, score, lattice, r) in zip(accepted, want):
        assert a["score"] == score and np.array_equal(a["pose"], lattice)
        assert np.array_equal(a["refined_pose"], r["pose"]) and a["refine_status"] == r["status"]
        assert (a["refined_covariance"] is None) == (r["covariance"] is None)
        if r["covariance"] is not None:
            assert np.array_equal(a["refined_covariance"], r["covariance"])
        # the objective at the refined pose against the objective at the start
        at = m.refineCandidates([a["refined_pose"], lattice], [pts], [window(i)], job_candidate=[0, 0], job_scan=[0, 0],
                                max_evals=1, neighbourhood=9)
        print("candidate %d: f/N %.9f at the lattice pose, %.9f refined (status %d)" % (i, at[1]["start_score"], at[0]["start_score"],
                                                                                  a["refine_status"]))
        assert at[0]["start_score"] <= at[1]["start_score"]
    assert np.array_equal(got_pose, pose)
    # without refine: the same accepts' lattice results as tests/test_gpu_closure.py checks, no refined entries
    plain_pose, plain = close_loops(m, guess, pts, cand_idx, g["poses"], rolling, typical, limit)
    assert all("refined_pose" not in a for a in plain) and plain[0]["candidate"] == accepted[0]["candidate"]
    assert np.array_equal(plain[0]["pose"], accepted[0]["pose"])
