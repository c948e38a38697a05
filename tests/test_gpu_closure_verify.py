"""Match verification on each loop-closure candidate's own map (ScanMatcherNDT.verifyCandidates,
ndt2d_closure_verify, csrc/closure/): the candidates' maps are built in the closure's slots and the
verification's kernel runs on them, a block per job, in one launch.

The yardstick is the sequential path on the same matcher -- reset(), addScansById(candidate),
verifyScans([job], [scan]) -- bit for bit, with no tolerance: the closure build makes the fused
build's grid and the kernel has one text for both map sources.  The CPU restatement
(tests/verify_restatement.py) over the oracle's build of each candidate pins the classes, the
pierce flags and the cells exactly and m2 to 1e-9 relative (DESIGN.md 3.15's bound).  Cases:
tests/closure_verify_cases.py over tests/closure_refine_cases.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import closure_refine_cases as CC
import closure_verify_cases as VC
import offgrid_cases
import refine_restatement as R
import verify_restatement as V
from ndt_2d_amd import Ndt2dError, ScanMatcherNDT, _capi, close_loops, loop_closure_window

pytestmark = pytest.mark.gpu

COUNTS = ("n_beams", "off", "unseen", "outlier", "inlier", "pierced", "walked")
BEAM_KEYS = ("classes", "m2", "cells", "pierced_mask")
_MATCHERS = {}
_GOT = {}


def _matcher(resolution):
    """A matcher with the graph's ten scans stored under their indices and the designed scan of
    this resolution behind them; one per resolution for the module."""
    if resolution not in _MATCHERS:
        c = CC.case(resolution)
        m = ScanMatcherNDT(0)
        m.initialize("closure_verify", **c["params"])
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
    _GOT.clear()


def _sequential(m, cand, job, scan, cells, **kw):
    m.reset()
    m.addScansById([p for _, p in cand], [i for i, _ in cand])
    return m.verifyScans([job], [scan], neighbourhood=cells, want_beams=True, **kw)[0]


def _same(got, want, where=None):
    for key in COUNTS:
        assert got[key] == want[key], (where, key, got[key], want[key])
    for key in BEAM_KEYS:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key], equal_nan=True), (where, key)


def _all_at_once(resolution, cells, rays=True):
    """The 30 jobs of the cases in ONE verifyCandidates call, on a matcher without an NDT; once per
    (resolution, neighbourhood, rays) for the module."""
    key = (resolution, cells, rays)
    if key not in _GOT:
        m = _matcher(resolution)
        jobs, scans, cands, jc, js = VC.jobs(resolution)
        m.reset()
        _GOT[key] = m.verifyCandidates(jobs, scans, cands, job_candidate=jc, job_scan=js, neighbourhood=cells, rays=rays,
                                       want_beams=True)
        assert m.has_ndt() is False
    return _GOT[key]


@pytest.mark.parametrize("cells,rays", [(1, True), (9, True), (9, False)])
@pytest.mark.parametrize("resolution", CC.RESOLUTIONS)
def test_the_bits_of_the_sequential_path(resolution, cells, rays):
    """The main test: reset(); addScansById(c); verifyScans([job], [scan]) per job, and the 30 jobs
    -- six slots of four grid sizes and both parities of ncell, five poses each -- in ONE
    verifyCandidates call: records, class bytes, m2 and both cell columns array_equal.  No
    tolerance.  (Rays off once per resolution, with nine cells.)"""
    m = _matcher(resolution)
    jobs, scans, cands, jc, js = VC.jobs(resolution)
    got = _all_at_once(resolution, cells, rays)
    want = [_sequential(m, cands[k], job, scans[s], cells, rays=rays) for job, k, s in zip(jobs, jc, js)]
    m.reset()
    assert len(got) == len(want) == 30
    for k, (g, w) in enumerate(zip(got, want)):
        _same(g, w, (resolution, cells, rays, k))
    # the jobs did run: every class, pierced beams with rays on, nothing walked with rays off
    total = {key: sum(g[key] for g in got) for key in COUNTS}
    print("res %.2f cells %d rays %s: %s" % (resolution, cells, rays, total))
    assert total["n_beams"] == 30 * CC.BEAMS and all(total[key] > 0 for key in ("off", "unseen", "outlier", "inlier"))
    assert (total["pierced"] > 0 and total["walked"] > 0) if rays else (total["pierced"] == 0 and total["walked"] == 0)


@pytest.mark.parametrize("cells", VC.NEIGHBOURHOODS)
@pytest.mark.parametrize("resolution", CC.RESOLUTIONS)
def test_against_the_restatement(resolution, cells):
    """Over the ORACLE's build of each candidate: records, classes, pierce flags and both cell
    columns equal exactly, m2 within 1e-9 relative.  No value of the restatement lies within 1e-8
    of a gate (asserted first), so no last-bit difference can change a class or a flag."""
    want = VC.restated(resolution, cells)
    for k, w in enumerate(want):
        assert V.near_gate(w, VC.GATE_INLIER, VC.GATE_PIERCE, rel=1e-8) == [] and not np.isnan(w["m2"]).any(), k
    got = _all_at_once(resolution, cells)
    worst = 0.0
    for k, (g, w) in enumerate(zip(got, want)):
        where = (resolution, cells, k)
        assert [g[key] for key in COUNTS] == [int(v) for v in w["record"][:7]], where
        assert np.array_equal(g["classes"], w["classes"]) and np.array_equal(g["pierced_mask"], w["pierced_mask"]), where
        assert np.array_equal(g["cells"], w["cells"]), where
        finite = np.isfinite(w["m2"])
        assert np.array_equal(np.isinf(g["m2"]), ~finite), where
        rel = np.abs(g["m2"][finite] - w["m2"][finite]) / np.maximum(np.abs(w["m2"][finite]), np.finfo(float).tiny)
        if rel.size:
            worst = max(worst, float(rel.max()))
            assert np.all(rel <= 1e-9), (where, float(rel.max()))
    print("res %.2f cells %d: largest relative m2 deviation %.3e" % (resolution, cells, worst))


def _closure_verify(m, c, cands, jobs, beams, job_scan, job_candidate, slots, cells, rays=True, want=(True, True, True),
                    sentinel=None):
    """ndt2d_closure_verify on a store and a closure object of their own (`slots` slots) on the
    matcher's context; beams: the scans as they travel.  want: which of (class, m2, cells) are
    asked for.  Returns (rc, message, records, classes, m2, cells); an output not asked for is None."""
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
            # ndt2d_verify's defaults, rules and refusals
            n, gi, gp, ry = C.c_uint32(0), C.c_double(0), C.c_double(0), C.c_int(-1)
            assert L.ndt2d_closure_verify_neighbourhood(closure, C.byref(n)) == _capi.OK and n.value == 1
            assert L.ndt2d_closure_verify_gates(closure, C.byref(gi), C.byref(gp)) == _capi.OK and (gi.value, gp.value) == (9.0, 1.0)
            assert L.ndt2d_closure_verify_rays(closure, C.byref(ry)) == _capi.OK and ry.value == 1
            assert L.ndt2d_closure_set_verify_neighbourhood(closure, 5) == _capi.ERR_INVALID
            assert b"5 cells" in L.ndt2d_closure_last_error(closure)
            assert L.ndt2d_closure_set_verify_gates(closure, -1.0, 1.0) == _capi.ERR_INVALID
            assert L.ndt2d_closure_set_verify_gates(closure, 9.0, float("inf")) == _capi.ERR_INVALID
            assert L.ndt2d_closure_set_verify_rays(closure, 2) == _capi.ERR_INVALID
            assert L.ndt2d_closure_verify_neighbourhood(closure, C.byref(n)) == _capi.OK and n.value == 1       # the old values stay
            assert L.ndt2d_closure_verify_gates(closure, C.byref(gi), C.byref(gp)) == _capi.OK and (gi.value, gp.value) == (9.0, 1.0)
            assert L.ndt2d_closure_set_verify_neighbourhood(closure, cells) == _capi.OK
            assert L.ndt2d_closure_set_verify_gates(closure, VC.GATE_INLIER, VC.GATE_PIERCE) == _capi.OK
            assert L.ndt2d_closure_set_verify_rays(closure, 1 if rays else 0) == _capi.OK
            # (apart from the refinement's neighbourhood)
            assert L.ndt2d_closure_neighbourhood(closure, C.byref(n)) == _capi.OK and n.value == 1
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
            total = int(sum(len(beams[s]) for s in job_scan if s < len(beams)))
            fill = 0 if sentinel is None else sentinel
            records = np.full((len(jp), 8), fill, dtype=np.uint32)
            classes = np.full(total, fill, dtype=np.uint8) if want[0] else None
            m2 = np.full(total, float(fill)) if want[1] else None
            cells_out = np.full((total, 2), fill, dtype=np.uint32) if want[2] else None
            p = c["params"]
            rc = L.ndt2d_closure_verify(closure, len(cands), szp(offsets), szp(ids), _capi.dptr(poses), p["ndt_resolution"],
                                        p["range_max"], _capi.dptr(jp), u32p(js), u32p(jc), len(jp), _capi.dptr(flat), szp(boff),
                                        len(beams), u32p(records), classes.ctypes.data_as(C.POINTER(C.c_uint8)) if want[0] else None,
                                        _capi.dptr(m2) if want[1] else None, u32p(cells_out) if want[2] else None)
            return rc, L.ndt2d_closure_last_error(closure).decode(), records, classes, m2, cells_out
        finally:
            L.ndt2d_closure_destroy(closure)
    finally:
        L.ndt2d_scanstore_destroy(store)


def test_a_job_depends_on_nothing_but_itself():
    """The same bits from a job alone, all together, twice and in shuffled order; with one candidate
    named by several jobs and a candidate no job names; five candidates through a 2-slot closure
    object against an 8-slot one (C-ABI); 17 candidates through the matcher's 16 slots."""
    resolution = 0.25
    c = CC.case(resolution)
    m = _matcher(resolution)
    g = CC.graph()
    jobs, scans, cands, jc, js = VC.jobs(resolution)
    for cells in VC.NEIGHBOURHOODS:
        together = _all_at_once(resolution, cells)
        again = m.verifyCandidates(jobs, scans, cands, job_candidate=jc, job_scan=js, neighbourhood=cells, want_beams=True)
        order = np.random.default_rng(99).permutation(len(jobs))
        shuffled = m.verifyCandidates(jobs[order], scans, cands, job_candidate=[jc[k] for k in order], job_scan=[js[k] for k in order],
                                      neighbourhood=cells, want_beams=True)
        for k in range(len(jobs)):
            _same(again[k], together[k], ("again", cells, k))
            _same(shuffled[int(np.flatnonzero(order == k)[0])], together[k], ("shuffled", cells, k))
        for k in (0, 2, 7, 13, 19, 24, 27, 29):          # every slot, every kind of pose
            alone = m.verifyCandidates([jobs[k]], [scans[js[k]]], [cands[jc[k]]], neighbourhood=cells, want_beams=True)[0]
            _same(alone, together[k], ("alone", cells, k))
        # candidate 1 named by three jobs, candidates 0 and 3 by none (they are not built), scans in another order
        some = [7, 12, 5, 9, 14]
        part = m.verifyCandidates(jobs[some], scans[::-1], cands, job_candidate=[jc[k] for k in some],
                                  job_scan=[1 - js[k] for k in some], neighbourhood=cells, want_beams=True)
        for k, r in zip(some, part):
            _same(r, together[k], ("some", cells, k))
    # 2 slots with 5 candidates (chunks of 2, 2 and 1) against 8 slots; the jobs name the candidates out of order
    cands5 = cands[:5]
    beams = [c["slots"][0]["beams"], R.subsample(g["points"][7], 63)]
    pick = [(4, 0), (0, 2), (3, 3), (1, 0), (2, 4), (0, 0), (4, 2), (2, 1)]
    jobs8 = np.array([VC.poses_of(c["slots"][k])[i] for k, i in pick])
    jc8, js8 = [k for k, _ in pick], [0, 1, 0, 0, 1, 0, 0, 0]
    for cells in VC.NEIGHBOURHOODS:
        two = _closure_verify(m, c, cands5, jobs8, beams, js8, jc8, 2, cells)
        eight = _closure_verify(m, c, cands5, jobs8, beams, js8, jc8, 8, cells)
        assert two[0] == eight[0] == _capi.OK, (two[1], eight[1])
        for a, b in zip(two[2:], eight[2:]):
            assert np.array_equal(a, b, equal_nan=True)
        assert np.all(two[2][:, 0] == [len(beams[s]) for s in js8]) and np.all(two[2][:, 6] > 0)
        # ... and they are the records behind the matcher's results (the jobs of scan 0)
        together = _all_at_once(resolution, cells)
        for b, (k, i) in enumerate(pick):
            if js8[b] == 0:
                assert [together[5 * k + i][key] for key in COUNTS] == [int(v) for v in two[2][b, :7]], (cells, b)
    # 17 candidates through the matcher's 16 slots
    cands17 = [[(i, g["poses"][i])] for i in range(10)] + [[(i, g["poses"][i]), (i + 1, g["poses"][i + 1])] for i in range(7)]
    jobs17 = np.array([g["guess"] + (0.05 * k, -0.03 * k, 0.02 * k) for k in range(17)])
    got = m.verifyCandidates(jobs17, [g["query"]], cands17, job_scan=[0] * 17, neighbourhood=9, want_beams=True)
    for k in range(17):
        _same(m.verifyCandidates([jobs17[k]], [g["query"]], [cands17[k]], neighbourhood=9, want_beams=True)[0], got[k], ("17", k))
    assert sum(r["pierced"] for r in got) > 0 and sum(r["inlier"] for r in got) > 0


def test_edges():
    c = CC.case(0.25)
    m = _matcher(0.25)
    g = CC.graph()
    slot = c["slots"][0]
    cand, start = slot["candidate"], slot["starts"][0]
    # scans of 1, 63, 64, 65, 256 and 257 beams: under, at and over a wave and a workgroup
    lengths = (1, 63, 64, 65, 256, 257)
    scans = [np.ascontiguousarray(g["query"][:n]) for n in lengths]
    for cells in VC.NEIGHBOURHOODS:
        got = m.verifyCandidates([start + (1.0, 0.0, 0.0)] * len(lengths), scans, [cand], job_candidate=[0] * len(lengths),
                                 max_beams=0, neighbourhood=cells, want_beams=True)
        for n, r, sc in zip(lengths, got, scans):
            assert r["n_beams"] == n == len(r["classes"]) == len(r["m2"]) == len(r["cells"])
            _same(r, _sequential(m, cand, start + (1.0, 0.0, 0.0), sc, cells, max_beams=0), ("length", cells, n))
            w = V.verify(slot["grid"], sc, start + (1.0, 0.0, 0.0), neighbourhood=cells)
            assert [r[key] for key in COUNTS] == [int(v) for v in w["record"][:7]] and np.array_equal(r["cells"], w["cells"])
        assert sum(r["pierced"] for r in got) > 0
    # NaN / +-inf / 1e300 / 2^32-cell beams at the off-grid tests' positions: OFF, no ray, and no other beam changes
    query = R.subsample(g["query"], CC.BEAMS)
    offg = offgrid_cases.off_grid_points(0.25, CC.RANGE_MAX)
    for i, k in enumerate(offgrid_cases.slots(len(query))):
        query[k] = offg[i % len(offg)][:2]
    bad = offgrid_cases.is_off_grid_value(query)
    assert np.sum(bad) >= 10 and np.sum(~np.isfinite(query).all(axis=1)) >= 5
    for resolution in CC.RESOLUTIONS:
        mr, cr = _matcher(resolution), CC.case(resolution)
        for cells in VC.NEIGHBOURHOODS:
            for k in (0, 3):
                s = cr["slots"][k]
                got = mr.verifyCandidates([s["starts"][0]], [query], [s["candidate"]], neighbourhood=cells, want_beams=True)[0]
                _same(got, _sequential(mr, s["candidate"], s["starts"][0], query, cells), ("off-grid", resolution, cells, k))
                assert np.all(got["classes"][bad] == _capi.BEAM_OFF) and not got["pierced_mask"][bad].any()
                assert np.all(np.isinf(got["m2"][bad])) and np.all(got["cells"][bad] == _capi.VERIFY_NO_CELL)
                clean = _all_at_once(resolution, cells)[5 * k]
                assert np.array_equal(got["classes"][~bad], clean["classes"][~bad])
                assert np.array_equal(got["m2"][~bad], clean["m2"][~bad])
                assert got["walked"] == int(np.sum(got["classes"] != _capi.BEAM_OFF)) < CC.BEAMS - int(np.sum(bad)) + 1
    # the robot stands off its slot's grid, some of its beams end on it: nothing is walked, the classes still come out
    away = start + (5.5, 0.0, 0.0)
    for cells in VC.NEIGHBOURHOODS:
        r = m.verifyCandidates([away], [g["query"]], [cand], neighbourhood=cells, want_beams=True)[0]
        w = V.verify(slot["grid"], slot["beams"], away, neighbourhood=cells)
        assert int(slot["grid"].index(np.array([away[0]]), np.array([away[1]]))[0]) < 0
        assert r["walked"] == 0 and r["pierced"] == 0 and 0 < r["off"] < CC.BEAMS and r["inlier"] + r["outlier"] > 0
        assert np.array_equal(r["classes"], w["classes"]) and np.array_equal(r["cells"], w["cells"])
        _same(r, _sequential(m, cand, away, g["query"], cells), ("robot off the grid", cells))
    # a job of a scan without points: zeros, no room in the per-beam arrays; the other job is what it is alone
    r = m.verifyCandidates([start, start], [np.zeros((0, 2)), g["query"]], [cand], job_candidate=[0, 0], job_scan=[0, 1],
                           want_beams=True)
    assert all(r[0][key] == 0 for key in COUNTS) and len(r[0]["classes"]) == 0 and len(r[0]["m2"]) == 0
    _same(r[1], _all_at_once(0.25, 9)[0], "beside an empty scan")
    only = m.verifyCandidates([start], [np.zeros((0, 2))], [cand], want_beams=True)
    assert all(only[0][key] == 0 for key in COUNTS)
    # max_beams: 0 takes every point, n the subsampling rule of scorePoints
    every = m.verifyCandidates([start], [g["query"]], [cand], max_beams=0, want_beams=True)[0]
    assert every["n_beams"] == len(g["query"]) == 720
    _same(every, _sequential(m, cand, start, g["query"], 9, max_beams=0), "max_beams 0")
    fifty = m.verifyCandidates([start], [g["query"]], [cand], max_beams=50, want_beams=True)[0]
    _same(fifty, m.verifyCandidates([start], [R.subsample(g["query"], 50)], [cand], max_beams=0, want_beams=True)[0], "max_beams 50")
    assert fifty["n_beams"] == 50
    # the per-beam outputs NULL in every combination (C-ABI): the others and the records are what they are with all three
    jobs = np.array([VC.poses_of(slot)[i] for i in (2, 0, 3)])
    beams = [slot["beams"], R.subsample(g["points"][7], 65)]
    full = _closure_verify(m, c, [cand], jobs, beams, [0, 1, 0], [0, 0, 0], 4, 9)
    assert full[0] == _capi.OK and full[2][:, 5].sum() > 0
    for want in itertools.product((False, True), repeat=3):
        part = _closure_verify(m, c, [cand], jobs, beams, [0, 1, 0], [0, 0, 0], 4, 9, want=want)
        assert part[0] == _capi.OK and np.array_equal(part[2], full[2]), want
        for asked, a, b in zip(want, part[3:], full[3:]):
            assert (a is None) if not asked else np.array_equal(a, b), want


def test_the_ndt_in_place_is_not_touched():
    c = CC.case(0.3)
    m = _matcher(0.3)
    g = CC.graph()
    other = c["slots"][1]["candidate"]
    jobs, scans, cands, jc, js = VC.jobs(0.3)
    m.reset()
    m.addScansById([p for _, p in other], [i for i, _ in other])
    before = m.grid()
    here = m.verifyScans(jobs[5:10], [scans[0]], job_scan=[0] * 5, want_beams=True)
    score = m.scorePoints(g["query"], g["guess"])
    assert m.has_ndt() is True
    got = m.verifyCandidates(jobs, scans, cands, job_candidate=jc, job_scan=js, want_beams=True)
    assert m.has_ndt() is True
    after = m.grid()
    assert np.array_equal(before[0], after[0], equal_nan=True) and before[1:] == after[1:]
    assert m.scorePoints(g["query"], g["guess"]) == score
    # verifyScans still answers against the map in place -- and that map is candidate 1's, so it agrees with the slots
    for k, (a, b) in enumerate(zip(m.verifyScans(jobs[5:10], [scans[0]], job_scan=[0] * 5, want_beams=True), here)):
        _same(a, b, ("in place", k))
        _same(a, got[5 + k], ("in place against the slot", k))
    # none in place: the call works (no NDT2D_ERR_NO_GRID) and leaves none
    m.reset()
    with pytest.raises(Ndt2dError) as ei:
        m.verifyScans(jobs[:1], [scans[0]])
    assert ei.value.code == _capi.ERR_NO_GRID
    none = m.verifyCandidates(jobs[:2], scans, cands, job_candidate=jc[:2], job_scan=js[:2], want_beams=True)
    assert m.has_ndt() is False
    for k in range(2):
        _same(none[k], got[k], ("none in place", k))


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
    m.verifyCandidates(jobs[:1], [g["query"]], cands[:1])       # (the matcher's closure object is made by its first call)
    closure = L.ndt2d_matcher_closure(m._m)
    assert closure
    L.ndt2d_closure_set_timing(C.c_void_p(closure), 1)

    def nothing_launched(what):
        # no timed chunk since timing was switched on
        a, b = C.c_float(0), C.c_float(0)
        assert L.ndt2d_closure_last_ms(C.c_void_p(closure), C.byref(a), C.byref(b)) == _capi.ERR_STATE, what

    def refused(what, *words, **kw):
        with pytest.raises(Ndt2dError) as ei:
            m.verifyCandidates(**kw)
        assert ei.value.code == _capi.ERR_INVALID, what
        for w in words:
            assert w in str(ei.value), (what, w, str(ei.value))
        nothing_launched(what)

    try:
        base = dict(jobs=jobs, scans=[g["query"]], candidates=cands, job_scan=[0, 0, 0])
        refused("job_candidate", "job 1", "candidate 7 of 3", **dict(base, job_candidate=[0, 7, 2]))
        refused("job_scan", "job 2", "scan 3 of 1", **dict(base, job_scan=[0, 0, 3]))
        refused("no job_candidate", "n_candidates must equal n_jobs", **dict(base, candidates=cands[:2]))
        wide = [(0, g["poses"][0]), (1, g["poses"][1] + (500.0, 0.0, 0.0))]          # 2,039 x 39 = 79,521 cells
        refused("fused limits", "candidate 1", "fused build's limits", **dict(base, candidates=[cands[0], wide, cands[2]]))
        refused("unknown id", "candidate 2", "unknown scan id 99", **dict(base, candidates=[cands[0], cands[1], [(99, g["poses"][0])]]))
        refused("no scans", "candidate 0", "has no scans", **dict(base, candidates=[[], cands[1], cands[2]]))
        refused("pose", "job 0", "not finite", **dict(base, jobs=np.array([[np.nan, 0, 0], jobs[1], jobs[2]])))
        refused("scan pose", "candidate 1", "not finite", **dict(base, candidates=[cands[0], [(4, (np.inf, 0.0, 0.0))], cands[2]]))
        for bad, word in ((dict(neighbourhood=5), "5 cells"), (dict(gate_inlier=-1.0), "gate"), (dict(gate_pierce=float("nan")), "gate")):
            refused("parameter", word, **dict(base, **bad))
        assert m.verify_parameters() == dict(neighbourhood=9, gate_inlier=9.0, gate_pierce=1.0, rays=True)
        # a refused call leaves the caller's output arrays as they were: the matcher's C entry point with a candidate
        # the closure does not take, and with per-beam arrays that are too small; sentinels in every output
        offsets = np.array([0, 1], dtype=np.uintp)
        pts = np.ascontiguousarray(g["query"], dtype=np.float64)
        poff = np.array([0, len(pts)], dtype=np.uintp)
        szp = lambda a: a.ctypes.data_as(C.POINTER(C.c_size_t))      # noqa: E731
        u32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))     # noqa: E731
        for ids, cap, word in ((np.array([99], dtype=np.uintp), CC.BEAMS, "unknown scan id 99"),
                               (np.array([4], dtype=np.uintp), CC.BEAMS - 1, "the jobs have 100")):
            records, table = np.full(8, 7, dtype=np.uint32), np.full(2, 7, dtype=np.uintp)
            classes, m2, cells = np.full(CC.BEAMS, 7, dtype=np.uint8), np.full(CC.BEAMS, -7.0), np.full((CC.BEAMS, 2), 7, dtype=np.uint32)
            rc = L.ndt2d_matcher_verify_candidates(
                m._m, szp(offsets), szp(ids), _capi.dptr(np.zeros(3)), 1, _capi.dptr(jobs[0].copy()), None, None, 1, _capi.dptr(pts),
                szp(poff), 1, CC.BEAMS, u32p(records), szp(table), classes.ctypes.data_as(C.POINTER(C.c_uint8)), _capi.dptr(m2),
                u32p(cells), cap)
            assert rc == _capi.ERR_INVALID and word in L.ndt2d_matcher_last_error(m._m).decode()
            assert np.all(records == 7) and np.all(table == 7) and np.all(classes == 7) and np.all(m2 == -7.0) and np.all(cells == 7)
            nothing_launched(word)
        # ... and the closure's own entry point: a job_candidate out of range, sentinels in every output
        rc, msg, records, classes, m2, cells = _closure_verify(m, c, cands, jobs, [c["slots"][0]["beams"]], [0, 0, 0], [0, 3, 1], 4, 9,
                                                               sentinel=7)
        assert rc == _capi.ERR_INVALID and "job 1" in msg and "candidate 3 of 3" in msg
        assert np.all(records == 7) and np.all(classes == 7) and np.all(m2 == 7.0) and np.all(cells == 7)
        rc, msg, records, _, _, _ = _closure_verify(m, c, cands, jobs, [c["slots"][0]["beams"]], [0, 1, 0], [0, 1, 2], 4, 9, sentinel=7)
        assert rc == _capi.ERR_INVALID and "job 1" in msg and "scan 1 of 1" in msg and np.all(records == 7)
        # the NDT in place is what it was, and a good call behind the refusals is timed and right
        after = m.grid()
        assert m.has_ndt() is True and np.array_equal(before[0], after[0], equal_nan=True)
        got = m.verifyCandidates(want_beams=True, **base)
        a, b = C.c_float(0), C.c_float(0)
        assert L.ndt2d_closure_last_ms(C.c_void_p(closure), C.byref(a), C.byref(b)) == _capi.OK and a.value > 0 and b.value > 0
        print("three jobs on three candidates: build %.1f us, verification %.1f us" % (1e3 * a.value, 1e3 * b.value))
        for k in range(3):
            _same(got[k], _sequential(m, cands[k], jobs[k], g["query"], 9), ("after the refusals", k))
    finally:
        L.ndt2d_closure_set_timing(C.c_void_p(closure), 0)


@pytest.mark.parametrize("refine", [None, dict(neighbourhood=9)])
def test_close_loops_with_verification_is_the_composed_walk(refine):
    """close_loops(verify=dict(...)) on tests/test_gpu_closure.py's walk: the pose and the accepted
    entries are those of the call without `verify`, every entry's `verify` is what a direct
    verifyCandidates gives on the candidate's own map at `verified_pose`, and that pose is the one
    the walk adopted -- with and without the refinement."""
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
    sizes = [len(p) for p in g["points"]]
    rules = dict(gate_pierce=1.0, neighbourhood=9)
    m.reset()
    plain_pose, plain = close_loops(m, guess, pts, cand_idx, g["poses"], rolling, typical, limit, scan_sizes=sizes, refine=refine)
    pose, accepted = close_loops(m, guess, pts, cand_idx, g["poses"], rolling, typical, limit, scan_sizes=sizes, refine=refine,
                                 verify=rules)
    assert m.has_ndt() is False and plain and plain[0]["candidate"] == cand_idx[1]
    assert np.array_equal(pose, plain_pose) and len(accepted) == len(plain)
    at = guess.copy()
    for a, p in zip(accepted, plain):
        assert np.array_equal(a["correction"] + at, a["pose"])          # the round started from the pose adopted before
        assert sorted(a) == sorted(list(p) + ["verify", "verified_pose"])
        for key in p:
            assert (a[key] is None and p[key] is None) or np.array_equal(a[key], p[key]), key
        direct = m.verifyCandidates([a["verified_pose"]], [pts], [window(a["candidate"])], **rules)[0]
        assert a["verify"] == direct and direct["n_beams"] == CC.BEAMS
        print("candidate %d (refine %s): %s" % (a["candidate"], refine is not None, direct))
        # the pose the walk adopted: what the next round started from
        ended = refine is not None and a["refine_status"] in (_capi.REFINE_CONVERGED, _capi.REFINE_MAX_EVALS)
        assert np.array_equal(a["verified_pose"], a["pose"]) or (ended and np.array_equal(a["verified_pose"], a["refined_pose"]))
        at = a["verified_pose"]
    assert np.array_equal(at, pose)
    if refine is not None:
        assert any(np.array_equal(a["verified_pose"], a["refined_pose"]) for a in accepted)     # (the refined pose was adopted somewhere)
