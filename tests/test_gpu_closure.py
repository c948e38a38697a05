"""Batched loop-closure match (ScanMatcherNDT.matchCandidates, csrc/closure/): one scan against K
candidate maps in one build launch, one search launch and one read-back.

The yardstick of every test is the sequential path on the same matcher -- reset(),
addScansById(candidate), matchScan(scan) -- and, for the parity test, the CPU oracle.  Raw scores
are compared bit for bit where the sequential path runs the small-lattice search (every lattice
here but those said otherwise): a lane of the batched search keeps that search's partial sums."""
import time

import numpy as np
import pytest

import offgrid_cases
import oracle_lib as O
from ndt_2d_amd import Ndt2dError, ScanMatcherNDT, _capi, close_loops, loop_closure_window, synth

pytestmark = pytest.mark.gpu

WORLD = (4.0, 4.0, 0.25)      # the room of synth cfg-1
RANGE_MAX = 4.75
NO_INDEX = 2 ** 64 - 1
TOL_TIGHT = 1e-9              # tests/test_gpu_parity.py: regression bound on raw scores and the score
# 5 theta steps x 7 x 7 translations
SMALL = dict(search_angular_size=0.045, search_angular_resolution=0.02,
             search_linear_size=0.065, search_linear_resolution=0.02, laser_max_beams=100)
N_POINTS = (720, 360, 90, 181, 720, 97, 512, 720, 333, 720)


@pytest.fixture(scope="module")
def graph():
    """Ten scans along a path through the room, 90 to 720 points, and the scan to close loops for."""
    w = synth.world_of(WORLD)
    poses, points = [], []
    for i, n in enumerate(N_POINTS):
        pose = (-0.9 + 0.2 * i, 0.35 - 0.08 * i + (0.11 if i % 2 else 0.0), 0.05 * i - 0.2)
        assert not synth.pose_blocked(w, pose[0], pose[1])
        poses.append(pose)
        points.append(synth.scan(w, pose, 7000 + i, n_beams=n))
    true_pose = (0.13, -0.07, 0.031)
    query = synth.scan(w, true_pose, 7100)
    return dict(world=w, poses=np.array(poses), points=points, query=query, guess=np.array([0.1, -0.05, 0.02]))


def _matcher(graph, extra=(), **params):
    p = dict(ndt_resolution=0.25, range_max=RANGE_MAX)
    p.update(params)
    m = ScanMatcherNDT(0)
    m.initialize("closure", **p)
    for i, pts in enumerate(graph["points"]):
        assert m.storeScan(pts) == i
    for pts in extra:
        m.storeScan(pts)
    return m


def _candidate(graph, ids):
    return [(i, graph["poses"][i]) for i in ids]


def _sequential(m, scan_pose, points, cand, want_scores=True, pose=None):
    m.reset()
    m.addScansById([p for _, p in cand], [i for i, _ in cand])
    return m.matchScan(scan_pose, points, pose=pose, want_scores=want_scores)


def _oracle(graph, params, scan_pose, points, cand):
    ref = O.ScanMatcherNDT()
    ref.initialize(**params)
    ref.addScans([(pose, graph["points"][i]) for i, pose in cand])
    return ref.matchScan(scan_pose, points, want_scores=True)


def _same_as_sequential(got, exp, exact_scores=True):
    assert got["n_candidates"] == exp["n_candidates"]
    assert got["best_index"] == exp["best_index"]
    assert np.array_equal(got["pose"], exp["pose"])
    if exact_scores:
        assert got["score"] == exp["score"] or (np.isnan(got["score"]) and np.isnan(exp["score"]))
        if got.get("scores") is not None and exp.get("scores") is not None:
            assert np.array_equal(got["scores"], exp["scores"], equal_nan=True)
    # the reduction order differs: the bound _check_match (tests/test_gpu_parity.py) uses
    assert np.allclose(got["covariance"], exp["covariance"], rtol=1e-9, atol=0, equal_nan=True)


@pytest.mark.parametrize("resolution", [0.25, 0.3])
def test_parity_with_the_sequential_path_and_the_oracle(graph, resolution):
    params = dict(SMALL, ndt_resolution=resolution, range_max=RANGE_MAX)
    m = _matcher(graph, **dict(SMALL, ndt_resolution=resolution))
    cands = [_candidate(graph, [4]), _candidate(graph, [5, 6]), _candidate(graph, [1, 2])]
    seq = [_sequential(m, graph["guess"], graph["query"], c) for c in cands]
    assert all(s["n_candidates"] == 5 * 7 * 7 for s in seq)
    assert m.last_variant().startswith("match/lane-per-candidate/small-lattice/" + ("pow2" if resolution == 0.25 else "div"))
    # no near tie for any candidate: the index comparison against the oracle means something
    assert m.adjudication_stats()[0] == 0
    got = m.matchCandidates(graph["guess"], graph["query"], cands, want_scores=True)
    assert m.adjudication_stats()[0] == 0 and m.has_ndt() == 0
    assert len(got) == 3
    for g, s, c in zip(got, seq, cands):
        assert np.array_equal(g["scores"], s["scores"])
        assert g["best_index"] == s["best_index"] and g["best_index"] != NO_INDEX
        assert np.array_equal(g["pose"], s["pose"])
        assert g["score"] == s["score"]
        assert np.allclose(g["covariance"], s["covariance"], rtol=1e-9, atol=0, equal_nan=True)
        exp = _oracle(graph, params, graph["guess"], graph["query"], c)
        assert g["n_candidates"] == exp["n_candidates"]
        assert g["best_index"] == exp["best_index"]
        assert np.array_equal(g["pose"], exp["pose"])
        assert abs(g["score"] - exp["score"]) < TOL_TIGHT
        assert np.max(np.abs(g["scores"] - exp["scores"])) < TOL_TIGHT
        assert np.allclose(g["covariance"], exp["covariance"], rtol=1e-9, atol=0, equal_nan=True)
    # the three maps differ (origins and sizes), and so do their results
    assert len({g["score"] for g in got}) == 3


def test_one_candidate_chunks_and_determinism(graph):
    m = _matcher(graph, **SMALL)
    one = _candidate(graph, [3, 4])
    m.reset()
    m.addScansById([p for _, p in one], [i for i, _ in one])
    exp = m.matchScan(graph["guess"], graph["query"], want_scores=True)
    got = m.matchCandidates(graph["guess"], graph["query"], [one], want_scores=True)
    assert len(got) == 1
    _same_as_sequential(got[0], exp)

    # K = 9 through 16 slots (the matcher's own) and through 4 (three chunks, the last of one)
    cands = [_candidate(graph, loop_closure_window(i, 9)) for i in range(1, 10)]
    a = m.matchCandidates(graph["guess"], graph["query"], cands, want_scores=True)
    b = m.matchCandidates(graph["guess"], graph["query"], cands, want_scores=True)
    for x, y in zip(a, b):   # two runs: the same bits, covariance included
        assert x["score"] == y["score"] and x["best_index"] == y["best_index"]
        assert np.array_equal(x["scores"], y["scores"]) and np.array_equal(x["pose"], y["pose"])
        assert np.array_equal(x["covariance"], y["covariance"], equal_nan=True)
    chunked = _closure_records(m, graph, cands, slots=4)
    whole = _closure_records(m, graph, cands, slots=16)
    assert np.array_equal(chunked[0], whole[0], equal_nan=True) and np.array_equal(chunked[1], whole[1])
    # ... and they are the records the matcher's call turned into its results
    for k, x in enumerate(a):
        assert np.array_equal(whole[1][k], x["scores"])
        # (a record's index is -1 when no lattice candidate scored below 0)
        assert whole[0][k, 0] / 100 == x["score"]
        assert (NO_INDEX if whole[0][k, 1] < 0 else int(whole[0][k, 1])) == x["best_index"]


def _closure_records(m, graph, cands, slots):
    """ndt2d_closure_match on a closure object of its own with `slots` slots: (records, scores)."""
    import ctypes as C
    L = _capi.lib()
    # a store of its own on the matcher's context, with the graph's scans under the same ids
    h = m.device_handle
    store, closure = C.c_void_p(), C.c_void_p()
    assert L.ndt2d_scanstore_create(h, 1 << 16, 64, C.byref(store)) == _capi.OK
    try:
        for pts in graph["points"]:
            p = np.ascontiguousarray(pts, dtype=np.float64)
            assert L.ndt2d_scanstore_append(store, _capi.dptr(p), len(p), None) == _capi.OK
        assert L.ndt2d_closure_create(h, store, slots, C.byref(closure)) == _capi.OK
        try:
            n_th, n_lin, n_beams = m.prepare_search(graph["guess"], graph["query"])   # (no NDT: tables only)
            p = m.params
            dth = np.ascontiguousarray(_search(p["search_angular_size"], p["search_angular_resolution"]))
            dlin = np.ascontiguousarray(_search(p["search_linear_size"], p["search_linear_resolution"]))
            assert (len(dth), len(dlin)) == (n_th, n_lin)
            cos_th, sin_th = np.zeros(n_th), np.zeros(n_th)
            libm = C.CDLL("libm.so.6")   # the pair as the matcher takes it: one sincos() per theta step
            libm.sincos.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
            for i, d in enumerate(dth):
                sn, cs = C.c_double(0.0), C.c_double(0.0)
                libm.sincos(float(graph["guess"][2] + d), C.byref(sn), C.byref(cs))
                cos_th[i], sin_th[i] = cs.value, sn.value
            step = len(graph["query"]) / n_beams
            beams = np.ascontiguousarray([graph["query"][int(i * step)] for i in range(n_beams)])
            offsets = np.zeros(len(cands) + 1, dtype=np.uint64)
            offsets[1:] = np.cumsum([len(c) for c in cands])
            ids = np.ascontiguousarray([i for c in cands for i, _ in c], dtype=np.uint64)
            poses = np.ascontiguousarray([q for c in cands for _, q in c], dtype=np.float64)
            records = np.zeros((len(cands), 12))
            scores = np.zeros((len(cands), n_th * n_lin * n_lin))
            szp = C.POINTER(C.c_size_t)
            rc = L.ndt2d_closure_match(closure, len(cands), offsets.ctypes.data_as(szp), ids.ctypes.data_as(szp),
                                       _capi.dptr(poses), p["ndt_resolution"], p["range_max"], _capi.dptr(beams), n_beams,
                                       graph["guess"][0], graph["guess"][1], _capi.dptr(dth), _capi.dptr(cos_th),
                                       _capi.dptr(sin_th), n_th, _capi.dptr(dlin), n_lin, _capi.dptr(records),
                                       _capi.dptr(scores))
            assert rc == _capi.OK, L.ndt2d_closure_last_error(closure)
            return records, scores
        finally:
            L.ndt2d_closure_destroy(closure)
    finally:
        L.ndt2d_scanstore_destroy(store)


def _search(size, res):
    from ndt_2d_amd import search_offsets
    return search_offsets(size, res)


def test_plugin_defaults(graph):
    """80 theta steps x 21 x 21 translations, 100 of 720 beams, K = 4: winner, score, covariance."""
    m = _matcher(graph)   # the plugin's declared defaults
    cands = [_candidate(graph, loop_closure_window(i, 9)) for i in (2, 4, 7, 9)]
    got = m.matchCandidates(graph["guess"], graph["query"], cands)
    assert got[0]["n_candidates"] == 80 * 21 * 21
    for g, c in zip(got, cands):
        exp = _sequential(m, graph["guess"], graph["query"], c, want_scores=False)
        assert g["best_index"] == exp["best_index"] and np.array_equal(g["pose"], exp["pose"])
        assert g["score"] == exp["score"]
        assert np.allclose(g["covariance"], exp["covariance"], rtol=1e-9, atol=0, equal_nan=True)


def test_edges_single_theta_step_and_single_beam(graph):
    m = _matcher(graph, **dict(SMALL, search_angular_size=0.01, search_angular_resolution=0.02))
    cands = [_candidate(graph, [7]), _candidate(graph, [8, 9])]
    got = m.matchCandidates(graph["guess"], graph["query"], cands, want_scores=True)
    assert got[0]["n_candidates"] == 1 * 7 * 7
    for g, c in zip(got, cands):
        _same_as_sequential(g, _sequential(m, graph["guess"], graph["query"], c))
    one_beam = graph["query"][100:101]
    got = m.matchCandidates(graph["guess"], one_beam, cands, want_scores=True)
    for g, c in zip(got, cands):
        _same_as_sequential(g, _sequential(m, graph["guess"], one_beam, c))


def test_edges_scan_off_every_candidate_map(graph):
    m = _matcher(graph, **SMALL)
    far = np.array([100.0, 100.0, 0.3])
    cands = [_candidate(graph, [0]), _candidate(graph, [1, 2])]
    got = m.matchCandidates(far, graph["query"], cands, want_scores=True)
    for g, c in zip(got, cands):
        assert np.all(g["scores"] == 0.0) and g["score"] == 0.0
        assert g["best_index"] == NO_INDEX
        assert np.array_equal(g["pose"], [0.0, 0.0, 0.0])    # untouched
        _same_as_sequential(g, _sequential(m, far, graph["query"], c))


def test_edges_candidate_without_points(graph):
    m = _matcher(graph, extra=[np.zeros((0, 2))], **SMALL)
    empty = len(graph["points"])
    cands = [_candidate(graph, [2]), [(empty, (0.2, 0.1, 0.0))], [(empty, (0.2, 0.1, 0.0)), (3, graph["poses"][3])]]
    got = m.matchCandidates(graph["guess"], graph["query"], cands, want_scores=True)
    for g, c in zip(got, cands):
        _same_as_sequential(g, _sequential(m, graph["guess"], graph["query"], c))
    assert got[1]["best_index"] == NO_INDEX and np.all(got[1]["scores"] == 0.0)
    # a scan without points, matched: what the sequential path says
    none = m.matchCandidates(graph["guess"], np.zeros((0, 2)), cands[:1], want_scores=True)
    exp = _sequential(m, graph["guess"], np.zeros((0, 2)), cands[0])
    _same_as_sequential(none[0], exp)
    assert none[0]["n_candidates"] == 5 * 7 * 7 and none[0]["best_index"] == NO_INDEX


def test_edges_off_grid_scan_points(graph):
    m = _matcher(graph, **SMALL)
    pts = graph["query"].copy()
    bad = offgrid_cases.off_grid_points(0.25, RANGE_MAX)
    step = len(pts) / 100
    for i, (x, y, _) in enumerate(bad):
        pts[int((3 * i + 1) * step)] = (x, y)     # points the subsampling takes
    cands = [_candidate(graph, [4]), _candidate(graph, [5, 6])]
    got = m.matchCandidates(graph["guess"], pts, cands, want_scores=True)
    for g, c in zip(got, cands):
        assert np.all(np.isfinite(g["scores"]))
        _same_as_sequential(g, _sequential(m, graph["guess"], pts, c))


def test_edges_more_beams_than_one_staging_piece(graph):
    """1,440 beams: the search block rotates them into LDS in two pieces of 1,024."""
    long_scan = synth.scan(graph["world"], (0.13, -0.07, 0.031), 7200, n_beams=1440)
    m = _matcher(graph, **dict(SMALL, laser_max_beams=1440))
    cands = [_candidate(graph, [4]), _candidate(graph, [6, 7])]
    got = m.matchCandidates(graph["guess"], long_scan, cands, want_scores=True)
    for g, c in zip(got, cands):
        exp = _sequential(m, graph["guess"], long_scan, c)
        small = m.last_variant().startswith("match/lane-per-candidate/small-lattice")
        _same_as_sequential(g, exp, exact_scores=small)
        if not small:
            # another mapping adds a candidate's 1,440 non-negative terms in another order: each of the
            # two sums is within n * 2^-53 (relative) of the exact one
            bound = 2 * 1440 * 2.0 ** -53
            assert np.all(np.abs(g["scores"] - exp["scores"]) <= bound * np.abs(exp["scores"]))


def test_near_tie_is_settled_by_the_sequential_path():
    """The construction of tests/test_gpu_near_ties.py: one beam aimed at the mean of a symmetric
    cell, translations placed symmetrically around it -- the top candidates tie."""
    cell = np.array([[2.0, 2.0], [3.0, 2.0], [1.0, 2.0], [2.0, 3.0], [2.0, 1.0],
                     [2.5, 2.5], [1.5, 1.5], [2.5, 1.5], [1.5, 2.5]])
    params = dict(ndt_resolution=4.0, range_max=8.0, laser_max_beams=100,
                  search_linear_size=0.1875, search_linear_resolution=0.125,
                  search_angular_size=0.001, search_angular_resolution=0.002)
    scan_pose = (0.0, 0.0, 0.001)
    beam = np.array([[2.0, 2.0]])
    m = ScanMatcherNDT(0)
    m.initialize("ties", **params)
    assert m.storeScan(cell) == 0
    cand = [(0, (0.0, 0.0, 0.0))]
    exp = _sequential(m, scan_pose, beam, cand)
    assert m.adjudication_stats()[0] == 1          # the sequential search comes back marked
    s = np.sort(exp["scores"])
    assert s[0] == s[1] < 0.0
    before = m.adjudication_stats()[0]
    got = m.matchCandidates(scan_pose, beam, [cand], want_scores=True)[0]
    assert m.adjudication_stats()[0] == before + 1
    assert m.has_ndt() == 0
    _same_as_sequential(got, exp)
    ref = O.ScanMatcherNDT()
    ref.initialize(**params)
    ref.addScans([((0.0, 0.0, 0.0), cell)])
    want = ref.matchScan(scan_pose, beam, want_scores=True)
    assert got["best_index"] == want["best_index"] and got["score"] == want["score"]


def test_refusals_name_the_candidate_and_leave_the_matcher_usable(graph):
    m = _matcher(graph, **SMALL)
    good = _candidate(graph, [4])
    nan_pose = [(4, (0.0, float("nan"), 0.0))]
    # two scans 60 m apart on both axes: 279 x 279 = 77,841 cells
    too_large = [(4, (0.0, 0.0, 0.0)), (5, (60.0, 60.0, 0.0))]
    cases = {"unknown id": [(99, (0.0, 0.0, 0.0))], "pose": nan_pose, "no scans": [], "limits": too_large}
    for name, bad in cases.items():
        m.reset()
        m.addScansById([p for _, p in good], [i for i, _ in good])
        with pytest.raises(Ndt2dError) as ei:
            m.matchCandidates(graph["guess"], graph["query"], [good, bad, good])
        assert ei.value.code == _capi.ERR_INVALID, name
        assert "candidate 1" in str(ei.value), (name, str(ei.value))
        assert m.has_ndt() == 1                      # nothing was launched, the NDT in place stays
        got = m.matchCandidates(graph["guess"], graph["query"], [good], want_scores=True)[0]
        _same_as_sequential(got, _sequential(m, graph["guess"], graph["query"], good))


def test_close_loops_end_to_end(graph):
    m = _matcher(graph, **SMALL)
    rolling, limit = 8, 4
    cand_idx = [2, 4, 6, 8]
    guess, pts = graph["guess"], graph["query"]

    # the plain loop of src/ndt_mapper.cpp:619-671 over the sequential calls
    def reference_loop(typical, cand_idx):
        pose, accepted, left = guess.copy(), [], limit
        for i in cand_idx:
            cand = _candidate(graph, loop_closure_window(i, rolling))
            res = _sequential(m, pose, pts, cand, want_scores=False)
            if np.isfinite(res["score"]) and res["score"] < typical:
                pose = res["pose"] + pose
                accepted.append((i, res["score"], pose.copy()))
            left -= 1
            if left == 0:
                break
        return pose, accepted

    first = [_sequential(m, guess, pts, _candidate(graph, loop_closure_window(i, rolling)), want_scores=False)["score"]
             for i in cand_idx]
    # The candidate with the weakest response goes first and is rejected; the one behind it is accepted
    # (and whatever scores below the threshold from the corrected pose): an accept in the middle.
    worst = int(np.argmax(first))
    order = [worst] + [k for k in range(len(cand_idx)) if k != worst]
    cand_idx = [cand_idx[k] for k in order]
    first = [first[k] for k in order]
    assert first[1] < first[0]
    typical = 0.5 * (first[0] + first[1])
    want_pose, want_acc = reference_loop(typical, cand_idx)
    assert want_acc and want_acc[0][0] == cand_idx[1]
    pose, accepted = close_loops(m, guess, pts, cand_idx, graph["poses"], rolling, typical, limit,
                                 scan_sizes=[len(p) for p in graph["points"]])
    assert [a["candidate"] for a in accepted] == [i for i, _, _ in want_acc]
    assert [a["score"] for a in accepted] == [s for _, s, _ in want_acc]
    for a, (_, _, p) in zip(accepted, want_acc):
        assert np.array_equal(a["pose"], p)
    assert np.array_equal(pose, want_pose)


def test_batched_is_not_slower_than_the_sequential_calls(graph):
    """Plugin defaults, K = 8: eight build read-backs and eight fetches against one."""
    m = _matcher(graph)
    m.set_timing(False)
    cands = [_candidate(graph, loop_closure_window(i, 9)) for i in range(1, 9)]
    guess, pts = graph["guess"], graph["query"]

    def batched():
        m.matchCandidates(guess, pts, cands)

    def sequential():
        for c in cands:
            _sequential(m, guess, pts, c, want_scores=False)

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
    print("K = 8, plugin defaults: batched %.1f us, sequential %.1f us" % (t_bat * 1e6, t_seq * 1e6))
    assert t_bat < t_seq
