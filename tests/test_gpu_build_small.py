"""The fused small-map NDT build (csrc/build_small/, build mode "fused", ndt2d_build_grid_small) and
the resident scans (ndt2d_scanstore, storeScan / addScansById) against the CPU oracle and the host
build: every comparison is np.array_equal on the cells6 records and on the geometry -- the build is
bit-identical by construction, there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from ndt_2d_amd import Ndt2dError, ScanMatcherNDT, _capi, synth

pytestmark = pytest.mark.gpu

FUSED = "build/fused-small-map"
WORKGROUP = 1024                       # threads of the fused kernel's one workgroup


def _max_points():
    return _capi.lib().ndt2d_build_small_max_points()


def _oracle(scans, **params):
    ref = O.ScanMatcherNDT()
    ref.initialize(**params)
    ref.addScans(scans)
    return ref


def _matcher(mode, **params):
    m = ScanMatcherNDT(0)
    m.initialize("t", **params)
    m.set_build_mode(mode)
    return m


def _assert_grid(m, ref, what=""):
    cells, sx, sy, cs, ox, oy = m.grid()
    assert (sx, sy, ox, oy) == (ref.ndt.size_x, ref.ndt.size_y) + ref.ndt.origin, what
    assert np.array_equal(cells, ref.ndt.cells6()), what


def _fused_equals_oracle(scans, what="", **params):
    ref = _oracle(scans, **params)
    m = _matcher("fused", **params)
    try:
        m.addScans(scans)
        assert m.last_build() == FUSED, what
        _assert_grid(m, ref, what)
    finally:
        m.close()
    return ref


def _lidar30_map():
    """A 30 m lidar's local map, 245 x 245 cells: nine scans around a pose in cfg-5's world."""
    w = synth.world_of(5)
    true = synth.query_scan(5)[2]
    scans = []
    for j in range(3):
        for i in range(3):
            x, y = true[0] + (i - 1) * 0.5, true[1] + (j - 1) * 0.5
            assert not synth.pose_blocked(w, x, y)
            scans.append(((x, y, 0.0), synth.scan(w, (x, y, 0.0), 77 + 10 * j + i)))
    params = dict(synth.matcher_params(5, search_linear_size=0.05, search_linear_resolution=0.005,
                                       search_angular_size=0.1, search_angular_resolution=0.0025,
                                       laser_max_beams=100), range_max=30.0)
    guess = true + np.array([0.02, -0.02, 0.01])
    return scans, params, guess, synth.query_scan(5)[1], (245, 245)


def _cfg1_map():
    guess, pts, _ = synth.query_scan(1)
    return synth.map_scans(1), synth.matcher_params(1), guess, pts, (41, 41)


MAPS = {"cfg1_41x41": _cfg1_map, "lidar30_245x245": _lidar30_map}


@pytest.mark.parametrize("form", ["eigen", "closed"])
@pytest.mark.parametrize("name", sorted(MAPS))
def test_synthetic_maps_equal_the_oracle_and_the_host_build(name, form):
    scans, params, guess, pts, size = MAPS[name]()
    O.set_eigen_form(form)
    try:
        ref = _oracle(scans, **params)
        want = ref.ndt.cells6()
        assert (ref.ndt.size_x, ref.ndt.size_y) == size
    finally:
        O.set_eigen_form("eigen")
    rng = np.random.default_rng(11)
    poses = np.asarray(guess) + rng.uniform(-0.05, 0.05, (64, 3))
    got = {}
    for mode in ("host", "fused"):
        m = _matcher(mode, **params)
        try:
            m.set_eigenvalue_form(form)
            # (the host build keeps a host NDT and would score one pose on the host, in another
            # summation order: both matchers score it with the device's single-pose kernel)
            m.set_single_pose_path("device")
            m.addScans(scans)
            variant = m.last_build()
            grid = m.grid()
            got[mode] = dict(variant=variant, grid=grid, poses=m.scorePoses(pts, poses), scan=m.scoreScan(guess, pts),
                             match=m.matchScan(guess, pts, want_scores=True))
        finally:
            m.close()
    f, h = got["fused"], got["host"]
    assert f["variant"] == FUSED and h["variant"] == "build/host"
    assert f["grid"][1:] == h["grid"][1:]
    assert np.array_equal(f["grid"][0], want)
    assert np.array_equal(h["grid"][0], want)
    assert np.array_equal(f["poses"], h["poses"])
    assert f["scan"] == h["scan"] and f["scan"] < 0.0
    fm, hm = f["match"], h["match"]
    assert fm["best_index"] == hm["best_index"] and fm["score"] == hm["score"] and fm["score"] < 0.0
    assert np.array_equal(fm["pose"], hm["pose"])
    assert np.array_equal(fm["scores"], hm["scores"])
    assert np.array_equal(fm["covariance"], hm["covariance"])


def test_edge_cases_of_the_device_build_through_fused():
    rng = np.random.default_rng(5)
    w = synth.world_of(1)
    # rotated scan poses, an empty scan in the middle, a scan entirely outside the extent
    scans = []
    for k in range(12):
        pose = (rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-3.1, 3.1))
        scans.append((pose, synth.scan(w, pose, 7000 + k, n_beams=300 + 17 * k)))
    scans.insert(3, ((0.2, 0.1, 1.0), np.zeros((0, 2))))
    scans.append(((0.0, 0.0, 0.0), np.full((40, 2), 500.0)))
    for res in (0.25, 0.1, 1.0):
        ref = _oracle(scans, ndt_resolution=res, range_max=4.75)
        gpu = _matcher("fused", ndt_resolution=res, range_max=4.75)
        try:
            gpu.addScans(scans)
            assert gpu.last_build() == FUSED
            _assert_grid(gpu, ref, res)
            if res == 1.0:
                # re-building with a different map replaces the grid; reset clears it
                gpu.addScans(scans[:2])
                ref.addScans(scans[:2])
                _assert_grid(gpu, ref)
                gpu.reset()
                assert not gpu.has_ndt()
        finally:
            gpu.close()


# A 17 x 17 grid of 0.25 m cells with its origin at (-2, -2): one scan pose at the origin, range_max 2.
SMALL = dict(ndt_resolution=0.25, range_max=2.0)
IDENT = (0.0, 0.0, 0.0)


@pytest.mark.parametrize("n", [0, 1, WORKGROUP - 1, WORKGROUP, WORKGROUP + 1])
def test_point_counts_around_the_workgroup_size(n):
    pts = np.random.default_rng(100 + n).uniform(-2.0, 2.0, (n, 2))
    ref = _fused_equals_oracle([(IDENT, pts)], n, **SMALL)
    assert (ref.ndt.size_x, ref.ndt.size_y) == (17, 17)


def test_one_cell_with_a_chain_longer_than_the_workgroup():
    pts = np.random.default_rng(1).uniform(0.01, 0.24, (1100, 2))
    ref = _fused_equals_oracle([(IDENT, pts[:400]), (IDENT, pts[400:])], **SMALL)
    cells = ref.ndt.cells6()
    assert np.count_nonzero(cells[:, 5]) == 1 and cells[:, 5].max() == 1100.0


def test_every_point_in_a_cell_of_its_own():
    c = -2.0 + 0.25 * np.arange(17) + 0.125
    pts = np.stack(np.meshgrid(c, c), axis=-1).reshape(-1, 2)
    pts = pts[np.random.default_rng(2).permutation(len(pts))]
    ref = _fused_equals_oracle([(IDENT, pts)], **SMALL)
    assert np.array_equal(ref.ndt.cells6()[:, 5], np.ones(17 * 17))


def test_points_on_cell_boundaries_and_the_far_edges():
    edges = -2.0 + 0.25 * np.arange(18)            # the last one, 2.25, is the grid's far edge: outside
    on = np.stack(np.meshgrid(edges, edges), axis=-1).reshape(-1, 2)
    jitter = np.random.default_rng(3).uniform(0.0, 0.01, (6, 1, 2))
    jitter[0] = 0.0                                 # exactly on the boundary, then just inside the cell
    pts = (on[None] + jitter).reshape(-1, 2)
    below = np.array([[np.nextafter(2.25, 0.0), 0.0], [0.0, np.nextafter(2.25, 0.0)], [-2.0, -2.0],
                      [np.nextafter(-2.0, -3.0), 0.0], [2.25, 2.25]])
    ref = _fused_equals_oracle([(IDENT, np.concatenate([pts, below]))], **SMALL)
    assert ref.ndt.cells6()[:, 5].sum() < len(pts) + len(below)   # the far edge's points were dropped


def test_non_finite_and_far_points_are_dropped():
    rng = np.random.default_rng(4)
    pts = rng.uniform(-2.0, 2.0, (600, 2))
    bad = np.array([[np.nan, 0.0], [0.0, np.nan], [np.inf, 0.0], [0.0, -np.inf], [-np.inf, np.inf],
                    [1.0e6, 0.0], [0.0, -1.0e6], [1.0e6, 1.0e6], [np.nan, np.nan]])
    at = rng.integers(0, len(pts), 60)
    pts[at] = bad[np.arange(60) % len(bad)]
    ref = _fused_equals_oracle([(IDENT, pts[:250]), ((0.1, -0.1, 0.7), pts[250:])], **SMALL)
    assert ref.ndt.cells6()[:, 5].sum() < 600


def test_a_grid_of_65534_cells_with_a_handful_of_points():
    # scan poses (0, 0) and (34, 55.25), range_max 10: 54 m x 75.25 m of 0.25 m cells = 217 x 302
    near = np.array([[0.0, 0.0], [0.03, 0.01], [0.01, 0.04], [0.05, 0.05], [0.02, 0.06], [0.06, 0.02]])
    scans = [(IDENT, np.concatenate([0.1 + near, [[9.9, -9.9]]])),
             ((34.0, 55.25, 0.0), np.concatenate([9.9 + near[:5], [[-3.0, 2.0], [10.01, 0.0]]]))]
    ref = _fused_equals_oracle(scans, ndt_resolution=0.25, range_max=10.0)
    assert ref.ndt.size_x * ref.ndt.size_y == 65534
    cells = ref.ndt.cells6()
    assert np.count_nonzero(cells[:, 5] >= 5) == 2 and cells[-1, 5] == 0.0 and not np.isnan(cells).any()
    assert cells[ref.ndt.getIndex(43.95, 65.2), 5] == 5.0        # next to the grid's far corner


def _order_sensitive_scans():
    """One cell fed by three scans, its points near (1000, 1000) with a 1 mm spread: correlation -
    mean^2 cancels, so the record depends on the order the cell saw its points in."""
    rng = np.random.default_rng(7)
    return [((1000.0, 1000.0, 0.0), 0.1 + rng.uniform(-0.0005, 0.0005, (7, 2))) for _ in range(3)]


def test_the_cell_sees_its_points_in_scan_order():
    scans = _order_sensitive_scans()
    ref_fwd, ref_rev = _oracle(scans, **SMALL), _oracle(scans[::-1], **SMALL)    # (the views need their owners)
    fwd, rev = ref_fwd.ndt.cells6(), ref_rev.ndt.cells6()
    cell = int(np.argmax(fwd[:, 5]))
    assert fwd[cell, 5] == 21.0 and np.count_nonzero(fwd[:, 5]) == 1
    assert not np.array_equal(fwd[cell], rev[cell])     # the oracle alone: the order changes bits
    _fused_equals_oracle(scans, "forward", **SMALL)
    _fused_equals_oracle(scans[::-1], "reversed", **SMALL)


def _build_grid_small(h, scans, res, range_max):
    L = _capi.lib()
    poses = np.ascontiguousarray([s[0] for s in scans], dtype=np.float64)
    pts = np.ascontiguousarray(np.concatenate([np.reshape(s[1], (-1, 2)) for s in scans]), dtype=np.float64)
    offsets = np.zeros(len(scans) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(np.reshape(s[1], (-1, 2))) for s in scans])
    return L.ndt2d_build_grid_small(h, res, range_max, _capi.dptr(poses), _capi.dptr(pts),
                                    offsets.ctypes.data_as(C.POINTER(C.c_size_t)), len(scans))


def test_maps_beyond_the_limits_take_the_auto_path():
    n_max = _max_points()
    assert n_max >= 16384
    rng = np.random.default_rng(8)
    too_many = [(IDENT, rng.uniform(-2.0, 2.0, (n_max + 1, 2)))]
    # scan poses (0, 0) and (43.5, 44), range_max 10: 63.5 m x 64 m of 0.25 m cells = 255 x 257 = 65,535
    too_wide = [(IDENT, rng.uniform(-2.0, 2.0, (50, 2))), ((43.5, 44.0, 0.0), rng.uniform(-2.0, 2.0, (50, 2)))]
    for scans, params in ((too_many, SMALL), (too_wide, dict(ndt_resolution=0.25, range_max=10.0))):
        ref = _oracle(scans, **params)
        m = _matcher("fused", **params)
        try:
            m.addScans(scans)
            assert m.last_build() == "build/host"        # what "auto" does below 73,728 points
            _assert_grid(m, ref)
            # the entry point itself refuses, and leaves the context without a grid
            h = m.device_handle
            assert _capi.lib().ndt2d_has_grid(h) == 1
            assert _build_grid_small(h, scans, params["ndt_resolution"], params["range_max"]) == _capi.ERR_INVALID
            assert b"limits" in _capi.lib().ndt2d_build_small_last_error(h)
            assert _capi.lib().ndt2d_has_grid(h) == 0
        finally:
            m.close()
    assert ref.ndt.size_x * ref.ndt.size_y == 65535
    # exactly at the point limit the fused path runs
    at_limit = [(IDENT, too_many[0][1][:n_max])]
    _fused_equals_oracle(at_limit, **SMALL)


def _twelve_scans():
    rng = np.random.default_rng(9)
    w = synth.world_of(1)
    poses = [(rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-3.1, 3.1)) for _ in range(12)]
    return poses, [synth.scan(w, p, 9000 + k, n_beams=200 + 31 * k) for k, p in enumerate(poses)]


def test_resident_scans_build_what_add_scans_builds():
    poses, points = _twelve_scans()
    params = dict(ndt_resolution=0.25, range_max=4.75)
    rng = np.random.default_rng(10)
    m = _matcher("host", **params)       # (by-id builds are fused whatever the mode of addScans)
    try:
        ids = [m.storeScan(p) for p in points]
        assert ids == list(range(12))
        for first in (0, 1, 2):
            window = list(range(first, first + 10))
            moved = [tuple(np.asarray(poses[k]) + rng.uniform(-0.02, 0.02, 3)) for k in window]
            m.addScansById(moved, window)
            assert m.last_build() == FUSED and m.has_ndt()
            _assert_grid(m, _oracle([(moved[i], points[k]) for i, k in enumerate(window)], **params), first)
        order = [7, 2, 11, 2, 0, 5]                   # not ascending, one scan twice
        m.addScansById([poses[k] for k in order], order)
        _assert_grid(m, _oracle([(poses[k], points[k]) for k in order], **params), "order")
    finally:
        m.close()


def test_refused_builds_leave_the_grid_scoring_as_before():
    poses, points = _twelve_scans()
    params = dict(ndt_resolution=0.25, range_max=4.75)
    probe = np.asarray(poses[0]) + np.random.default_rng(12).uniform(-0.05, 0.05, (16, 3))
    m = _matcher("fused", **params)
    try:
        for p in points[:4]:
            m.storeScan(p)
        m.addScansById(poses[:4], [0, 1, 2, 3])
        before = m.scorePoses(points[0], probe)
        assert np.any(before < 0.0)
        with pytest.raises(Ndt2dError) as ei:
            m.addScansById(poses[:2], [0, 4])         # an unknown id
        assert ei.value.code == _capi.ERR_INVALID and "unknown scan id" in str(ei.value)
        assert np.array_equal(m.scorePoses(points[0], probe), before)
        with pytest.raises(Ndt2dError) as ei:
            m.addScansById([poses[0], (0.0, np.nan, 0.0)], [0, 1])
        assert ei.value.code == _capi.ERR_INVALID and "not finite" in str(ei.value)
        with pytest.raises(Ndt2dError) as ei:
            m.addScansById([poses[0], (np.inf, 0.0, 0.0)], [0, 1])
        assert ei.value.code == _capi.ERR_INVALID
        assert m.has_ndt() and np.array_equal(m.scorePoses(points[0], probe), before)
        # a store that is full refuses the scan and keeps what it holds
        with pytest.raises(Ndt2dError) as ei:
            m.storeScan(np.zeros((262144, 2)))
        assert ei.value.code == _capi.ERR_INVALID and "full" in str(ei.value)
        assert m.storeScan(points[4]) == 4
        assert np.array_equal(m.scorePoses(points[0], probe), before)
        # after dropScans the old ids are unknown, and ids start over
        m.dropScans()
        with pytest.raises(Ndt2dError) as ei:
            m.addScansById(poses[:1], [0])
        assert ei.value.code == _capi.ERR_INVALID
        assert np.array_equal(m.scorePoses(points[0], probe), before)
        assert m.storeScan(points[5]) == 0
        m.addScansById([poses[5]], [0])
        _assert_grid(m, _oracle([(poses[5], points[5])], **params))
    finally:
        m.close()


def test_scan_store_object_capacities():
    """The device-layer object: capacities of its own, refusals before anything is launched."""
    L = _capi.lib()
    m = _matcher("fused", **SMALL)
    store = C.c_void_p()
    try:
        h = m.device_handle
        assert L.ndt2d_scanstore_create(h, 100, 2, C.byref(store)) == _capi.OK
        rng = np.random.default_rng(13)
        a, b = rng.uniform(-2, 2, (60, 2)), rng.uniform(-2, 2, (40, 2))
        sid = C.c_size_t(99)
        assert L.ndt2d_scanstore_append(store, _capi.dptr(a), 60, C.byref(sid)) == _capi.OK and sid.value == 0
        assert L.ndt2d_scanstore_append(store, _capi.dptr(a), 41, C.byref(sid)) == _capi.ERR_INVALID   # points
        assert b"full" in L.ndt2d_scanstore_last_error(store)
        assert L.ndt2d_scanstore_append(store, _capi.dptr(b), 40, C.byref(sid)) == _capi.OK and sid.value == 1
        assert L.ndt2d_scanstore_append(store, _capi.dptr(b), 0, C.byref(sid)) == _capi.ERR_INVALID    # scans
        n = C.c_size_t(0)
        assert L.ndt2d_scanstore_count(store, C.byref(n)) == _capi.OK and n.value == 2
        poses = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.5]])
        ids = (C.c_size_t * 2)(1, 0)
        assert L.ndt2d_has_grid(h) == 0
        assert L.ndt2d_scanstore_build(store, ids, _capi.dptr(poses), 2, 0.25, 2.0) == _capi.OK
        assert L.ndt2d_has_grid(h) == 1
        ref = _oracle([(poses[0], b), (poses[1], a)], **SMALL)
        cells = np.zeros((ref.ndt.size_x * ref.ndt.size_y, 6))
        assert L.ndt2d_get_grid(h, _capi.dptr(cells), len(cells), None, None, None, None, None) == _capi.OK
        assert np.array_equal(cells, ref.ndt.cells6())
        # the store's own eigenvalue form
        assert L.ndt2d_scanstore_set_eigenvalue_form(store, b"neither") == _capi.ERR_INVALID
        assert L.ndt2d_scanstore_set_eigenvalue_form(store, b"closed") == _capi.OK
        assert L.ndt2d_scanstore_build(store, ids, _capi.dptr(poses), 2, 0.25, 2.0) == _capi.OK
        O.set_eigen_form("closed")
        try:
            ref_closed = _oracle([(poses[0], b), (poses[1], a)], **SMALL)
            closed = ref_closed.ndt.cells6()
        finally:
            O.set_eigen_form("eigen")
        assert L.ndt2d_get_grid(h, _capi.dptr(cells), len(cells), None, None, None, None, None) == _capi.OK
        assert np.array_equal(cells, closed)
        bad = (C.c_size_t * 2)(0, 2)
        assert L.ndt2d_scanstore_build(store, bad, _capi.dptr(poses), 2, 0.25, 2.0) == _capi.ERR_INVALID
        assert L.ndt2d_has_grid(h) == 1
        assert L.ndt2d_scanstore_reset(store) == _capi.OK
        assert L.ndt2d_scanstore_build(store, ids, _capi.dptr(poses), 2, 0.25, 2.0) == _capi.ERR_INVALID
    finally:
        if store:
            L.ndt2d_scanstore_destroy(store)
        m.close()


def test_two_contexts_on_one_gpu_build_by_id():
    poses, points = _twelve_scans()
    params = dict(ndt_resolution=0.25, range_max=4.75)
    L = _capi.lib()
    m = ScanMatcherNDT(device_ids=[0, 0])
    try:
        m.initialize("two", **params)
        assert m.device_count() == 2
        ids = [m.storeScan(p) for p in points[:6]]
        order = ids[::-1]
        m.addScansById([poses[k] for k in order], order)
        ref = _oracle([(poses[k], points[k]) for k in order], **params)
        want = ref.ndt.cells6()
        for rank in range(2):
            h = C.c_void_p(L.ndt2d_matcher_device_at(m._m, rank))
            sx, sy = C.c_uint32(0), C.c_uint32(0)
            ox, oy = C.c_double(0), C.c_double(0)
            cells = np.zeros_like(want)
            assert L.ndt2d_get_grid(h, _capi.dptr(cells), len(cells), C.byref(sx), C.byref(sy), None,
                                    C.byref(ox), C.byref(oy)) == _capi.OK
            assert (sx.value, sy.value, ox.value, oy.value) == (ref.ndt.size_x, ref.ndt.size_y) + ref.ndt.origin
            assert np.array_equal(cells, want), rank
    finally:
        m.close()
