"""The resident occupancy map (ndt2d_occupancy_map, ndt_2d_amd.OccupancyMap) against the CPU
oracle's generator and the existing renderer.  Counts are integers: adding the new scans' rays to
the counters of the last publish gives exactly the map a full re-trace gives, so every comparison
here is np.array_equal / ==, and the mode of every update is predicted from the oracle alone (the
rule in include/ndt2d_hip.h: INCREMENTAL iff the counters are valid, the geometry is bit for bit
that of the last update, the old poses are bit for bit those of the last update, and the count
grew)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from ndt_2d_amd import OccupancyMap, ScanMatcherNDT, _capi, synth
from ndt_2d_amd.occupancy_grid import OccupancyGrid

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    m = ScanMatcherNDT(0)
    m.initialize("occmap", **synth.matcher_params(1))
    return m


def _same(got, want):
    for k in ("resolution", "width", "height", "origin_x", "origin_y"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["data"].shape == want["data"].shape
    assert np.array_equal(got["data"], want["data"])


def _geo(msg):
    return (np.float64(msg["origin_x"]).tobytes(), np.float64(msg["origin_y"]).tobytes(),
            msg["width"], msg["height"])


def _poses_bytes(scans, n):
    return np.ascontiguousarray([s[0] for s in scans[:n]], dtype=np.float64).tobytes()


class Carried:
    """An OccupancyMap and an oracle generator carried through the same calls; the expected mode
    comes from the oracle's messages and the poses passed, never from the object under test."""

    def __init__(self, resolution, occ_thresh, device, grid=False):
        self.res, self.thresh, self.device = resolution, occ_thresh, device
        self.gpu = OccupancyMap(resolution, occ_thresh, device)
        self.grid = grid
        self.modes = []
        self._fresh()

    def _fresh(self):
        self.ref = O.OccupancyGrid(self.res, self.thresh)
        self.old = OccupancyGrid(self.res, self.thresh, self.device) if self.grid else None
        self.prev_geo = None
        self.prev_scans = []

    def reset(self):
        self.gpu.reset()
        self._fresh()
        assert self.gpu.num_scans == 0 and np.array_equal(self.gpu.bounds, np.zeros(4))

    def publish(self, scans):
        scans = list(scans)
        want = self.ref.getMsg(scans)
        got = self.gpu.getMsg(scans)
        n_old = len(self.prev_scans)
        keep = (self.prev_geo is not None and _geo(want) == self.prev_geo and
                _poses_bytes(scans, n_old) == _poses_bytes(self.prev_scans, n_old))
        expect = "FULL" if not keep else ("INCREMENTAL" if len(scans) > n_old else "UNCHANGED")
        assert self.gpu.last_mode == expect, (len(scans), n_old, self.gpu.last_mode, expect)
        _same(got, want)
        assert np.array_equal(self.gpu.bounds, self.ref.bounds)
        assert self.gpu.num_scans == self.ref.num_scans == len(scans)
        if self.old is not None:
            _same(got, self.old.getMsg(scans))
        x0, y0, w, h = self.gpu.last_rect
        assert x0 + w <= want["width"] and y0 + h <= want["height"]
        if expect == "FULL":
            assert (x0, y0, w, h) == (0, 0, want["width"], want["height"])
            assert self.gpu.last_beams_traced == sum(len(s[1]) for s in scans)
        elif expect == "INCREMENTAL":
            assert self.gpu.last_beams_traced == sum(len(s[1]) for s in scans[n_old:])
        else:
            assert self.gpu.last_beams_traced == 0 and w * h == 0
        self.prev_geo = _geo(want)
        self.prev_scans = scans
        self.modes.append(expect)
        return got, want


@pytest.mark.parametrize("cfg,resolution,occ_thresh", [(1, 0.05, 0.25), (3, 0.1, 0.25)])
def test_grown_scan_by_scan(device, cfg, resolution, occ_thresh):
    """Every prefix of the cfg's map scans, one scan more per publish: info, data, bounds and
    num_scans equal the oracle generator's and the existing renderer's at every step."""
    scans = synth.map_scans(cfg)
    c = Carried(resolution, occ_thresh, device, grid=True)
    for k in range(1, len(scans) + 1):
        c.publish(scans[:k])
    assert c.modes[0] == "FULL"
    share = c.modes.count("INCREMENTAL") / float(len(c.modes))
    print("cfg-%d: %d publishes, share of incremental steps %.4f" % (cfg, len(c.modes), share))


STABLE_RES = 0.0625   # a power of two: floor(b / r) * r reproduces a rounded bound exactly


def _stable_sequence(seed=11, n=30):
    """A frame scan with four far corner points that fixes the bounds, then scans strictly inside."""
    rng = np.random.default_rng(seed)
    frame = ((0.0, 0.0, 0.0), np.array([[-8.0, -8.0], [8.0, -8.0], [8.0, 8.0], [-8.0, 8.0]]))
    scans = [frame]
    for _ in range(n):
        x, y, th = rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-np.pi, np.pi)
        npts = int(rng.integers(1, 301))
        target = rng.uniform(-7, 7, size=(npts, 2)) - (x, y)
        c, s = np.cos(th), np.sin(th)
        pts = np.stack([c * target[:, 0] + s * target[:, 1], -s * target[:, 0] + c * target[:, 1]], axis=1)
        scans.append(((x, y, th), pts))
    return scans


def _cells(v, origin, resolution):
    """int((v - origin) / resolution), the renderer's cell coordinate"""
    return np.trunc((np.asarray(v, dtype=np.float64) - origin) / resolution).astype(np.int64)


def test_stable_geometry_is_incremental_every_time(device):
    scans = _stable_sequence()
    c = Carried(STABLE_RES, 0.25, device)
    c.publish(scans[:1])
    for k in range(2, len(scans) + 1):
        c.publish(scans[:k])
        assert c.gpu.last_mode == "INCREMENTAL"
        assert c.gpu.last_beams_traced == len(scans[k - 1][1])
    assert c.modes == ["FULL"] + ["INCREMENTAL"] * 30


def test_dirty_rectangle_covers_every_changed_cell_and_no_more_than_the_box(device):
    scans = _stable_sequence(seed=12)
    c = Carried(STABLE_RES, 0.25, device)
    _, prev = c.publish(scans[:1])
    for k in range(2, len(scans) + 1):
        _, want = c.publish(scans[:k])
        x0, y0, w, h = c.gpu.last_rect
        ys, xs = np.nonzero(want["data"] != prev["data"])
        if len(xs):
            assert x0 <= xs.min() and xs.max() < x0 + w and y0 <= ys.min() and ys.max() < y0 + h
        # the cell bounding box of the new scan's start and end cells, grown by one cell, clipped
        (px, py, th), pts = scans[k - 1]
        cs, sn = np.cos(th), np.sin(th)
        mx = pts[:, 0] * cs - pts[:, 1] * sn + px
        my = pts[:, 0] * sn + pts[:, 1] * cs + py
        cx = np.concatenate([_cells(mx, want["origin_x"], STABLE_RES), _cells([px], want["origin_x"], STABLE_RES)])
        cy = np.concatenate([_cells(my, want["origin_y"], STABLE_RES), _cells([py], want["origin_y"], STABLE_RES)])
        bx0, bx1 = max(cx.min() - 1, 0), min(cx.max() + 1, want["width"] - 1)
        by0, by1 = max(cy.min() - 1, 0), min(cy.max() + 1, want["height"] - 1)
        assert w > 0 and h > 0
        assert bx0 <= x0 and x0 + w - 1 <= bx1 and by0 <= y0 and y0 + h - 1 <= by1
        assert w * h < want["width"] * want["height"]
        prev = want


def test_pose_changes(device):
    scans = synth.map_scans(1)
    c = Carried(0.05, 0.25, device)
    c.publish(scans[:5])
    c.publish(scans)
    bounds = c.gpu.bounds.copy()
    # one old pose moved by one ulp
    (x, y, th), pts = scans[2]
    moved = list(scans)
    moved[2] = ((np.nextafter(x, np.inf), y, th), pts)
    c.publish(moved)
    assert c.gpu.last_mode == "FULL"
    assert np.array_equal(c.gpu.bounds, bounds)        # the count did not change (:51-54)
    # the same call again
    got1, _ = c.publish(moved)
    assert c.gpu.last_mode == "UNCHANGED" and c.gpu.last_beams_traced == 0
    assert c.gpu.last_rect[2] * c.gpu.last_rect[3] == 0
    got2, _ = c.publish(moved)
    assert c.gpu.last_mode == "UNCHANGED" and np.array_equal(got1["data"], got2["data"])
    # every pose perturbed (a graph optimisation)
    rng = np.random.default_rng(5)
    shaken = [((p[0] + rng.normal(0, 0.02), p[1] + rng.normal(0, 0.02), p[2] + rng.normal(0, 0.01)), pts)
              for p, pts in moved]
    c.publish(shaken)
    assert c.gpu.last_mode == "FULL"
    assert np.array_equal(c.gpu.bounds, bounds)
    # 0.0 -> -0.0 in an old pose
    assert shaken[4][0][2] != 0.0
    zero = list(shaken)
    zero[4] = ((shaken[4][0][0], shaken[4][0][1], 0.0), shaken[4][1])
    c.publish(zero)
    assert c.gpu.last_mode == "FULL"
    c.publish(zero)
    assert c.gpu.last_mode == "UNCHANGED"
    minus = list(zero)
    minus[4] = ((zero[4][0][0], zero[4][0][1], -0.0), zero[4][1])
    c.publish(minus)
    assert c.gpu.last_mode == "FULL"


def test_geometry_growth(device):
    scans = synth.map_scans(1)
    c = Carried(STABLE_RES, 0.25, device)      # re-rounding a rounded bound changes nothing
    c.publish(scans[:4])
    far = ((6.0, -5.0, 0.7), np.array([[1.0, 0.0], [0.0, 2.0], [-1.5, 0.5]]))
    got, _ = c.publish(scans[:4] + [far])
    assert c.gpu.last_mode == "FULL"
    assert c.gpu.bounds[1] > 6.0 and c.gpu.bounds[2] < -5.0
    inside = ((1.0, -1.0, 0.2), np.array([[1.0, 0.5], [0.5, -1.0], [2.0, 0.0]]))
    before = _geo(got)
    got, _ = c.publish(scans[:4] + [far, inside])
    assert _geo(got) == before
    assert c.gpu.last_mode == "INCREMENTAL" and c.gpu.last_beams_traced == 3


EDGE_CASES = {
    # the pose lies outside the bounding box of all points: rays start outside and are clipped
    "pose_outside": (0.1, [((20.0, 20.0, 0.0), np.array([[-18.0, -19.0], [-17.0, -19.5]])),
                           ((-30.0, 5.0, 1.0), np.array([[31.0, -4.0], [30.5, -6.0]]))]),
    # zero-length rays hit their own cell
    "zero_length": (0.1, [((0.5, 0.5, 0.3), np.zeros((3, 2))), ((0.25, 0.75, 0.0), np.zeros((2, 2)))]),
    # empty scans in the middle of the sequence
    "empty_in_the_middle": (0.1, [((0.0, 0.0, 0.0), np.array([[2.0, 1.0], [-1.0, 2.0], [-2.0, -2.0]])),
                                  ((1.0, 1.0, 0.0), np.zeros((0, 2))),
                                  ((0.5, 0.5, 0.0), np.zeros((0, 2))),
                                  ((0.5, -0.5, 0.5), np.array([[1.0, 0.5], [0.5, 1.0]])),
                                  ((0.0, 0.5, 0.0), np.zeros((0, 2)))]),
}


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_edge_cases_fresh_and_incremental(device, name):
    resolution, scans = EDGE_CASES[name]
    fresh = Carried(resolution, 0.25, device, grid=True)
    got, _ = fresh.publish(scans)
    if name == "zero_length":
        assert (got["data"] == 100).sum() == 2 and (got["data"] == 0).sum() == 0
    grown = Carried(resolution, 0.25, device, grid=True)
    for k in range(1, len(scans) + 1):
        grown.publish(scans[:k])
    grown.publish(scans)
    assert grown.gpu.last_mode == "UNCHANGED"


def test_no_scans_at_all(device):
    """The 10 x 10 padding map, all unknown; then scans arrive."""
    c = Carried(0.1, 0.25, device, grid=True)
    got, _ = c.publish([])
    assert c.gpu.last_mode == "FULL"
    assert got["width"] == 10 and got["height"] == 10 and np.all(got["data"] == -1)
    c.publish([])
    assert c.gpu.last_mode == "UNCHANGED"
    scans = EDGE_CASES["empty_in_the_middle"][1]
    for k in range(1, len(scans) + 1):
        c.publish(scans[:k])


def test_random_operation_sequences(device):
    """48 seeded sequences of append-and-publish, publish again, perturb poses and reset, each
    against an oracle generator carried through the same calls; every publish is compared."""
    rng = np.random.default_rng(2024)
    n_publishes = 0
    modes = {"FULL": 0, "INCREMENTAL": 0, "UNCHANGED": 0}
    for seq in range(48):
        res = float(rng.choice([0.05, 0.1, 0.25, 0.3]))
        thresh = float(rng.choice([0.1, 0.25, 0.5]))
        c = Carried(res, thresh, device, grid=(seq % 8 == 0))
        scans = []
        # half of the sequences start with a frame scan, so that later ones land inside
        if seq % 2 == 0:
            scans.append(((0.0, 0.0, 0.0), np.array([[-12.0, -12.0], [12.0, -12.0], [12.0, 12.0], [-12.0, 12.0]])))
        for _ in range(int(rng.integers(6, 13))):
            op = rng.choice(["append", "append", "append", "again", "perturb", "reset"],
                            p=[0.25, 0.25, 0.2, 0.12, 0.12, 0.06])
            if op == "append" or not scans:
                for _ in range(int(rng.integers(1, 5))):
                    pose = (rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-np.pi, np.pi))
                    n = int(rng.integers(0, 300))
                    scans.append((pose, rng.uniform(-6, 6, size=(n, 2))))
            elif op == "perturb":
                for k in rng.choice(len(scans), size=int(rng.integers(1, len(scans) + 1)), replace=False):
                    p, pts = scans[k]
                    scans[k] = ((p[0] + rng.normal(0, 0.01), p[1] + rng.normal(0, 0.01),
                                 p[2] + rng.normal(0, 0.005)), pts)
            elif op == "reset":
                c.reset()
                scans = []
                for _ in range(int(rng.integers(1, 4))):
                    pose = (rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-np.pi, np.pi))
                    scans.append((pose, rng.uniform(-6, 6, size=(int(rng.integers(0, 300)), 2))))
            c.publish(scans)
            n_publishes += 1
        for m in c.modes:
            modes[m] += 1
    print("random sequences: %d publishes, modes %r" % (n_publishes, modes))
    assert n_publishes >= 48 * 6 and min(modes.values()) > 0


def test_buffer_growth_by_scans_and_by_points(device):
    """More scans and more points than the buffers start with (256 scans, 16384 points)."""
    rng = np.random.default_rng(8)
    # by scans: 700 small scans, published at a few lengths
    scans = [((0.0, 0.0, 0.0), np.array([[-7.0, -7.0], [7.0, -7.0], [7.0, 7.0], [-7.0, 7.0]]))]
    for _ in range(700):
        pose = (rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-np.pi, np.pi))
        scans.append((pose, rng.uniform(-2, 2, size=(int(rng.integers(0, 4)), 2))))
    c = Carried(0.25, 0.25, device)
    for k in (1, 200, 255, 256, 257, 258, 600, 701):
        c.publish(scans[:k])
    assert "INCREMENTAL" in c.modes
    # by points: scans of 5000 points, grown across three doublings, one publish per scan
    big = [((0.0, 0.0, 0.0), np.array([[-7.0, -7.0], [7.0, -7.0], [7.0, 7.0], [-7.0, 7.0]]))]
    for _ in range(14):
        pose = (rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-np.pi, np.pi))
        big.append((pose, rng.uniform(-2.5, 2.5, size=(5000, 2))))
    c = Carried(0.25, 0.25, device, grid=True)
    for k in range(1, len(big) + 1):
        c.publish(big[:k])
    assert c.modes.count("INCREMENTAL") == 14
    # one scan larger than the whole initial buffer, as the first
    c = Carried(0.1, 0.5, device)
    c.publish([((0.5, 0.5, 0.1), rng.uniform(-4, 4, size=(40000, 2)))])


def _raw(device, resolution=0.1, occ_thresh=0.25):
    L = _capi.lib()
    m = C.c_void_p()
    assert L.ndt2d_occmap_create(device.device_handle, resolution, occ_thresh, C.byref(m)) == _capi.OK
    return L, m


def test_read_returns_any_rectangle(device):
    scans = synth.map_scans(1)
    om = OccupancyMap(0.05, 0.25, device)
    whole = om.getMsg(scans)["data"]
    H, W = whole.shape
    L, m = om._L, om._map
    rng = np.random.default_rng(3)
    rects = [(0, 0, W, H), (0, 0, 1, 1), (W - 1, H - 1, 1, 1), (0, 5, W, 3), (7, 0, 2, H)]
    for _ in range(20):
        x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
        rects.append((x0, y0, int(rng.integers(1, W - x0 + 1)), int(rng.integers(1, H - y0 + 1))))
    for x0, y0, w, h in rects:
        for stride in (w, w + 5):
            out = np.full((h, stride), 77, dtype=np.int8)
            assert L.ndt2d_occmap_read(m, x0, y0, w, h, out.ctypes.data_as(C.c_void_p), stride) == _capi.OK
            assert np.array_equal(out[:, :w], whole[y0:y0 + h, x0:x0 + w])
            assert np.all(out[:, w:] == 77)
    # empty rectangles are fine, rectangles that leave the map and strides below w are not
    assert L.ndt2d_occmap_read(m, 3, 3, 0, 0, None, 0) == _capi.OK
    out = np.zeros((H + 1, W + 1), dtype=np.int8)
    p = out.ctypes.data_as(C.c_void_p)
    for x0, y0, w, h in [(0, 0, W + 1, 1), (0, 0, 1, H + 1), (W, 0, 1, 1), (1, H - 1, W, 2),
                         (2 ** 32 - 1, 0, 2, 1)]:
        assert L.ndt2d_occmap_read(m, x0, y0, w, h, p, W + 1) == _capi.ERR_INVALID
        assert L.ndt2d_occmap_last_error(m)
    assert L.ndt2d_occmap_read(m, 0, 0, 4, 2, p, 3) == _capi.ERR_INVALID
    assert L.ndt2d_occmap_read(m, 0, 0, 4, 2, None, 4) == _capi.ERR_INVALID
    assert np.array_equal(om.getMsg(scans)["data"], whole) and om.last_mode == "UNCHANGED"


def test_refusals_leave_the_object_usable(device):
    L = _capi.lib()
    m = C.c_void_p()
    h = device.device_handle
    # creation
    assert L.ndt2d_occmap_create(h, 0.1, 0.25, None) == _capi.ERR_INVALID
    assert L.ndt2d_occmap_create(None, 0.1, 0.25, C.byref(m)) == _capi.ERR_INVALID and not m.value
    for bad in (0.0, -0.1, float("nan")):
        assert L.ndt2d_occmap_create(h, bad, 0.25, C.byref(m)) == _capi.ERR_INVALID and not m.value
    # NULL objects
    res = _capi.OccmapResult()
    n = C.c_size_t(0)
    b = np.zeros(4)
    assert L.ndt2d_occmap_destroy(None) == _capi.ERR_INVALID
    assert L.ndt2d_occmap_reset(None) == _capi.ERR_INVALID
    assert L.ndt2d_occmap_append_scan(None, None, 0, None) == _capi.ERR_INVALID
    assert L.ndt2d_occmap_scan_count(None, C.byref(n)) == _capi.ERR_INVALID
    assert L.ndt2d_occmap_update(None, None, 0, C.byref(res)) == _capi.ERR_INVALID
    assert L.ndt2d_occmap_read(None, 0, 0, 0, 0, None, 0) == _capi.ERR_INVALID
    assert L.ndt2d_occmap_bounds(None, _capi.dptr(b), C.byref(n)) == _capi.ERR_INVALID

    L, m = _raw(device)
    try:
        def refused(rc):
            assert rc == _capi.ERR_INVALID, rc
            assert L.ndt2d_occmap_last_error(m)

        scans = EDGE_CASES["empty_in_the_middle"][1]
        ref = O.OccupancyGrid(0.1, 0.25)
        out = np.zeros(16, dtype=np.int8)
        assert L.ndt2d_occmap_read(m, 0, 0, 1, 1, out.ctypes.data_as(C.c_void_p), 1) == _capi.ERR_STATE
        refused(L.ndt2d_occmap_append_scan(m, None, 3, None))
        refused(L.ndt2d_occmap_scan_count(m, None))
        refused(L.ndt2d_occmap_bounds(m, None, C.byref(n)))
        refused(L.ndt2d_occmap_bounds(m, _capi.dptr(b), None))
        ids = []
        for _, pts in scans[:4]:
            sid = C.c_size_t(99)
            p = np.ascontiguousarray(pts, dtype=np.float64)
            assert L.ndt2d_occmap_append_scan(m, _capi.dptr(p), len(p), C.byref(sid)) == _capi.OK
            ids.append(sid.value)
        assert ids == [0, 1, 2, 3]
        assert L.ndt2d_occmap_scan_count(m, C.byref(n)) == _capi.OK and n.value == 4
        poses = np.ascontiguousarray([s[0] for s in scans], dtype=np.float64)
        refused(L.ndt2d_occmap_update(m, _capi.dptr(poses), 4, None))
        refused(L.ndt2d_occmap_update(m, None, 4, C.byref(res)))
        refused(L.ndt2d_occmap_update(m, _capi.dptr(poses), 5, C.byref(res)))     # above the appended count
        assert L.ndt2d_occmap_update(m, _capi.dptr(poses), 4, C.byref(res)) == _capi.OK
        assert res.mode == _capi.OCCMAP_FULL
        refused(L.ndt2d_occmap_update(m, _capi.dptr(poses), 3, C.byref(res)))     # below the last update's
        refused(L.ndt2d_occmap_update(m, _capi.dptr(poses), 0, C.byref(res)))

        def whole():
            data = np.zeros((res.info.height, res.info.width), dtype=np.int8)
            assert L.ndt2d_occmap_read(m, 0, 0, res.info.width, res.info.height,
                                       data.ctypes.data_as(C.c_void_p), res.info.width) == _capi.OK
            return data

        # still usable: the same update again changes nothing, and the map is the oracle's
        assert L.ndt2d_occmap_update(m, _capi.dptr(poses), 4, C.byref(res)) == _capi.OK
        assert res.mode == _capi.OCCMAP_UNCHANGED
        want = ref.getMsg(scans[:4])
        assert np.array_equal(whole(), want["data"])
        # degenerate extent: a point 10^12 m away makes a map no message can hold
        bad = np.array([[1e12, 0.0]])
        assert L.ndt2d_occmap_append_scan(m, _capi.dptr(bad), 1, None) == _capi.OK
        refused(L.ndt2d_occmap_update(m, _capi.dptr(poses), 5, C.byref(res)))
        # the object keeps the state it had
        assert L.ndt2d_occmap_bounds(m, _capi.dptr(b), C.byref(n)) == _capi.OK
        assert n.value == 4 and np.array_equal(b, ref.bounds)
        assert L.ndt2d_occmap_update(m, _capi.dptr(poses), 4, C.byref(res)) == _capi.OK
        assert res.mode == _capi.OCCMAP_UNCHANGED
        assert np.array_equal(whole(), want["data"])
        # refused again with other old poses, then the old ones: the counters are still those of
        # the old poses, the scan table is made again
        poses2 = poses.copy()
        poses2[0, 0] += 0.5
        refused(L.ndt2d_occmap_update(m, _capi.dptr(poses2), 5, C.byref(res)))
        assert L.ndt2d_occmap_update(m, _capi.dptr(poses), 4, C.byref(res)) == _capi.OK
        assert res.mode == _capi.OCCMAP_UNCHANGED
        assert L.ndt2d_occmap_update(m, _capi.dptr(poses2), 4, C.byref(res)) == _capi.OK
        assert res.mode == _capi.OCCMAP_FULL
        moved = [(tuple(poses2[k]), scans[k][1]) for k in range(4)]
        assert np.array_equal(whole(), ref.getMsg(moved)["data"])
        # and after a reset it is a new generator
        assert L.ndt2d_occmap_reset(m) == _capi.OK
        assert L.ndt2d_occmap_scan_count(m, C.byref(n)) == _capi.OK and n.value == 0
        assert L.ndt2d_occmap_bounds(m, _capi.dptr(b), C.byref(n)) == _capi.OK
        assert n.value == 0 and np.array_equal(b, np.zeros(4))
    finally:
        assert L.ndt2d_occmap_destroy(m) == _capi.OK

    # the Python mirror: a seen scan that changes its point count is refused, reset() recovers
    om = OccupancyMap(0.1, 0.25, device)
    om.getMsg(scans[:4])
    changed = list(scans[:4])
    changed[0] = (changed[0][0], changed[0][1][:2])
    with pytest.raises(ValueError, match="reset"):
        om.getMsg(changed)
    om.reset()
    _same(om.getMsg(changed), O.OccupancyGrid(0.1, 0.25).getMsg(changed))
    with pytest.raises(_capi.Ndt2dError):
        OccupancyMap(0.0, 0.25, device)


def test_runs_on_a_caller_owned_stream(device):
    import torch
    scans = synth.map_scans(1)
    plain = OccupancyMap(0.05, 0.25, device)
    want = [plain.getMsg(scans[:k]) for k in (3, 4, 9)]
    stream = torch.cuda.Stream()
    om = OccupancyMap(0.05, 0.25, device)
    got = [om.getMsg(scans[:3])]            # on the context's own stream
    device.set_stream(stream.cuda_stream)
    try:
        got.append(om.getMsg(scans[:4]))    # the object follows the context to the caller's stream
        got.append(om.getMsg(scans))
        other = OccupancyMap(0.05, 0.25, device)
        _same(other.getMsg(scans), want[2])
    finally:
        device.set_stream(None)
    for g, w in zip(got, want):
        _same(g, w)
    _same(om.getMsg(scans), want[2])
    assert om.last_mode == "UNCHANGED"
