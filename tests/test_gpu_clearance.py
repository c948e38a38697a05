"""The clearance map on the device (csrc/clearance/ndt2d_clearance.hip; ClearanceMap) against the
numpy yardstick (tests/clearance_restatement.py, itself pinned by tests/test_clearance_restatement.py)
-- never against the device code itself.  d2 is uint32 and the mask int8: everything is compared with
np.array_equal, there is no tolerance.

The boundaries of the kernels: a strip of the column pass is 64 rows (1030 rows: 17 strips, the last
of 6 rows; 65 rows: two strips), a workgroup is 256 threads over consecutive columns (widths 63, 64,
65, 257, 300), the row pass holds a whole row in LDS (no segments: the widest row, 32,768 cells, is
the one further size it has) and scans outwards up to the distance it finds (300 x 300 at 0.0002:
over a hundred steps)."""
import ctypes as C
import functools

import numpy as np
import pytest

import clearance_restatement as R
from ndt_2d_amd import ClearanceMap, OccupancyMap, ScanMatcherNDT, _capi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def device():
    m = ScanMatcherNDT(0)
    m.initialize("clearance", **synth.matcher_params(1))
    m.addScans(synth.map_scans(1))
    return m


@pytest.fixture(scope="module")
def clearance(device):
    """One object for the whole module, so that every transform also runs in buffers that other
    sizes have used before it."""
    c = ClearanceMap(device)
    yield c
    c.close()


def _placed(height, width, cells, value=100):
    grid = np.zeros((height, width), dtype=np.int8)
    for y, x in cells:
        grid[y, x] = value
    return grid


def _stray():
    grid = R.random_map(9, 70, 21, 0.0)
    rng = np.random.default_rng(22)
    at = rng.random(grid.shape) < 0.03
    grid[at] = rng.choice(np.array([1, 50, -2, 99], dtype=np.int8), size=int(at.sum()))
    return grid


CASES = dict(R.SHAPES)
CASES.update({
    "1x1 unknown": lambda: np.full((1, 1), -1, dtype=np.int8),
    "only obstacle in the last cell": lambda: _placed(6, 71, [(5, 70)]),
    "only obstacle in the first cell": lambda: _placed(70, 6, [(0, 0)]),
    "obstacles in the four corners": lambda: _placed(67, 130, [(0, 0), (0, 129), (66, 0), (66, 129)]),
    "equidistant obstacles": lambda: _placed(21, 41, [(10, 4), (10, 36), (2, 20), (18, 20)]),
    "no obstacle": lambda: np.zeros((37, 41), dtype=np.int8),
    "no obstacle but unknown cells": lambda: _placed(70, 9, [(3, 3), (68, 8)], value=-1),
    "all obstacles": lambda: np.full((37, 41), 100, dtype=np.int8),
    "stray bytes": _stray,
})


@functools.lru_cache(maxsize=None)
def case(name):
    grid = CASES[name]()
    grid.setflags(write=False)
    return grid


@functools.lru_cache(maxsize=None)
def yardstick(name, unknown=False, cap=0):
    out = R.d2_separable(case(name), unknown, cap)
    out.setflags(write=False)
    return out


def on_device(torch, grid):
    d = torch.from_numpy(np.array(grid, copy=True)).cuda()
    torch.cuda.synchronize()
    return d


# ---- 1. the transform ----------------------------------------------------------------------------

@pytest.mark.parametrize("unknown", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_d2_is_the_yardsticks(torch, clearance, name, unknown):
    grid = case(name)
    want = yardstick(name, unknown)
    clearance.compute(grid, unknown_is_obstacle=unknown)
    got = clearance.d2()
    assert got.dtype == np.uint32 and got.shape == grid.shape and np.array_equal(got, want)
    # a device map gives the same bits, and so does the same call again
    d = on_device(torch, grid)
    clearance.compute_device(d.data_ptr(), grid.shape[1], grid.shape[0], unknown_is_obstacle=unknown)
    assert np.array_equal(clearance.d2(), want)
    clearance.compute_device(d.data_ptr(), grid.shape[1], grid.shape[0], unknown_is_obstacle=unknown)
    assert np.array_equal(clearance.d2(), want)
    # the resident d2 is what read copies
    ptr, w, h = clearance.device_d2()
    assert ptr and (w, h) == (grid.shape[1], grid.shape[0])
    if name == "no obstacle":
        assert np.all(got == _capi.CLEARANCE_FAR)
    if name == "no obstacle but unknown cells":
        assert np.all(got == _capi.CLEARANCE_FAR) != unknown and (got == 0).sum() == (2 if unknown else 0)
    if name == "all obstacles":
        assert not got.any()


def test_the_widest_row_and_the_largest_columns(torch, clearance):
    """32,768 cells a side, the largest the contract takes: the row of 64 KB in LDS with its only
    obstacle 32,767 columns away, and a column whose nearest obstacle is 32,767 rows (512 strips)
    away.  A single obstacle: d2 = dx^2 + dy^2 in closed form."""
    side = 32768
    wide = _placed(2, side, [(1, 0)])
    xs = np.arange(side, dtype=np.int64)
    clearance.compute(wide)
    got = clearance.d2()
    assert np.array_equal(got[1], (xs * xs).astype(np.uint32)) and np.array_equal(got[0], (xs * xs + 1).astype(np.uint32))
    tall = _placed(side, 3, [(side - 1, 2)])
    clearance.compute(tall)
    got = clearance.d2()
    ys = (side - 1 - xs)
    for x in range(3):
        assert np.array_equal(got[:, x], (ys * ys + (2 - x) ** 2).astype(np.uint32))
    assert int(got.max()) == 32767 * 32767 + 4


# ---- 2. caps ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["9x257", "1030x70", "300x300 dense", "300x300 sparse", "equidistant obstacles"])
def test_caps_keep_every_cell_within_them_exact(clearance, name):
    grid = case(name)
    exact = yardstick(name)
    largest = int(np.ceil(np.sqrt(float(exact[exact != R.FAR].max()))))
    for cap in (1, 5, largest):
        want = yardstick(name, False, cap)
        clearance.compute(grid, max_cells=cap)
        got = clearance.d2()
        assert np.array_equal(got, want), cap
        within = exact.astype(np.int64) <= cap * cap
        assert np.array_equal(got[within], exact[within]) and np.all(got[~within] == R.FAR)
    assert np.array_equal(yardstick(name, False, largest), exact)          # the cap that removes nothing


def test_cap_equality_is_exact_and_one_more_is_far(clearance):
    # 3-4-5: at R = 5 the cell at offset (3, 4) keeps its 25, the cell at offset (1, 5) (26) is FAR
    grid = _placed(20, 20, [(8, 8)])
    clearance.compute(grid, max_cells=5)
    got = clearance.d2()
    assert got[12, 11] == 25 and got[11, 12] == 25 and got[13, 8] == 25 and got[8, 13] == 25
    assert got[13, 9] == R.FAR and got[9, 13] == R.FAR and got[8, 14] == R.FAR
    assert np.array_equal(got, R.d2_separable(grid, False, 5))
    # a cap beyond every distance a map can hold is no cap
    for cap in (46340, 46341, 2 ** 40):
        clearance.compute(grid, max_cells=cap)
        assert np.array_equal(clearance.d2(), R.d2_separable(grid))


# ---- 3. a resident map, rectangles, buffers -----------------------------------------------------------

def test_resident_map_against_its_own_read(device, clearance):
    occ = OccupancyMap(0.05, 0.25, device)
    msg = occ.getMsg(synth.map_scans(1))
    grid = msg["data"]
    assert set(np.unique(grid).tolist()) == {-1, 0, 100}
    for unknown in (False, True):
        info = clearance.compute_occupancy_map(occ, unknown_is_obstacle=unknown)
        assert (info.width, info.height) == (msg["width"], msg["height"])
        resident = clearance.d2()
        assert np.array_equal(resident, R.d2_separable(grid, unknown))
        clearance.compute(grid, unknown_is_obstacle=unknown)
        assert np.array_equal(clearance.d2(), resident)
    # metres: sqrt(d2) * resolution, inf for FAR
    clearance.compute(grid, max_cells=6)
    d2 = clearance.d2()
    metres = clearance.distance(0.05)
    far = d2 == R.FAR
    assert far.any() and np.all(np.isinf(metres[far]))
    assert np.array_equal(metres[~far], np.sqrt(d2[~far].astype(np.float64)) * 0.05)
    occ.close()


def test_rectangles_and_buffer_growth(clearance):
    small, large = case("7x63"), case("300x300 dense")
    for name in ("7x63", "300x300 dense", "7x63", "1030x70", "1x1 obstacle", "300x300 sparse"):
        clearance.compute(case(name))
        assert np.array_equal(clearance.d2(), yardstick(name)), name
    clearance.compute(large)
    want = yardstick("300x300 dense")
    for rect in ((0, 0, 300, 300), (0, 0, 1, 1), (299, 299, 1, 1), (17, 250, 283, 50), (64, 0, 65, 300), (5, 7, 0, 3)):
        x0, y0, w, h = rect
        got = clearance.d2(rect)
        assert got.shape == (h, w) and np.array_equal(got, want[y0:y0 + h, x0:x0 + w]), rect
    # a row stride above w leaves the cells between the rows alone
    out = np.full((4, 10), 7, dtype=np.uint32)
    rc = _capi.lib().ndt2d_clearance_read(clearance._c, 100, 200, 6, 4, out.ctypes.data_as(C.c_void_p), 10)
    assert rc == _capi.OK and np.array_equal(out[:, :6], want[200:204, 100:106]) and np.all(out[:, 6:] == 7)
    assert small.shape == (7, 63)


# ---- 4. the mask -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["300x300 dense", "stray bytes", "9x257", "no obstacle", "all obstacles"])
def test_mask_is_the_yardsticks(torch, clearance, name):
    grid = case(name)
    d2 = yardstick(name)
    clearance.compute(grid)
    for threshold in (0, 1, 2, 25, 26, 2 ** 31, R.FAR):
        ptr = clearance.mask(min_d2=threshold)
        assert ptr
        got = clearance.inflated()
        assert got.dtype == np.int8 and np.array_equal(got, R.mask(grid, d2, threshold)), threshold
        assert np.array_equal(got[grid != 0], grid[grid != 0])          # non-free bytes are untouched
        if threshold == 0:
            assert np.array_equal(got, grid)                            # the map itself
    # the threshold in metres: 0.25 m at 0.05 m is 25
    clearance.mask(min_clearance=0.25, resolution=0.05)
    assert np.array_equal(clearance.inflated(), R.mask(grid, d2, 25))
    assert np.array_equal(clearance.inflated((3, 2, 5, 4)), R.mask(grid, d2, 25)[2:6, 3:8])
    # the transform is still there after a mask
    assert np.array_equal(clearance.d2(), d2)


def test_mask_threshold_equality(clearance):
    grid = _placed(20, 20, [(8, 8)])
    clearance.compute(grid)
    clearance.mask(min_d2=25)
    kept = clearance.inflated()
    assert kept[12, 11] == 0 and kept[13, 8] == 0 and kept[12, 10] == 99 and kept[8, 8] == 100
    clearance.mask(min_d2=26)
    dropped = clearance.inflated()
    assert dropped[12, 11] == 99 and dropped[13, 8] == 99 and dropped[13, 9] == 0
    # under a cap the far cells have every clearance the cap allows
    clearance.compute(grid, max_cells=5)
    clearance.mask(min_clearance=0.25, resolution=0.05)
    assert np.array_equal(clearance.inflated(), R.mask(grid, R.d2_separable(grid), 25))
    with pytest.raises(_capi.Ndt2dError) as ei:
        clearance.mask(min_clearance=0.3, resolution=0.05)             # 36 > 5 * 5
    assert ei.value.code == _capi.ERR_INVALID


# ---- 5. refusals ---------------------------------------------------------------------------------------

def test_refusals_leave_the_earlier_result_readable(torch, device):
    L = _capi.lib()
    h = device.device_handle
    c = C.c_void_p()
    assert L.ndt2d_clearance_create(h, None) == _capi.ERR_INVALID
    assert L.ndt2d_clearance_create(None, C.byref(c)) == _capi.ERR_INVALID and not c.value
    grid = case("7x63")
    p = grid.ctypes.data_as(C.c_void_p)
    ms, u, vp = C.c_float(0.0), C.c_uint32(0), C.c_void_p()
    for rc in (L.ndt2d_clearance_destroy(None), L.ndt2d_clearance_compute(None, p, 63, 7, 0, 0),
               L.ndt2d_clearance_compute_device(None, p, 63, 7, 0, 0), L.ndt2d_clearance_read(None, 0, 0, 1, 1, p, 1),
               L.ndt2d_clearance_device(None, C.byref(vp), C.byref(u), C.byref(u)), L.ndt2d_clearance_mask(None, 1, C.byref(vp)),
               L.ndt2d_clearance_read_mask(None, 0, 0, 1, 1, p, 1), L.ndt2d_clearance_set_timing(None, 1),
               L.ndt2d_clearance_last_ms(None, C.byref(ms), C.byref(ms))):
        assert rc == _capi.ERR_INVALID
    assert L.ndt2d_clearance_last_error(None) == b""

    cm = ClearanceMap(device)

    def refused(call, code, text):
        with pytest.raises(_capi.Ndt2dError) as ei:
            call()
        assert ei.value.code == code and text in str(ei.value), str(ei.value)

    # nothing computed yet
    refused(lambda: cm.d2((0, 0, 1, 1)), _capi.ERR_STATE, "no transform")
    refused(lambda: cm.device_d2(), _capi.ERR_STATE, "no transform")
    refused(lambda: cm.mask(min_d2=4), _capi.ERR_STATE, "no transform")
    refused(lambda: cm.inflated((0, 0, 1, 1)), _capi.ERR_STATE, "no mask")
    refused(lambda: cm.last_ms(), _capi.ERR_STATE, "no timed launch")

    cm.compute(grid)
    want = yardstick("7x63")
    refused(lambda: cm.inflated(), _capi.ERR_STATE, "no mask")
    cm.mask(min_d2=9)
    want_mask = R.mask(grid, want, 9)
    d = on_device(torch, grid)
    other = np.full((3, 4), 100, dtype=np.int8)
    for form in ("host", "device"):
        fn = L.ndt2d_clearance_compute if form == "host" else L.ndt2d_clearance_compute_device
        ptr = other.ctypes.data_as(C.c_void_p) if form == "host" else d.data_ptr()
        for args, word in (((None, 4, 3, 0, 0), "null map"), ((ptr, 0, 3, 0, 0), "zero"), ((ptr, 4, 0, 0, 0), "zero"),
                           ((ptr, 32769, 3, 0, 0), "32768"), ((ptr, 4, 32769, 0, 0), "32768"),
                           ((ptr, 0xffffffff, 0xffffffff, 0, 0), "32768"), ((ptr, 4, 3, 0, -1), "max_cells"),
                           ((ptr, 4, 3, 1, -(2 ** 62)), "max_cells")):
            rc = fn(cm._c, *args)
            assert rc == _capi.ERR_INVALID and word in L.ndt2d_clearance_last_error(cm._c).decode(), (form, args)
            # the transform and the mask are those of the accepted map
            assert (cm.width, cm.height) == (63, 7)
            assert np.array_equal(cm.d2(), want) and np.array_equal(cm.inflated(), want_mask)
    for rect in ((60, 0, 4, 1), (0, 6, 1, 2), (0xffffffff, 0, 2, 1), (64, 0, 0, 0)):
        refused(lambda: cm.d2(rect), _capi.ERR_INVALID, "rectangle")
        refused(lambda: cm.inflated(rect), _capi.ERR_INVALID, "rectangle")
    out = np.zeros((2, 2), dtype=np.uint32)
    assert L.ndt2d_clearance_read(cm._c, 0, 0, 2, 2, None, 2) == _capi.ERR_INVALID
    assert L.ndt2d_clearance_read(cm._c, 0, 0, 2, 2, out.ctypes.data_as(C.c_void_p), 1) == _capi.ERR_INVALID
    assert "row stride" in L.ndt2d_clearance_last_error(cm._c).decode() and not out.any()
    assert L.ndt2d_clearance_read_mask(cm._c, 0, 0, 2, 2, None, 2) == _capi.ERR_INVALID
    assert L.ndt2d_clearance_mask(cm._c, 4, None) == _capi.ERR_INVALID
    assert L.ndt2d_clearance_device(cm._c, None, C.byref(u), C.byref(u)) == _capi.ERR_INVALID
    assert L.ndt2d_clearance_last_ms(cm._c, None, C.byref(ms)) == _capi.ERR_INVALID
    with pytest.raises(ValueError):
        cm.compute(np.zeros((2, 2, 2), dtype=np.int8))
    with pytest.raises(ValueError):
        cm.compute(np.full((2, 2), 256))                                 # would wrap to 0 as int8
    with pytest.raises(ValueError):
        cm.mask()
    assert np.array_equal(cm.d2(), want) and np.array_equal(cm.inflated(), want_mask)
    # a new transform forgets the mask of the earlier one
    cm.compute(grid, max_cells=2)
    refused(lambda: cm.inflated(), _capi.ERR_STATE, "no mask")
    # the timer
    cm.set_timing(True)
    cm.compute(grid)
    transform_ms, mask_ms = cm.last_ms()
    assert transform_ms > 0.0 and mask_ms == 0.0
    cm.mask(min_d2=9)
    transform_ms, mask_ms = cm.last_ms()
    assert transform_ms > 0.0 and mask_ms > 0.0
    cm.set_timing(False)
    refused(lambda: cm.last_ms(), _capi.ERR_STATE, "no timed launch")
    cm.close()
