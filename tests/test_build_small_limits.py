"""Host-only parts of the fused small-map build: its limits and the argument refusals that need
no device (no GPU is touched)."""
import ctypes as C

import numpy as np

from ndt_2d_amd import _capi


def _fits(poses, n_points, res=0.25, range_max=10.0):
    p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    return _capi.lib().ndt2d_build_grid_small_fits(res, range_max, _capi.dptr(p), len(p), n_points)


def test_limits_of_the_fused_build():
    n_max = _capi.lib().ndt2d_build_small_max_points()
    assert n_max >= 16384            # ten scans of a 1,440-beam lidar
    one = [(0.0, 0.0, 0.0)]
    assert _fits(one, 0) == 1 and _fits(one, n_max) == 1 and _fits(one, n_max + 1) == 0
    # 217 x 302 = 65,534 cells fit, 255 x 257 = 65,535 do not (the compacted form's uint16 ranks)
    assert _fits([(0.0, 0.0, 0.0), (34.0, 55.25, 0.0)], 100) == 1
    assert _fits([(0.0, 0.0, 0.0), (43.5, 44.0, 0.0)], 100) == 0
    # the mapper's maps: 41 x 41 (range_max 4.75) and 245 x 245 (30 m lidar, poses 0.5 m apart)
    assert _fits([(-0.25, -0.25, 0.0), (0.25, 0.25, 0.0)], 6480, range_max=4.75) == 1
    assert _fits([(0.5, 0.0, 0.0), (1.5, 1.0, 0.0)], 6480, range_max=30.0) == 1


def test_bad_arguments_do_not_fit():
    L = _capi.lib()
    one = np.zeros((1, 3))
    assert L.ndt2d_build_grid_small_fits(0.0, 10.0, _capi.dptr(one), 1, 10) == 0
    assert L.ndt2d_build_grid_small_fits(float("nan"), 10.0, _capi.dptr(one), 1, 10) == 0
    assert L.ndt2d_build_grid_small_fits(0.25, 10.0, None, 1, 10) == 0
    assert L.ndt2d_build_grid_small_fits(0.25, 10.0, _capi.dptr(one), 0, 10) == 0
    assert L.ndt2d_build_grid_small_fits(0.25, float("inf"), _capi.dptr(one), 1, 10) == 0   # degenerate extent


def test_null_handles_are_refused():
    L = _capi.lib()
    one = np.zeros((1, 3))
    pts = np.zeros((4, 2))
    off = (C.c_size_t * 2)(0, 4)
    sid = C.c_size_t(0)
    store = C.c_void_p()
    assert L.ndt2d_build_grid_small(None, 0.25, 2.0, _capi.dptr(one), _capi.dptr(pts), off, 1) == _capi.ERR_INVALID
    assert L.ndt2d_scanstore_create(None, 10, 10, C.byref(store)) == _capi.ERR_INVALID and not store
    assert L.ndt2d_scanstore_append(None, _capi.dptr(pts), 4, C.byref(sid)) == _capi.ERR_INVALID
    assert L.ndt2d_scanstore_count(None, C.byref(sid)) == _capi.ERR_INVALID
    assert L.ndt2d_scanstore_reset(None) == _capi.ERR_INVALID
    assert L.ndt2d_scanstore_build(None, off, _capi.dptr(one), 1, 0.25, 2.0) == _capi.ERR_INVALID
    assert L.ndt2d_scanstore_destroy(None) == _capi.ERR_INVALID
    assert L.ndt2d_scanstore_last_error(None) == b"null scan store"
    assert L.ndt2d_scanstore_set_eigenvalue_form(None, b"eigen") == _capi.ERR_INVALID
    assert L.ndt2d_build_small_set_eigenvalue_form(None, b"eigen") == _capi.ERR_INVALID
    assert L.ndt2d_build_small_release(None) == _capi.ERR_INVALID
    assert L.ndt2d_build_small_last_error(None) == b"null handle"
    assert L.ndt2d_matcher_last_build(None) == b""
    assert L.ndt2d_matcher_store_scan(None, _capi.dptr(pts), 4, C.byref(sid)) == _capi.ERR_INVALID
    assert L.ndt2d_matcher_add_scans_by_id(None, _capi.dptr(one), off, 1) == _capi.ERR_INVALID
    assert L.ndt2d_matcher_drop_scans(None) == _capi.ERR_INVALID
