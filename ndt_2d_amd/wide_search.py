"""Wide search (include/ndt2d_hip.h, "wide search"): the winner of an exhaustive (x, y, theta)
lattice -- its score bits, its index, its near-tie mark -- found by scoring only the tiles of the
translation lattice whose rigorous upper bound can still hold it.  ScanMatcherNDT.matchWide is
built on the matcher's own object; WideSearch is the device object on its own, for callers that
bring their beams and offsets (and for the tests, which compare it with ndt2d_starts_match).
"""
import ctypes as C
import weakref

import numpy as np

from . import _capi
from ._capi import Ndt2dError, dptr


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.reshape(shape) if shape is not None else a


class WideSearch:
    """ndt2d_wide on the device context of `device` (an ndt_2d_amd.ScanMatcherNDT, which must
    outlive it).  It reads the grid installed in that context at the time of each call."""

    def __init__(self, device, max_tiles=1 << 16):
        self._L = _capi.lib()
        self._w = None
        self._device = device
        w = C.c_void_p()
        rc = self._L.ndt2d_wide_create(device.device_handle, int(max_tiles), C.byref(w))
        if rc != _capi.OK:
            raise Ndt2dError(rc, "ndt2d_wide_create")
        self._w = w
        if not hasattr(device, "_seeders"):
            device._seeders = weakref.WeakSet()
        device._seeders.add(self)     # (the matcher's list of objects closed before its context is destroyed)

    def close(self):
        if getattr(self, "_w", None):
            self._L.ndt2d_wide_destroy(self._w)
            self._w = None
        self._device = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, where):
        if rc != _capi.OK:
            msg = self._L.ndt2d_wide_last_error(self._w)
            raise Ndt2dError(rc, where, msg.decode() if msg else "")

    def set_tile(self, tile_steps=None, pixels_per_tile=None):
        t, p = self.tile()
        self._check(self._L.ndt2d_wide_set_tile(self._w, int(t if tile_steps is None else tile_steps),
                                                int(p if pixels_per_tile is None else pixels_per_tile)),
                    "ndt2d_wide_set_tile")

    def tile(self):
        """(tile_steps, pixels_per_tile)."""
        t, p = C.c_uint32(0), C.c_uint32(0)
        self._check(self._L.ndt2d_wide_tile(self._w, C.byref(t), C.byref(p)), "ndt2d_wide_tile")
        return t.value, p.value

    def match(self, pose, beams, dth, dlin, reuse_image=False, want_bounds=False):
        """Returns dict(best_score, best_index (-1: none), near_tie, record, tiles_scored,
        tiles_total[, bounds, evaluated]): `record` is the raw {best_score, best_index (+ 0.5: near
        tie)} pair, bounds / evaluated are per tile job [n_th, n_tiles, n_tiles]."""
        sp, b = _f64(pose, (3,)), _f64(beams, (-1, 2))
        th, lin = _f64(dth, (-1,)), _f64(dlin, (-1,))
        t = self.tile()[0]
        n_tiles = (len(lin) + t - 1) // t
        record = np.zeros(2)
        stats = (C.c_uint64 * 2)(0, 0)
        bounds = np.zeros((len(th), n_tiles, n_tiles)) if want_bounds else None
        evaluated = np.zeros((len(th), n_tiles, n_tiles), dtype=np.uint8) if want_bounds else None
        self._check(self._L.ndt2d_wide_match(
            self._w, dptr(sp), dptr(b), len(b), dptr(th), len(th), dptr(lin), len(lin), 1 if reuse_image else 0,
            dptr(record), stats, dptr(bounds) if want_bounds else None,
            evaluated.ctypes.data_as(C.POINTER(C.c_uint8)) if want_bounds else None), "ndt2d_wide_match")
        index = float(record[1])
        return dict(best_score=float(record[0]), best_index=int(np.floor(index)) if index >= 0.0 else -1,
                    near_tie=bool(index >= 0.0 and index != np.floor(index)), record=record,
                    tiles_scored=int(stats[0]), tiles_total=int(stats[1]), bounds=bounds, evaluated=evaluated)

    def read_image(self):
        """(info, data): info = dict(nx, ny, origin_x, origin_y, pitch, window, guard) of the last
        image made, data = its values [ny, nx]."""
        raw = np.zeros(8)
        self._check(self._L.ndt2d_wide_read_image(self._w, dptr(raw), None, 0), "ndt2d_wide_read_image")
        nx, ny = int(raw[0]), int(raw[1])
        data = np.zeros((ny, nx))
        self._check(self._L.ndt2d_wide_read_image(self._w, dptr(raw), dptr(data), data.size), "ndt2d_wide_read_image")
        info = dict(nx=nx, ny=ny, origin_x=float(raw[2]), origin_y=float(raw[3]), pitch=float(raw[4]),
                    window=float(raw[5]), guard=float(raw[6]))
        return info, data

    def set_timing(self, enabled):
        self._check(self._L.ndt2d_wide_set_timing(self._w, 1 if enabled else 0), "ndt2d_wide_set_timing")

    def last_ms(self):
        """(image, bounds, sort, exact rounds) of the last timed match, in ms."""
        v = [C.c_float(0.0) for _ in range(4)]
        self._check(self._L.ndt2d_wide_last_ms(self._w, *[C.byref(x) for x in v]), "ndt2d_wide_last_ms")
        return tuple(x.value for x in v)
