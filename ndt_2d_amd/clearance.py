"""The clearance map (include/ndt2d_hip.h, "Clearance map"): for every cell of an int8 occupancy map
the exact squared Euclidean distance in cells to the nearest obstacle, on the GPU, and the map with
the free cells nearer than a threshold marked 99 ("inscribed").  Seeder.set_map(min_clearance=...)
and ParticleFilter.init_global(min_clearance=...) are built on it; on its own it gives the distance
field and the inflated map a planner takes.

The transform is exact and its cost per cell grows with the distance it finds (an outward scan of
sqrt(d2) steps): on a map with wide open areas pass max_cells, the largest radius of interest in
cells, and every cell beyond it is reported as CLEARANCE_FAR after at most that many steps.
Measured (profiles/clearance_timing*.json, one MI355X): the uncapped transform takes longer than
the init_global it serves -- 0.047 against 0.041 ms on cfg-5's 772 x 772 map, 0.47 against 0.19 ms
on the same world at 0.05 m -- and capped at 0.5 m it does not (0.041 and 0.17 ms).  A caller who
only needs the band along the walls should cap; Seeder and ParticleFilter.init_global always do.
"""
import ctypes as C
import weakref

import numpy as np

from . import _capi
from ._capi import CLEARANCE_FAR, Ndt2dError


def min_d2_of(min_clearance, resolution, max_cells=0):
    """ceil((min_clearance / resolution)^2) as the library computes it (host arithmetic only)."""
    out = C.c_uint32(0)
    rc = _capi.lib().ndt2d_clearance_min_d2(float(min_clearance), float(resolution), int(max_cells), C.byref(out))
    if rc != _capi.OK:
        raise Ndt2dError(rc, "ndt2d_clearance_min_d2",
                         "clearance %r m at resolution %r m, max_cells %r" % (min_clearance, resolution, max_cells))
    return out.value


class ClearanceMap:
    """ndt2d_clearance on the device context of `device` (an ndt_2d_amd.ScanMatcherNDT, which must
    outlive it).  Launches go to the stream that context is bound to."""

    def __init__(self, device):
        self._L = _capi.lib()
        self._c = None
        self._device = device
        c = C.c_void_p()
        rc = self._L.ndt2d_clearance_create(device.device_handle, C.byref(c))
        if rc != _capi.OK:
            raise Ndt2dError(rc, "ndt2d_clearance_create")
        self._c = c
        if not hasattr(device, "_seeders"):
            device._seeders = weakref.WeakSet()
        device._seeders.add(self)     # closed before the context is destroyed, as a Seeder is
        self.width = self.height = 0
        self.max_cells = 0

    def close(self):
        if getattr(self, "_c", None):
            self._L.ndt2d_clearance_destroy(self._c)
            self._c = None
        self._device = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, where):
        if rc != _capi.OK:
            msg = self._L.ndt2d_clearance_last_error(self._c)
            raise Ndt2dError(rc, where, msg.decode() if msg else "")

    def compute(self, grid, unknown_is_obstacle=False, max_cells=0):
        """grid: HOST int8 [height, width].  max_cells = R > 0: cells farther than R are CLEARANCE_FAR."""
        g = np.ascontiguousarray(grid, dtype=np.int8)
        if g.ndim != 2 or not np.array_equal(g, grid):     # (a value that does not fit int8 could wrap to 0)
            raise ValueError("the map must be a 2-D array [height, width] of int8 values")
        h, w = g.shape
        self._check(self._L.ndt2d_clearance_compute(self._c, g.ctypes.data_as(C.c_void_p), w, h,
                                                    1 if unknown_is_obstacle else 0, int(max_cells)),
                    "ndt2d_clearance_compute")
        self.width, self.height, self.max_cells = w, h, int(max_cells)

    def compute_device(self, map_ptr, width, height, unknown_is_obstacle=False, max_cells=0):
        """The same from a DEVICE int8 map [height][width]."""
        self._check(self._L.ndt2d_clearance_compute_device(self._c, map_ptr, int(width), int(height),
                                                           1 if unknown_is_obstacle else 0, int(max_cells)),
                    "ndt2d_clearance_compute_device")
        self.width, self.height, self.max_cells = int(width), int(height), int(max_cells)

    def compute_occupancy_map(self, occupancy_map, unknown_is_obstacle=False, max_cells=0):
        """The resident map of an OccupancyMap's last getMsg: nothing is uploaded.  Returns its
        ndt2d_occupancy_info."""
        ptr, info = occupancy_map.device_map()
        self.compute_device(ptr, info.width, info.height, unknown_is_obstacle, max_cells)
        return info

    def _rect(self, rect):
        if rect is None:
            return 0, 0, self.width, self.height
        r = [int(v) for v in rect]
        if len(r) != 4 or min(r) < 0 or max(r) > 0xffffffff:
            raise ValueError("rect must be (x0, y0, w, h) in cells")
        return r

    def d2(self, rect=None):
        """uint32 [h, w]: the squared distances of the whole map, or of rect = (x0, y0, w, h)."""
        x0, y0, w, h = self._rect(rect)
        out = np.empty((h, w), dtype=np.uint32)
        self._check(self._L.ndt2d_clearance_read(self._c, x0, y0, w, h, out.ctypes.data_as(C.c_void_p), max(w, 1)),
                    "ndt2d_clearance_read")
        return out

    def distance(self, resolution):
        """float64 [height, width] in metres: sqrt(d2) * resolution, inf where d2 is CLEARANCE_FAR."""
        d2 = self.d2()
        out = np.sqrt(d2.astype(np.float64)) * np.float64(resolution)
        out[d2 == CLEARANCE_FAR] = np.inf
        return out

    def device_d2(self):
        """(DEVICE pointer of the resident uint32 d2, width, height); read-only."""
        p, w, h = C.c_void_p(), C.c_uint32(0), C.c_uint32(0)
        self._check(self._L.ndt2d_clearance_device(self._c, C.byref(p), C.byref(w), C.byref(h)),
                    "ndt2d_clearance_device")
        return p.value, w.value, h.value

    def mask(self, min_clearance=None, resolution=None, min_d2=None):
        """The object's own DEVICE int8 map in which every free cell with d2 < min_d2 is 99; returns
        its pointer.  Either min_d2 (an integer, in cells squared) or min_clearance with resolution
        (both in metres)."""
        if (min_d2 is None) == (min_clearance is None):
            raise ValueError("mask takes either min_d2 or min_clearance with resolution")
        if min_d2 is None:
            if resolution is None:
                raise ValueError("min_clearance needs the resolution")
            min_d2 = min_d2_of(min_clearance, resolution, self.max_cells)
        min_d2 = int(min_d2)
        if not 0 <= min_d2 <= 0xffffffff:
            raise ValueError("min_d2 must fit 32 bits")
        p = C.c_void_p()
        self._check(self._L.ndt2d_clearance_mask(self._c, min_d2, C.byref(p)), "ndt2d_clearance_mask")
        return p.value

    def inflated(self, rect=None):
        """int8 [h, w]: the host copy of the last mask."""
        x0, y0, w, h = self._rect(rect)
        out = np.empty((h, w), dtype=np.int8)
        self._check(self._L.ndt2d_clearance_read_mask(self._c, x0, y0, w, h, out.ctypes.data_as(C.c_void_p),
                                                      max(w, 1)), "ndt2d_clearance_read_mask")
        return out

    def set_timing(self, enabled):
        self._check(self._L.ndt2d_clearance_set_timing(self._c, 1 if enabled else 0), "ndt2d_clearance_set_timing")

    def last_ms(self):
        """(transform, mask) of the last timed calls, in ms."""
        a, b = C.c_float(0.0), C.c_float(0.0)
        self._check(self._L.ndt2d_clearance_last_ms(self._c, C.byref(a), C.byref(b)), "ndt2d_clearance_last_ms")
        return a.value, b.value
