"""Global localisation's seeder (include/ndt2d_hip.h, "Global localisation"): the free cells of an
occupancy map as a table on the GPU, particles drawn uniformly over them, and the replacement of a
share of a particle set by fresh such particles.  ParticleFilter.init_global / inject
(particle_filter.py) are built on it; it is usable on its own with any DEVICE pose array.
"""
import ctypes as C
import weakref

import numpy as np

from . import _capi
from ._capi import Ndt2dError


def _region4(region):
    if region is None:
        return None
    r = [int(v) for v in region]
    if len(r) != 4 or min(r) < 0 or max(r) > 0xffffffff:
        raise ValueError("region must be (x0, y0, w, h) in cells")
    return (C.c_uint32 * 4)(*r)


class Seeder:
    """ndt2d_seeder on the device context of `device` (an ndt_2d_amd.ScanMatcherNDT, which must
    outlive it).  Launches go to the stream that context is bound to."""

    def __init__(self, device):
        self._L = _capi.lib()
        self._s = None
        self._device = device
        s = C.c_void_p()
        rc = self._L.ndt2d_seed_create(device.device_handle, C.byref(s))
        if rc != _capi.OK:
            raise Ndt2dError(rc, "ndt2d_seed_create")
        self._s = s
        if not hasattr(device, "_seeders"):
            device._seeders = weakref.WeakSet()
        device._seeders.add(self)     # closed before the context is destroyed
        self.width = self.height = 0
        self.origin_x = self.origin_y = self.resolution = 0.0
        self._clearance = None        # a ClearanceMap, made by the first call with min_clearance > 0

    def close(self):
        if getattr(self, "_clearance", None) is not None:
            self._clearance.close()
            self._clearance = None
        if getattr(self, "_s", None):
            self._L.ndt2d_seed_destroy(self._s)
            self._s = None
        self._device = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, where):
        if rc != _capi.OK:
            msg = self._L.ndt2d_seed_last_error(self._s)
            raise Ndt2dError(rc, where, msg.decode() if msg else "")

    def _took(self, width, height, origin_x, origin_y, resolution):
        self.width, self.height = int(width), int(height)
        self.origin_x, self.origin_y, self.resolution = float(origin_x), float(origin_y), float(resolution)

    def _masked(self, compute, resolution, min_clearance, unknown_is_obstacle):
        """The DEVICE map of this seeder's ClearanceMap in which the free cells nearer than
        min_clearance (metres) to an obstacle are no longer byte 0.  compute(clearance_map,
        unknown_is_obstacle, max_cells) runs the transform, capped at the radius the clearance needs:
        the transform then costs at most that many steps a cell, however open the map is."""
        from .clearance import ClearanceMap, min_d2_of
        min_d2 = min_d2_of(min_clearance, resolution)                  # (refuses what is not a clearance)
        cap = int(np.ceil(np.float64(min_clearance) / np.float64(resolution)))   # cap^2 >= min_d2
        if self._clearance is None:
            self._clearance = ClearanceMap(self._device)
        compute(self._clearance, unknown_is_obstacle, cap)
        return self._clearance.mask(min_d2=min_d2)

    def set_map(self, grid, origin_x, origin_y, resolution, region=None, min_clearance=0.0,
                unknown_is_obstacle=False):
        """grid: HOST int8 [height, width], as OccupancyMap.getMsg()["data"]; region = (x0, y0, w, h)
        in cells or None.  Returns the number of free cells.  With min_clearance > 0 (metres) only
        the free cells at least that far from every obstacle of the WHOLE map are kept (obstacles:
        bytes that are neither 0 nor -1, or with unknown_is_obstacle every byte but 0); with 0.0 the
        call is what it was without the argument."""
        if min_clearance != 0.0:
            ptr = self._masked(lambda c, unknown, cap: c.compute(grid, unknown, cap), resolution, min_clearance,
                               unknown_is_obstacle)
            h, w = np.shape(grid)
            return self.set_map_device(ptr, w, h, origin_x, origin_y, resolution, region)
        g = np.ascontiguousarray(grid, dtype=np.int8)
        if g.ndim != 2 or not np.array_equal(g, grid):     # (a value that does not fit int8 could wrap to 0)
            raise ValueError("the map must be a 2-D array [height, width] of int8 values")
        h, w = g.shape
        self._check(self._L.ndt2d_seed_set_map(self._s, g.ctypes.data_as(C.c_void_p), w, h, float(origin_x),
                                               float(origin_y), float(resolution), _region4(region)),
                    "ndt2d_seed_set_map")
        self._took(w, h, origin_x, origin_y, resolution)
        return self.free_count()

    def set_map_device(self, map_ptr, width, height, origin_x, origin_y, resolution, region=None):
        """The same from a DEVICE int8 map [height][width]."""
        self._check(self._L.ndt2d_seed_set_map_device(self._s, map_ptr, int(width), int(height), float(origin_x),
                                                      float(origin_y), float(resolution), _region4(region)),
                    "ndt2d_seed_set_map_device")
        self._took(width, height, origin_x, origin_y, resolution)
        return self.free_count()

    def set_occupancy_map(self, occupancy_map, region=None, min_clearance=0.0, unknown_is_obstacle=False):
        """The resident map of an OccupancyMap's last getMsg: nothing is uploaded.  min_clearance as
        in set_map."""
        ptr, info = occupancy_map.device_map()
        if min_clearance != 0.0:
            source = ptr
            ptr = self._masked(lambda c, unknown, cap: c.compute_device(source, info.width, info.height, unknown, cap),
                               info.resolution, min_clearance, unknown_is_obstacle)
        return self.set_map_device(ptr, info.width, info.height, info.origin_x, info.origin_y, info.resolution,
                                   region)

    def free_count(self):
        n = C.c_size_t(0)
        self._check(self._L.ndt2d_seed_free_count(self._s, C.byref(n)), "ndt2d_seed_free_count")
        return n.value

    def read_table(self):
        """free_cells as uint32 [F] (for tests and tools)."""
        out = np.empty(max(self.free_count(), 1), dtype=np.uint32)
        n = C.c_size_t(0)
        self._check(self._L.ndt2d_seed_read_table(self._s, out.ctypes.data_as(C.POINTER(C.c_uint32)), len(out),
                                                  C.byref(n)), "ndt2d_seed_read_table")
        return out[:n.value].copy()

    def launch(self, poses_ptr, n, seed, step, first_index=0):
        """Asynchronous: n poses into DEVICE double [n][3].  Consumes steps `step` and `step + 1`."""
        self._check(self._L.ndt2d_seed_launch(self._s, poses_ptr, int(n), int(seed), int(step), int(first_index)),
                    "ndt2d_seed_launch")

    def inject_launch(self, poses_ptr, n, probability, seed, step, first_index=0, count_ptr=None):
        """Asynchronous: particle i is replaced by its sample where its inject draw is below
        `probability`; count_ptr = DEVICE uint64 for the number replaced, or None."""
        self._check(self._L.ndt2d_seed_inject_launch(self._s, poses_ptr, int(n), float(probability), int(seed),
                                                     int(step), int(first_index), count_ptr),
                    "ndt2d_seed_inject_launch")

    def set_timing(self, enabled):
        self._check(self._L.ndt2d_seed_set_timing(self._s, 1 if enabled else 0), "ndt2d_seed_set_timing")

    def last_ms(self):
        """(table build, sample or inject launch) of the last timed calls, in ms."""
        a, b = C.c_float(0.0), C.c_float(0.0)
        self._check(self._L.ndt2d_seed_last_ms(self._s, C.byref(a), C.byref(b)), "ndt2d_seed_last_ms")
        return a.value, b.value
