"""ndt_2d::OccupancyGrid for a caller that publishes after every scan.

The same `getMsg(scans)` and the same returned dict as occupancy_grid.OccupancyGrid, over
ndt2d_occupancy_map (include/ndt2d_hip.h): the scans' points, the hit / empty counters and the
int8 map stay on the GPU.  A publish after one more scan uploads that scan, traces its beams
into the counters of the last publish and patches the cells that can have changed into the
array kept here.  Counts are integers, so the map is the one a full re-trace gives.

One object per generator.  A scan's points never change once it has been passed in; a caller
that drops or replaces scans calls reset().
"""
import ctypes as C
import weakref

import numpy as np

from . import _capi
from ._capi import Ndt2dError, dptr
from .scan_matcher import _f64

MODES = {_capi.OCCMAP_FULL: "FULL", _capi.OCCMAP_INCREMENTAL: "INCREMENTAL",
         _capi.OCCMAP_UNCHANGED: "UNCHANGED"}


class OccupancyMap:
    """`device` is an ndt_2d_amd.ScanMatcherNDT (its GPU context is used and must outlive this)."""

    def __init__(self, resolution, occ_thresh, device):
        self.resolution = float(resolution)
        self.occ_thresh = float(occ_thresh)
        self._device = device
        self._L = _capi.lib()
        self._map = None
        m = C.c_void_p()
        rc = self._L.ndt2d_occmap_create(device.device_handle, self.resolution, self.occ_thresh,
                                         C.byref(m))
        if rc != _capi.OK:
            raise Ndt2dError(rc, "ndt2d_occmap_create")
        self._map = m
        if not hasattr(device, "_occupancy_maps"):
            device._occupancy_maps = weakref.WeakSet()
        device._occupancy_maps.add(self)     # closed before the context is destroyed
        self._seen = []                      # point count of every scan appended
        self._poses = np.zeros((0, 3))       # of the last update
        self._data = np.zeros((0, 0), dtype=np.int8)
        self.last_mode = None
        self.last_rect = (0, 0, 0, 0)        # x0, y0, w, h
        self.last_beams_traced = 0
        # bytes moved by the last getMsg: points and poses up, bounds and map cells down
        self.last_bytes_up = 0
        self.last_bytes_down = 0

    def close(self):
        if getattr(self, "_map", None):
            self._L.ndt2d_occmap_destroy(self._map)
            self._map = None
        self._device = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, where):
        if rc != _capi.OK:
            msg = self._L.ndt2d_occmap_last_error(self._map)
            raise Ndt2dError(rc, where, msg.decode() if msg else "")

    def _state(self):
        b = np.zeros(4, dtype=np.float64)
        n = C.c_size_t(0)
        self._check(self._L.ndt2d_occmap_bounds(self._map, dptr(b), C.byref(n)), "ndt2d_occmap_bounds")
        return b, int(n.value)

    @property
    def bounds(self):
        """min_x_, max_x_, min_y_, max_y_ (reference occupancy_grid.cpp:37-40)"""
        return self._state()[0]

    @property
    def num_scans(self):
        return self._state()[1]

    def device_map(self):
        """(DEVICE address of the int8 map of the last getMsg, its _capi.OccupancyInfo): the resident
        map for a consumer on the same GPU (Seeder.set_occupancy_map), valid until the next getMsg,
        reset or close."""
        ptr = C.c_void_p()
        info = _capi.OccupancyInfo()
        self._check(self._L.ndt2d_occmap_device_map(self._map, C.byref(ptr), C.byref(info)),
                    "ndt2d_occmap_device_map")
        return ptr.value, info

    def reset(self):
        """A new generator: scans, counters and bounds are forgotten."""
        self._check(self._L.ndt2d_occmap_reset(self._map), "ndt2d_occmap_reset")
        self._seen = []
        self._poses = np.zeros((0, 3))
        self._data = np.zeros((0, 0), dtype=np.int8)
        self.last_mode = None
        self.last_rect = (0, 0, 0, 0)
        self.last_beams_traced = 0

    def getMsg(self, scans, copy=True):
        """scans: iterable of (pose_xyt, points[n, 2]); the scans of the last call, in their
        order, followed by any new ones.  Returns dict(resolution, width, height, origin_x,
        origin_y, data[height, width] int8).  copy=False returns the array kept here, which
        the next call patches in place."""
        scans = list(scans)
        up = 0
        for k, (_, pts) in enumerate(scans):
            n = len(pts)
            if k < len(self._seen):
                if n != self._seen[k]:
                    raise ValueError("OccupancyMap: scan %d had %d points and now has %d; appended scans "
                                     "are immutable, call reset() after replacing or dropping scans"
                                     % (k, self._seen[k], n))
                continue
            p = _f64(pts, (-1, 2))
            self._check(self._L.ndt2d_occmap_append_scan(self._map, dptr(p), len(p), None),
                        "ndt2d_occmap_append_scan")
            self._seen.append(len(p))
            up += p.nbytes + 4
        poses = _f64([s[0] for s in scans], (-1, 3)) if scans else np.zeros((0, 3))
        res = _capi.OccmapResult()
        n_before = len(self._poses)
        kept = poses[:n_before].tobytes() == self._poses.tobytes()
        self._check(self._L.ndt2d_occmap_update(self._map, dptr(poses), len(scans), C.byref(res)),
                    "ndt2d_occmap_update")
        info = res.info
        self.last_mode = MODES[res.mode]
        self.last_rect = (int(res.rect_x0), int(res.rect_y0), int(res.rect_w), int(res.rect_h))
        self.last_beams_traced = int(res.beams_traced)
        x0, y0, w, h = self.last_rect
        if res.mode == _capi.OCCMAP_FULL:
            self._data = np.zeros((info.height, info.width), dtype=np.int8)
        # the scan table (pose and cos / sin per scan): the records whose pose is new
        up += 32 * (len(scans) - n_before if kept else len(scans))
        new_points = sum(self._seen[n_before:len(scans)])
        self._poses = poses.copy()
        if w and h:
            # the rows of the rectangle, in place in the array kept here
            view = self._data[y0:y0 + h, x0:x0 + w]
            self._check(self._L.ndt2d_occmap_read(self._map, x0, y0, w, h,
                                                  view.ctypes.data_as(C.c_void_p), self._data.shape[1]),
                        "ndt2d_occmap_read")
        self.last_bytes_up = up
        self.last_bytes_down = w * h + (32 if new_points else 0)   # the bounds of the new points
        return dict(resolution=info.resolution, width=int(info.width), height=int(info.height),
                    origin_x=info.origin_x, origin_y=info.origin_y,
                    data=self._data.copy() if copy else self._data)
