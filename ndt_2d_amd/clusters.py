"""Pose clusters of a particle set (include/ndt2d_hip.h, "Pose clusters"): the particles grouped on
the GPU into connected clusters of occupied pose bins, the heaviest of them with updateStatistics'
quantities each.  ParticleFilter.clusters / estimate (particle_filter.py) are built on it; it is
usable on its own with any DEVICE pose and weight arrays.  A verdict with no policy: what share
makes a filter "localised" is the caller's.
"""
import ctypes as C
import weakref
from collections import namedtuple

import numpy as np

from . import _capi
from ._capi import Ndt2dError

ClusterHeader = namedtuple("ClusterHeader", "n n_left_out n_bins n_clusters rounds w_total")

LEFT_OUT = 0xffffffff
PHASES = ("table", "bins", "labels", "select", "statistics")


class PoseCluster:
    """One cluster: `label` (its smallest particle index), `count`, `mass` (Q 2^-40, what the
    clusters are ranked by), `weight` (W), `mean` [x, y, theta], `covariance` 3 x 3 with the centred
    xx, xy, yy and, as the filter fills it, only [2, 2] for theta, and `share` = W / W_total."""

    __slots__ = ("label", "count", "mass", "weight", "mean", "covariance", "share")

    def __init__(self, record, w_total):
        self.label = int(record.label)
        self.count = int(record.count)
        self.mass = float(record.mass)
        self.weight = float(record.weight)
        self.mean = np.array([record.mean_x, record.mean_y, record.mean_theta])
        c = np.zeros((3, 3))
        c[0, 0] = record.cxx
        c[0, 1] = c[1, 0] = record.cxy
        c[1, 1] = record.cyy
        c[2, 2] = record.var_theta
        self.covariance = c
        self.share = self.weight / w_total if w_total > 0.0 else 0.0

    def __repr__(self):
        return "PoseCluster(label=%d, count=%d, share=%.4f, mean=%s)" % (self.label, self.count, self.share,
                                                                          self.mean.tolist())


class Clusterer:
    """ndt2d_clusterer for sets of up to `max_particles` on the device context of `device` (an
    ndt_2d_amd.ScanMatcherNDT, which must outlive it).  Launches go to the stream that context is
    bound to."""

    def __init__(self, device, max_particles):
        self._L = _capi.lib()
        self._c = None
        self._device = device
        c = C.c_void_p()
        rc = self._L.ndt2d_cluster_create(device.device_handle, int(max_particles), C.byref(c))
        if rc != _capi.OK:
            raise Ndt2dError(rc, "ndt2d_cluster_create")
        self._c = c
        self.max_particles = int(max_particles)
        self._n = 0
        if not hasattr(device, "_seeders"):
            device._seeders = weakref.WeakSet()
        device._seeders.add(self)     # (the matcher's list of objects closed before its context is destroyed)

    def close(self):
        if getattr(self, "_c", None):
            self._L.ndt2d_cluster_destroy(self._c)
            self._c = None
        self._device = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, where):
        if rc != _capi.OK:
            msg = self._L.ndt2d_cluster_last_error(self._c)
            raise Ndt2dError(rc, where, msg.decode() if msg else "")

    def set_bins(self, cell_x=0.5, cell_y=0.5, n_theta=24):
        self._check(self._L.ndt2d_cluster_set_bins(self._c, float(cell_x), float(cell_y), int(n_theta)),
                    "ndt2d_cluster_set_bins")

    def set_max_clusters(self, max_clusters):
        self._check(self._L.ndt2d_cluster_set_max_clusters(self._c, int(max_clusters)),
                    "ndt2d_cluster_set_max_clusters")

    def launch(self, poses_ptr, weights_ptr, n):
        """Asynchronous: DEVICE double [n][3] and [n] (weights_ptr None: every weight 1 / n).  Both
        arrays must stay as they are until fetch()."""
        self._check(self._L.ndt2d_cluster_launch(self._c, poses_ptr, weights_ptr, int(n)), "ndt2d_cluster_launch")
        self._n = int(n)

    def fetch_raw(self):
        """(ClusterHeader, [ndt2d_cluster_record]) of the last launch, heaviest first."""
        header = _capi.ClusterHeader()
        records = (_capi.ClusterRecord * _capi.CLUSTER_MAX_RECORDS)()
        n = C.c_size_t(0)
        self._check(self._L.ndt2d_cluster_fetch(self._c, C.byref(header), records, _capi.CLUSTER_MAX_RECORDS,
                                                C.byref(n)), "ndt2d_cluster_fetch")
        head = ClusterHeader(header.n, header.n_left_out, header.n_bins, header.n_clusters, header.rounds,
                             header.w_total)
        return head, [records[k] for k in range(n.value)]

    def fetch(self):
        """(ClusterHeader, [PoseCluster]) of the last launch, heaviest first."""
        head, records = self.fetch_raw()
        return head, [PoseCluster(r, head.w_total) for r in records]

    def labels(self):
        """Every particle's cluster label of the last fetched call as uint32 [n]; 0xFFFFFFFF where
        the particle was left out (for tests and tools)."""
        out = np.empty(max(self._n, 1), dtype=np.uint32)
        self._check(self._L.ndt2d_cluster_read_labels(self._c, out.ctypes.data_as(C.POINTER(C.c_uint32)), self._n),
                    "ndt2d_cluster_read_labels")
        return out[:self._n].copy()

    def set_timing(self, enabled):
        self._check(self._L.ndt2d_cluster_set_timing(self._c, 1 if enabled else 0), "ndt2d_cluster_set_timing")

    def last_ms(self):
        """{phase: ms} of the last fetched call that was timed (PHASES)."""
        ms = (C.c_float * len(PHASES))()
        self._check(self._L.ndt2d_cluster_last_ms(self._c, ms), "ndt2d_cluster_last_ms")
        return dict(zip(PHASES, [float(v) for v in ms]))
