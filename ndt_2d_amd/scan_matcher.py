"""Python-side handle on the matcher layer of libndt2d_hip.so.

`ScanMatcherNDT` mirrors the reference's ndt_2d::ScanMatcherNDT plugin object
(reference include/ndt_2d/scan_matcher_ndt.hpp:42-105): the same six methods
with the same argument meaning and error behaviour, so the parity tests read
like tests of the reference.  Every score is computed by the HIP kernels
through the C-ABI; nothing here evaluates a likelihood.
"""
import ctypes as C
import weakref

import numpy as np

from . import _capi
from ._capi import Ndt2dError, dptr

# defaults of the declared parameters, reference src/scan_matcher_ndt.cpp:37-44
DEFAULT_PARAMS = dict(ndt_resolution=0.25, search_angular_resolution=0.0025,
                      search_angular_size=0.1, search_linear_resolution=0.005,
                      search_linear_size=0.05, laser_max_beams=100)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.reshape(shape) if shape is not None else a


def search_offsets(size, res):
    """Values visited by the reference's `for (v = -size; v < size; v += res)`."""
    L = _capi.lib()
    n = C.c_size_t(0)
    L.ndt2d_search_offsets(size, res, None, 0, C.byref(n))
    out = np.zeros(n.value, dtype=np.float64)
    if n.value:
        L.ndt2d_search_offsets(size, res, dptr(out), n.value, C.byref(n))
    return out


def _pack_scans(scans):
    poses = _f64([s[0] for s in scans], (-1, 3)) if scans else np.zeros((0, 3))
    pts = [_f64(s[1], (-1, 2)) for s in scans]
    offsets = np.zeros(len(scans) + 1, dtype=np.uint64)
    if scans:
        offsets[1:] = np.cumsum([len(p) for p in pts])
    allpts = _f64(np.concatenate(pts) if pts else np.zeros((0, 2)))
    return poses, allpts, offsets


class _BatchResults:
    """What the three batched matches (matchCandidates, matchStarts, matchScans) write per slot --
    pose, covariance, score, best index, optionally the lattice's raw scores -- and the list of
    result dicts made of it.  `args`: the trailing arguments of the C call."""

    def __init__(self, params, K, want_scores, best_fill=_capi.NO_INDEX):
        self.K = K
        self.poses = np.zeros((K, 3))
        self.covs = np.full((K, 9), np.nan)
        self.scores = np.zeros(K)
        self.best = np.full(K, best_fill, dtype=np.uint64)
        self.n_lat = C.c_size_t(0)
        self.all_scores, as_ptr, cap = None, None, 0
        if want_scores:
            n_th = len(search_offsets(params["search_angular_size"], params["search_angular_resolution"]))
            n_lin = len(search_offsets(params["search_linear_size"], params["search_linear_resolution"]))
            self.all_scores = np.zeros((K, n_th * n_lin * n_lin), dtype=np.float64)
            as_ptr, cap = dptr(self.all_scores), self.all_scores.size
        self.args = (dptr(self.poses), dptr(self.covs), dptr(self.scores), self.best.ctypes.data_as(C.POINTER(C.c_uint64)),
                     as_ptr, cap, C.byref(self.n_lat))

    def dicts(self, has_ndt):
        return [dict(score=float(self.scores[k]), pose=self.poses[k].copy(),
                     covariance=self.covs[k].reshape(3, 3).copy() if has_ndt else None,
                     n_candidates=self.n_lat.value, best_index=int(self.best[k]),
                     scores=self.all_scores[k] if self.all_scores is not None else None) for k in range(self.K)]


BUILD_SEQUENTIAL = 1      # include/ndt2d_hip.h NDT2D_BUILD_SEQUENTIAL
BUILD_CLOSED_FORM = 2     # NDT2D_BUILD_CLOSED_FORM


def host_build_grid(ndt_resolution, range_max, scans, flags=0):
    """addScans' NDT build on the host only (no GPU): (cells6, size_x, size_y, ox, oy).
    flags: BUILD_SEQUENTIAL (the reference's loop as it stands instead of a scan's four
    quarters side by side: same bits), BUILD_CLOSED_FORM."""
    L = _capi.lib()
    poses, allpts, offsets = _pack_scans(scans)
    sx, sy = C.c_uint32(0), C.c_uint32(0)
    ox, oy = C.c_double(0), C.c_double(0)
    off_p = offsets.ctypes.data_as(C.POINTER(C.c_size_t))
    rc = L.ndt2d_host_build_grid_ex(ndt_resolution, range_max, dptr(poses), dptr(allpts), off_p,
                                    len(scans), flags, None, 0, C.byref(sx), C.byref(sy), C.byref(ox),
                                    C.byref(oy))
    if rc != _capi.OK:
        raise Ndt2dError(rc, "ndt2d_host_build_grid")
    cells = np.zeros((sx.value * sy.value, 6), dtype=np.float64)
    rc = L.ndt2d_host_build_grid_ex(ndt_resolution, range_max, dptr(poses), dptr(allpts), off_p,
                                    len(scans), flags, dptr(cells), len(cells), C.byref(sx), C.byref(sy),
                                    C.byref(ox), C.byref(oy))
    if rc != _capi.OK:
        raise Ndt2dError(rc, "ndt2d_host_build_grid")
    return cells, sx.value, sy.value, ox.value, oy.value


def _free_pinned(lib, state, address):
    lib.ndt2d_host_free(state["handle"], C.c_void_p(address))


class ScanMatcherNDT:
    """ndt_2d::ScanMatcherNDT over the MI355X kernels."""

    def __init__(self, device_id=0, device_ids=None):
        """device_ids (a list): one matcher over several GPUs of this process
        (ndt2d_matcher_create_multi) -- matchScan's theta steps and particle batches are
        dealt to them; a device may be named twice (several contexts on one GPU, host
        exchange)."""
        self._L = _capi.lib()
        self._m = C.c_void_p()
        if device_ids is None:
            rc = self._L.ndt2d_matcher_create(C.byref(self._m), int(device_id))
        else:
            ids = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
            rc = self._L.ndt2d_matcher_create_multi(C.byref(self._m), ids, len(device_ids))
        if rc != _capi.OK:
            self._m = None
            raise Ndt2dError(rc, "ndt2d_matcher_create",
                             "no usable GPU; this library has no CPU fallback")
        self.params = dict(DEFAULT_PARAMS, range_max=0.0)

    def device_count(self):
        return self._L.ndt2d_matcher_device_count(self._m)

    def set_exchange(self, mode):
        """How a multi-device matcher exchanges its per-device records: "auto", "host"
        (host-coherent result blocks, no collective) or "rccl" (one all-reduce)."""
        self._check(self._L.ndt2d_matcher_set_exchange(self._m, mode.encode()), "set_exchange")

    def set_multi_min_units(self, units):
        """Work (candidates x beams, particles x beams) below which a multi-device matcher
        stays on its first device."""
        self._check(self._L.ndt2d_matcher_set_multi_min_units(self._m, float(units)),
                    "set_multi_min_units")

    def set_multi_thresholds(self, min_search_units, min_pose_units):
        """The two thresholds apart: candidates x beams of a search (default 1e9), particles x
        beams of a pose batch (default 2e8)."""
        self._check(self._L.ndt2d_matcher_set_multi_thresholds(self._m, float(min_search_units),
                                                               float(min_pose_units)), "set_multi_thresholds")

    def multi_thresholds(self):
        a, b = _capi.C.c_double(0.0), _capi.C.c_double(0.0)
        self._check(self._L.ndt2d_matcher_get_multi_thresholds(self._m, _capi.C.byref(a), _capi.C.byref(b)),
                    "get_multi_thresholds")
        return a.value, b.value

    def last_fanout_us(self):
        """Of the last dealt call: when each device's launch had been queued (us from the call's start)."""
        out = np.zeros(64, dtype=np.float64)
        n = _capi.C.c_size_t(0)
        self._check(self._L.ndt2d_matcher_last_fanout_us(self._m, _capi.dptr(out), 64, _capi.C.byref(n)),
                    "last_fanout_us")
        return out[:min(n.value, 64)].copy()

    def matcher_variant(self):
        """ndt2d_matcher_last_variant: "multi[n]/rccl/..." when the last call was dealt out."""
        v = self._L.ndt2d_matcher_last_variant(self._m)
        return v.decode() if v else ""

    def close(self):
        if getattr(self, "_m", None):
            # host_alloc() buffers stay valid while any numpy view of them is alive: each is
            # freed by its own finalizer (with a NULL handle once this context is gone)
            state = getattr(self, "_pinned_state", None)
            if state is not None:
                state["handle"] = None
            # resamplers live on this context's device layer: they go first
            for r in list(getattr(self, "_resamplers", ())):
                r.close()
            for o in list(getattr(self, "_occupancy_maps", ())):
                o.close()
            for o in list(getattr(self, "_seeders", ())):
                o.close()
            self._L.ndt2d_matcher_destroy(self._m)
            self._m = None

    def host_alloc(self, shape):
        """float64 array in pinned, GPU-mapped host memory (ndt2d_host_alloc): the
        host-pointer entry points read / write such buffers in place over PCIe instead
        of staging and copying them.  The memory is released when the last numpy view of
        it is gone -- before or after close(), never under a live array."""
        shape = (shape,) if np.isscalar(shape) else tuple(shape)
        n = int(np.prod(shape))
        ptr = C.c_void_p()
        self._dev_check(self._L.ndt2d_host_alloc(self.device_handle, max(n, 1) * 8, C.byref(ptr)),
                        "ndt2d_host_alloc")
        if not hasattr(self, "_pinned_state"):
            self._pinned_state = {"handle": self.device_handle}
        buf = (C.c_double * max(n, 1)).from_address(ptr.value)
        # every view of the array keeps `buf` alive (numpy's base chain); the block goes with it
        weakref.finalize(buf, _free_pinned, self._L, self._pinned_state, ptr.value)
        return np.ctypeslib.as_array(buf)[:n].reshape(shape)

    def set_timing(self, enabled):
        """HIP events around every launch (last_launch_ms) on / off; the pluginlib shim
        runs with them off (~4.5 us per call)."""
        self._dev_check(self._L.ndt2d_set_timing(self.device_handle, 1 if enabled else 0),
                        "ndt2d_set_timing")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, where):
        if rc != _capi.OK:
            msg = self._L.ndt2d_matcher_last_error(self._m)
            raise Ndt2dError(rc, where, msg.decode() if msg else "")

    @property
    def device_handle(self):
        """The ndt2d_handle of the device layer (for sharded / device-pointer launches)."""
        return C.c_void_p(self._L.ndt2d_matcher_device(self._m))

    # -- ScanMatcher interface (reference include/ndt_2d/scan_matcher.hpp:42-91) --

    def initialize(self, name="scan_matcher", range_max=0.0, **params):
        """initialize(name, node, range_max): `params` stands for the node's parameters
        `<name>.ndt_resolution` etc. (reference src/scan_matcher_ndt.cpp:35-47)."""
        unknown = set(params) - set(DEFAULT_PARAMS)
        if unknown:
            raise KeyError("undeclared parameter(s): %s" % sorted(unknown))
        p = dict(DEFAULT_PARAMS)
        p.update(params)
        p["range_max"] = float(range_max)
        self.name = name
        self.params = p
        self._check(self._L.ndt2d_matcher_initialize(
            self._m, p["ndt_resolution"], p["search_angular_resolution"],
            p["search_angular_size"], p["search_linear_resolution"], p["search_linear_size"],
            int(p["laser_max_beams"]), p["range_max"]), "initialize")

    def addScans(self, scans):
        """scans: iterable of (pose_xyt, points[n, 2]) -- the [begin, end) range."""
        scans = list(scans)
        poses, allpts, offsets = _pack_scans(scans)
        self._check(self._L.ndt2d_matcher_add_scans(
            self._m, dptr(poses), dptr(allpts),
            offsets.ctypes.data_as(C.POINTER(C.c_size_t)), len(scans)), "addScans")

    def matchScan(self, scan_pose, points, pose=None, want_scores=False):
        """Returns dict(score, pose, covariance, n_candidates, best_index[, scores]).
        `pose` is the caller's pre-initialised out-parameter (default (0,0,0)); it is
        returned untouched when no candidate scores below 0, and covariance is
        None when there is no NDT (the reference leaves both untouched then)."""
        sp = _f64(scan_pose, (3,))
        pts = _f64(points, (-1, 2))
        pose_io = np.array([0.0, 0.0, 0.0] if pose is None else pose, dtype=np.float64)
        cov = np.full(9, np.nan)
        score = C.c_double(0.0)
        ncand = C.c_size_t(0)
        best = C.c_uint64(0)
        scores, sp_ptr, cap = None, None, 0
        if want_scores:
            p = self.params
            n_th = len(search_offsets(p["search_angular_size"], p["search_angular_resolution"]))
            n_lin = len(search_offsets(p["search_linear_size"], p["search_linear_resolution"]))
            cap = n_th * n_lin * n_lin
            scores = np.zeros(cap, dtype=np.float64)
            sp_ptr = dptr(scores)
        self._check(self._L.ndt2d_matcher_match_scan_ex(
            self._m, dptr(sp), dptr(pts), len(pts), dptr(pose_io), dptr(cov), C.byref(score),
            sp_ptr, cap, C.byref(ncand), C.byref(best)), "matchScan")
        has = bool(self._L.ndt2d_matcher_has_ndt(self._m))
        return dict(score=score.value, pose=pose_io,
                    covariance=cov.reshape(3, 3) if has else None,
                    n_candidates=ncand.value, best_index=best.value, scores=scores)

    @staticmethod
    def _laser_scan(angle_min, angle_increment, range_max, inverted, laser, motion):
        return _capi.LaserScan(angle_min, angle_increment, range_max, 1 if inverted else 0,
                               laser[0], laser[1], laser[2], motion[0], motion[1], motion[2])

    def convertScan(self, ranges, angle_min, angle_increment, range_max, inverted=False,
                    laser=(0.0, 0.0, 0.0), motion=(0.0, 0.0, 0.0)):
        """LaserScan -> Scan points on the device (reference src/ndt_mapper.cpp:385-453):
        ranges float32[n]; laser = laser_transform_; motion = odometry motion over the
        sweep (`translation`, :386-389).  Returns points[m, 2]."""
        r = np.ascontiguousarray(ranges, dtype=np.float32)
        d = self._laser_scan(angle_min, angle_increment, range_max, inverted, laser, motion)
        out = np.zeros((max(len(r), 1), 2), dtype=np.float64)
        n = C.c_size_t(0)
        self._dev_check(self._L.ndt2d_convert_scan(
            self.device_handle, r.ctypes.data_as(C.POINTER(C.c_float)), len(r), C.byref(d),
            dptr(out), C.byref(n)), "ndt2d_convert_scan")
        return out[:n.value].copy()

    def matchLaserScan(self, scan_pose, ranges, angle_min, angle_increment, range_max,
                       inverted=False, laser=(0.0, 0.0, 0.0), motion=(0.0, 0.0, 0.0), pose=None):
        """Conversion fused with matchScan: only the raw ranges cross PCIe.  Returns
        dict(score, pose, covariance, n_points)."""
        sp = _f64(scan_pose, (3,))
        r = np.ascontiguousarray(ranges, dtype=np.float32)
        d = self._laser_scan(angle_min, angle_increment, range_max, inverted, laser, motion)
        pose_io = np.array([0.0, 0.0, 0.0] if pose is None else pose, dtype=np.float64)
        cov = np.full(9, np.nan)
        score = C.c_double(0.0)
        npts = C.c_size_t(0)
        self._check(self._L.ndt2d_matcher_match_laser_scan(
            self._m, dptr(sp), r.ctypes.data_as(C.POINTER(C.c_float)), len(r), C.byref(d),
            dptr(pose_io), dptr(cov), C.byref(score), C.byref(npts)), "matchLaserScan")
        has = bool(self._L.ndt2d_matcher_has_ndt(self._m))
        return dict(score=score.value, pose=pose_io,
                    covariance=cov.reshape(3, 3) if has else None, n_points=npts.value)

    def scoreScan(self, scan_pose, points):
        sp = _f64(scan_pose, (3,))
        pts = _f64(points, (-1, 2))
        out = C.c_double(0.0)
        self._check(self._L.ndt2d_matcher_score_scan(self._m, dptr(sp), dptr(pts), len(pts),
                                                     C.byref(out)), "scoreScan")
        return out.value

    def scorePoints(self, points, pose):
        pts = _f64(points, (-1, 2))
        ps = _f64(pose, (3,))
        out = C.c_double(0.0)
        self._check(self._L.ndt2d_matcher_score_points(self._m, dptr(pts), len(pts), dptr(ps),
                                                       C.byref(out)), "scorePoints")
        return out.value

    def reset(self):
        self._check(self._L.ndt2d_matcher_reset(self._m), "reset")

    def set_search_ahead(self, enabled):
        """scoreScan launching the scan's search behind itself once the mapper's scoreScan /
        matchScan pair has been seen (include/ndt2d_hip.h, ndt2d_matcher_score_scan): on by default."""
        self._check(self._L.ndt2d_matcher_set_search_ahead(self._m, 1 if enabled else 0), "set_search_ahead")

    def search_ahead_stats(self):
        """(searches scoreScan launched ahead, how many a matchScan collected)."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.ndt2d_matcher_search_ahead_stats(self._m, C.byref(a), C.byref(b)), "search_ahead_stats")
        return a.value, b.value

    def set_adjudication(self, enabled):
        """Near-tie adjudication of matchScan (on by default): candidates within 2^-36 (1.5e-11, relative) of the
        best are rescored on the host with the reference's arithmetic and its first-wins rule."""
        self._check(self._L.ndt2d_matcher_set_adjudication(self._m, 1 if enabled else 0), "set_adjudication")

    def settle_near_tie(self, scan_pose, record):
        """A combined record of a search sharded from outside: a marked winner (index + 0.5) is
        settled with the reference's arithmetic; returns the record with a plain index."""
        sp = _f64(scan_pose, (3,))
        rec = _f64(record, (_capi.MATCH_RECORD_DOUBLES,)).copy()
        self._check(self._L.ndt2d_matcher_settle_near_tie(self._m, dptr(sp), dptr(rec)), "settle_near_tie")
        return rec

    def adjudication_stats(self):
        """(searches whose winner came back marked near-tie, of those: winner changed, list truncated)."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.ndt2d_matcher_adjudication_stats(self._m, C.byref(a), C.byref(b), C.byref(c)),
                    "adjudication_stats")
        return a.value, b.value, c.value

    def match_near_best(self, th_begin, th_end, rel=2.0 ** -36, capacity=256):
        """ndt2d_match_near_best on the prepared search: flat indices (ascending) of the candidates
        within rel * |best| of the slab's best (the first `capacity` in visiting order), and how many
        there are."""
        idx = (C.c_uint64 * capacity)()
        n = C.c_size_t(0)
        self._dev_check(self._L.ndt2d_match_near_best(self.device_handle, th_begin, th_end, rel, idx, capacity,
                                                      C.byref(n), None), "ndt2d_match_near_best")
        return [idx[k] for k in range(min(n.value, capacity))], n.value

    def set_single_pose_path(self, where, max_beams=0):
        """Where scorePoints / scoreScan score their one pose: "host" (default; scans of up to
        max_beams subsampled beams, from the host NDT in the reference's order) or "device"."""
        self._check(self._L.ndt2d_matcher_set_single_pose_path(self._m, where.encode(), int(max_beams)),
                    "set_single_pose_path")

    def set_build_mode(self, mode):
        """Where addScans builds the NDT: "host", "device" or "auto" (bit-identical grids), or
        "fused": the one-workgroup device build for maps of up to 16,384 points on fewer than
        65,535 cells, otherwise what "auto" does."""
        self._check(self._L.ndt2d_matcher_set_build_mode(self._m, mode.encode()), "set_build_mode")

    def storeScan(self, points):
        """Keep a scan's robot-frame points on the device(s); returns its id (from 0, in order)."""
        pts = _f64(points, (-1, 2))
        out = C.c_size_t(0)
        self._check(self._L.ndt2d_matcher_store_scan(self._m, dptr(pts), len(pts), C.byref(out)), "storeScan")
        return out.value

    def addScansById(self, poses, ids):
        """addScans of the stored scans `ids`, in that order, with `poses[k]` for ids[k]: only the
        poses and the id table travel.  Same grid as addScans of those scans and poses."""
        ps = _f64(poses, (-1, 3))
        idx = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        if len(ps) != len(idx):
            raise ValueError("addScansById: %d poses for %d ids" % (len(ps), len(idx)))
        self._check(self._L.ndt2d_matcher_add_scans_by_id(
            self._m, dptr(ps), idx.ctypes.data_as(C.POINTER(C.c_size_t)), len(idx)), "addScansById")

    def matchCandidates(self, scan_pose, points, candidates, want_scores=False):
        """The loop-closure thread's inner loop in one call: `candidates` is a list of candidate
        maps, each a list of (stored scan id, pose_xyt).  Returns one dict per candidate, the
        dict matchScan returns after reset() / addScansById(candidate): every candidate starts
        from the same scan_pose, `pose` is (0, 0, 0) unless a lattice candidate scores below 0.
        One build launch, one search launch and one read-back for all of them; the matcher holds
        no NDT afterwards."""
        sp = _f64(scan_pose, (3,))
        pts = _f64(points, (-1, 2))
        K = len(candidates)
        offsets, ids, poses = _pack_candidates(candidates)
        out = _BatchResults(self.params, K, want_scores, best_fill=0)
        self._check(self._L.ndt2d_matcher_match_candidates(
            self._m, dptr(sp), dptr(pts), len(pts), offsets.ctypes.data_as(C.POINTER(C.c_size_t)),
            ids.ctypes.data_as(C.POINTER(C.c_size_t)), dptr(poses), K, *out.args), "matchCandidates")
        return out.dicts(has_ndt=True)

    def _batch_set_timing(self, noun, call, enabled):
        """ndt2d_<noun>_set_timing on the matcher's batched-match object, which `call` makes."""
        obj = getattr(self._L, "ndt2d_matcher_" + noun)(self._m)
        if not obj:
            raise Ndt2dError(_capi.ERR_STATE, noun + "_set_timing", "no %s call yet" % call)
        rc = getattr(self._L, "ndt2d_%s_set_timing" % noun)(C.c_void_p(obj), 1 if enabled else 0)
        if rc != _capi.OK:
            raise Ndt2dError(rc, "ndt2d_%s_set_timing" % noun)

    def _batch_last_ms(self, noun):
        """The two times of ndt2d_<noun>_last_ms on the matcher's batched-match object."""
        obj = getattr(self._L, "ndt2d_matcher_" + noun)(self._m)
        a, b = C.c_float(0.0), C.c_float(0.0)
        rc = getattr(self._L, "ndt2d_%s_last_ms" % noun)(C.c_void_p(obj), C.byref(a), C.byref(b)) if obj else _capi.ERR_STATE
        if rc != _capi.OK:
            raise Ndt2dError(rc, "ndt2d_%s_last_ms" % noun)
        return a.value, b.value

    def closure_set_timing(self, enabled):
        """HIP events around the batched match's build and search launches on / off
        (after the first matchCandidates: the closure object is made by it)."""
        self._batch_set_timing("closure", "matchCandidates", enabled)

    def closure_last_ms(self):
        """(build_ms, search_ms) of the last timed matchCandidates (its last chunk); after a
        refineCandidates or a verifyCandidates: the build and that call's own launch."""
        return self._batch_last_ms("closure")

    def matchStarts(self, start_poses, points, want_scores=False):
        """matchScan of one scan from K start poses against the NDT in place, in one call (one
        upload, one search launch over start x lattice, one read-back): relocalisation in a loaded
        map, several hypotheses of a tracker.  Returns one dict per start, the dict
        matchScan(start, points) returns: `pose` is (0, 0, 0) unless a lattice candidate scores
        below 0, covariance is None when there is no NDT.  The NDT stays in place."""
        sp = _f64(start_poses, (-1, 3))
        pts = _f64(points, (-1, 2))
        K = len(sp)
        out = _BatchResults(self.params, K, want_scores)
        self._check(self._L.ndt2d_matcher_match_starts(
            self._m, dptr(sp), K, dptr(pts), len(pts), *out.args), "matchStarts")
        return out.dicts(has_ndt=bool(self._L.ndt2d_matcher_has_ndt(self._m)))

    def matchWide(self, scan_pose, points, linear_size, linear_resolution, angular_size, angular_resolution,
                  tile_steps=None):
        """matchScan over a lattice of the CALL's sizes by the wide search (ndt2d_matcher_match_wide):
        the exhaustive lattice's winner, found by scoring only the tiles whose upper bound can
        still hold it.  Returns dict(score, pose, best_index, near_tie, tiles_scored, tiles_total):
        score is per beam used and pose the correction, as matchScan gives them; pose stays (0, 0, 0)
        and best_index is NO_INDEX without a winner.  No covariance: refineScans(neighbourhood=9) on
        the winner gives one."""
        sp = _f64(scan_pose, (3,))
        pts = _f64(points, (-1, 2))
        pose = np.zeros(3)
        score = C.c_double(0.0)
        best = C.c_uint64(_capi.NO_INDEX)
        near = C.c_int(0)
        stats = (C.c_uint64 * 2)(0, 0)
        self._check(self._L.ndt2d_matcher_match_wide(
            self._m, dptr(sp), dptr(pts), len(pts), float(linear_size), float(linear_resolution), float(angular_size),
            float(angular_resolution), 0 if tile_steps is None else int(tile_steps), dptr(pose), C.byref(score),
            C.byref(best), C.byref(near), stats), "matchWide")
        return dict(score=score.value, pose=pose, best_index=best.value, near_tie=bool(near.value),
                    tiles_scored=int(stats[0]), tiles_total=int(stats[1]))

    def starts_set_timing(self, enabled):
        """HIP events around the batched match's search and reduce launches on / off (after the
        first matchStarts with an NDT in place: the object is made by it)."""
        self._batch_set_timing("starts", "matchStarts", enabled)

    def starts_last_ms(self):
        """(search_ms, reduce_ms) of the last timed matchStarts (its last chunk)."""
        return self._batch_last_ms("starts")

    def matchScans(self, jobs, scans, job_scan=None, want_scores=False):
        """matchScan of K jobs -- (scan, pose) pairs -- against the NDT in place, in one call (one
        upload, the search launches over job x lattice, one read-back): a fleet of robots on one
        map, a recorded bag replayed against a loaded map, a graph's scans matched again after an
        optimisation.  jobs: K poses; scans: a sequence of S point arrays; job_scan[k]: the scan
        of job k (several jobs may share one), None: job k uses scan k.  Returns one dict per
        job, the dict matchScan(jobs[k], scans[job_scan[k]]) returns: `pose` is (0, 0, 0) unless
        a lattice candidate scores below 0, covariance is None when there is no NDT.  The NDT
        stays in place."""
        lst = _JobList("matchScans", jobs, scans, job_scan)
        out = _BatchResults(self.params, lst.K, want_scores)
        self._check(self._L.ndt2d_matcher_match_scans(self._m, *lst.args, *out.args), "matchScans")
        return out.dicts(has_ndt=bool(self._L.ndt2d_matcher_has_ndt(self._m)))

    def scans_set_timing(self, enabled):
        """HIP events around the batched scan tracking's search and reduce launches on / off (after
        the first matchScans with an NDT in place: the object is made by it)."""
        self._batch_set_timing("scans", "matchScans", enabled)

    def scans_last_ms(self):
        """(search_ms, reduce_ms) of the last timed matchScans (its last chunk)."""
        return self._batch_last_ms("scans")

    def refineScans(self, jobs, scans, job_scan=None, max_evals=32, tol_lin=1e-6, tol_ang=1e-6, neighbourhood=1):
        """Newton NDT registration of K jobs -- (scan, pose) pairs, as matchScans takes them --
        against the NDT in place, in one call (one upload, one kernel launch for the whole
        iteration of all jobs, one read-back): from each job's pose to the optimum of the scan's
        score under it (include/ndt2d_hip.h, "Newton NDT registration").  Returns one dict per job:
        pose (absolute, not a correction), score and start_score (what scorePoints gives at the
        pose and at the job's own), gradient[3] and hessian[3, 3] of that score, evals, steps
        (accepted), status (_capi.REFINE_*), covariance.  No NDT, or a scan without points: score
        0.0, the job's own pose, status REFINE_NO_OVERLAP.  The NDT stays in place.

        neighbourhood: 1 (a point is scored against the cell it falls in: scorePoints' objective,
        whose cell borders are jumps of f) or 9 (against the 3 x 3 cells round it: score,
        start_score, gradient and hessian are then that objective's, and score is no longer what
        scorePoints gives).  It is set on the matcher for this call and stays
        (set_refine_neighbourhood).  covariance: the inverse of hessian x N (the sum's Hessian, N
        the scan's beams in use) through ndt2d_refine_covariance, a [3, 3] array -- or None where
        that Hessian is not positive definite; meant to be taken with neighbourhood 9."""
        self.set_refine_neighbourhood(neighbourhood)
        call = _RefineCall("refineScans", self.params, jobs, scans, job_scan, max_evals)
        self._check(self._L.ndt2d_matcher_refine_scans(
            self._m, *call.job_args, int(max_evals), float(tol_lin), float(tol_ang), *call.out_args), "refineScans")
        return call.dicts()

    def refineCandidates(self, jobs, scans, candidates, job_candidate=None, job_scan=None, max_evals=32, tol_lin=1e-6,
                         tol_ang=1e-6, neighbourhood=1):
        """refineScans of K jobs, each on a loop-closure candidate's OWN map, in one call: `candidates`
        as matchCandidates takes them (a list of candidate maps, each a list of (stored scan id,
        pose_xyt)), jobs / scans / job_scan as refineScans takes them, job_candidate[k]: the
        candidate of job k (None: job k uses candidate k).  Returns the dicts refineScans returns
        after reset() / addScansById(candidates[job_candidate[k]]), bit for bit, covariance
        included -- from one upload, one build launch for the candidates named, one launch of the
        refinement and one read-back per chunk.  The NDT in place is not touched: has_ndt() and the
        grid are the same before and after.  A scan without points: score 0.0, the job's own pose,
        status REFINE_NO_OVERLAP."""
        self.set_refine_neighbourhood(neighbourhood)
        call = _RefineCall("refineCandidates", self.params, jobs, scans, job_scan, max_evals)
        K = len(candidates)
        offsets, ids, poses = _pack_candidates(candidates)
        jc = _index_array("refineCandidates", "job_candidate", "candidate", job_candidate, call.K)
        self._check(self._L.ndt2d_matcher_refine_candidates(
            self._m, offsets.ctypes.data_as(C.POINTER(C.c_size_t)), ids.ctypes.data_as(C.POINTER(C.c_size_t)), dptr(poses), K,
            call.job_args[0], call.job_args[1], jc.ctypes.data_as(C.POINTER(C.c_uint32)) if jc is not None else None,
            *call.job_args[2:], int(max_evals), float(tol_lin), float(tol_ang), *call.out_args), "refineCandidates")
        return call.dicts()

    def set_refine_neighbourhood(self, cells):
        """The neighbourhood of the later refineScans calls: 1 or 9 cells per point."""
        if not 0 <= int(cells) < 2 ** 32:
            raise ValueError("set_refine_neighbourhood: 1 or 9 cells")
        self._check(self._L.ndt2d_matcher_set_refine_neighbourhood(self._m, int(cells)), "set_refine_neighbourhood")

    def refine_neighbourhood(self):
        out = C.c_uint32(0)
        self._check(self._L.ndt2d_matcher_refine_neighbourhood(self._m, C.byref(out)), "refine_neighbourhood")
        return int(out.value)

    def refine_set_timing(self, enabled):
        """HIP events around the Newton registration's kernel launch and read-back on / off (after
        the first refineScans with an NDT in place: the object is made by it)."""
        self._batch_set_timing("refine", "refineScans", enabled)

    def refine_last_ms(self):
        """(kernel_ms, fetch_ms) of the last timed refineScans (its last chunk)."""
        return self._batch_last_ms("refine")

    def verifyScans(self, jobs, scans, job_scan=None, max_beams=None, neighbourhood=9, gate_inlier=9.0, gate_pierce=1.0,
                    rays=True, want_beams=False):
        """Is this match right?  Match verification of K jobs -- (scan, pose) pairs, as refineScans
        takes them -- against the NDT in place, in one call (one upload, one kernel launch, one
        read-back): which beams of each scan the map explains at the job's pose
        (include/ndt2d_hip.h, "Match verification").  Returns one dict per job: n_beams, off (beams
        that end off the grid), unseen (on the grid, where no cell of the neighbourhood can score),
        outlier, inlier (m2 <= gate_inlier against the best cell of the neighbourhood), pierced
        (beams whose ray from the robot passes through a cell's Gaussian before it reaches the
        end's 3 x 3: in a wrong basin rays pass through walls), walked (beams whose ray was walked).
        A verdict, no policy: nothing is accepted or rejected here.

        max_beams: None takes the matcher's laser_max_beams -- the beams matchScan / scorePoints
        computed the score from; 0 every point of the scan (filtering a scan before storeScan); n
        min(n, the scan's points) by the same subsampling rule.  neighbourhood (1 or 9),
        gate_inlier, gate_pierce, rays are set on the matcher for this call and stay.  The gates'
        defaults are starting values, not tuned.
        want_beams: each dict also holds classes (uint8, _capi.BEAM_OFF / _UNSEEN / _OUTLIER /
        _INLIER), m2 (+inf for off and unseen), cells ([n, 2] uint32: the cell whose m2 won, the
        first piercing cell; _capi.VERIFY_NO_CELL: none) and pierced_mask (bool).
        No NDT in place: Ndt2dError (NDT2D_ERR_NO_GRID).  A scan without points: zeros."""
        self.set_verify(neighbourhood=neighbourhood, gate_inlier=gate_inlier, gate_pierce=gate_pierce, rays=rays)
        return self._verify_call("verifyScans", jobs, scans, job_scan, max_beams, want_beams,
                                 lambda job_args, out_args: self._L.ndt2d_matcher_verify_scans(self._m, *job_args, *out_args))

    def verifyCandidates(self, jobs, scans, candidates, job_candidate=None, job_scan=None, max_beams=None, neighbourhood=9,
                         gate_inlier=9.0, gate_pierce=1.0, rays=True, want_beams=False):
        """verifyScans of K jobs, each on a loop-closure candidate's OWN map, in one call: `candidates`
        as matchCandidates takes them (a list of candidate maps, each a list of (stored scan id,
        pose_xyt)), jobs / scans / job_scan and the keywords as verifyScans takes them,
        job_candidate[k]: the candidate of job k (None: job k uses candidate k).  Returns the dicts
        verifyScans returns after reset() / addScansById(candidates[job_candidate[k]]), bit for bit,
        the per-beam arrays included -- from one upload, one build launch for the candidates named,
        one launch of the verification and one read-back per chunk.  The NDT in place is not
        touched: has_ndt() and the grid are the same before and after, and none in place is no
        error.  A scan without points: zeros.  A verdict, no policy."""
        self.set_verify(neighbourhood=neighbourhood, gate_inlier=gate_inlier, gate_pierce=gate_pierce, rays=rays)
        K = len(candidates)
        offsets, ids, poses = _pack_candidates(candidates)
        szp = C.POINTER(C.c_size_t)

        def launch(job_args, out_args):
            jc = _index_array("verifyCandidates", "job_candidate", "candidate", job_candidate, job_args[2])
            return self._L.ndt2d_matcher_verify_candidates(
                self._m, offsets.ctypes.data_as(szp), ids.ctypes.data_as(szp), dptr(poses), K, job_args[0], job_args[1],
                jc.ctypes.data_as(C.POINTER(C.c_uint32)) if jc is not None else None, *job_args[2:], *out_args)
        return self._verify_call("verifyCandidates", jobs, scans, job_scan, max_beams, want_beams, launch)

    def _verify_call(self, who, jobs, scans, job_scan, max_beams, want_beams, launch):
        """The arrays of a verification call, the call (launch(job_args, out_args): the C entry's
        arguments from jobs_xyt to max_beams, and from records_out on) and its result dicts."""
        lst = _JobList(who, jobs, scans, job_scan)
        K, arrays = lst.K, lst.arrays
        if job_scan is None and len(arrays) != K:
            raise ValueError(who + ": without job_scan job k uses scan k: one scan per job")
        limit = int(self.params["laser_max_beams"]) if max_beams is None else int(max_beams)
        if limit < 0:
            raise ValueError(who + ": max_beams must not be negative")
        which = lst.js if lst.js is not None else np.arange(K)
        if K and len(arrays) and np.any(np.asarray(which) >= len(arrays)):
            cap = 0     # (the call refuses the job; nothing is written)
        else:
            sizes = [len(arrays[int(sc)]) for sc in which] if len(arrays) else []
            cap = int(sum(n if limit == 0 else min(limit, n) for n in sizes))
        records = np.zeros((K, _capi.VERIFY_RECORD_U32), dtype=np.uint32)
        table = np.zeros(K + 1, dtype=np.uintp)
        classes = np.zeros(cap, dtype=np.uint8) if want_beams else None
        m2 = np.zeros(cap, dtype=np.float64) if want_beams else None
        cells = np.zeros((cap, 2), dtype=np.uint32) if want_beams else None
        u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        self._check(launch(
            lst.args + (limit,),
            (records.ctypes.data_as(u32p), table.ctypes.data_as(C.POINTER(C.c_size_t)),
             classes.ctypes.data_as(u8p) if want_beams else None, dptr(m2) if want_beams else None,
             cells.ctypes.data_as(u32p) if want_beams else None, cap)), who)
        out = []
        for k in range(K):
            r = records[k]
            d = dict(n_beams=int(r[0]), off=int(r[1]), unseen=int(r[2]), outlier=int(r[3]), inlier=int(r[4]), pierced=int(r[5]),
                     walked=int(r[6]))
            if want_beams:
                a, b = int(table[k]), int(table[k + 1])
                d.update(classes=classes[a:b] & 3, m2=m2[a:b].copy(), cells=cells[a:b].copy(),
                         pierced_mask=(classes[a:b] & _capi.BEAM_PIERCED) != 0)
            out.append(d)
        return out

    def set_verify(self, neighbourhood=None, gate_inlier=None, gate_pierce=None, rays=None):
        """The parameters of the later verifyScans calls (None: as it is): the neighbourhood (1 or
        9 cells per point), the gates (each >= 0 and finite), the ray walk (bool)."""
        if neighbourhood is not None:
            if not 0 <= int(neighbourhood) < 2 ** 32:
                raise ValueError("set_verify: 1 or 9 cells")
            self._check(self._L.ndt2d_matcher_set_verify_neighbourhood(self._m, int(neighbourhood)), "set_verify_neighbourhood")
        if gate_inlier is not None or gate_pierce is not None:
            have = self.verify_parameters()
            self._check(self._L.ndt2d_matcher_set_verify_gates(
                self._m, float(have["gate_inlier"] if gate_inlier is None else gate_inlier),
                float(have["gate_pierce"] if gate_pierce is None else gate_pierce)), "set_verify_gates")
        if rays is not None:
            self._check(self._L.ndt2d_matcher_set_verify_rays(self._m, 1 if rays else 0), "set_verify_rays")

    def verify_parameters(self):
        """dict(neighbourhood, gate_inlier, gate_pierce, rays) of the later verifyScans calls."""
        cells, rays = C.c_uint32(0), C.c_int(0)
        gi, gp = C.c_double(0.0), C.c_double(0.0)
        self._check(self._L.ndt2d_matcher_verify_neighbourhood(self._m, C.byref(cells)), "verify_neighbourhood")
        self._check(self._L.ndt2d_matcher_verify_gates(self._m, C.byref(gi), C.byref(gp)), "verify_gates")
        self._check(self._L.ndt2d_matcher_verify_rays(self._m, C.byref(rays)), "verify_rays")
        return dict(neighbourhood=int(cells.value), gate_inlier=gi.value, gate_pierce=gp.value, rays=bool(rays.value))

    def verify_set_timing(self, enabled):
        """HIP events around the verification's kernel launch and read-back on / off (after the
        first verifyScans with an NDT in place: the object is made by it)."""
        self._batch_set_timing("verify", "verifyScans", enabled)

    def verify_last_ms(self):
        """(kernel_ms, fetch_ms) of the last timed verifyScans (its last chunk)."""
        return self._batch_last_ms("verify")

    def last_build(self):
        """How the NDT in place was built: "build/fused-small-map", "build/device", "build/host" or ""."""
        v = self._L.ndt2d_matcher_last_build(self._m)
        return v.decode() if v else ""

    def dropScans(self):
        """Forget every stored scan; ids start from 0 again."""
        self._check(self._L.ndt2d_matcher_drop_scans(self._m), "dropScans")

    def set_eigenvalue_form(self, form):
        """How Cell::compute's eigenvalues (src/ndt_model.cpp:84-85) are formed: "eigen" (default:
        Eigen 3.4.0's EigenSolver transcribed) or "closed" (the closed form of rounds 1-4)."""
        self._check(self._L.ndt2d_matcher_set_eigenvalue_form(self._m, form.encode()), "set_eigenvalue_form")

    # -- additive batched interface ------------------------------------------------

    def scorePoses(self, points, poses, out=None):
        """scores[i] == scorePoints(points, poses[i]), one launch.  `poses` / `out` from
        host_alloc() are used in place by the kernel (no copies)."""
        pts = _f64(points, (-1, 2))
        ps = _f64(poses, (-1, 3))
        if out is None:
            out = np.zeros(len(ps), dtype=np.float64)
        assert out.dtype == np.float64 and out.flags.c_contiguous and out.size == len(ps)
        self._check(self._L.ndt2d_matcher_score_poses(self._m, dptr(pts), len(pts), dptr(ps),
                                                      len(ps), dptr(out)), "scorePoses")
        return out

    # -- split matchScan / device-pointer launches (multi-GPU sharding, bench) ---------

    def prepare_search(self, scan_pose, points):
        """Subsample + build/upload the search tables.  Returns (n_th, n_lin, n_beams)."""
        sp = _f64(scan_pose, (3,))
        pts = _f64(points, (-1, 2))
        n_th, n_lin, n_b = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self._check(self._L.ndt2d_matcher_prepare_search(
            self._m, dptr(sp), dptr(pts), len(pts), C.byref(n_th), C.byref(n_lin),
            C.byref(n_b)), "prepare_search")
        return n_th.value, n_lin.value, n_b.value

    def prepare_beams(self, points):
        pts = _f64(points, (-1, 2))
        n_b = C.c_size_t(0)
        self._check(self._L.ndt2d_matcher_prepare_beams(self._m, dptr(pts), len(pts),
                                                        C.byref(n_b)), "prepare_beams")
        return n_b.value

    def _dev_check(self, rc, where):
        if rc != _capi.OK:
            msg = self._L.ndt2d_last_error(self.device_handle)
            raise Ndt2dError(rc, where, msg.decode() if msg else "")

    def match_launch(self, th_begin, th_end, record_ptr=None, scores_ptr=None):
        """Asynchronous slab search; record_ptr / scores_ptr are DEVICE addresses
        (e.g. torch tensor .data_ptr()) or None."""
        self._dev_check(self._L.ndt2d_match_launch(self.device_handle, th_begin, th_end,
                                                   scores_ptr, record_ptr), "ndt2d_match_launch")

    def match_launch_strided(self, th_first, th_stride, th_count, record_ptr=None, scores_ptr=None):
        """Asynchronous search of the theta steps th_first, th_first + th_stride, ...: one
        rank's share of an interleaved sharding (ndt_2d_amd.dist.shard_strided)."""
        self._dev_check(self._L.ndt2d_match_launch_strided(
            self.device_handle, th_first, th_stride, th_count, scores_ptr, record_ptr),
            "ndt2d_match_launch_strided")

    def match_fetch(self):
        res = _capi.MatchResult()
        self._dev_check(self._L.ndt2d_match_fetch(self.device_handle, C.byref(res)),
                        "ndt2d_match_fetch")
        rec = np.zeros(_capi.MATCH_RECORD_DOUBLES)
        rec[0] = res.best_score
        rec[1] = -1.0 if res.best_index == _capi.NO_INDEX else float(res.best_index) + (0.5 if res.near_tie else 0.0)
        rec[2:] = res.acc[:]
        return rec

    def finish_match(self, record, pose=None):
        """matchScan's outputs from a (combined) 12-double record."""
        rec = _f64(record, (_capi.MATCH_RECORD_DOUBLES,))
        pose_io = np.array([0.0, 0.0, 0.0] if pose is None else pose, dtype=np.float64)
        cov = np.zeros(9)
        score = C.c_double(0.0)
        self._check(self._L.ndt2d_matcher_finish_match(self._m, dptr(rec), dptr(pose_io),
                                                       dptr(cov), C.byref(score)), "finish_match")
        return dict(score=score.value, pose=pose_io, covariance=cov.reshape(3, 3))

    def score_poses_launch(self, poses_ptr, n_poses, scores_ptr, stats_ptr=None):
        """Asynchronous batched scorePoints on DEVICE pointers."""
        self._dev_check(self._L.ndt2d_score_poses_launch(self.device_handle, poses_ptr, n_poses,
                                                         scores_ptr, stats_ptr),
                        "ndt2d_score_poses_launch")

    def pf_finalize_launch(self, poses_ptr, n_poses, weights_ptr, stats_ptr, out_ptr):
        """updateStatistics on DEVICE pointers: weights normalised in place by the
        total weight in stats (all-reduced over ranks when sharded), out[8] =
        {sum w, mean x, mean y, mean theta, cov xx, cov xy, cov yy, theta-variance part}."""
        self._dev_check(self._L.ndt2d_pf_finalize_launch(self.device_handle, poses_ptr, n_poses,
                                                         weights_ptr, stats_ptr, out_ptr),
                        "ndt2d_pf_finalize_launch")

    def pf_noise_launch(self, seed, step, first_index, n, noise_ptr):
        """Write the Philox standard-normal stream of (seed, step) for particles
        first_index .. first_index + n into DEVICE float[n][3]."""
        self._dev_check(self._L.ndt2d_pf_noise_launch(self.device_handle, seed, step, first_index,
                                                      n, noise_ptr), "ndt2d_pf_noise_launch")

    def pf_motion_launch(self, poses_ptr, n, dx, dy, dth, alphas, noise_ptr=None, seed=0, step=0,
                         first_index=0):
        """MotionModel::sample (reference src/motion_model.cpp:45-83) in place on DEVICE
        poses[n][3]; noise_ptr = DEVICE float[n][3] standard normals or None (Philox)."""
        a = _f64(alphas, (5,))
        self._dev_check(self._L.ndt2d_pf_motion_launch(self.device_handle, poses_ptr, n, dx, dy,
                                                       dth, dptr(a), noise_ptr, seed, step,
                                                       first_index), "ndt2d_pf_motion_launch")

    def pf_init_launch(self, poses_ptr, n, x, y, theta, sigma_x, sigma_y, sigma_theta,
                       noise_ptr=None, seed=0, step=0, first_index=0):
        """ParticleFilter::init sampling loop (reference src/particle_filter.cpp:53-65)."""
        self._dev_check(self._L.ndt2d_pf_init_launch(self.device_handle, poses_ptr, n, x, y, theta,
                                                     sigma_x, sigma_y, sigma_theta, noise_ptr,
                                                     seed, step, first_index),
                        "ndt2d_pf_init_launch")

    def pose_moments_launch(self, poses_ptr, n, weights_ptr, stats_ptr):
        """Moment sums of updateStatistics for DEVICE weights (None = uniform 1/n)."""
        self._dev_check(self._L.ndt2d_pose_moments_launch(self.device_handle, poses_ptr, n,
                                                          weights_ptr, stats_ptr),
                        "ndt2d_pose_moments_launch")

    def create_resampler(self, n_capacity, max_particles_capacity):
        """A Resampler (ParticleFilter::resample on the device) on this matcher's device
        context: it draws from up to n_capacity particles, up to max_particles_capacity times."""
        r = Resampler(self, n_capacity, max_particles_capacity)
        if not hasattr(self, "_resamplers"):
            self._resamplers = weakref.WeakSet()
        self._resamplers.add(r)
        return r

    def pf_resample(self, particles, weights, min_particles, max_particles, kld_err, kld_z, uniforms,
                    leaf=(0.5, 0.5, 0.2671)):
        """ndt2d_pf_resample: kld_resample_native's arguments, computed on the device from host
        arrays.  Returns the indices of the draws kept."""
        pa = _f64(particles, (-1, 3))
        w = _f64(weights)
        u = _f64(uniforms)
        lf = _f64(leaf, (3,))
        out = np.empty(max(int(max_particles), 1), dtype=np.uint32)
        n_out = C.c_size_t(0)
        self._dev_check(self._L.ndt2d_pf_resample(
            self.device_handle, dptr(pa), dptr(w), len(w), int(min_particles), int(max_particles),
            float(kld_err), float(kld_z), dptr(lf), dptr(u), len(u),
            out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n_out)), "ndt2d_pf_resample")
        return out[:n_out.value].copy()

    def set_stream(self, stream_ptr):
        self._dev_check(self._L.ndt2d_set_stream(self.device_handle, stream_ptr),
                        "ndt2d_set_stream")
        self._bound_stream = bool(stream_ptr)

    def get_stream(self):
        """The caller-owned stream bound with set_stream, or None while the context
        launches on its own stream."""
        cur = self._L.ndt2d_get_stream(self.device_handle)
        return cur if getattr(self, "_bound_stream", None) else None

    def synchronize(self):
        self._dev_check(self._L.ndt2d_synchronize(self.device_handle), "ndt2d_synchronize")

    # -- introspection ---------------------------------------------------------------

    def has_ndt(self):
        return bool(self._L.ndt2d_matcher_has_ndt(self._m))

    def grid(self):
        """(cells6[ncell, 6], size_x, size_y, cell_size, origin_x, origin_y) of the host NDT."""
        sx, sy = C.c_uint32(0), C.c_uint32(0)
        cs, ox, oy = C.c_double(0), C.c_double(0), C.c_double(0)
        self._check(self._L.ndt2d_matcher_grid_info(self._m, C.byref(sx), C.byref(sy),
                                                    C.byref(cs), C.byref(ox), C.byref(oy)),
                    "grid_info")
        cells = np.zeros((sx.value * sy.value, 6), dtype=np.float64)
        self._check(self._L.ndt2d_matcher_grid_cells6(self._m, dptr(cells), len(cells)),
                    "grid_cells6")
        return cells, sx.value, sy.value, cs.value, ox.value, oy.value

    def last_launch_ms(self):
        ms = C.c_float(0)
        nk = C.c_int(0)
        rc = self._L.ndt2d_last_launch_ms(self.device_handle, C.byref(ms), C.byref(nk))
        if rc != _capi.OK:
            raise Ndt2dError(rc, "ndt2d_last_launch_ms")
        return ms.value, nk.value

    def launch_history_ms(self, n=256):
        """Kernel durations (ms) of the last up-to-n launches, oldest first; blocks until
        the newest has finished."""
        buf = (C.c_float * n)()
        got = C.c_size_t(0)
        self._dev_check(self._L.ndt2d_launch_history_ms(self.device_handle, buf, n, C.byref(got)),
                        "ndt2d_launch_history_ms")
        return [buf[i] for i in range(got.value)]

    def last_variant(self):
        v = self._L.ndt2d_last_variant(self.device_handle)
        return v.decode() if v else ""

    def set_pipeline_pieces(self, pieces):
        """ndt2d_set_pipeline_pieces: how a large pose batch from host memory is cut into
        overlapped upload / scoring / download pieces (0 default, 1 off)."""
        rc = self._L.ndt2d_set_pipeline_pieces(self.device_handle, int(pieces))
        if rc != 0:
            raise Ndt2dError(rc, "ndt2d_set_pipeline_pieces")

    def last_pipeline_pieces(self):
        return int(self._L.ndt2d_last_pipeline_pieces(self.device_handle))

    def set_variant(self, name):
        rc = self._L.ndt2d_set_variant(self.device_handle, name.encode())
        if rc != _capi.OK:
            raise Ndt2dError(rc, "ndt2d_set_variant")


class Resampler:
    """ndt2d_resampler: the KLD draw-and-stop loop of ParticleFilter::resample (reference
    src/particle_filter.cpp:91-137) as kernels on DEVICE pointers.  Launches go to the stream
    the matcher's device context is bound to; indices and count are those of the host form
    (particle_filter.kld_resample_native) for the same inputs."""

    def __init__(self, matcher, n_capacity, max_particles_capacity):
        self._L = matcher._L
        self._r = None
        self._matcher = matcher   # the context must outlive the resampler
        r = C.c_void_p()
        matcher._dev_check(self._L.ndt2d_resampler_create(matcher.device_handle, int(n_capacity),
                                                          int(max_particles_capacity), C.byref(r)),
                           "ndt2d_resampler_create")
        self._r = r
        self.n_capacity = int(n_capacity)
        self.max_particles_capacity = int(max_particles_capacity)

    def close(self):
        if getattr(self, "_r", None):
            self._L.ndt2d_resampler_destroy(self._r)
            self._r = None
        self._matcher = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, where):
        if rc != _capi.OK:
            msg = self._L.ndt2d_resampler_last_error(self._r)
            raise Ndt2dError(rc, where, msg.decode() if msg else "")

    def uniforms_launch(self, seed, step, first_index, n, out_ptr):
        """The Philox uniform stream of (seed, step) for draws first_index .. first_index + n
        into DEVICE double[n]: what launch() uses when uniforms_ptr is None."""
        self._check(self._L.ndt2d_resample_uniforms_launch(self._r, seed, step, first_index, n,
                                                           out_ptr),
                    "ndt2d_resample_uniforms_launch")

    def launch(self, particles_ptr, weights_ptr, n, min_particles, max_particles, kld_err, kld_z,
               particles_out_ptr, weights_out_ptr, indices_out_ptr=None, uniforms_ptr=None, seed=0,
               step=0, leaf=(0.5, 0.5, 0.2671)):
        """Asynchronous: draws, stop rule and the gather of the kept particles; every pointer
        is a DEVICE address.  fetch() returns the count kept."""
        lf = _f64(leaf, (3,))
        self._check(self._L.ndt2d_resample_launch(
            self._r, particles_ptr, weights_ptr, int(n), int(min_particles), int(max_particles),
            float(kld_err), float(kld_z), dptr(lf), uniforms_ptr, int(seed), int(step),
            particles_out_ptr, weights_out_ptr, indices_out_ptr), "ndt2d_resample_launch")

    def fetch(self):
        n = C.c_size_t(0)
        self._check(self._L.ndt2d_resample_fetch(self._r, C.byref(n)), "ndt2d_resample_fetch")
        return n.value

    def set_timing(self, enabled):
        self._check(self._L.ndt2d_resampler_set_timing(self._r, 1 if enabled else 0),
                    "ndt2d_resampler_set_timing")

    def cdf_ms(self):
        """Kernel time of the last launch's cumulative-weights chain (set_timing(True))."""
        ms = C.c_float(0.0)
        self._check(self._L.ndt2d_resampler_cdf_ms(self._r, C.byref(ms)), "ndt2d_resampler_cdf_ms")
        return ms.value


def pf_measure(matcher, particles, points, cov_prev=None):
    """ParticleFilter::measure (reference src/particle_filter.cpp:78-89) including its
    updateStatistics (:163-218).  Returns (normalised weights, mean[3], cov[3, 3]);
    cov_prev carries cov_(2,2), which the reference accumulates across calls."""
    L = _capi.lib()
    pa = _f64(particles, (-1, 3))
    pts = _f64(points, (-1, 2))
    w = np.zeros(len(pa), dtype=np.float64)
    mean = np.zeros(3)
    cov = np.zeros(9) if cov_prev is None else np.array(cov_prev, dtype=np.float64).reshape(9)
    matcher._check(L.ndt2d_matcher_pf_measure(matcher._m, dptr(pa), len(pa), dptr(pts),
                                              len(pts), dptr(w), dptr(mean), dptr(cov)),
                   "pf_measure")
    return w, mean, cov.reshape(3, 3)


def pf_update(matcher, particles, weights, dx, dy, dth, alphas, noise=None, seed=0, step=0,
              cov_prev=None):
    """ParticleFilter::update (reference src/particle_filter.cpp:71-76): the motion model
    on every particle, then updateStatistics.  noise = float32[n, 3] standard normals, or
    None for the device's Philox stream of (seed, step).  Returns (particles, normalised
    weights, mean[3], cov[3, 3])."""
    L = _capi.lib()
    pa = _f64(particles, (-1, 3)).copy()
    w = _f64(weights, (len(pa),)).copy()
    a = _f64(alphas, (5,))
    out = np.zeros(_capi.PF_RESULT_DOUBLES)
    zp = None
    if noise is not None:
        z = np.ascontiguousarray(noise, dtype=np.float32).reshape(len(pa), 3)
        zp = z.ctypes.data_as(C.POINTER(C.c_float))
    matcher._dev_check(L.ndt2d_pf_update(matcher.device_handle, dptr(pa), len(pa), dx, dy, dth,
                                         dptr(a), zp, seed, step, dptr(w), dptr(out)),
                       "ndt2d_pf_update")
    cov = np.zeros((3, 3)) if cov_prev is None else np.array(cov_prev, dtype=np.float64).reshape(3, 3)
    return pa, w, out[1:4].copy(), statistics_covariance(out, cov)


def statistics_covariance(out, cov_prev):
    """cov_ after updateStatistics from an NDT2D_PF_RESULT_DOUBLES record: the x/y block
    is overwritten (:208-211), (2,2) accumulates (:216), the rest is kept."""
    cov = np.array(cov_prev, dtype=np.float64).reshape(3, 3).copy()
    cov[0, 0] = out[4]
    cov[0, 1] = out[5]
    cov[1, 0] = out[5]
    cov[1, 1] = out[6]
    cov[2, 2] += out[7]
    return cov


def _index_array(call, name, what, values, K):
    """An optional per-job index list as the C-ABI takes it: uint32[K], or None."""
    if values is None:
        return None
    v = np.ascontiguousarray(values, dtype=np.int64).reshape(-1)
    if len(v) != K:
        raise ValueError("%s: %s must name one %s per job" % (call, name, what))
    if np.any(v < 0) or np.any(v >= 2 ** 32):
        raise ValueError("%s: %s must hold %s indices" % (call, name, what))
    return np.ascontiguousarray(v, dtype=np.uint32)


class _JobList:
    """K (scan, pose) jobs over S scans as the C-ABI takes them (matchScans, refineScans,
    verifyScans, refineCandidates, verifyCandidates): jp [K, 3], arrays (the scans), pts (their
    points, each scan once), offsets (uintp [S + 1]), js (uint32 [K], or None: job k uses scan k).
    args: jobs_xyt, job_scan, n_jobs, points_xy, point_offsets, n_scans."""

    def __init__(self, call, jobs, scans, job_scan):
        self.jp = _f64(jobs, (-1, 3))
        self.K = len(self.jp)
        self.arrays = [_f64(pts, (-1, 2)) for pts in scans]
        self.offsets = np.zeros(len(self.arrays) + 1, dtype=np.uintp)
        if self.arrays:
            self.offsets[1:] = np.cumsum([len(a) for a in self.arrays])
        self.pts = np.ascontiguousarray(np.concatenate(self.arrays) if self.arrays else np.zeros((0, 2)), dtype=np.float64)
        self.js = _index_array(call, "job_scan", "scan", job_scan, self.K)
        self.args = (dptr(self.jp), self.js.ctypes.data_as(C.POINTER(C.c_uint32)) if self.js is not None else None, self.K,
                     dptr(self.pts), self.offsets.ctypes.data_as(C.POINTER(C.c_size_t)), len(self.arrays))

    def scan_of(self, k):
        return int(self.js[k]) if self.js is not None else k


def _pack_candidates(candidates):
    """Candidate maps, each a list of (stored scan id, pose_xyt), as the C-ABI takes them:
    (cand_offsets uintp [K + 1], ids uintp, poses_xyt [n, 3])."""
    offsets = np.zeros(len(candidates) + 1, dtype=np.uintp)
    if len(candidates):
        offsets[1:] = np.cumsum([len(c) for c in candidates])
    flat = [entry for c in candidates for entry in c]
    ids = np.ascontiguousarray([e[0] for e in flat], dtype=np.uintp).reshape(-1)
    poses = _f64([e[1] for e in flat], (-1, 3)) if flat else np.zeros((0, 3))
    return offsets, ids, poses


class _RefineCall:
    """The jobs and scans of a Newton registration as the C-ABI takes them, its output arrays, and
    the dicts they become (refineScans, refineCandidates)."""

    def __init__(self, call, params, jobs, scans, job_scan, max_evals):
        self.list = _JobList(call, jobs, scans, job_scan)
        self.K = K = self.list.K
        if not 0 <= int(max_evals) < 2 ** 32:
            raise ValueError("%s: max_evals must fit 32 bits" % call)
        self.beams_max = int(params["laser_max_beams"])
        self.poses, self.scores, self.starts = np.zeros((K, 3)), np.zeros(K), np.zeros(K)
        self.grads, self.hess = np.zeros((K, 3)), np.zeros((K, 3, 3))
        self.status, self.evals = np.zeros(K, dtype=np.int32), np.zeros((K, 2), dtype=np.uint32)
        self.job_args = self.list.args
        self.out_args = (dptr(self.poses), dptr(self.scores), dptr(self.starts), dptr(self.grads), dptr(self.hess),
                         self.status.ctypes.data_as(C.POINTER(C.c_int32)), self.evals.ctypes.data_as(C.POINTER(C.c_uint32)))

    def dicts(self):
        out = []
        for k in range(self.K):
            n = min(self.beams_max, len(self.list.arrays[self.list.scan_of(k)]))
            out.append(dict(pose=self.poses[k].copy(), score=float(self.scores[k]), start_score=float(self.starts[k]),
                            gradient=self.grads[k].copy(), hessian=self.hess[k].copy(), evals=int(self.evals[k, 0]),
                            steps=int(self.evals[k, 1]), status=int(self.status[k]),
                            covariance=refine_covariance(self.hess[k] * float(n))))
        return out


def loop_closure_window(i, rolling):
    """The scans a loop-closure candidate map is built from (reference src/ndt_mapper.cpp:
    628-631): [begin_idx, end_idx) = "one additional scan on either side of candidate" as the
    reference computes it -- the scan before `i` and `i` itself, only scan 0 for i == 0, and, its
    quirk, only scan i - 1 for the candidate i == rolling (end_idx stays i there)."""
    begin_idx = i - 1 if i > 0 else i
    end_idx = i + 1 if i < rolling else i
    return list(range(begin_idx, end_idx))


def _refine_usable(r):
    """close_loops adopts a refined pose: the registration ended in order and f did not rise."""
    return r["status"] in (_capi.REFINE_CONVERGED, _capi.REFINE_MAX_EVALS) and r["score"] <= r["start_score"]


def close_loops(matcher, scan_pose, points, candidate_indices, graph_poses, rolling, typical_response, limit,
                scan_sizes=None, refine=None, verify=None):
    """The loop-closure thread's walk over one new scan's candidates (reference
    src/ndt_mapper.cpp:619-671) on the batched match.  candidate_indices: what findNearest
    returned, in its order; graph_poses[i]: the pose of graph scan i, which is stored on the
    matcher under id i; scan_sizes (optional): graph scan i's point count, to skip candidates
    whose scan is empty (:625).  A skipped candidate does not count against `limit`, every
    other one does (:670, `if (--num_scans_to_check == 0) break;` -- so limit == 0 never
    reaches zero and checks them all, as the reference's unsigned counter does).

    All remaining candidates are matched in one matchCandidates call from the scan's current
    pose; the results are walked in order, and a candidate is accepted when
    isfinite(score) and score < typical_response (:645).  An accept moves the scan's pose
    (:652-655), which every later candidate of the reference's loop starts from: the rest is
    matched again, in one batch, from the corrected pose.

    Returns (pose, accepted): the scan's final pose and a list of dict(candidate, score,
    correction, covariance, pose) in the order the constraints would be added.

    refine: None, or dict(max_evals=..., tol_lin=..., tol_ang=..., neighbourhood=...) (any subset:
    refineCandidates' arguments).  With it every round's matchCandidates is followed by ONE
    refineCandidates call -- the Newton registration on each candidate's own map -- for every
    candidate of the round that passes the accept test, each started from pose + its correction.
    The accept test stays the reference's, on the lattice score, and the walk consumes the first
    accepted candidate as before; its entry gains refined_pose, refined_covariance (None where the
    Hessian is not positive definite), refine_status and refine_usable, the rule of the next
    sentence as a flag (its `pose` stays the lattice pose).  The
    scan's pose -- what the next round starts from, and what is returned -- is the refined pose
    where the status is CONVERGED or MAX_EVALS and f did not rise, the lattice pose otherwise.

    verify: None, or dict(max_beams=..., neighbourhood=..., gate_inlier=..., gate_pierce=..., rays=...)
    (any subset: verifyCandidates' arguments, as relocalize's `verify`).  With it every round makes
    ONE verifyCandidates call over the candidates that pass the accept test, each on its own map at
    the pose the walk would adopt for it -- the refined pose where `refine` is given and usable by
    the rule above, the lattice pose otherwise.  The accepted entry gains `verify` (the counts) and
    `verified_pose`.  The walk, the accepted list and the returned pose are what they are without
    it: a verdict, no policy."""
    pose = np.array(scan_pose, dtype=np.float64).reshape(3).copy()
    todo = []
    for i in candidate_indices:
        if scan_sizes is not None and scan_sizes[i] == 0:
            continue                                   # `if (candidate->getPoints().empty()) continue;`
        todo.append(int(i))
        if limit and len(todo) == limit:               # `if (--num_scans_to_check == 0) break;`
            break
    accepted = []
    while todo:
        batch = [[(j, graph_poses[j]) for j in loop_closure_window(i, rolling)] for i in todo]
        results = matcher.matchCandidates(pose, points, batch)
        passing = [k for k, res in enumerate(results) if np.isfinite(res["score"]) and res["score"] < typical_response]
        refined = None
        if refine is not None and passing:
            starts = [np.array(results[k]["pose"], dtype=np.float64) + pose for k in passing]
            refined = matcher.refineCandidates(starts, [points], [batch[k] for k in passing], job_scan=[0] * len(passing),
                                               **refine)
        verdicts = None
        if verify is not None and passing:
            adopted = []
            for n, k in enumerate(passing):
                at = np.array(results[k]["pose"], dtype=np.float64) + pose
                if refined is not None and _refine_usable(refined[n]):
                    at = refined[n]["pose"].copy()
                adopted.append(at)
            verdicts = matcher.verifyCandidates(adopted, [points], [batch[k] for k in passing], job_scan=[0] * len(passing),
                                                **verify)
        rest = []
        for k in passing[:1]:
            i, res = todo[k], results[k]
            correction = np.array(res["pose"], dtype=np.float64)
            pose = correction + pose                   # correction.x += scan->getPose().x; ... (:652-654)
            entry = dict(candidate=i, score=res["score"], correction=correction, covariance=res["covariance"], pose=pose.copy())
            if refined is not None:
                r = refined[0]
                entry.update(refined_pose=r["pose"].copy(), refined_covariance=r["covariance"], refine_status=r["status"],
                             refine_usable=_refine_usable(r))
                if _refine_usable(r):
                    pose = r["pose"].copy()
            if verdicts is not None:
                entry.update(verify=verdicts[0], verified_pose=adopted[0].copy())
            accepted.append(entry)
            rest = todo[k + 1:]
        todo = rest
    return pose, accepted


def heading_fan(poses, n_headings):
    """Every pose under n_headings equally spaced headings, the first its own: pose k gives
    (x, y, theta + 2 pi j / n_headings), j = 0 .. n_headings - 1, in that order.  Seeds for
    relocalize() from graph nodes, whose stored heading says nothing about the robot's."""
    ps = np.array(poses, dtype=np.float64).reshape(-1, 3)
    n = int(n_headings)
    if n < 1:
        raise ValueError("heading_fan: n_headings must be at least 1")
    out = np.repeat(ps, n, axis=0)
    out[:, 2] += np.tile(np.arange(n) * (2.0 * np.pi / n), len(ps))
    return out


def relocalize(matcher, points, start_poses, accept_below=None, verify=None):
    """Where in the matcher's map was this scan taken?  One matchStarts call from every start
    pose -- what a node that loaded its map does instead of refusing scans until somebody posts
    `initialpose` (reference src/ndt_mapper.cpp:315-320).  Returns the starts ranked by score
    (lower is better), ties in start order: a list of dict(start = index into start_poses,
    correction = matchScan's pose output, pose = start pose + correction as the reference adds
    it (:557-561), score, covariance).  Starts without a winner (no lattice candidate below 0)
    follow those with one, non-finite scores come last.  accept_below: keep only
    isfinite(score) and score < accept_below, the loop-closure rule (:645).

    verify: None, or dict(max_beams=..., neighbourhood=..., gate_inlier=..., gate_pierce=..., rays=...)
    (any subset: verifyScans' arguments).  With it the ranked starts gain `verify`: the
    verification counts of the scan at their corrected pose, from ONE extra verifyScans call over
    all of them.  The ranking and what is kept stay as they are: a verdict, no policy."""
    starts = np.array(start_poses, dtype=np.float64).reshape(-1, 3)
    if len(starts) == 0:
        return []
    results = matcher.matchStarts(starts, points)
    ranked = []
    for k, res in enumerate(results):
        score = float(res["score"])
        if accept_below is not None and not (np.isfinite(score) and score < accept_below):
            continue
        correction = np.array(res["pose"], dtype=np.float64)
        finite = bool(np.isfinite(score))
        winner = res["best_index"] != _capi.NO_INDEX
        key = (0 if finite else 1, 0 if winner else 1, score if finite else 0.0, k)
        ranked.append((key, dict(start=k, correction=correction, pose=correction + starts[k], score=score,
                                 covariance=res["covariance"])))
    ranked.sort(key=lambda e: e[0])
    entries = [entry for _, entry in ranked]
    if verify is not None and entries:
        counts = matcher.verifyScans([e["pose"] for e in entries], [points], job_scan=[0] * len(entries), **verify)
        for e, c in zip(entries, counts):
            e["verify"] = c
    return entries


def track_scans(matcher, jobs, scans, job_scan=None):
    """Localisation by scan matching for many scans at once (reference src/ndt_mapper.cpp:547-566):
    one matchScans call over the (scan, pose) jobs against the matcher's map.  Returns, in job
    order, a list of dict(job = index into jobs, scan = index into scans, score, correction =
    matchScan's pose output, pose = job pose + correction as the reference adds it (:557-561),
    covariance).  A job without a winner (no lattice candidate below 0) keeps its pose."""
    poses = np.array(jobs, dtype=np.float64).reshape(-1, 3)
    if len(poses) == 0:
        return []
    which = np.arange(len(poses)) if job_scan is None else np.array(job_scan, dtype=np.int64).reshape(-1)
    results = matcher.matchScans(poses, scans, job_scan=job_scan)
    out = []
    for k, res in enumerate(results):
        correction = np.array(res["pose"], dtype=np.float64)
        out.append(dict(job=k, scan=int(which[k]), score=float(res["score"]), correction=correction,
                        pose=correction + poses[k], covariance=res["covariance"]))
    return out


def explained_mask(result):
    """The beams of a verifyScans result (one job's dict, want_beams=True) worth storing: the map
    does not contradict them -- class is not BEAM_OUTLIER and the ray is not pierced.  A bool array
    over the job's beams (with max_beams=0: over the scan's points)."""
    return (np.asarray(result["classes"]) != _capi.BEAM_OUTLIER) & ~np.asarray(result["pierced_mask"], dtype=bool)


def refine_covariance(hessian):
    """H^-1 through ndt2d_refine_covariance (host arithmetic, no device): hessian is the SUM's
    Hessian, a [3, 3] array or the record's six entries xx, xy, xt, yy, yt, tt.  A [3, 3] array, or
    None where H is not positive definite or not finite."""
    h = np.asarray(hessian, dtype=np.float64)
    if h.size == 9:
        h = h.reshape(3, 3)
        h = np.array([h[0, 0], h[0, 1], h[0, 2], h[1, 1], h[1, 2], h[2, 2]])
    h6 = np.ascontiguousarray(h.reshape(6), dtype=np.float64)
    cov = np.zeros(9)
    rc = _capi.lib().ndt2d_refine_covariance(dptr(h6), dptr(cov))
    if rc == _capi.OK:
        return cov.reshape(3, 3)
    if rc == _capi.ERR_STATE:
        return None
    raise Ndt2dError(rc, "ndt2d_refine_covariance", "")


def refine_matches(matcher, jobs, scans, job_scan=None, **kw):
    """The lattice search, then the Newton registration from its winners: one matchScans call over
    the (scan, pose) jobs, one refineScans call from each job's winner -- job pose + correction as
    the reference adds it (src/ndt_mapper.cpp:557-561), the job's own pose where no lattice
    candidate scored below 0.  kw: refineScans' max_evals, tol_lin, tol_ang, neighbourhood.  Returns, in job
    order, a list of dict(job, scan, match = matchScans' dict, start = the pose handed on,
    refined = refineScans' dict, pose = refined["pose"], score = refined["score"])."""
    poses = np.array(jobs, dtype=np.float64).reshape(-1, 3)
    if len(poses) == 0:
        return []
    which = np.arange(len(poses)) if job_scan is None else np.array(job_scan, dtype=np.int64).reshape(-1)
    matches = matcher.matchScans(poses, scans, job_scan=job_scan)
    starts = np.array([np.array(res["pose"], dtype=np.float64) + poses[k] if res["best_index"] != _capi.NO_INDEX
                       else poses[k] for k, res in enumerate(matches)]).reshape(-1, 3)
    refined = matcher.refineScans(starts, scans, job_scan=job_scan, **kw)
    return [dict(job=k, scan=int(which[k]), match=matches[k], start=starts[k].copy(), refined=refined[k],
                 pose=np.array(refined[k]["pose"], dtype=np.float64), score=float(refined[k]["score"]))
            for k in range(len(poses))]
