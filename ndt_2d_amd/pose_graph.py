"""The pose graph on the device: ndt2d_posegraph (include/ndt2d_hip.h, "Pose graph") and what turns
the loop-closure results into its constraints.

`PoseGraph(matcher)` stands beside the matcher's device context, as `Resampler` does: `set_graph`
uploads poses and constraints, `evaluate` gives the residuals and the cost, `optimize` moves the
poses -- K masks over one graph in one launch.  `make_constraint` restates the reference's
makeConstraint (src/constraint.cpp:35-56), `closure_constraints` turns `close_loops`' accepted list
into the switchable constraints the loop-closure thread adds (src/ndt_mapper.cpp:658-661).
`graph_io.Graph.optimize` is CeresSolver::optimize on top of these."""
import ctypes as C
import math

import numpy as np

from . import _capi
from ._capi import Ndt2dError, dptr
from .graph_io import Constraint

DEFAULT_COVARIANCE_WORKSPACE = 1 << 30   # bytes of the dense covariance's workspace: 2,700 poses a job
DEFAULT_DIRECT_WORKSPACE = 1 << 30       # bytes of the direct solve's workspace: 3,800 poses a job
DEFAULT_TOLERANCES = dict(max_iterations=100, gradient_tolerance=1e-10, function_tolerance=1e-6, parameter_tolerance=1e-8)
# the objects that stand beside the pose graph's, by the noun of their ndt2d_<noun>_* functions: the attribute with the handle
DEFAULT_SPARSE_WORKSPACE = 1 << 30       # bytes of the sparse solve's workspace: about 1 KiB a pose and 72 s^2 for s separators
DEFAULT_SPARSECOV_WORKSPACE = 1 << 30     # bytes of the sparse covariance's workspace: about 1.3 KiB a pose and 144 s^2 for s separators
_COMPANIONS = dict(covariance="_cov", direct="_direct", sparse="_sparse", sparsecov="_sparsecov")


def _tolerances(who, given):
    """(max_iterations, gradient, function, parameter tolerance) as a solve takes them: DEFAULT_TOLERANCES under the
    caller's keywords; TypeError names `who` and the keywords that are none of them."""
    unknown = set(given) - set(DEFAULT_TOLERANCES)
    if unknown:
        raise TypeError("%s: unknown argument(s) %s" % (who, sorted(unknown)))
    tol = dict(DEFAULT_TOLERANCES, **given)
    return int(tol["max_iterations"]), float(tol["gradient_tolerance"]), float(tol["function_tolerance"]), float(tol["parameter_tolerance"])


def _inverse3(m):
    """The inverse of a 3 x 3 by cofactors (Eigen's Matrix3d::inverse)."""
    a, b, c, d, e, f, g, h, i = (float(v) for v in np.asarray(m, dtype=np.float64).reshape(9))
    c00, c01, c02 = e * i - f * h, f * g - d * i, d * h - e * g
    det = a * c00 + b * c01 + c * c02
    inv = 1.0 / det
    return np.array([[c00 * inv, (c * h - b * i) * inv, (b * f - c * e) * inv],
                     [c01 * inv, (a * i - c * g) * inv, (c * d - a * f) * inv],
                     [c02 * inv, (b * g - a * h) * inv, (a * e - b * d) * inv]])


def make_constraint(begin, end, from_pose, to_pose, covariance):
    """makeConstraint (src/constraint.cpp:35-56): the transform is to_pose in from_pose's frame, the
    heading difference is not wrapped, the information is the covariance's inverse; not switchable."""
    fx, fy, fth = (float(v) for v in from_pose)
    tx, ty, tth = (float(v) for v in to_pose)
    dx, dy = tx - fx, ty - fy
    costh, sinth = math.cos(fth), math.sin(fth)
    transform = (costh * dx + sinth * dy, -sinth * dx + costh * dy, tth - fth)
    return Constraint(begin, end, transform, _inverse3(covariance), switchable=False)


def closure_constraints(accepted, scan_index, graph_poses):
    """`close_loops`' accepted list as the constraints the loop-closure thread adds: for each entry
    makeConstraint(candidate, scan, covariance) with the scan at the pose the walk adopted for it,
    switchable.  Where the entry has a refined pose the walk adopted (`refine_usable`, close_loops'
    own rule) and a refined covariance, these are used; the lattice pose and covariance otherwise."""
    out = []
    for entry in accepted:
        pose, covariance = entry["pose"], entry["covariance"]
        if entry.get("refine_usable") and entry.get("refined_covariance") is not None:
            pose, covariance = entry["refined_pose"], entry["refined_covariance"]
        c = make_constraint(entry["candidate"], scan_index, graph_poses[entry["candidate"]], pose, covariance)
        c.switchable = True
        out.append(c)
    return out


def check_masks(masks, switchable):
    """masks [K, m] as bytes (non-zero: on).  A mask may switch off switchable constraints only:
    ValueError names the first mask and constraint that break the rule."""
    switchable = np.asarray(switchable, dtype=bool).reshape(-1)
    en = np.ascontiguousarray(np.asarray(masks).reshape(-1, len(switchable)) != 0, dtype=np.uint8)
    off = (en == 0) & ~switchable[None, :]
    if off.any():
        k, c = (int(v) for v in np.argwhere(off)[0])
        raise ValueError("mask %d switches off constraint %d, which is not switchable" % (k, c))
    return en


def robust_weights(kind, scale, chi2):
    """rho'(chi2) of the loss `kind` at `scale`, elementwise: what ndt2d_robust_rho gives as rho',
    bit for bit (IEEE division and square root only), without a call per value."""
    s = np.asarray(chi2, dtype=np.float64)
    a = float(scale)
    b = a * a
    tiny = np.finfo(np.float64).tiny
    if kind == "trivial":
        return np.ones_like(s)
    if kind == "huber":
        inside = s <= b
        return np.where(inside, 1.0, np.maximum(tiny, a / np.sqrt(np.where(inside, 1.0, s))))
    if kind == "cauchy":
        with np.errstate(over="ignore"):   # (s / b beyond the doubles: rho' is DBL_MIN there)
            return np.maximum(tiny, 1.0 / (1.0 + s / b))
    raise ValueError("robust_weights: \"%s\" (\"trivial\", \"huber\" or \"cauchy\")" % kind)


def relative_covariance(pose_a, pose_b, joint):
    """ndt2d_marginals_relative: (transform [3], covariance [3, 3]) of pose b in pose a's frame from
    the joint marginal [2, 2, 3, 3] = [[aa, ab], [ba, bb]] (marginals' blocks for nodes = [a, b])."""
    pa = np.ascontiguousarray(pose_a, dtype=np.float64).reshape(3)
    pb = np.ascontiguousarray(pose_b, dtype=np.float64).reshape(3)
    j = np.ascontiguousarray(joint, dtype=np.float64).reshape(36)
    t, cov = np.zeros(3), np.zeros((3, 3))
    rc = _capi.lib().ndt2d_marginals_relative(dptr(pa), dptr(pb), dptr(j), dptr(t), dptr(cov))
    if rc != _capi.OK:
        raise Ndt2dError(rc, "ndt2d_marginals_relative", "a value is not finite")
    return t, cov


def closure_distance(transform_pred, covariance_pred, transform_meas, covariance_meas):
    """ndt2d_marginals_distance: d^2 = e^T (covariance_pred + covariance_meas)^-1 e of
    e = meas - pred, the heading through Normalize.  Ndt2dError where the sum is not positive
    definite.  A verdict: against chi^2 with 3 degrees of freedom if both covariances are honest."""
    args = [np.ascontiguousarray(v, dtype=np.float64).reshape(size)
            for v, size in ((transform_pred, 3), (covariance_pred, 9), (transform_meas, 3), (covariance_meas, 9))]
    d2 = np.zeros(1)
    rc = _capi.lib().ndt2d_marginals_distance(dptr(args[0]), dptr(args[1]), dptr(args[2]), dptr(args[3]), dptr(d2))
    if rc != _capi.OK:
        raise Ndt2dError(rc, "ndt2d_marginals_distance", "a value is not finite, or the covariances' sum is not positive definite")
    return float(d2[0])


class PoseGraph:
    """ndt2d_posegraph on the matcher's device context.  The capacities grow with the graphs given
    to set_graph (the object is made anew when one is passed)."""

    def __init__(self, matcher, max_nodes=1024, max_constraints=4096, max_jobs=256):
        self._L = matcher._L
        self._p = None
        self._matcher = matcher   # the context must outlive the object
        self._caps = (0, 0, 0)
        self._weighting = "reference"
        self._preconditioner = "jacobi"
        self._loss = ("trivial", 1.0, "all")   # kind, scale, on
        self._timing = False
        self._cov = None           # the dense covariance's object (covariances), made at its first call
        self._cov_bytes = 0
        self._direct = None        # the direct solve's object (optimize_direct), made at its first call
        self._direct_bytes = 0
        self._sparse = None        # the sparse solve's object (optimize_sparse, sparse_layout), made at its first call
        self._sparse_bytes = 0
        self._sparsecov = None     # the sparse covariance's object (covariances_sparse), made at its first call
        self._sparsecov_bytes = 0
        self.n = self.m = 0
        self.switchable = np.zeros(0, dtype=bool)
        self._create(int(max_nodes), int(max_constraints), int(max_jobs))

    def _create(self, max_nodes, max_constraints, max_jobs):
        p = C.c_void_p()
        self._matcher._dev_check(self._L.ndt2d_posegraph_create(self._matcher.device_handle, max_nodes, max_constraints, max_jobs, C.byref(p)),
                                 "ndt2d_posegraph_create")
        self._close_companions()   # (they refer to the object that goes)
        old, self._p = self._p, p
        if old:
            self._L.ndt2d_posegraph_destroy(old)
        self._caps = (max_nodes, max_constraints, max_jobs)
        self._check(self._L.ndt2d_posegraph_set_weighting(self._p, self._weighting.encode()), "ndt2d_posegraph_set_weighting")
        self._check(self._L.ndt2d_pose_graph_set_preconditioner(self._p, self._preconditioner.encode()), "ndt2d_pose_graph_set_preconditioner")
        if self._loss[0] != "trivial":
            self._check(self._L.ndt2d_robust_set_loss(self._p, self._loss[0].encode(), self._loss[1]), "ndt2d_robust_set_loss")
        if self._timing:
            self.set_timing(True)

    def _companion(self, noun, workspace_bytes):
        """The object ndt2d_<noun> beside the graph's: made at its first use and again when workspace_bytes changes,
        with the timing flag passed on."""
        attr, lib = _COMPANIONS[noun], self._L
        if getattr(self, attr) is None or getattr(self, attr + "_bytes") != int(workspace_bytes):
            self._close_companion(noun)
            p = C.c_void_p()
            rc = getattr(lib, "ndt2d_%s_create" % noun)(self._p, int(workspace_bytes), C.byref(p))
            if rc != _capi.OK:
                raise Ndt2dError(rc, "ndt2d_%s_create" % noun, "workspace_bytes = %d" % int(workspace_bytes))
            setattr(self, attr, p)
            setattr(self, attr + "_bytes", int(workspace_bytes))
            if self._timing:
                getattr(lib, "ndt2d_%s_set_timing" % noun)(p, 1)
        return getattr(self, attr)

    def _companion_check(self, noun, rc, where):
        """_check with the companion's own last error."""
        if rc != _capi.OK:
            msg = getattr(self._L, "ndt2d_%s_last_error" % noun)(getattr(self, _COMPANIONS[noun]))
            raise Ndt2dError(rc, where, msg.decode() if msg else "")

    def _companion_last_ms(self, noun):
        a, b = C.c_float(0.0), C.c_float(0.0)
        rc = getattr(self._L, "ndt2d_%s_last_ms" % noun)(getattr(self, _COMPANIONS[noun]), C.byref(a), C.byref(b))
        self._companion_check(noun, rc, "ndt2d_%s_last_ms" % noun)
        return a.value, b.value

    def _close_companion(self, noun):
        if getattr(self, _COMPANIONS[noun], None):
            getattr(self._L, "ndt2d_%s_destroy" % noun)(getattr(self, _COMPANIONS[noun]))
        setattr(self, _COMPANIONS[noun], None)

    def _close_companions(self):
        for noun in _COMPANIONS:
            self._close_companion(noun)

    def close(self):
        self._close_companions()
        if getattr(self, "_p", None):
            self._L.ndt2d_posegraph_destroy(self._p)
            self._p = None
        self._matcher = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, where):
        if rc != _capi.OK:
            msg = self._L.ndt2d_posegraph_last_error(self._p)
            raise Ndt2dError(rc, where, msg.decode() if msg else "")

    def set_weighting(self, weighting):
        """"reference": W = L, the reference's; "information": W = L^T, the cost is e^T information e."""
        self._check(self._L.ndt2d_posegraph_set_weighting(self._p, str(weighting).encode()), "ndt2d_posegraph_set_weighting")
        self._weighting = str(weighting)

    def weighting(self):
        return self._L.ndt2d_posegraph_weighting(self._p).decode()

    def set_preconditioner(self, preconditioner):
        """The CG's preconditioner: "jacobi" (the default: each node's 3 x 3 block of H + lambda D) or
        "chain" (the block-tridiagonal band of H + lambda D over the nodes in node order, solved exactly
        by block cyclic reduction: for graphs whose odometry runs along the node order)."""
        self._check(self._L.ndt2d_pose_graph_set_preconditioner(self._p, str(preconditioner).encode()), "ndt2d_pose_graph_set_preconditioner")
        self._preconditioner = str(preconditioner)

    def preconditioner(self):
        return self._L.ndt2d_pose_graph_preconditioner(self._p).decode()

    def set_loss(self, kind, scale=1.0, on="all"):
        """The loss rho of the cost F = 1/2 sum rho(chi2): "trivial" (the default, rho(s) = s),
        "huber" or "cauchy" at `scale` (include/ndt2d_hip.h, "Robust losses").  on: the constraints
        it applies to -- "all", "switchable" (those set_graph was told are switchable: the closures)
        or a byte array [m] (non-zero: applied).  Kept across set_graph; "all" and "switchable" are
        applied anew to every graph, an array to graphs of its length."""
        kind = str(kind)
        if not isinstance(on, str):
            on = np.ascontiguousarray(np.asarray(on).reshape(-1) != 0, dtype=np.uint8)
            if self.n and len(on) != self.m:
                raise ValueError("set_loss: on has %d entries, the graph has %d constraints" % (len(on), self.m))
        elif on not in ("all", "switchable"):
            raise ValueError("set_loss: on = %r (\"all\", \"switchable\" or a byte array)" % (on,))
        self._check(self._L.ndt2d_robust_set_loss(self._p, kind.encode(), float(scale)), "ndt2d_robust_set_loss")
        self._loss = (kind, self.loss()[1], on)
        if self.n:
            self._select()

    def loss(self):
        """(kind, scale) as the object holds them."""
        scale = C.c_double(0.0)
        return self._L.ndt2d_robust_loss(self._p, C.byref(scale)).decode(), scale.value

    def _select(self):
        """The loss's selection for the graph in place."""
        on = self._loss[2]
        if isinstance(on, str):
            sel = None if on == "all" else np.ascontiguousarray(self.switchable, dtype=np.uint8)
        else:
            if len(on) != self.m:
                raise ValueError("set_loss: on has %d entries, the graph has %d constraints" % (len(on), self.m))
            sel = on
        self._check(self._L.ndt2d_robust_select(self._p, self._u8(sel), self.m), "ndt2d_robust_select")

    def set_graph(self, poses, constraints=None, fixed=0, begin=None, end=None, transform=None, information=None, switchable=None):
        """poses [n, 3]; the constraints as graph_io.Constraint objects, or as the arrays begin, end
        [m], transform [m, 3], information [m, 3, 3] and (optional) switchable [m]."""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        if constraints is not None:
            begin = [c.begin for c in constraints]
            end = [c.end for c in constraints]
            transform = [c.transform for c in constraints]
            information = [c.information for c in constraints]
            switchable = [c.switchable for c in constraints]
        m = 0 if begin is None else len(begin)
        for name, idx in (("begin", begin), ("end", end)):
            for c in range(m):
                if not 0 <= int(idx[c]) < 2 ** 32:
                    raise ValueError("constraint %d: %s = %d" % (c, name, int(idx[c])))
        b = np.ascontiguousarray(np.zeros(0) if m == 0 else begin, dtype=np.uint32).reshape(m)
        e = np.ascontiguousarray(np.zeros(0) if m == 0 else end, dtype=np.uint32).reshape(m)
        t = np.ascontiguousarray(np.zeros((0, 3)) if m == 0 else transform, dtype=np.float64).reshape(m, 3)
        info = np.ascontiguousarray(np.zeros((0, 9)) if m == 0 else information, dtype=np.float64).reshape(m, 9)
        caps = self._caps
        if len(poses) > caps[0] or m > caps[1]:
            self._create(max(caps[0], len(poses)), max(caps[1], m), caps[2])
        u32p = C.POINTER(C.c_uint32)
        self._check(self._L.ndt2d_posegraph_set_graph(self._p, dptr(poses), len(poses), b.ctypes.data_as(u32p), e.ctypes.data_as(u32p), dptr(t),
                                                      dptr(info), m, int(fixed)), "ndt2d_posegraph_set_graph")
        self.n, self.m = len(poses), m
        self.switchable = np.zeros(m, dtype=bool) if switchable is None else np.array(switchable, dtype=bool).reshape(m)
        if self._loss[0] != "trivial" and not (isinstance(self._loss[2], str) and self._loss[2] == "all"):
            self._select()                                            # (set_graph has reset the selection to every constraint)

    @staticmethod
    def _solved(poses, records, chi2, fields, weights):
        """A solve's records as its dicts: fields = (key, type) per double of a record behind the status."""
        out = []
        for k in range(len(records)):
            status = int(records[k, 0])
            d = dict(poses=poses[k].copy(), status=status, status_name=_capi.POSEGRAPH_STATUS_NAMES[status])
            d.update((key, kind(records[k, 1 + i])) for i, (key, kind) in enumerate(fields))
            d.update(chi2_start=chi2[k, 0].copy(), chi2=chi2[k, 1].copy())
            if weights is not None:
                d["weights"] = weights[k]
            out.append(d)
        return out

    def _masks(self, masks):
        """(bytes [K, m] or None, K); a mask may switch off switchable constraints only."""
        if masks is None:
            return None, 1
        en = check_masks(masks, self.switchable)
        return en, len(en)

    @staticmethod
    def _u8(a):
        return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))

    def evaluate(self, masks=None, want_residuals=False):
        """At the graph's poses, per mask (None: one job, every constraint on): dict(cost, chi2 [m],
        and with want_residuals e [m, 3] and r [m, 3])."""
        en, K = self._masks(masks)
        cost = np.zeros(K)
        chi2 = np.zeros((K, self.m))
        res = np.zeros((K, self.m, 6)) if want_residuals else None
        self._check(self._L.ndt2d_posegraph_evaluate(self._p, self._u8(en), K, dptr(cost), dptr(chi2), None if res is None else dptr(res)),
                    "ndt2d_posegraph_evaluate")
        out = []
        for k in range(K):
            d = dict(cost=float(cost[k]), chi2=chi2[k].copy())
            if want_residuals:
                d.update(e=res[k, :, :3].copy(), r=res[k, :, 3:].copy())
            out.append(d)
        return out

    def optimize(self, masks=None, **tolerances):
        """One job per mask (None: one job, every constraint on), all in one launch.  tolerances:
        max_iterations, gradient_tolerance, function_tolerance, parameter_tolerance (Ceres's defaults;
        0 disables a rule).  Returns per job dict(poses [n, 3], status, status_name, iterations,
        cg_iterations, initial_cost, final_cost, gradient, chi2_start [m], chi2 [m]).  Under a loss
        (set_loss) the costs are the robust F, chi2 stays |r|^2, and a job's dict gains weights [m]:
        rho'(chi2) of each constraint at the job's final poses, 1 where the loss does not apply."""
        tol = _tolerances("optimize", tolerances)
        en, K = self._masks(masks)
        poses = np.zeros((K, self.n, 3))
        records = np.zeros((K, _capi.POSEGRAPH_RECORD_DOUBLES))
        chi2 = np.zeros((K, 2, self.m))
        self._check(self._L.ndt2d_posegraph_solve(self._p, self._u8(en), K, *tol, dptr(poses), dptr(records), dptr(chi2)), "ndt2d_posegraph_solve")
        fields = (("iterations", int), ("cg_iterations", int), ("initial_cost", float), ("final_cost", float), ("gradient", float))
        return self._solved(poses, records, chi2, fields, self._weights(chi2[:, 1]) if self._loss[0] != "trivial" else None)

    def optimize_direct(self, masks=None, workspace_bytes=DEFAULT_DIRECT_WORKSPACE, **tolerances):
        """optimize's problem, LM rules, arguments and tolerances with an exact linear step (include/ndt2d_hip.h,
        "Direct solve"): H_FF + lambda D assembled densely, factored by the dense covariance's blocked Cholesky, and
        L L^T delta = -g by substitution -- a cost per iteration that does not depend on the closures.  workspace_bytes:
        the device memory the jobs of a chunk may take (one 3n x 3n matrix of doubles a job); the object is made at the
        first call and again when this changes.  Returns optimize's dicts with rejected (steps not taken),
        not_positive_definite (factorisations that failed, counted among them) and pivot_ratio (of the last successful
        factorisation) in place of cg_iterations; weights [m] under a loss."""
        tol = _tolerances("optimize_direct", tolerances)
        en, K = self._masks(masks)
        direct = self._companion("direct", workspace_bytes)
        poses = np.zeros((K, self.n, 3))
        records = np.zeros((K, _capi.DIRECT_RECORD_DOUBLES))
        chi2 = np.zeros((K, 2, self.m))
        self._companion_check("direct", self._L.ndt2d_direct_solve(direct, self._u8(en), K, *tol, dptr(poses), dptr(records), dptr(chi2)),
                              "ndt2d_direct_solve")
        fields = (("iterations", int), ("rejected", int), ("not_positive_definite", int), ("initial_cost", float), ("final_cost", float),
                  ("gradient", float), ("pivot_ratio", float))
        return self._solved(poses, records, chi2, fields, self._weights(chi2[:, 1]) if self._loss[0] != "trivial" else None)

    def direct_last_ms(self):
        """(kernel_ms, fetch_ms) of the last optimize_direct call's last chunk (set_timing(True)): its iterations with the
        read-backs between them, and its final read-back."""
        return self._companion_last_ms("direct")

    def optimize_sparse(self, masks=None, workspace_bytes=DEFAULT_SPARSE_WORKSPACE, **tolerances):
        """optimize_direct's problem, LM rules, arguments, tolerances and result with the exact linear step taken sparsely
        (include/ndt2d_hip.h, "Sparse solve"): the chain along the node order by one block cyclic reduction over the
        interior nodes, the nodes closures touch (the separators) by a dense Cholesky of their Schur complement -- O(n) +
        O(s^3) an iteration and no 3n x 3n matrix, for large maps with many closures.  workspace_bytes: the device memory
        the jobs of a chunk may take; the object is made at the first call and again when this changes.  pivot_ratio is
        the Schur complement's (1 without a closure); not_positive_definite counts the reduction's failures and its."""
        tol = _tolerances("optimize_sparse", tolerances)
        en, K = self._masks(masks)
        sparse = self._companion("sparse", workspace_bytes)
        poses = np.zeros((K, self.n, 3))
        records = np.zeros((K, _capi.DIRECT_RECORD_DOUBLES))
        chi2 = np.zeros((K, 2, self.m))
        self._companion_check("sparse", self._L.ndt2d_sparse_solve(sparse, self._u8(en), K, *tol, dptr(poses), dptr(records), dptr(chi2)),
                              "ndt2d_sparse_solve")
        fields = (("iterations", int), ("rejected", int), ("not_positive_definite", int), ("initial_cost", float), ("final_cost", float),
                  ("gradient", float), ("pivot_ratio", float))
        return self._solved(poses, records, chi2, fields, self._weights(chi2[:, 1]) if self._loss[0] != "trivial" else None)

    def sparse_layout(self, workspace_bytes=DEFAULT_SPARSE_WORKSPACE):
        """dict(separators, interior): what the sparse solve's plan makes of the graph in place -- the nodes that are an
        end of a constraint with |begin - end| != 1, and the others."""
        sparse = self._companion("sparse", self._sparse_bytes if self._sparse is not None else workspace_bytes)
        s, ni = C.c_size_t(0), C.c_size_t(0)
        self._companion_check("sparse", self._L.ndt2d_sparse_layout(sparse, C.byref(s), C.byref(ni)), "ndt2d_sparse_layout")
        return dict(separators=int(s.value), interior=int(ni.value))

    def sparse_last_ms(self):
        """(kernel_ms, fetch_ms) of the last optimize_sparse call's last chunk (set_timing(True))."""
        return self._companion_last_ms("sparse")

    def marginals(self, nodes, masks=None, poses=None, damping=0.0, tolerance=1e-10, max_cg_iterations=0, want_columns=False):
        """Block columns of (H_FF + damping clamp(diag H_FF))^-1 for the query `nodes` [Q]
        (include/ndt2d_hip.h, "Marginal covariances"): one job per mask (None: one job, every
        constraint on), at the graph's poses or at poses [K, n, 3] (optimize's, one set per job).
        Returns per job dict(blocks [Q, Q, 3, 3], status [Q], cg_iterations [Q], residuals [Q, 3],
        and with want_columns columns [Q, n, 3, 3])."""
        en, K = self._masks(masks)
        q = np.asarray(nodes).reshape(-1)
        for v in q:
            if not 0 <= int(v) < 2 ** 32:
                raise ValueError("marginals: node %d" % int(v))
        q = np.ascontiguousarray(q, dtype=np.uint32)
        Q = len(q)
        if poses is not None:
            poses = np.ascontiguousarray(poses, dtype=np.float64)
            if poses.size != K * self.n * 3:
                raise ValueError("marginals: poses has %d values, %d jobs of %d poses need %d" % (poses.size, K, self.n, K * self.n * 3))
        blocks = np.zeros((K, Q, Q, 3, 3))
        records = np.zeros((K, Q, _capi.MARGINALS_RECORD_DOUBLES))
        columns = np.zeros((K, Q, self.n, 3, 3)) if want_columns else None
        self._check(self._L.ndt2d_marginals_columns(self._p, self._u8(en), K, None if poses is None else dptr(poses),
                                                    q.ctypes.data_as(C.POINTER(C.c_uint32)), Q, float(damping), float(tolerance),
                                                    int(max_cg_iterations), dptr(blocks), None if columns is None else dptr(columns),
                                                    dptr(records)), "ndt2d_marginals_columns")
        out = []
        for k in range(K):
            d = dict(blocks=blocks[k].copy(), status=records[k, :, 0].astype(np.int64), cg_iterations=records[k, :, 1].astype(np.int64),
                     residuals=records[k, :, 2:].copy())
            if want_columns:
                d["columns"] = columns[k].copy()
            out.append(d)
        return out

    def relative_covariance(self, a, b, poses=None, mask=None, **kw):
        """The predicted transform of node b in node a's frame and its covariance from the joint
        marginal of the two: one marginals call with nodes = [a, b], then ndt2d_marginals_relative.
        poses [n, 3]: where to linearise (required: the object does not read its poses back).
        Returns dict(transform [3], covariance [3, 3], status [2], joint [2, 2, 3, 3])."""
        if poses is None:
            raise ValueError("relative_covariance: poses [n, 3] (the poses the graph was given, or optimize's)")
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(self.n, 3)
        got = self.marginals([a, b], masks=None if mask is None else np.asarray(mask).reshape(1, -1), poses=poses[None], **kw)[0]
        t, cov = relative_covariance(poses[int(a)], poses[int(b)], got["blocks"])
        return dict(transform=t, covariance=cov, status=got["status"], joint=got["blocks"])

    def covariances(self, masks=None, poses=None, damping=0.0, pairs=None, workspace_bytes=DEFAULT_COVARIANCE_WORKSPACE):
        """Every node's 3 x 3 block and the blocks of chosen (a, b) pairs of
        (H_FF + damping clamp(diag H_FF))^-1 by a dense Cholesky on the device (include/ndt2d_hip.h,
        "Dense covariance"): one job per mask (None: one job, every constraint on), at the graph's
        poses or at poses [K, n, 3].  pairs [P, 2]: block = the rows of node a in the columns of
        node b.  workspace_bytes: the device memory the jobs of a chunk may take (two 3n x 3n
        matrices of doubles a job); the object is made at the first call and again when this changes.
        Returns dict(diagonal [K, n, 3, 3], pairs [K, P, 3, 3], status [K], failed [K] (the first
        failing unknown or -1), pivot_ratio [K])."""
        en, K = self._masks(masks)
        if poses is not None:
            poses = np.ascontiguousarray(poses, dtype=np.float64)
            if poses.size != K * self.n * 3:
                raise ValueError("covariances: poses has %d values, %d jobs of %d poses need %d" % (poses.size, K, self.n, K * self.n * 3))
        pr = np.zeros((0, 2), dtype=np.uint32) if pairs is None else np.asarray(pairs).reshape(-1, 2)
        if pr.size and not (0 <= int(pr.min()) and int(pr.max()) < 2 ** 32):
            raise ValueError("covariances: a pair names node %d" % int(pr.min() if pr.min() < 0 else pr.max()))
        pr = np.ascontiguousarray(pr, dtype=np.uint32)
        P = len(pr)
        cov = self._companion("covariance", workspace_bytes)
        diagonal = np.zeros((K, self.n, 3, 3))
        blocks = np.zeros((K, P, 3, 3))
        records = np.zeros((K, _capi.COVARIANCE_RECORD_DOUBLES))
        rc = self._L.ndt2d_covariance_compute(cov, self._u8(en), K, None if poses is None else dptr(poses), float(damping),
                                              pr.ctypes.data_as(C.POINTER(C.c_uint32)) if P else None, P, dptr(diagonal),
                                              dptr(blocks) if P else None, dptr(records))
        self._companion_check("covariance", rc, "ndt2d_covariance_compute")
        return dict(diagonal=diagonal, pairs=blocks, status=records[:, 0].astype(np.int64), failed=records[:, 1].astype(np.int64),
                    pivot_ratio=records[:, 2].copy())

    def covariance_last_ms(self):
        """(kernel_ms, fetch_ms) of the last covariances call's last chunk (set_timing(True))."""
        return self._companion_last_ms("covariance")

    def _covariance_call(self, noun, who, masks, poses, damping, pairs, workspace_bytes):
        """The arguments and the outputs the dense and the sparse covariance share: (diagonal [K, n, 3, 3],
        pairs [K, P, 3, 3], records [K, 3]) of ndt2d_<noun>_compute."""
        en, K = self._masks(masks)
        if poses is not None:
            poses = np.ascontiguousarray(poses, dtype=np.float64)
            if poses.size != K * self.n * 3:
                raise ValueError("%s: poses has %d values, %d jobs of %d poses need %d" % (who, poses.size, K, self.n, K * self.n * 3))
        pr = np.zeros((0, 2), dtype=np.uint32) if pairs is None else np.asarray(pairs).reshape(-1, 2)
        if pr.size and not (0 <= int(pr.min()) and int(pr.max()) < 2 ** 32):
            raise ValueError("%s: a pair names node %d" % (who, int(pr.min() if pr.min() < 0 else pr.max())))
        pr = np.ascontiguousarray(pr, dtype=np.uint32)
        P = len(pr)
        obj = self._companion(noun, workspace_bytes)
        diagonal = np.zeros((K, self.n, 3, 3))
        blocks = np.zeros((K, P, 3, 3))
        records = np.zeros((K, _capi.COVARIANCE_RECORD_DOUBLES))
        rc = getattr(self._L, "ndt2d_%s_compute" % noun)(obj, self._u8(en), K, None if poses is None else dptr(poses), float(damping),
                                                         pr.ctypes.data_as(C.POINTER(C.c_uint32)) if P else None, P, dptr(diagonal),
                                                         dptr(blocks) if P else None, dptr(records))
        self._companion_check(noun, rc, "ndt2d_%s_compute" % noun)
        return diagonal, blocks, records

    def covariances_sparse(self, masks=None, poses=None, damping=0.0, pairs=None, workspace_bytes=DEFAULT_SPARSECOV_WORKSPACE):
        """covariances' blocks, arguments and layout from the sparse solve's factorisation (include/ndt2d_hip.h, "Sparse
        covariance"): the chain by the block cyclic reduction and a selected inversion down its levels, the nodes closures
        touch (the separators) by a dense Cholesky of their Schur complement and its inverse -- O(n) + O(s^3) and no
        3n x 3n matrix, for large maps.  Returns dict(diagonal [K, n, 3, 3], pairs [K, P, 3, 3], status [K], stage [K]
        (0: none, 1: a pivot of the reduction, 2: a pivot of the Schur complement), pivot_ratio [K] (the Schur
        complement's, 1 without a closure))."""
        diagonal, blocks, records = self._covariance_call("sparsecov", "covariances_sparse", masks, poses, damping, pairs, workspace_bytes)
        return dict(diagonal=diagonal, pairs=blocks, status=records[:, 0].astype(np.int64), stage=records[:, 1].astype(np.int64),
                    pivot_ratio=records[:, 2].copy())

    def sparsecov_last_ms(self):
        """(kernel_ms, fetch_ms) of the last covariances_sparse call's last chunk (set_timing(True))."""
        return self._companion_last_ms("sparsecov")

    def relative_covariances(self, pairs, poses=None, mask=None, damping=0.0, workspace_bytes=DEFAULT_COVARIANCE_WORKSPACE, method="dense"):
        """relative_covariance for every (a, b) of pairs [P, 2] from ONE covariances call: the joint
        marginal of each pair is {diagonal[a], block (a, b), block (b, a), diagonal[b]}, then
        ndt2d_marginals_relative per pair.  poses [n, 3]: where to linearise (required, as for
        relative_covariance).  method: "dense" (covariances) or "schur" (covariances_sparse).  Returns a
        list of dict(transform [3], covariance [3, 3], joint [2, 2, 3, 3], status: the job's)."""
        if method not in ("dense", "schur"):
            raise ValueError("relative_covariances: method = %r (\"dense\" or \"schur\")" % (method,))
        if poses is None:
            raise ValueError("relative_covariances: poses [n, 3] (the poses the graph was given, or optimize's)")
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(self.n, 3)
        pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        both = np.concatenate([pr, pr[:, ::-1]])
        call = self.covariances if method == "dense" else self.covariances_sparse
        got = call(masks=None if mask is None else np.asarray(mask).reshape(1, -1), poses=poses[None], damping=damping, pairs=both,
                   workspace_bytes=workspace_bytes)
        out = []
        for q, (a, b) in enumerate(pr):
            joint = np.array([[got["diagonal"][0, a], got["pairs"][0, q]], [got["pairs"][0, len(pr) + q], got["diagonal"][0, b]]])
            t, cov = relative_covariance(poses[a], poses[b], joint)
            out.append(dict(transform=t, covariance=cov, joint=joint, status=int(got["status"][0])))
        return out

    def _weights(self, chi2):
        """rho'(chi2) [K, m] (ndt2d_robust_rho's, by robust_weights), 1 where the loss does not apply."""
        kind, scale, on = self._loss
        applies = np.ones(self.m, dtype=bool) if isinstance(on, str) and on == "all" else (self.switchable if isinstance(on, str) else on != 0)
        return np.where(applies[None, :], robust_weights(kind, scale, chi2), 1.0)

    def set_timing(self, enabled):
        self._check(self._L.ndt2d_posegraph_set_timing(self._p, 1 if enabled else 0), "ndt2d_posegraph_set_timing")
        for noun, attr in _COMPANIONS.items():
            if getattr(self, attr) is not None:
                getattr(self._L, "ndt2d_%s_set_timing" % noun)(getattr(self, attr), 1 if enabled else 0)
        self._timing = bool(enabled)

    def last_ms(self):
        """(kernel_ms, fetch_ms) of the last call's last chunk (set_timing(True))."""
        a, b = C.c_float(0.0), C.c_float(0.0)
        self._check(self._L.ndt2d_posegraph_last_ms(self._p, C.byref(a), C.byref(b)), "ndt2d_posegraph_last_ms")
        return a.value, b.value
