"""The host side of the pose graph's marginal covariances without a GPU: the plain-C++ header of
`relative` and `distance` in a program of its own (plainly and under the sanitizers) against the
numpy restatement bit for bit, the three ndt2d_marginals_* entry points' declarations, bindings,
guards and refusals, the Python functions over the two host entry points, and the plugin mirror's
compile."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import posegraph_marginals_restatement as MR
from ndt_2d_amd import Ndt2dError, _capi, build, closure_distance, relative_covariance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "ndt_2d_amd", "csrc", "posegraph", "ndt2d_posegraph_relative.h")


def _hex(words):
    return np.array([float.fromhex(w) for w in words])


def test_the_relative_header_in_a_program_of_its_own_and_under_the_sanitizers(tmp_path):
    """tests/cpp/posegraph_relative_check.cpp over csrc/posegraph/ndt2d_posegraph_relative.h: built
    with the host compiler, plainly and with -fsanitize=address,undefined (the runtime linked into
    the program), run directly, nothing preloaded.  Here: every printed result equals the
    restatement's of the printed inputs bit for bit."""
    src = os.path.join(ROOT, "tests", "cpp", "posegraph_relative_check.cpp")
    inc = os.path.join(ROOT, "ndt_2d_amd", "csrc", "posegraph")
    common = ["g++", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", inc, src]
    plain, sanitized = os.path.join(str(tmp_path), "relative_check"), os.path.join(str(tmp_path), "relative_check_san")
    subprocess.check_call(common + ["-O2", "-o", plain])
    subprocess.check_call(common + ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", sanitized])
    outputs = []
    for exe in (plain, sanitized):
        done = subprocess.run([exe], capture_output=True, text=True)
        assert done.returncode == 0 and not done.stderr, done.stderr
        assert done.stdout.splitlines()[-1] == "ok"
        outputs.append(done.stdout)
    assert outputs[0] == outputs[1]
    rows = [line.split() for line in outputs[0].splitlines()]
    rel, dist = [r[1:] for r in rows if r[0] == "R"], [r[1:] for r in rows if r[0] == "D"]
    assert len(rel) == 20 and len(dist) == 20
    for r in rel:
        v = _hex(r)
        c, s, pa, pb, joint, t, cov = v[0], v[1], v[2:5], v[5:8], v[8:44], v[44:47], v[47:56]
        want_t, want_cov = MR.relative(c, s, pa, pb, joint.reshape(2, 2, 3, 3))
        assert t.tobytes() == want_t.tobytes() and cov.tobytes() == want_cov.reshape(9).tobytes(), r[:8]
    refused = 0
    for r in dist:
        v = _hex(r[:24])
        want = MR.distance(v[0:3], v[3:12], v[12:15], v[15:24])
        if r[24] == "refused":
            refused += 1
            assert want is None
        else:
            assert want is not None and np.float64(float.fromhex(r[24])).tobytes() == np.float64(want).tobytes(), r[24]
    assert refused == 2


def test_the_entry_points_are_declared_bound_guarded_and_hashed():
    header = open(os.path.join(ROOT, "include", "ndt2d_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    prose = re.sub(r"\s+", " ", re.sub(r"\n \*", "\n", header))                      # (the comment's lines joined)
    assert "#define NDT2D_ABI_VERSION 4" in header
    for line in ("int ndt2d_marginals_columns(ndt2d_posegraph * posegraph, const uint8_t * enabled, size_t n_jobs, const double * poses, "
                 "const uint32_t * nodes, size_t n_nodes, double damping, double tolerance, uint32_t max_cg_iterations, double * blocks_out, "
                 "double * columns_out, double * records_out);",
                 "int ndt2d_marginals_relative(const double * pose_a, const double * pose_b, const double * joint, double * transform_out, "
                 "double * covariance_out);",
                 "int ndt2d_marginals_distance(const double * transform_pred, const double * covariance_pred, const double * transform_meas, "
                 "const double * covariance_meas, double * d2_out);",
                 "#define NDT2D_MARGINALS_RECORD_DOUBLES 5", "#define NDT2D_MARGINALS_CONVERGED 0", "#define NDT2D_MARGINALS_CG_CAP 1",
                 "#define NDT2D_MARGINALS_BREAKDOWN 2", "#define NDT2D_MARGINALS_NOT_FREE 3"):
        assert line in flat, line
    for line in ("H_FF + damping clamp(diag H_FF)", "the Gauss-Newton covariance", "the reference's own quirky H",
                 "45 doubles a node, 54 under \"chain\""):
        assert line in prose, line
    names = sorted(n for n in _capi.SIGNATURES if n.startswith("ndt2d_marginals_"))
    assert names == ["ndt2d_marginals_columns", "ndt2d_marginals_distance", "ndt2d_marginals_relative"]
    assert sorted(re.findall(r"\bndt2d_marginals_\w+(?=\()", header)) == names
    assert (_capi.MARGINALS_CONVERGED, _capi.MARGINALS_CG_CAP, _capi.MARGINALS_BREAKDOWN, _capi.MARGINALS_NOT_FREE) == (0, 1, 2, 3)
    assert _capi.MARGINALS_RECORD_DOUBLES == 5 and len(_capi.MARGINALS_STATUS_NAMES) == 4
    assert HEADER in build.HEADERS
    assert "posegraph/ndt2d_posegraph_marginals.hip" in build.SOURCES
    posegraph = os.path.dirname(HEADER)
    unit = open(os.path.join(posegraph, "ndt2d_posegraph_marginals.hip")).read()
    assert '#include "posegraph/ndt2d_posegraph_relative.h"' in unit and '#include "posegraph/ndt2d_posegraph_kernel.h"' in unit
    for name in sorted(n for n in os.listdir(posegraph) if n.endswith((".hip", ".h"))):
        assert "atomic" not in re.sub(r"//[^\n]*", "", open(os.path.join(posegraph, name)).read()), name
    solver = open(os.path.join(posegraph, "ndt2d_posegraph.hip")).read()
    assert "marginals_" not in re.sub(r"//[^\n]*", "", solver)                        # the family and its kernels live in one unit
    bodies = re.findall(r"\nint ndt2d_marginals_\w+\([^)]*\)\n\{\n(.*?)\n\}\n", unit, flags=re.S)
    assert len(bodies) == 3
    for body in bodies:
        assert body.lstrip().startswith("NDT2D_C_TRY") and "NDT2D_C_CATCH(" in body.splitlines()[-1], body[:80]
    for kernel in ("marginals_linearize_kernel", "marginals_columns_kernel"):
        assert re.search(r"__global__ void __launch_bounds__\(kPgThreads\) " + kernel + r"\(", unit), kernel
    text = re.sub(r"//[^\n]*", "", open(HEADER).read())
    assert "hip" not in text.lower().replace("__hipcc__", "") and "cos(" not in text and "sin(" not in text    # plain C++, IEEE operations only


def test_null_objects_and_bad_arguments_are_refused_without_a_gpu():
    L = _capi.lib()
    z = np.zeros(64)
    u = np.zeros(4, dtype=np.uint32)
    up = u.ctypes.data_as(C.POINTER(C.c_uint32))
    d = _capi.dptr
    assert L.ndt2d_marginals_columns(None, None, 1, None, up, 1, 0.0, 1e-10, 0, d(z), None, d(z)) == _capi.ERR_INVALID
    assert L.ndt2d_marginals_columns(None, None, 0, None, None, 0, 0.0, 1e-10, 0, None, None, None) == _capi.ERR_INVALID
    eye = np.eye(3).reshape(9)
    joint = np.concatenate([eye, 0 * eye, 0 * eye, eye])
    pa, pb, t, cov = np.array([0.0, 0.0, 0.0]), np.array([1.0, 2.0, 0.5]), np.full(3, 9.0), np.full(9, 9.0)
    for args in ((None, d(pb), d(joint), d(t), d(cov)), (d(pa), None, d(joint), d(t), d(cov)), (d(pa), d(pb), None, d(t), d(cov)),
                 (d(pa), d(pb), d(joint), None, d(cov)), (d(pa), d(pb), d(joint), d(t), None)):
        assert L.ndt2d_marginals_relative(*args) == _capi.ERR_INVALID
    bad = pb.copy()
    bad[1] = math.inf
    assert L.ndt2d_marginals_relative(d(pa), d(bad), d(joint), d(t), d(cov)) == _capi.ERR_INVALID
    bad_joint = joint.copy()
    bad_joint[35] = math.nan
    assert L.ndt2d_marginals_relative(d(pa), d(pb), d(bad_joint), d(t), d(cov)) == _capi.ERR_INVALID
    assert t.tolist() == [9.0] * 3 and cov.tolist() == [9.0] * 9
    d2 = np.full(1, -7.0)
    for args in ((None, d(eye), d(pb), d(eye), d(d2)), (d(pa), None, d(pb), d(eye), d(d2)), (d(pa), d(eye), None, d(eye), d(d2)),
                 (d(pa), d(eye), d(pb), None, d(d2)), (d(pa), d(eye), d(pb), d(eye), None)):
        assert L.ndt2d_marginals_distance(*args) == _capi.ERR_INVALID
    assert L.ndt2d_marginals_distance(d(pa), d(eye), d(pb), d(-2.0 * eye), d(d2)) == _capi.ERR_INVALID          # S is not positive definite
    assert L.ndt2d_marginals_distance(d(pa), d(eye), d(bad), d(eye), d(d2)) == _capi.ERR_INVALID
    assert L.ndt2d_marginals_distance(d(pa), d(eye * math.nan), d(pb), d(eye), d(d2)) == _capi.ERR_INVALID
    assert d2[0] == -7.0


def test_the_python_functions_are_the_restatements():
    """ndt2d_marginals_relative takes cos and sin from the host's libm, the restatement from
    Python's math: the same library here, so the bits agree; 4 ulp of the largest entry otherwise."""
    rng = np.random.default_rng(4)
    for k in range(10):
        pa, pb = rng.normal(0.0, 3.0, 3), rng.normal(0.0, 3.0, 3)
        g = rng.normal(0.0, 0.2, (6, 6))
        joint = (g @ g.T + 1e-3 * np.eye(6)).reshape(2, 3, 2, 3).transpose(0, 2, 1, 3)
        if k == 3:
            joint[0, 0] = joint[0, 1] = joint[1, 0] = 0.0                     # a held
        t, cov = relative_covariance(pa, pb, joint)
        want_t, want_cov = MR.relative(math.cos(pa[2]), math.sin(pa[2]), pa, pb, joint)
        assert np.all(np.abs(t - want_t) <= 4.0 * np.spacing(np.max(np.abs(want_t))))
        assert np.all(np.abs(cov - want_cov) <= 4.0 * np.spacing(np.max(np.abs(want_cov))))
        meas = want_t + rng.normal(0.0, 0.3, 3) + (np.array([0.0, 0.0, 2.0 * math.pi]) if k % 2 else 0.0)
        cov_meas = np.diag([0.01, 0.02, 0.0025])
        got = closure_distance(t, cov, meas, cov_meas)
        assert np.float64(got).tobytes() == np.float64(MR.distance(t, cov, meas, cov_meas)).tobytes()
        assert got >= 0.0
    with pytest.raises(Ndt2dError) as ei:
        closure_distance(t, -cov, meas, 0.5 * cov)
    assert ei.value.code == _capi.ERR_INVALID
    with pytest.raises(Ndt2dError):
        relative_covariance([0.0, math.nan, 0.0], pb, joint)


def test_the_plugin_mirror_with_marginals_compiles():
    stub = os.path.join(ROOT, "tests", "stubs", "pose_graph_marginals_instantiation.cpp")
    done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "stubs"), stub], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr
    text = open(os.path.join(ROOT, "ndt_2d_amd", "plugin", "pose_graph_hip.hpp")).read()
    for member in ("bool marginals(", "bool relativeCovariance(", "bool closureDistance(", "ndt2d_marginals_columns(", "ndt2d_marginals_relative(",
                   "ndt2d_marginals_distance("):
        assert member in text, member
    code = re.sub(r"//[^\n]*", "", text)
    assert "Eigen" not in code and "rclcpp" not in code and "ceres" not in code
