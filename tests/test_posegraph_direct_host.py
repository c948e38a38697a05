"""The host side of the direct solve without a GPU: the decisions' header in a program of its own
(plainly and under the sanitizers), the six ndt2d_direct_* entry points' declarations, bindings and
guards, the unit's place in the build, NULL-object refusals, the Python layer's signatures and the
plugin mirror's compile."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from ndt_2d_amd import PoseGraph, _capi, build, graph_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ndt_2d_amd", "csrc")
DIRECT = os.path.join(CSRC, "direct")
FILES = ["ndt2d_direct.hip", "ndt2d_direct_kernel.h", "ndt2d_direct_plan.h", "ndt2d_direct_step.h"]
NAMES = ["ndt2d_direct_create", "ndt2d_direct_destroy", "ndt2d_direct_last_error", "ndt2d_direct_last_ms", "ndt2d_direct_set_timing",
         "ndt2d_direct_solve"]


def _code(path):
    return re.sub(r"//[^\n]*", "", open(path).read())


def test_the_step_header_in_a_program_of_its_own_and_under_the_sanitizers(tmp_path):
    """tests/cpp/direct_step_check.cpp over csrc/direct/ndt2d_direct_step.h: built with the host compiler,
    plainly and with -fsanitize=address,undefined (the runtime linked into the program), run directly,
    nothing preloaded."""
    src = os.path.join(ROOT, "tests", "cpp", "direct_step_check.cpp")
    common = ["g++", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", DIRECT, src]
    plain, sanitized = os.path.join(str(tmp_path), "step_check"), os.path.join(str(tmp_path), "step_check_san")
    subprocess.check_call(common + ["-O2", "-o", plain])
    subprocess.check_call(common + ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", sanitized])
    for exe in (plain, sanitized):
        done = subprocess.run([exe], capture_output=True, text=True)
        assert done.returncode == 0 and not done.stderr, done.stdout + done.stderr
        assert done.stdout.splitlines() == ["ok"], done.stdout
    text = _code(os.path.join(DIRECT, "ndt2d_direct_step.h"))
    assert "hip" not in text.lower().replace("__hipcc__", "") and "__global__" not in text and "#include <hip" not in text   # plain C++
    for rule in ("kLambda0 = 1e-4", "kLambdaMin = 1e-32", "kLambdaMax = 1e32", "kMinGain = 1e-3", "256.0 * 2.220446049250313e-16"):
        assert rule in text, rule


def test_the_entry_points_are_declared_bound_guarded_and_built():
    header = open(os.path.join(ROOT, "include", "ndt2d_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    prose = re.sub(r"\s+", " ", re.sub(r"\n \*", "\n", header))
    assert "#define NDT2D_ABI_VERSION 4" in header
    for line in ("typedef struct ndt2d_direct ndt2d_direct;",
                 "int ndt2d_direct_create(ndt2d_posegraph * posegraph, size_t workspace_bytes, ndt2d_direct ** out);",
                 "int ndt2d_direct_destroy(ndt2d_direct * direct);",
                 "const char * ndt2d_direct_last_error(ndt2d_direct * direct);",
                 "int ndt2d_direct_solve(ndt2d_direct * direct, const uint8_t * enabled, size_t n_jobs, uint32_t max_iterations, "
                 "double gradient_tolerance, double function_tolerance, double parameter_tolerance, double * poses_out, double * records_out, "
                 "double * chi2_out);",
                 "int ndt2d_direct_set_timing(ndt2d_direct * direct, int enabled);",
                 "int ndt2d_direct_last_ms(ndt2d_direct * direct, float * kernel_ms, float * fetch_ms);",
                 "#define NDT2D_DIRECT_RECORD_DOUBLES 8"):
        assert line in flat, line
    for line in ("Direct solve", "predicted = 1/2 (lambda delta^T D delta - g^T delta)", "counts as a rejected step", "destroyed before",
                 "one small read-back per LM iteration", "the message gives the bytes a job needs", "ONE matrix of padded(d)^2 doubles"):
        assert line in prose, line
    assert sorted(n for n in _capi.SIGNATURES if n.startswith("ndt2d_direct_")) == NAMES
    assert sorted(set(re.findall(r"\bndt2d_direct_\w+(?=\()", header))) == NAMES
    assert _capi.SIGNATURES["ndt2d_direct_solve"] == _capi.SIGNATURES["ndt2d_posegraph_solve"]                 # the same arguments
    assert _capi.DIRECT_RECORD_DOUBLES == 8
    # the closed lists stay closed
    for prefix, count in (("ndt2d_covariance_", 6),):
        assert len([n for n in _capi.SIGNATURES if n.startswith(prefix)]) == count
    assert "direct/ndt2d_direct.hip" in build.SOURCES
    for name in FILES[1:]:
        assert os.path.join(DIRECT, name) in build.HEADERS, name
    assert sorted(n for n in os.listdir(DIRECT) if n.endswith((".hip", ".h"))) == FILES
    assert sorted(n for n in os.listdir(os.path.join(CSRC, "covariance")) if n.endswith((".hip", ".h"))) == \
        ["ndt2d_covariance.hip", "ndt2d_covariance_kernel.h", "ndt2d_covariance_launch.h", "ndt2d_covariance_plan.h"]
    assert len([n for n in os.listdir(os.path.join(CSRC, "posegraph")) if n.endswith((".hip", ".h"))]) == 10
    unit = open(os.path.join(DIRECT, "ndt2d_direct.hip")).read()
    for name in ("posegraph/ndt2d_posegraph_state.h", "posegraph/ndt2d_posegraph_kernel.h", "covariance/ndt2d_covariance_kernel.h",
                 "covariance/ndt2d_covariance_plan.h", "covariance/ndt2d_covariance_launch.h", "direct/ndt2d_direct_step.h"):
        assert '#include "%s"' % name in unit, name
    kernels = open(os.path.join(DIRECT, "ndt2d_direct_kernel.h")).read()
    assert '#include "direct/ndt2d_direct_step.h"' in kernels and "direct::propose(" in kernels and "direct::take(" in kernels
    for name in FILES:
        code = _code(os.path.join(DIRECT, name))
        assert "atomic" not in code.lower(), name
        assert not re.search(r'#include\s+"[^"]*\.hip"', code), name                          # no unit includes a .hip
        assert "hipLaunchCooperativeKernel" not in code and "__threadfence" not in code, name  # no waiting on another workgroup
    bodies = re.findall(r"\nint ndt2d_direct_\w+\([^)]*\)\n\{\n(.*?)\n\}\n", unit, flags=re.S)
    assert len(bodies) == 5                                                                    # (last_error is one line)
    for body in bodies:
        assert body.lstrip().startswith("NDT2D_C_TRY") and "NDT2D_C_CATCH(" in body.splitlines()[-1], body[:80]
    for kernel in ("direct_begin_kernel", "direct_substitute_kernel", "direct_step_kernel", "direct_finish_kernel"):
        assert re.search(r"__global__ void __launch_bounds__\(\w+\) " + kernel + r"\(", kernels), kernel
    # the factor is the covariance's: its kernels on this unit's layout, the inversion's launches not taken.  The launch
    # header is the only file that names those kernels in a launch, on the layout it is instantiated with; this unit
    # instantiates it with DirectJob and without the inversion, the covariance's unit includes it too
    launch = _code(os.path.join(CSRC, "covariance", "ndt2d_covariance_launch.h"))
    for kernel in ("covariance_nodes_kernel<Job>", "covariance_fill_kernel<Job>", "covariance_assemble_kernel<decltype(loss)::value, Job>",
                   "covariance_factor_kernel<Job>", "covariance_solve_kernel<false, Job>", "covariance_update_kernel<false, Job>",
                   "covariance_solve_kernel<true, Job>", "covariance_update_kernel<true, Job>"):
        assert len(re.findall(r"hipLaunchKernelGGL\(\(?" + re.escape(kernel) + r"\)?,", launch)) == 1, kernel
    inversion = launch[launch.index("if constexpr (kInverse)"):]
    assert launch.count("<true, Job>") == 2 and inversion.count("<true, Job>") == 2            # the inversion's, behind the flag only
    for root, _, names in os.walk(CSRC):
        for name in names:
            if name.endswith((".hip", ".h", ".cpp")) and name != "ndt2d_covariance_launch.h":
                launches = re.findall(r"hipLaunchKernelGGL\(\(?\s*(?:ndt2d::)?(\w+)", _code(os.path.join(root, name)))
                assert not [k for k in launches if re.fullmatch(r"covariance_(nodes|fill|assemble|factor|solve|update)_kernel", k)], name
    assert unit.count("cov_enqueue_factor<DirectJob, false>(") == 1 and unit.count("cov_enqueue_factor<") == 1
    assert "cov_launch_list(3 * n, false, " in unit                                            # the list cut to the factor's part
    assert "covariance_blocks_kernel" not in unit and "<true" not in unit and ", true>" not in unit
    cov_unit = open(os.path.join(CSRC, "covariance", "ndt2d_covariance.hip")).read()
    assert '#include "covariance/ndt2d_covariance_launch.h"' in cov_unit and "cov_enqueue_factor<ndt2d::CovJob, true>(" in cov_unit
    # nothing of the pose graph's own units moved: the direct solve is not named there
    for name in os.listdir(os.path.join(CSRC, "posegraph")):
        if name.endswith((".hip", ".h")):
            assert "ndt2d_direct" not in open(os.path.join(CSRC, "posegraph", name)).read(), name


def test_null_objects_are_refused_without_a_gpu():
    L = _capi.lib()
    z = np.zeros(16)
    d = _capi.dptr
    p = C.c_void_p()
    assert L.ndt2d_direct_create(None, 1 << 20, C.byref(p)) == _capi.ERR_INVALID and not p
    assert L.ndt2d_direct_create(None, 1 << 20, None) == _capi.ERR_INVALID
    assert L.ndt2d_direct_destroy(None) == _capi.ERR_INVALID
    assert L.ndt2d_direct_last_error(None) == b"null direct"
    assert L.ndt2d_direct_solve(None, None, 1, 10, 1e-10, 1e-6, 1e-8, d(z), d(z), None) == _capi.ERR_INVALID
    assert L.ndt2d_direct_solve(None, None, 0, 10, 1e-10, 1e-6, 1e-8, None, None, None) == _capi.ERR_INVALID
    assert L.ndt2d_direct_set_timing(None, 1) == _capi.ERR_INVALID
    a, b = C.c_float(0.0), C.c_float(0.0)
    assert L.ndt2d_direct_last_ms(None, C.byref(a), C.byref(b)) == _capi.ERR_INVALID
    assert np.all(z == 0.0)


def test_the_python_layer_and_the_plugin_mirror():
    sig = inspect.signature(PoseGraph.optimize_direct)
    assert list(sig.parameters) == ["self", "masks", "workspace_bytes", "tolerances"]
    assert sig.parameters["masks"].default is None and sig.parameters["workspace_bytes"].default > 0
    assert sig.parameters["tolerances"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(PoseGraph.optimize).parameters) == ["self", "masks", "tolerances"]      # unchanged
    assert list(inspect.signature(PoseGraph.direct_last_ms).parameters) == ["self"]
    method = inspect.signature(graph_io.Graph.optimize).parameters["method"]
    assert method.default == "cg"                                                             # the default is what it was
    try:
        graph_io.Graph(False).optimize(None, method="sparse")
    except ValueError as e:
        assert "method" in str(e)
    else:
        raise AssertionError("method=\"sparse\" was taken")
    assert graph_io.Graph(False).optimize(None, method="direct") is False                     # no scans, as the reference
    stub = os.path.join(ROOT, "tests", "stubs", "pose_graph_direct_instantiation.cpp")
    done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "stubs"), stub], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr
    text = open(os.path.join(ROOT, "ndt_2d_amd", "plugin", "pose_graph_hip.hpp")).read()
    for member in ("bool setSolver(", "ndt2d_direct_create(", "ndt2d_direct_solve(", "ndt2d_direct_destroy(", "void dropDirect()"):
        assert member in text, member
    code = re.sub(r"//[^\n]*", "", text)
    assert "Eigen" not in code and "rclcpp" not in code and "ceres" not in code
    assert code.index("dropDirect();") < code.index("ndt2d_posegraph_destroy(pg_)")           # destroyed before the pose graph
