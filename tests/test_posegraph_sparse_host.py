"""The host side of the sparse solve without a GPU: the plan's and the Schur step's headers in programs
of their own (plainly and under the sanitizers), the seven ndt2d_sparse_* entry points' declarations,
bindings and guards, the unit's place in the build, NULL-object refusals, the Python layer's signatures
and the plugin mirror's compile."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from ndt_2d_amd import PoseGraph, _capi, build, graph_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ndt_2d_amd", "csrc")
SPARSE = os.path.join(CSRC, "sparse")
FILES = ["ndt2d_sparse.hip", "ndt2d_sparse_kernel.h", "ndt2d_sparse_plan.h", "ndt2d_sparse_schur.h"]
NAMES = ["ndt2d_sparse_create", "ndt2d_sparse_destroy", "ndt2d_sparse_last_error", "ndt2d_sparse_last_ms", "ndt2d_sparse_layout",
         "ndt2d_sparse_set_timing", "ndt2d_sparse_solve"]


def _code(path):
    return re.sub(r"//[^\n]*", "", open(path).read())


@pytest.mark.parametrize("check", ("sparse_plan_check", "sparse_schur_check"))
def test_the_plain_headers_in_programs_of_their_own_and_under_the_sanitizers(check, tmp_path):
    """tests/cpp/sparse_plan_check.cpp over csrc/sparse/ndt2d_sparse_plan.h and tests/cpp/sparse_schur_check.cpp
    over csrc/sparse/ndt2d_sparse_schur.h: built with the host compiler, plainly and with
    -fsanitize=address,undefined (the runtime linked into the program), run directly, nothing preloaded.
    The Schur check's bound is 4 x the worst residual ratio it measures against its own dense Cholesky."""
    src = os.path.join(ROOT, "tests", "cpp", check + ".cpp")
    common = ["g++", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src]
    plain, sanitized = os.path.join(str(tmp_path), check), os.path.join(str(tmp_path), check + "_san")
    subprocess.check_call(common + ["-O2", "-o", plain])
    subprocess.check_call(common + ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", sanitized])
    for exe in (plain, sanitized):
        done = subprocess.run([exe], capture_output=True, text=True)
        assert done.returncode == 0 and not done.stderr, done.stdout + done.stderr
        lines = done.stdout.splitlines()
        assert lines[-1] == "ok" and not [line for line in lines if line.startswith("FAILED")], done.stdout
        if check == "sparse_schur_check":
            found = re.fullmatch(r"worst ratio ([0-9.]+) over (\d+) systems \((\d+) against the floor\), the bound ([0-9.]+)", lines[-2])
            assert found, lines[-2]
            worst, systems, bound = float(found.group(1)), int(found.group(2)), float(found.group(4))
            print(lines[-2])
            assert systems >= 500 and worst <= bound and abs(bound - 4.0 * 4.70) < 0.05   # the margin of 4 over the measured 4.70
    for name in ("ndt2d_sparse_plan.h", "ndt2d_sparse_schur.h"):
        text = _code(os.path.join(SPARSE, name))
        assert "hip" not in text.lower().replace("__hipcc__", "") and "__global__" not in text and "#include <hip" not in text   # plain C++


def test_the_entry_points_are_declared_bound_guarded_and_built():
    header = open(os.path.join(ROOT, "include", "ndt2d_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    prose = re.sub(r"\s+", " ", re.sub(r"\n \*", "\n", header))
    assert "#define NDT2D_ABI_VERSION 4" in header
    for line in ("typedef struct ndt2d_sparse ndt2d_sparse;",
                 "int ndt2d_sparse_create(ndt2d_posegraph * posegraph, size_t workspace_bytes, ndt2d_sparse ** out);",
                 "int ndt2d_sparse_destroy(ndt2d_sparse * sparse);",
                 "const char * ndt2d_sparse_last_error(ndt2d_sparse * sparse);",
                 "int ndt2d_sparse_solve(ndt2d_sparse * sparse, const uint8_t * enabled, size_t n_jobs, uint32_t max_iterations, "
                 "double gradient_tolerance, double function_tolerance, double parameter_tolerance, double * poses_out, double * records_out, "
                 "double * chi2_out);",
                 "int ndt2d_sparse_layout(ndt2d_sparse * sparse, size_t * n_separators, size_t * n_interior);",
                 "int ndt2d_sparse_set_timing(ndt2d_sparse * sparse, int enabled);",
                 "int ndt2d_sparse_last_ms(ndt2d_sparse * sparse, float * kernel_ms, float * fetch_ms);"):
        assert line in flat, line
    for line in ("Sparse solve", "whatever the masks", "they only cut the chain", "ONE block-tridiagonal SPD system", "six right-hand-side columns",
                 "S = A_ss - A_si Z", "With s = 0 nothing dense is launched", "the pivot ratio is S's",
                 "the message gives the bytes a job needs", "one small read-back per LM iteration", "destroyed before"):
        assert line in prose, line
    assert sorted(n for n in _capi.SIGNATURES if n.startswith("ndt2d_sparse_")) == NAMES
    assert sorted(set(re.findall(r"\bndt2d_sparse_\w+(?=\()", header))) == NAMES
    assert _capi.SIGNATURES["ndt2d_sparse_solve"] == _capi.SIGNATURES["ndt2d_direct_solve"]                    # the same arguments
    assert "sparse/ndt2d_sparse.hip" in build.SOURCES
    for name in FILES[1:]:
        assert os.path.join(SPARSE, name) in build.HEADERS, name
    assert sorted(n for n in os.listdir(SPARSE) if n.endswith((".hip", ".h"))) == FILES
    unit = open(os.path.join(SPARSE, "ndt2d_sparse.hip")).read()
    for name in ("posegraph/ndt2d_posegraph_state.h", "posegraph/ndt2d_posegraph_kernel.h", "covariance/ndt2d_covariance_kernel.h",
                 "covariance/ndt2d_covariance_launch.h", "direct/ndt2d_direct_kernel.h", "direct/ndt2d_direct_step.h",
                 "sparse/ndt2d_sparse_kernel.h", "sparse/ndt2d_sparse_plan.h"):
        assert '#include "%s"' % name in unit, name
    kernels = open(os.path.join(SPARSE, "ndt2d_sparse_kernel.h")).read()
    assert '#include "sparse/ndt2d_sparse_schur.h"' in kernels
    for call in ("sparse::schur_separator(", "sparse::expand_node(", "sparse::forward_columns<K>(", "sparse::back_columns<K>(",
                 "pg::chain::factor_node(", "sparse::set_columns("):
        assert call in kernels, call                                                           # the kernels run the headers' steps
    for name in FILES:
        code = _code(os.path.join(SPARSE, name))
        assert "atomic" not in code.lower(), name
        assert not re.search(r'#include\s+"[^"]*\.hip"', code), name                          # no unit includes a .hip
        assert "hipLaunchCooperativeKernel" not in code and "__threadfence" not in code, name  # no waiting on another workgroup
    bodies = re.findall(r"\nint ndt2d_sparse_\w+\([^)]*\)\n\{\n(.*?)\n\}\n", unit, flags=re.S)
    assert len(bodies) == 6                                                                    # (last_error is one line)
    for body in bodies:
        assert body.lstrip().startswith("NDT2D_C_TRY") and "NDT2D_C_CATCH(" in body.splitlines()[-1], body[:80]
    for kernel in ("sparse_assemble_kernel", "sparse_reduce_kernel", "sparse_schur_kernel", "sparse_expand_kernel"):
        assert re.search(r"__global__ void __launch_bounds__\(\w+\) " + kernel + r"\(", kernels), kernel
    # what is reused is launched, not copied: the direct solve's kernels by name, the dense factor through the launch header
    for launch in ("ndt2d::direct_begin_kernel<", "direct_step_kernel<", "direct_substitute_kernel<SparseChunk>", "ndt2d::direct_finish_kernel",
                   "ndt2d::direct_chi2_kernel", "cov_enqueue_fill<SparseJob>(", "cov_enqueue_launches<SparseJob, false>("):
        assert launch in unit, launch
    assert "cov_launch_list(3 * ns, false, " in unit                                           # the list cut to the factor's part
    assert "covariance_blocks_kernel" not in unit and "<true" not in unit and ", true>" not in unit
    direct = open(os.path.join(CSRC, "direct", "ndt2d_direct_kernel.h")).read()
    assert "template <class Chunk = DirectChunk>" in direct                                    # today's type by default
    # nothing of the pose graph's, the covariance's or the direct solve's units names the sparse solve's object
    for folder in ("posegraph", "covariance", "direct"):
        for name in os.listdir(os.path.join(CSRC, folder)):
            if name.endswith((".hip", ".h")):
                text = _code(os.path.join(CSRC, folder, name))
                assert not re.search(r"\bndt2d_sparse\b|ndt2d_sparse_(create|destroy|solve|layout|last|set)", text), name


def test_null_objects_are_refused_without_a_gpu():
    L = _capi.lib()
    z = np.zeros(16)
    d = _capi.dptr
    p = C.c_void_p()
    assert L.ndt2d_sparse_create(None, 1 << 20, C.byref(p)) == _capi.ERR_INVALID and not p
    assert L.ndt2d_sparse_create(None, 1 << 20, None) == _capi.ERR_INVALID
    assert L.ndt2d_sparse_destroy(None) == _capi.ERR_INVALID
    assert L.ndt2d_sparse_last_error(None) == b"null sparse"
    assert L.ndt2d_sparse_solve(None, None, 1, 10, 1e-10, 1e-6, 1e-8, d(z), d(z), None) == _capi.ERR_INVALID
    assert L.ndt2d_sparse_solve(None, None, 0, 10, 1e-10, 1e-6, 1e-8, None, None, None) == _capi.ERR_INVALID
    s, ni = C.c_size_t(7), C.c_size_t(7)
    assert L.ndt2d_sparse_layout(None, C.byref(s), C.byref(ni)) == _capi.ERR_INVALID and s.value == 7 and ni.value == 7
    assert L.ndt2d_sparse_set_timing(None, 1) == _capi.ERR_INVALID
    a, b = C.c_float(0.0), C.c_float(0.0)
    assert L.ndt2d_sparse_last_ms(None, C.byref(a), C.byref(b)) == _capi.ERR_INVALID
    assert np.all(z == 0.0)


def test_the_python_layer_and_the_plugin_mirror():
    sig = inspect.signature(PoseGraph.optimize_sparse)
    assert list(sig.parameters) == ["self", "masks", "workspace_bytes", "tolerances"]
    assert sig.parameters["masks"].default is None and sig.parameters["workspace_bytes"].default > 0
    assert sig.parameters["tolerances"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(PoseGraph.optimize).parameters) == ["self", "masks", "tolerances"]           # unchanged
    assert list(inspect.signature(PoseGraph.optimize_direct).parameters) == ["self", "masks", "workspace_bytes", "tolerances"]
    assert list(inspect.signature(PoseGraph.sparse_last_ms).parameters) == ["self"]
    assert "workspace_bytes" in inspect.signature(PoseGraph.sparse_layout).parameters
    method = inspect.signature(graph_io.Graph.optimize).parameters["method"]
    assert method.default == "cg"                                                             # the default is what it was
    assert graph_io.Graph(False).optimize(None, method="schur") is False                      # no scans, as the reference
    with pytest.raises(ValueError, match="schur"):
        graph_io.Graph(False).optimize(None, method="multigrid")
    stub = os.path.join(ROOT, "tests", "stubs", "pose_graph_sparse_instantiation.cpp")
    done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "stubs"), stub], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr
    text = open(os.path.join(ROOT, "ndt_2d_amd", "plugin", "pose_graph_hip.hpp")).read()
    for member in ("bool setSolver(", 'solver != "sparse"', "ndt2d_sparse_create(", "ndt2d_sparse_solve(", "ndt2d_sparse_destroy(", "void dropSparse()"):
        assert member in text, member
    code = re.sub(r"//[^\n]*", "", text)
    assert "Eigen" not in code and "rclcpp" not in code and "ceres" not in code
    assert code.index("dropSparse();") < code.index("ndt2d_posegraph_destroy(pg_)")           # destroyed before the pose graph
    assert 'direct_solver_ = solver == "direct";' in code                                     # "cg" stays the default, "direct" what it was
