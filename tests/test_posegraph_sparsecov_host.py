"""The host side of the sparse covariance without a GPU: the plan's and the selected inversion's headers in
programs of their own (plainly and under the sanitizers), the six ndt2d_sparsecov_* entry points'
declarations, bindings and guards, the unit's place in the build, NULL-object refusals, the Python layer's
signatures and the plugin mirror's compile."""
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
UNIT = os.path.join(CSRC, "sparsecov")
FILES = ["ndt2d_sparsecov.hip", "ndt2d_sparsecov_kernel.h", "ndt2d_sparsecov_plan.h", "ndt2d_sparsecov_select.h"]
NAMES = ["ndt2d_sparsecov_compute", "ndt2d_sparsecov_create", "ndt2d_sparsecov_destroy", "ndt2d_sparsecov_last_error", "ndt2d_sparsecov_last_ms",
         "ndt2d_sparsecov_set_timing"]
MEASURED = 23.13   # the worst ratio tests/cpp/sparsecov_select_check.cpp measures; its bound is 4 x that


def _code(path):
    return re.sub(r"//[^\n]*", "", open(path).read())


@pytest.mark.parametrize("check", ("sparsecov_plan_check", "sparsecov_select_check"))
def test_the_plain_headers_in_programs_of_their_own_and_under_the_sanitizers(check, tmp_path):
    """tests/cpp/sparsecov_plan_check.cpp over csrc/sparsecov/ndt2d_sparsecov_plan.h and
    tests/cpp/sparsecov_select_check.cpp over csrc/sparsecov/ndt2d_sparsecov_select.h: built with the host
    compiler, plainly and with -fsanitize=address,undefined (the runtime linked into the program), run
    directly, nothing preloaded.  The select check's bound is 4 x the worst ratio it measures, 23.13: the
    driver's block error over the dense double inverse's own, both against a long-double inverse, floored at
    4 ulps of |Sigma|_max.  (A forward error on the generator's ill-conditioned systems -- weights over four
    decades, lambda down to 1e-6.  It was 2165.17 while the cyclic reduction multiplied by explicitly inverted
    3 x 3 pivots; the pivots are kept factored now.)"""
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
        if check == "sparsecov_select_check":
            found = re.fullmatch(r"worst ratio ([0-9.]+) over (\d+) systems \((\d+) against the floor\), the bound ([0-9.]+)", lines[-2])
            assert found, lines[-2]
            worst, systems, bound = float(found.group(1)), int(found.group(2)), float(found.group(4))
            print(lines[-2])
            assert systems >= 500 and worst <= bound and abs(bound - 4.0 * MEASURED) < 0.5
    for name in ("ndt2d_sparsecov_plan.h", "ndt2d_sparsecov_select.h"):
        text = _code(os.path.join(UNIT, name))
        assert "hip" not in text.lower().replace("__hipcc__", "") and "__global__" not in text and "#include <hip" not in text   # plain C++


def test_the_entry_points_are_declared_bound_guarded_and_built():
    header = open(os.path.join(ROOT, "include", "ndt2d_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    prose = re.sub(r"\s+", " ", re.sub(r"\n \*", "\n", header))
    assert "#define NDT2D_ABI_VERSION 4" in header
    for line in ("typedef struct ndt2d_sparsecov ndt2d_sparsecov;",
                 "int ndt2d_sparsecov_create(ndt2d_posegraph * posegraph, size_t workspace_bytes, ndt2d_sparsecov ** out);",
                 "int ndt2d_sparsecov_destroy(ndt2d_sparsecov * sparsecov);",
                 "const char * ndt2d_sparsecov_last_error(ndt2d_sparsecov * sparsecov);",
                 "int ndt2d_sparsecov_compute(ndt2d_sparsecov * sparsecov, const uint8_t * enabled, size_t n_jobs, const double * poses, "
                 "double damping, const uint32_t * pairs, size_t n_pairs, double * diagonal_out, double * pairs_out, double * records_out);",
                 "int ndt2d_sparsecov_set_timing(ndt2d_sparsecov * sparsecov, int enabled);",
                 "int ndt2d_sparsecov_last_ms(ndt2d_sparsecov * sparsecov, float * kernel_ms, float * fetch_ms);"):
        assert line in flat, line
    for line in ("Sparse covariance", "Sigma_ss = S^-1", "Sigma_is = -Z Sigma_ss", "a selected inversion down the levels", "one barrier a level",
                 "stage is 0 for none, 1 for a pivot of the reduction, 2 for a pivot of S", "The reduction keeps no pivot ratio",
                 "a clean return with either status", "transposes bit for bit", "a pair's block does not depend on the other pairs",
                 "the message gives the bytes a job needs", "\"null sparsecov\"", "destroyed before"):
        assert line in prose, line
    assert sorted(n for n in _capi.SIGNATURES if n.startswith("ndt2d_sparsecov_")) == NAMES
    assert sorted(set(re.findall(r"\bndt2d_sparsecov_\w+(?=\()", header))) == NAMES
    assert _capi.SIGNATURES["ndt2d_sparsecov_compute"] == _capi.SIGNATURES["ndt2d_covariance_compute"]        # the same arguments
    assert "sparsecov/ndt2d_sparsecov.hip" in build.SOURCES
    for name in FILES[1:]:
        assert os.path.join(UNIT, name) in build.HEADERS, name
    assert sorted(n for n in os.listdir(UNIT) if n.endswith((".hip", ".h"))) == FILES
    unit = open(os.path.join(UNIT, "ndt2d_sparsecov.hip")).read()
    for name in ("posegraph/ndt2d_posegraph_state.h", "posegraph/ndt2d_posegraph_args.h", "covariance/ndt2d_covariance_launch.h",
                 "sparse/ndt2d_sparse_kernel.h", "sparse/ndt2d_sparse_plan.h", "sparsecov/ndt2d_sparsecov_kernel.h", "sparsecov/ndt2d_sparsecov_plan.h"):
        assert '#include "%s"' % name in unit, name
    kernels = open(os.path.join(UNIT, "ndt2d_sparsecov_kernel.h")).read()
    assert '#include "sparsecov/ndt2d_sparsecov_select.h"' in kernels
    for call in ("sparsecov::select_root(", "sparsecov::select_node(", "sparsecov::diagonal_block(", "sparsecov::pair_block(", "sparsecov::pass_seed(",
                 "sparsecov::pass_gather(", "sparse::forward_columns<sparsecov::kPassColumns>(", "sparse::back_columns<sparsecov::kPassColumns>(",
                 "pg_linearize<kPgJacobi, kLoss>("):
        assert call in kernels, call                                                           # the kernels run the headers' steps
    plan = open(os.path.join(UNIT, "ndt2d_sparsecov_plan.h")).read()
    select = open(os.path.join(UNIT, "ndt2d_sparsecov_select.h")).read()
    for reused in ("sparse::schur_doubles(", "sparse::interior_doubles(", "sparse::work_doubles(", "covariance::padded(", "sparse::Tables", "sparse::refusal("):
        assert reused in plan, reused                                                          # reused, not copied
    assert "make_layout" not in _code(os.path.join(UNIT, "ndt2d_sparsecov_plan.h")) and "sparse::make_layout(" in unit
    for reused in ("sparse::forward_columns<kPassColumns>(", "sparse::root_columns<kPassColumns>(", "sparse::back_columns<kPassColumns>(",
                   "sparse::schur_separator(", "chain::factor("):
        assert reused in select, reused
    for name in FILES:
        code = _code(os.path.join(UNIT, name))
        assert "atomic" not in code.lower(), name
        assert not re.search(r'#include\s+"[^"]*\.hip"', code), name                          # no unit includes a .hip
        assert "hipLaunchCooperativeKernel" not in code and "__threadfence" not in code, name  # no waiting on another workgroup
    bodies = re.findall(r"\nint ndt2d_sparsecov_\w+\([^)]*\)\n\{\n(.*?)\n\}\n", unit, flags=re.S)
    assert len(bodies) == 5                                                                    # (last_error is one line)
    for body in bodies:
        assert body.lstrip().startswith("NDT2D_C_TRY") and "NDT2D_C_CATCH(" in body.splitlines()[-1], body[:80]
    for kernel, threads in (("sparsecov_begin_kernel", "kPgThreads"), ("sparsecov_blocks_kernel", "kWave"), ("sparsecov_select_kernel", "kPgThreads"),
                            ("sparsecov_columns_kernel", "kPgThreads"), ("sparsecov_diagonal_kernel", "kSparsecovThreads"),
                            ("sparsecov_pairs_kernel", "kSparsecovThreads")):
        assert re.search(r"__global__ void __launch_bounds__\(" + threads + r"\) " + kernel + r"\(", kernels), kernel
    # what exists is launched, not copied: the sparse solve's kernels by name, the dense factor and inverse through the launch header
    for launch in ("sparse_assemble_kernel<decltype(loss)::value>", "sparse_reduce_kernel<sparse::kColumns>", "sparse_reduce_kernel<1>", "sparse_schur_kernel,",
                   "cov_enqueue_fill<SparsecovJob>(", "cov_enqueue_launches<SparsecovJob, true>(", "cov_launch_list(3 * ns, true, "):
        assert launch in unit, launch
    for name in FILES:
        assert "covariance_blocks_kernel" not in _code(os.path.join(UNIT, name)), name
    # the units it stands beside are as they were: none of them names the new object, none has a new file or entry point
    for folder, files in (("sparse", 4), ("covariance", 4), ("direct", 4)):
        names = [n for n in os.listdir(os.path.join(CSRC, folder)) if n.endswith((".hip", ".h"))]
        assert len(names) == files, (folder, names)
        for name in names:
            assert "sparsecov" not in _code(os.path.join(CSRC, folder, name)), name
    sparse_unit = open(os.path.join(CSRC, "sparse", "ndt2d_sparse.hip")).read()
    assert "<true" not in sparse_unit and "covariance_blocks_kernel" not in sparse_unit
    assert len(set(re.findall(r"\bndt2d_sparse_\w+(?=\()", header))) == 7 and len(set(re.findall(r"\bndt2d_covariance_\w+(?=\()", header))) == 6


def test_null_objects_are_refused_without_a_gpu():
    L = _capi.lib()
    z = np.zeros(16)
    d = _capi.dptr
    p = C.c_void_p()
    assert L.ndt2d_sparsecov_create(None, 1 << 20, C.byref(p)) == _capi.ERR_INVALID and not p
    assert L.ndt2d_sparsecov_create(None, 1 << 20, None) == _capi.ERR_INVALID
    assert L.ndt2d_sparsecov_destroy(None) == _capi.ERR_INVALID
    assert L.ndt2d_sparsecov_last_error(None) == b"null sparsecov"
    assert L.ndt2d_sparsecov_compute(None, None, 1, None, 0.0, None, 0, d(z), None, d(z)) == _capi.ERR_INVALID
    assert L.ndt2d_sparsecov_compute(None, None, 0, None, 0.0, None, 0, None, None, None) == _capi.ERR_INVALID
    assert L.ndt2d_sparsecov_set_timing(None, 1) == _capi.ERR_INVALID
    a, b = C.c_float(0.0), C.c_float(0.0)
    assert L.ndt2d_sparsecov_last_ms(None, C.byref(a), C.byref(b)) == _capi.ERR_INVALID
    assert np.all(z == 0.0)


def test_the_python_layer_and_the_plugin_mirror():
    sig = inspect.signature(PoseGraph.covariances_sparse)
    assert list(sig.parameters) == ["self", "masks", "poses", "damping", "pairs", "workspace_bytes"]
    assert sig.parameters["masks"].default is None and sig.parameters["poses"].default is None and sig.parameters["damping"].default == 0.0
    assert sig.parameters["pairs"].default is None and sig.parameters["workspace_bytes"].default > 0
    assert list(inspect.signature(PoseGraph.covariances).parameters) == list(sig.parameters)                    # the dense call's, unchanged
    assert list(inspect.signature(PoseGraph.sparsecov_last_ms).parameters) == ["self"]
    relative = inspect.signature(PoseGraph.relative_covariances).parameters
    assert list(relative) == ["self", "pairs", "poses", "mask", "damping", "workspace_bytes", "method"] and relative["method"].default == "dense"
    method = inspect.signature(graph_io.Graph.closure_distances).parameters["method"]
    assert method.default == "cg"                                                              # the default is what it was
    assert graph_io.Graph(False).closure_distances(None, [], method="schur") == []             # nothing proposed
    stub = os.path.join(ROOT, "tests", "stubs", "pose_graph_sparsecov_instantiation.cpp")
    done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "stubs"), stub], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr
    text = open(os.path.join(ROOT, "ndt_2d_amd", "plugin", "pose_graph_hip.hpp")).read()
    for member in ("bool covariancesSparse(", "ndt2d_sparsecov_create(", "ndt2d_sparsecov_compute(", "ndt2d_sparsecov_destroy(", "void dropSparsecov()"):
        assert member in text, member
    code = re.sub(r"//[^\n]*", "", text)
    assert "Eigen" not in code and "rclcpp" not in code and "ceres" not in code
    assert code.index("dropSparsecov();") < code.index("ndt2d_posegraph_destroy(pg_)")        # destroyed before the pose graph
    dense = re.search(r"bool covariances\((.*?)\)\n", code, flags=re.S).group(1)
    sparse = re.search(r"bool covariancesSparse\((.*?)\)\n", code, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", dense) == re.sub(r"\s+", " ", sparse)                           # the same arguments
