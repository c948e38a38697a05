"""The host side of the dense covariance without a GPU: the plan header in a program of its own
(plainly and under the sanitizers), the six ndt2d_covariance_* entry points' declarations, bindings
and guards, the unit's place in the build, NULL-object refusals, and the plugin mirror's compile."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from ndt_2d_amd import PoseGraph, _capi, build, graph_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVARIANCE = os.path.join(ROOT, "ndt_2d_amd", "csrc", "covariance")
PLAN = os.path.join(COVARIANCE, "ndt2d_covariance_plan.h")
KERNELS = os.path.join(COVARIANCE, "ndt2d_covariance_kernel.h")
NAMES = ["ndt2d_covariance_compute", "ndt2d_covariance_create", "ndt2d_covariance_destroy", "ndt2d_covariance_last_error",
         "ndt2d_covariance_last_ms", "ndt2d_covariance_set_timing"]


def test_the_plan_header_in_a_program_of_its_own_and_under_the_sanitizers(tmp_path):
    """tests/cpp/covariance_plan_check.cpp over csrc/covariance/ndt2d_covariance_plan.h: built with the
    host compiler, plainly and with -fsanitize=address,undefined (the runtime linked into the
    program), run directly, nothing preloaded.  Exhaustive for d = 3 ... 300 and 3,069 / 3,072 / 3,075."""
    src = os.path.join(ROOT, "tests", "cpp", "covariance_plan_check.cpp")
    common = ["g++", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", COVARIANCE, src]
    plain, sanitized = os.path.join(str(tmp_path), "plan_check"), os.path.join(str(tmp_path), "plan_check_san")
    subprocess.check_call(common + ["-O2", "-o", plain])
    subprocess.check_call(common + ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", sanitized])
    outputs = []
    for exe in (plain, sanitized):
        done = subprocess.run([exe], capture_output=True, text=True)
        assert done.returncode == 0 and not done.stderr, done.stdout + done.stderr
        assert done.stdout.splitlines()[-1] == "ok"
        outputs.append(done.stdout)
    assert outputs[0] == outputs[1]
    # 3,075 unknowns: 65 panels of 48, 3 launches a panel but the last's one, then 2 a panel but the last's one
    assert outputs[0].splitlines()[0] == "dimensions 301, panels of 3075: 65, launches of 3075: 322, padded(3069 / 3072 / 3075): 3072 3072 3120"
    text = re.sub(r"//[^\n]*", "", open(PLAN).read())
    assert "hip" not in text.lower().replace("__hipcc__", "") and "__global__" not in text                # plain C++


def test_the_entry_points_are_declared_bound_guarded_and_built():
    header = open(os.path.join(ROOT, "include", "ndt2d_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    prose = re.sub(r"\s+", " ", re.sub(r"\n \*", "\n", header))
    assert "#define NDT2D_ABI_VERSION 4" in header
    for line in ("typedef struct ndt2d_covariance ndt2d_covariance;",
                 "int ndt2d_covariance_create(ndt2d_posegraph * posegraph, size_t workspace_bytes, ndt2d_covariance ** out);",
                 "int ndt2d_covariance_destroy(ndt2d_covariance * covariance);",
                 "const char * ndt2d_covariance_last_error(ndt2d_covariance * covariance);",
                 "int ndt2d_covariance_compute(ndt2d_covariance * covariance, const uint8_t * enabled, size_t n_jobs, const double * poses, "
                 "double damping, const uint32_t * pairs, size_t n_pairs, double * diagonal_out, double * pairs_out, double * records_out);",
                 "int ndt2d_covariance_set_timing(ndt2d_covariance * covariance, int enabled);",
                 "int ndt2d_covariance_last_ms(ndt2d_covariance * covariance, float * kernel_ms, float * fetch_ms);",
                 "#define NDT2D_COVARIANCE_RECORD_DOUBLES 3", "#define NDT2D_COVARIANCE_OK 0", "#define NDT2D_COVARIANCE_NOT_POSITIVE_DEFINITE 1"):
        assert line in flat, line
    for line in ("Sigma = (H_FF + damping clamp(diag H_FF))^-1", "transposes of each other bit for bit", "only the lower triangle of A is assembled",
                 "destroyed before", "the message gives the bytes a job needs"):
        assert line in prose, line
    assert sorted(n for n in _capi.SIGNATURES if n.startswith("ndt2d_covariance_")) == NAMES
    assert sorted(re.findall(r"\bndt2d_covariance_\w+(?=\()", header)) == NAMES
    assert (_capi.COVARIANCE_OK, _capi.COVARIANCE_NOT_POSITIVE_DEFINITE, _capi.COVARIANCE_RECORD_DOUBLES) == (0, 1, 3)
    assert len(_capi.COVARIANCE_STATUS_NAMES) == 2
    assert "covariance/ndt2d_covariance.hip" in build.SOURCES and PLAN in build.HEADERS and KERNELS in build.HEADERS
    files = ["ndt2d_covariance.hip", "ndt2d_covariance_kernel.h", "ndt2d_covariance_launch.h", "ndt2d_covariance_plan.h"]
    assert sorted(os.listdir(COVARIANCE)) == files or sorted(n for n in os.listdir(COVARIANCE) if n.endswith((".hip", ".h"))) == files
    assert os.path.join(COVARIANCE, "ndt2d_covariance_launch.h") in build.HEADERS
    unit = open(os.path.join(COVARIANCE, "ndt2d_covariance.hip")).read()
    for name in ("posegraph/ndt2d_posegraph_state.h", "covariance/ndt2d_covariance_kernel.h", "covariance/ndt2d_covariance_plan.h",
                 "covariance/ndt2d_covariance_launch.h"):
        assert '#include "%s"' % name in unit
    kernels = open(KERNELS).read()
    for name in ("posegraph/ndt2d_posegraph_kernel.h", "posegraph/ndt2d_posegraph_fn.h", "posegraph/ndt2d_posegraph_loss.h"):
        assert '#include "%s"' % name in kernels
    for name in files:
        code = re.sub(r"//[^\n]*", "", open(os.path.join(COVARIANCE, name)).read())
        assert "atomic" not in code.lower(), name                                            # a block has one writer, no split sums
        assert not re.search(r'#include\s+"[^"]*\.hip"', code), name                         # no unit includes a .hip
    assert re.findall(r"\bndt2d_covariance_\w+(?=\()", re.sub(r"//[^\n]*", "", unit)).count("ndt2d_covariance_compute") == 1
    bodies = re.findall(r"\nint ndt2d_covariance_\w+\([^)]*\)\n\{\n(.*?)\n\}\n", unit, flags=re.S)
    assert len(bodies) == 5                                                                  # (last_error is one line)
    for body in bodies:
        assert body.lstrip().startswith("NDT2D_C_TRY") and "NDT2D_C_CATCH(" in body.splitlines()[-1], body[:80]
    for kernel in ("covariance_nodes_kernel", "covariance_fill_kernel", "covariance_assemble_kernel", "covariance_factor_kernel",
                   "covariance_solve_kernel", "covariance_update_kernel", "covariance_blocks_kernel"):
        assert re.search(r"__global__ void __launch_bounds__\(\w+\) " + kernel + r"\(", kernels), kernel
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in kernels
    # nothing of the pose graph's own units moved: the dense covariance is not named there
    posegraph = os.path.join(ROOT, "ndt_2d_amd", "csrc", "posegraph")
    for name in os.listdir(posegraph):
        if name.endswith((".hip", ".h")):
            assert "ndt2d_covariance" not in open(os.path.join(posegraph, name)).read(), name


def test_null_objects_are_refused_without_a_gpu():
    L = _capi.lib()
    z = np.zeros(16)
    d = _capi.dptr
    p = C.c_void_p()
    assert L.ndt2d_covariance_create(None, 1 << 20, C.byref(p)) == _capi.ERR_INVALID and not p
    assert L.ndt2d_covariance_create(None, 1 << 20, None) == _capi.ERR_INVALID
    assert L.ndt2d_covariance_destroy(None) == _capi.ERR_INVALID
    assert L.ndt2d_covariance_last_error(None) == b"null covariance"
    assert L.ndt2d_covariance_compute(None, None, 1, None, 0.0, None, 0, d(z), None, d(z)) == _capi.ERR_INVALID
    assert L.ndt2d_covariance_compute(None, None, 0, None, 0.0, None, 0, None, None, None) == _capi.ERR_INVALID
    assert L.ndt2d_covariance_set_timing(None, 1) == _capi.ERR_INVALID
    a, b = C.c_float(0.0), C.c_float(0.0)
    assert L.ndt2d_covariance_last_ms(None, C.byref(a), C.byref(b)) == _capi.ERR_INVALID
    assert np.all(z == 0.0)


def test_the_python_layer_and_the_plugin_mirror():
    import inspect
    sig = inspect.signature(PoseGraph.covariances)
    assert list(sig.parameters) == ["self", "masks", "poses", "damping", "pairs", "workspace_bytes"]
    assert sig.parameters["damping"].default == 0.0 and sig.parameters["workspace_bytes"].default > 0
    assert list(inspect.signature(PoseGraph.relative_covariances).parameters)[:2] == ["self", "pairs"]
    method = inspect.signature(graph_io.Graph.closure_distances).parameters["method"]
    assert method.default == "cg"                                                           # the default is what it was
    stub = os.path.join(ROOT, "tests", "stubs", "pose_graph_covariance_instantiation.cpp")
    done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "stubs"), stub], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr
    text = open(os.path.join(ROOT, "ndt_2d_amd", "plugin", "pose_graph_hip.hpp")).read()
    for member in ("bool covariances(", "double pivotRatio(", "ndt2d_covariance_create(", "ndt2d_covariance_compute(", "ndt2d_covariance_destroy("):
        assert member in text, member
    code = re.sub(r"//[^\n]*", "", text)
    assert "Eigen" not in code and "rclcpp" not in code and "ceres" not in code
    assert code.index("dropCovariance();") < code.index("ndt2d_posegraph_destroy(pg_)")     # destroyed before the pose graph
