"""The host side of the pose graph's "chain" preconditioner without a GPU: the plain-C++ reduction
header in a program of its own (plainly and under the sanitizers), the two entry points in the header
and the bindings, their null handling, the ABI version, and the header in the library's hash."""
import os
import re
import subprocess

from ndt_2d_amd import _capi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_reduction_header_in_a_program_of_its_own_and_under_the_sanitizers(tmp_path):
    """tests/cpp/posegraph_chain_check.cpp over csrc/posegraph/ndt2d_posegraph_chain.h: built with the
    host compiler, plainly and with -fsanitize=address,undefined (the runtime linked into the
    program), run directly.  Its own checks: the level arithmetic, the drivers against a Cholesky on
    random positive definite systems of 1 .. 9, 31, 32, 33, 1,023, 1,024, 1,025 and 2,049 nodes with
    cut edges (|M z - r| <= 1e-12 |r|), and that a block that is not positive definite is reported.
    Here: every size was run with every cut, and the printed residuals meet the bound."""
    src = os.path.join(ROOT, "tests", "cpp", "posegraph_chain_check.cpp")
    inc = os.path.join(ROOT, "ndt_2d_amd", "csrc", "posegraph")
    common = ["g++", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", inc, src]
    plain, sanitized = os.path.join(str(tmp_path), "chain_check"), os.path.join(str(tmp_path), "chain_check_san")
    subprocess.check_call(common + ["-O2", "-o", plain])
    subprocess.check_call(common + ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", sanitized])
    outputs = []
    for exe in (plain, sanitized):
        done = subprocess.run([exe], capture_output=True, text=True)
        assert done.returncode == 0 and not done.stderr, done.stderr
        assert done.stdout.splitlines()[-1] == "ok"
        outputs.append(done.stdout)
    rows = [line.split() for line in outputs[0].splitlines() if line.startswith("S ")]
    assert sorted({int(r[1]) for r in rows}) == [1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 32, 33, 1023, 1024, 1025, 2049]
    assert len(rows) == 16 * 4 and {int(r[2]) for r in rows} == {0, 1, 2, 3}
    for r in rows:
        assert float(r[3]) <= 1e-12 and float(r[4]) <= 1e-10, r
    assert [line.split()[:3] for line in outputs[1].splitlines() if line.startswith("S ")] == [r[:3] for r in rows]


def test_the_entry_points_are_declared_bound_and_hashed():
    header = open(os.path.join(ROOT, "include", "ndt2d_hip.h")).read()
    assert "#define NDT2D_ABI_VERSION 4" in header
    assert "int ndt2d_pose_graph_set_preconditioner(ndt2d_posegraph * posegraph, const char * preconditioner);" in header
    assert "const char * ndt2d_pose_graph_preconditioner(ndt2d_posegraph * posegraph);" in header
    assert "block-tridiagonal band of H + lambda D" in header
    for name in ("ndt2d_pose_graph_set_preconditioner", "ndt2d_pose_graph_preconditioner"):
        assert name in _capi.SIGNATURES, name
    assert _capi.SIGNATURES["ndt2d_pose_graph_preconditioner"][0] is _capi.C.c_char_p
    assert os.path.join(ROOT, "ndt_2d_amd", "csrc", "posegraph", "ndt2d_posegraph_chain.h") in build.HEADERS
    # the reduction is used by the chain's device functions, which every pose-graph kernel takes from the kernel header
    kernel = open(os.path.join(ROOT, "ndt_2d_amd", "csrc", "posegraph", "ndt2d_posegraph_kernel.h")).read()
    assert '#include "posegraph/ndt2d_posegraph_chain.h"' in kernel and "pg::chain::factor_node(" in kernel
    assert os.path.join(ROOT, "ndt_2d_amd", "csrc", "posegraph", "ndt2d_posegraph_kernel.h") in build.HEADERS
    unit = open(os.path.join(ROOT, "ndt_2d_amd", "csrc", "posegraph", "ndt2d_posegraph.hip")).read()
    assert '#include "posegraph/ndt2d_posegraph_kernel.h"' in unit
    # as tests/test_posegraph_host.py asks of the ten ndt2d_posegraph_* bodies: a multi-line body sits in the guard
    bodies = re.findall(r"\n(?:int|const char \*) ndt2d_pose_graph_\w+\([^)]*\)\n\{\n(.*?)\n\}\n", unit, flags=re.S)
    assert len(bodies) == 2
    for body in bodies:
        if body.count("\n") > 1:
            assert body.lstrip().startswith("NDT2D_C_TRY") and "NDT2D_C_CATCH(" in body.splitlines()[-1], body[:80]
    plugin = open(os.path.join(ROOT, "ndt_2d_amd", "plugin", "pose_graph_hip.hpp")).read()
    assert "void setPreconditioner(const std::string & preconditioner)" in plugin and "ndt2d_pose_graph_set_preconditioner(" in plugin


def test_a_null_object_is_refused_without_a_gpu():
    L = _capi.lib()
    assert L.ndt2d_abi_version() == 4
    assert L.ndt2d_pose_graph_set_preconditioner(None, b"chain") == _capi.ERR_INVALID
    assert L.ndt2d_pose_graph_set_preconditioner(None, None) == _capi.ERR_INVALID
    assert L.ndt2d_pose_graph_preconditioner(None) == b""
