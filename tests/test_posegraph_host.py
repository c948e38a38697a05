"""The host side of the pose graph without a GPU: the plain-C++ arithmetic header in a program of
its own (plainly and under the sanitizers), the plugin mirror's compile, the Python conversions
(make_constraint, closure_constraints), the mask rule, and the entry points' null handling."""
import os
import re
import subprocess

import numpy as np
import pytest

import posegraph_restatement as R
from ndt_2d_amd import _capi, build, closure_constraints, graph_io, make_constraint
from ndt_2d_amd.pose_graph import check_masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_cpp_arithmetic_in_a_program_of_its_own_and_under_the_sanitizers(tmp_path):
    """tests/cpp/posegraph_fn_check.cpp over csrc/posegraph/ndt2d_posegraph_fn.h: built with the host
    compiler, plainly and with -fsanitize=address,undefined (the runtime linked into the program),
    run directly.  Its own checks: the Jacobians against differences, the products, the inverse,
    the Cholesky's refusals.  Here: Normalize's printed results equal the restatement's bit for bit."""
    src = os.path.join(ROOT, "tests", "cpp", "posegraph_fn_check.cpp")
    inc = os.path.join(ROOT, "ndt_2d_amd", "csrc", "posegraph")
    common = ["g++", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", inc, src]
    plain, sanitized = os.path.join(str(tmp_path), "fn_check"), os.path.join(str(tmp_path), "fn_check_san")
    subprocess.check_call(common + ["-O2", "-o", plain])
    subprocess.check_call(common + ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", sanitized])
    outputs = []
    for exe in (plain, sanitized):
        done = subprocess.run([exe], capture_output=True, text=True)
        assert done.returncode == 0 and not done.stderr, done.stderr
        assert done.stdout.splitlines()[-1] == "ok"
        outputs.append(done.stdout)
    assert outputs[0] == outputs[1]
    rows = [line.split() for line in outputs[0].splitlines() if line.startswith("N ")]
    values = [float.fromhex(r[1]) for r in rows]
    assert len(rows) >= 12
    for wanted in (-R.PI, R.PI, np.nextafter(R.PI, 0.0), 3.0 * R.PI, -3.0 * R.PI, 1e6):
        assert wanted in values
    for r in rows:
        v, got = float.fromhex(r[1]), float.fromhex(r[2])
        assert got == float(R.normalize(v)) and np.signbit(got) == np.signbit(float(R.normalize(v))), r


def test_the_plugin_mirror_compiles():
    stub = os.path.join(ROOT, "tests", "stubs", "pose_graph_instantiation.cpp")
    done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "stubs"), stub], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr
    text = open(os.path.join(ROOT, "ndt_2d_amd", "plugin", "pose_graph_hip.hpp")).read()
    for member in ("bool optimize(const Constraints & constraints, Scans & scans)", "ndt2d_posegraph_solve(", "ndt2d_posegraph_set_graph(",
                   "bool consistency("):
        assert member in text, member
    code = re.sub(r"//[^\n]*", "", text)
    assert "Eigen" not in code and "rclcpp" not in code and "ceres" not in code


def test_the_unit_is_built_hashed_and_bound():
    posegraph = os.path.join(ROOT, "ndt_2d_amd", "csrc", "posegraph")
    for unit in ("ndt2d_posegraph.hip", "ndt2d_posegraph_robust.hip", "ndt2d_posegraph_marginals.hip"):
        assert "posegraph/" + unit in build.SOURCES, unit
    for name in ("ndt2d_posegraph_fn.h", "ndt2d_posegraph_kernel.h", "ndt2d_posegraph_state.h", "ndt2d_posegraph_args.h"):
        assert os.path.join(posegraph, name) in build.HEADERS, name
    names = [n for n in _capi.SIGNATURES if n.startswith("ndt2d_posegraph_")]
    assert sorted(names) == sorted("ndt2d_posegraph_" + n for n in (
        "create", "destroy", "last_error", "set_graph", "set_weighting", "weighting", "evaluate", "solve", "set_timing", "last_ms"))
    header = open(os.path.join(ROOT, "include", "ndt2d_hip.h")).read()
    assert "#define NDT2D_ABI_VERSION 4" in header and "e^T L^T L e" in header
    sources = sorted(n for n in os.listdir(posegraph) if n.endswith((".hip", ".h")))
    assert len(sources) == 10, sources                           # three units, the kernel and state headers, five of plain C++
    for name in sources:                                         # a result is bit-identical run to run
        assert "atomic" not in re.sub(r"//[^\n]*", "", open(os.path.join(posegraph, name)).read()), name
        assert len(open(os.path.join(posegraph, name)).read().splitlines()) <= 900, name
    unit = open(os.path.join(posegraph, "ndt2d_posegraph.hip")).read()
    assert '#include "posegraph/ndt2d_posegraph_fn.h"' in unit and '#include "posegraph/ndt2d_posegraph_kernel.h"' in unit
    assert '#include "batch/ndt2d_batch_state.h"' in unit and "ndt2d_batch_host.h" not in unit and "ndt2d_batch_search.h" not in unit
    bodies = re.findall(r"\n(?:int|const char \*) ndt2d_posegraph_\w+\([^)]*\)\n\{\n(.*?)\n\}\n", unit, flags=re.S)
    assert len(bodies) == 10
    for body in bodies:
        if body.count("\n") > 1:                                 # every multi-line body sits in the guard
            assert body.lstrip().startswith("NDT2D_C_TRY") and "NDT2D_C_CATCH(" in body.splitlines()[-1], body[:80]


def test_null_objects_are_refused_without_a_gpu():
    L = _capi.lib()
    out = _capi.C.c_void_p()
    assert L.ndt2d_posegraph_create(None, 4, 4, 1, _capi.C.byref(out)) == _capi.ERR_INVALID and not out.value
    assert L.ndt2d_posegraph_create(None, 4, 4, 1, None) == _capi.ERR_INVALID
    z = np.zeros(9)
    assert L.ndt2d_posegraph_destroy(None) == _capi.ERR_INVALID
    assert L.ndt2d_posegraph_set_graph(None, _capi.dptr(z), 1, None, None, None, None, 0, 0) == _capi.ERR_INVALID
    assert L.ndt2d_posegraph_set_weighting(None, b"reference") == _capi.ERR_INVALID
    assert L.ndt2d_posegraph_evaluate(None, None, 1, _capi.dptr(z), None, None) == _capi.ERR_INVALID
    assert L.ndt2d_posegraph_solve(None, None, 1, 100, 0.0, 0.0, 0.0, _capi.dptr(z), _capi.dptr(z), None) == _capi.ERR_INVALID
    assert L.ndt2d_posegraph_set_timing(None, 1) == _capi.ERR_INVALID
    assert L.ndt2d_posegraph_last_ms(None, None, None) == _capi.ERR_INVALID
    assert L.ndt2d_posegraph_last_error(None) == b"null posegraph" and L.ndt2d_posegraph_weighting(None) == b""


def test_make_constraint_is_the_references():
    """src/constraint.cpp:35-56; the information against numpy's inverse within the project's 1e-12
    relative bound, on well-conditioned covariances."""
    rng = np.random.default_rng(8)
    for _ in range(20):
        a = rng.normal(0.0, 1.0, (3, 3))
        cov = a @ a.T + 3.0 * np.eye(3)                                        # condition number of a few
        cov *= 10.0 ** rng.uniform(-4, 0)
        frm, to = rng.normal(0.0, 3.0, 3), rng.normal(0.0, 3.0, 3)
        c = make_constraint(3, 7, frm, to, cov)
        want_t, want_i = R.make_constraint(frm, to, cov)
        assert (c.begin, c.end, c.switchable) == (3, 7, False)
        assert np.array_equal(c.transform, want_t)
        assert np.all(np.abs(c.information - want_i) <= 1e-12 * np.max(np.abs(want_i)))
        assert R.cholesky_lower(c.information) is not None
    # the heading difference is not wrapped, the translation is in the from-pose's frame
    c = make_constraint(0, 1, (1.0, 1.0, np.pi / 2), (1.0, 3.0, -3.0), np.eye(3))
    assert np.allclose(c.transform, [2.0, 0.0, -3.0 - np.pi / 2], atol=1e-15)


def test_closure_constraints_on_hand_made_accepted_lists():
    poses = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [2.0, 1.0, 1.0]])
    cov, rcov = np.diag([0.04, 0.04, 0.01]), np.diag([0.01, 0.02, 0.0025])
    lattice = dict(candidate=1, score=-0.4, correction=np.zeros(3), covariance=cov, pose=np.array([1.5, 0.5, 0.75]))
    usable = dict(lattice, candidate=2, refined_pose=np.array([1.52, 0.49, 0.76]), refined_covariance=rcov, refine_status=_capi.REFINE_CONVERGED,
                  refine_usable=True)
    rose = dict(usable, candidate=0, refine_usable=False)                      # f rose or the iteration failed: the lattice's
    no_cov = dict(usable, candidate=1, refined_covariance=None)                # the Hessian was not definite: the lattice's
    got = closure_constraints([lattice, usable, rose, no_cov], 9, poses)
    assert [(c.begin, c.end, c.switchable) for c in got] == [(1, 9, True), (2, 9, True), (0, 9, True), (1, 9, True)]
    for c, entry, pose, covariance in ((got[0], lattice, lattice["pose"], cov), (got[1], usable, usable["refined_pose"], rcov),
                                       (got[2], rose, lattice["pose"], cov), (got[3], no_cov, lattice["pose"], cov)):
        want = make_constraint(entry["candidate"], 9, poses[entry["candidate"]], pose, covariance)
        assert np.array_equal(c.transform, want.transform) and np.array_equal(c.information, want.information)
        assert isinstance(c, graph_io.Constraint)
    assert closure_constraints([], 9, poses) == []


def test_masks_may_switch_off_switchable_constraints_only():
    switchable = np.array([False, False, True, True])
    en = check_masks([[1, 1, 0, 1], [1, 1, 1, 0], [5, 1, 0, 0]], switchable)
    assert en.dtype == np.uint8 and en.flags["C_CONTIGUOUS"] and en.tolist() == [[1, 1, 0, 1], [1, 1, 1, 0], [1, 1, 0, 0]]
    with pytest.raises(ValueError, match="mask 1 switches off constraint 0, which is not switchable"):
        check_masks([[1, 1, 0, 1], [0, 1, 1, 1]], switchable)
    with pytest.raises(ValueError):
        check_masks([[1, 1, 1]], switchable)                                   # not [K, m]


def test_graph_optimize_without_scans_is_false_as_the_references():
    assert graph_io.Graph(False).optimize(None) is False
