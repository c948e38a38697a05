"""Host side of the Newton NDT registration's 3 x 3 neighbourhood and of the covariance from H
(csrc/refine/): the symbols, the restatement of the 3 x 3 objective (tests/
refine_neighbours_restatement.py) against the one-cell restatement and against central differences,
its smoothness along a line, ndt2d_refine_covariance, the covariance header under the sanitizers,
and the plugin's new members.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import refine_cases
import refine_neighbours_restatement as R9
import refine_restatement as R
from test_gpu_match_starts import NEAR, STARTS, fixture  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ndt2d_refine_set_neighbourhood", "ndt2d_refine_neighbourhood", "ndt2d_refine_covariance",
               "ndt2d_matcher_set_refine_neighbourhood", "ndt2d_matcher_refine_neighbourhood")


def test_header_declares_and_library_exports_the_new_symbols():
    from ndt_2d_amd import _capi
    raw = open(os.path.join(ROOT, "include", "ndt2d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(ndt2d_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert _capi.lib().ndt2d_abi_version() == 4
    # the contract is in the header
    for phrase in ("(dy, dx) = (j / 3 - 1, j % 3 - 1)", "i = K beam + j", "clipped on", "H -> sum J^T I J",
                   "no longer\n * what score_points gives"):
        assert phrase in raw, phrase


def test_setters_refuse_without_a_device():
    """No object can be made without a device: every value, the legal ones too, is refused on a
    null object, as the existing entry points refuse theirs (the refusal of 0, 5 and 10 on a real
    object is tests/test_gpu_refine_neighbours.py's)."""
    from ndt_2d_amd import _capi
    L = _capi.lib()
    out = C.c_uint32(77)
    for cells in (0, 5, 10, 1, 9):
        assert L.ndt2d_refine_set_neighbourhood(None, cells) == _capi.ERR_INVALID
        assert L.ndt2d_matcher_set_refine_neighbourhood(None, cells) == _capi.ERR_INVALID
    assert L.ndt2d_refine_neighbourhood(None, C.byref(out)) == _capi.ERR_INVALID and out.value == 77
    assert L.ndt2d_matcher_refine_neighbourhood(None, C.byref(out)) == _capi.ERR_INVALID and out.value == 77
    z = np.zeros(9)
    assert L.ndt2d_refine_covariance(None, _capi.dptr(z)) == _capi.ERR_INVALID
    assert L.ndt2d_refine_covariance(_capi.dptr(z), None) == _capi.ERR_INVALID


def _poses(fixture):
    """tests/test_refine_host.py's: the fixture's starts beside the truth and the six near starts."""
    return np.vstack([STARTS[list(NEAR)], refine_cases.NEAR6])


def _flat(e):
    f, g, H = e
    return np.array([f] + list(g) + list(H))


def test_one_cell_restatement_has_the_bits_of_the_existing_one(fixture):
    for resolution, beams in ((0.25, 100), (0.3, 100), (0.25, 720)):
        c = refine_cases.case(fixture, resolution, beams)
        for pose in np.vstack([STARTS, refine_cases.NEAR6]):
            for order in ("sequential", "strided"):
                want, wmag = R.evaluate(c["grid"], c["beams"], pose, order=order)
                got, gmag = R9.evaluate(c["grid"], c["beams"], pose, cells=1, order=order)
                assert np.array_equal(_flat(got), _flat(want), equal_nan=True), (resolution, beams, order, tuple(pose))
                assert np.array_equal(gmag, wmag)
    # ... and the iteration on top of it
    c = refine_cases.case(fixture, 0.25, 100)
    for order in ("sequential", "strided"):
        want = R.refine(c["grid"], c["beams"], c["jobs"][0], order=order)
        got = R9.refine(c["grid"], c["beams"], c["jobs"][0], cells=1, order=order)
        assert (got["status"], got["evals"], got["steps"]) == (want["status"], want["evals"], want["steps"])
        assert np.array_equal(got["pose"], want["pose"]) and got["f"] == want["f"] and got["f_start"] == want["f_start"]
        assert np.array_equal(got["H"], want["H"]) and got["lam"] == want["lam"]


def test_nine_cells_only_add_and_both_orders_agree(fixture):
    """The added terms are e >= 0: f9 <= f1 wherever both are finite.  The strided order adds the
    same items: the same sums to 9 N units of 2^-53 of the magnitudes."""
    lower = 0
    for resolution, beams in ((0.25, 100), (0.3, 100), (0.25, 720), (0.3, 720)):
        c = refine_cases.case(fixture, resolution, beams)
        for pose in np.vstack([STARTS, refine_cases.NEAR6, c["winners"]]):
            (f1, _, _), _ = R.evaluate(c["grid"], c["beams"], pose)
            (f9, g9, H9), mag = R9.evaluate(c["grid"], c["beams"], pose)
            if np.isfinite(f1) and np.isfinite(f9):
                assert f9 <= f1, (resolution, beams, tuple(pose), f9, f1)
                lower += f9 < f1
            assert (f1 == 0.0) <= (f9 <= 0.0)
            strided, _ = R9.evaluate(c["grid"], c["beams"], pose, order="strided")
            dev = np.abs(_flat(strided) - _flat((f9, g9, H9)))
            assert np.all(dev <= 9 * beams * 2.0 ** -53 * mag), (resolution, beams, tuple(pose))
    assert lower >= 40      # the neighbours do add something wherever the scan overlaps the map


def test_nine_cell_gradient_and_hessian_agree_with_central_differences(fixture):
    """tests/test_refine_host.py's method and bound on the 3 x 3 objective: g against central
    differences (step 1e-6) of the restated f9, H against central differences of the restated g, to
    1e-5 relative to the sum of the magnitudes of the terms."""
    h = 1e-6
    worst = 0.0
    for resolution in (0.25, 0.3):
        c = refine_cases.case(fixture, resolution, 100)
        for k, pose in enumerate(_poses(fixture)):
            (f, g, H), mag = R9.evaluate(c["grid"], c["beams"], pose)
            assert f / c["n"] < -0.05, (resolution, k)
            g, H = np.array(g), np.array(H)
            full = np.array([[H[0], H[1], H[2]], [H[1], H[3], H[4]], [H[2], H[4], H[5]]])
            hmag = np.array([[mag[4], mag[5], mag[6]], [mag[5], mag[7], mag[8]], [mag[6], mag[8], mag[9]]])
            for j in range(3):
                up, down = np.array(pose), np.array(pose)
                up[j] += h
                down[j] -= h
                (f_up, g_up, _), _ = R9.evaluate(c["grid"], c["beams"], up)
                (f_down, g_down, _), _ = R9.evaluate(c["grid"], c["beams"], down)
                dev = abs((f_up - f_down) / (2 * h) - g[j])
                print("res %.2f pose %d g[%d] %.6e: deviation %.2e of the magnitude" % (resolution, k, j, g[j], dev / mag[1 + j]))
                assert dev <= 1e-5 * mag[1 + j], (resolution, k, j)
                worst = max(worst, dev / mag[1 + j])
                column = (np.array(g_up) - np.array(g_down)) / (2 * h)
                assert np.all(np.abs(column - full[:, j]) <= 1e-5 * hmag[:, j]), (resolution, k, j, column, full[:, j])
    print("largest deviation of g: %.2e of the magnitude" % worst)


def _line_defect(c, cells):
    poses = R9.line_poses(c["jobs"][1])
    f, g = [], []
    for p in poses:
        (fk, gk, _), _ = R9.evaluate(c["grid"], c["beams"], p, cells=cells)
        f.append(fk)
        g.append(gk)
    return R9.trapezoid_defect(poses, f, g)


def test_the_nine_cell_objective_is_smooth_along_a_line(fixture):
    """300 poses jobs[1] + k (0.5 mm, 0.3 mm, 0) on the 0.25 m grid: the trapezoid defect
    |f(p2) - f(p1) - 1/2 (g1 + g2) . (p2 - p1)| summed over the line -- O(h^3) per step for a smooth
    function, O(jump) at a cell border -- is for the 3 x 3 objective at most 1/50 of the one-cell
    objective's (here: 7.8 -> 0.048 with 100 beams, 34 -> 0.14 with 720)."""
    for beams in (100, 720):
        c = refine_cases.case(fixture, 0.25, beams)
        one, one_max = _line_defect(c, 1)
        nine, nine_max = _line_defect(c, 9)
        print("%d beams: defect %.4g (largest step %.4g) with one cell, %.4g (%.4g) with 3 x 3: 1/%.0f" % (
            beams, one, one_max, nine, nine_max, one / nine))
        assert one > 1.0                  # the line does cross borders
        assert nine <= one / 50.0, (beams, one, nine)


def test_covariance_entry_point():
    from ndt_2d_amd import _capi, refine_covariance
    L = _capi.lib()

    def call(h6, fill=-3.0):
        h6 = np.ascontiguousarray(h6, dtype=np.float64)
        out = np.full(9, fill)
        return L.ndt2d_refine_covariance(_capi.dptr(h6), _capi.dptr(out)), out

    # a diagonal H whose pivots have exact square roots: exact reciprocals
    rc, cov = call([4.0, 0.0, 0.0, 16.0, 0.0, 0.25])
    assert rc == _capi.OK and np.array_equal(cov.reshape(3, 3), np.diag([0.25, 0.0625, 4.0]))
    # ... any other diagonal: to two units in the last place (sqrt, reciprocal and square each round)
    rc, cov = call([3.0, 0.0, 0.0, 7.0, 0.0, 0.1])
    assert rc == _capi.OK and np.allclose(np.diag(cov.reshape(3, 3)), [1 / 3.0, 1 / 7.0, 10.0], rtol=4 * 2.0 ** -53, atol=0)
    # a fixed symmetric positive definite H of the size a 100-beam scan gives
    H = np.array([[30411.5, -176.32, 5.6667], [-176.32, 8617.3, 444.44], [5.6667, 444.44, 333333.3]])
    rc, cov = call([H[0, 0], H[0, 1], H[0, 2], H[1, 1], H[1, 2], H[2, 2]])
    want = np.linalg.inv(H)
    assert rc == _capi.OK and np.all(np.abs(cov.reshape(3, 3) - want) <= 1e-12 * np.abs(want)), (cov, want)
    assert np.array_equal(cov.reshape(3, 3), cov.reshape(3, 3).T)            # symmetric bit for bit
    assert np.array_equal(cov.reshape(3, 3), R9.covariance([H[0, 0], H[0, 1], H[0, 2], H[1, 1], H[1, 2], H[2, 2]]))
    # refused, the output untouched: indefinite, singular, zero, NaN, infinite
    for bad in ([-1.0, 0.0, 0.0, 2.0, 0.0, 3.0], [1.0, 2.0, 0.0, 1.0, 0.0, 1.0], [1.0, 1.0, 0.0, 1.0, 0.0, 1.0],
                [0.0] * 6, [float("nan"), 0.0, 0.0, 1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 1.0, float("nan"), 1.0],
                [1.0, 0.0, 0.0, float("inf"), 0.0, 1.0]):
        rc, cov = call(bad)
        assert rc == _capi.ERR_STATE and np.all(cov == -3.0), (bad, rc, cov)
        assert R9.covariance(bad) is None and refine_covariance(bad) is None
    # the Python helper takes the 3 x 3 form too
    assert np.array_equal(refine_covariance(H), cov_of(H))


def cov_of(H):
    return R9.covariance([H[0, 0], H[0, 1], H[0, 2], H[1, 1], H[1, 2], H[2, 2]])


def test_covariance_of_the_restated_converged_jobs(fixture):
    """Every CONVERGED job of the 3 x 3 restatement at (0.25, 100) and (0.3, 100) ends on a positive
    definite H: a covariance exists (here: all 20, one sigma 1.5 .. 5.4 mm and 0.16 .. 0.73 mrad)."""
    from ndt_2d_amd import refine_covariance
    converged = 0
    for resolution in (0.25, 0.3):
        c = refine_cases.case(fixture, resolution, 100)
        for k, job in enumerate(c["jobs"]):
            r = R9.refine(c["grid"], c["beams"], job)
            assert r["f"] <= r["f_start"] < 0.0 and r["status"] in (R.CONVERGED, R.MAX_EVALS, R.STALLED)
            if r["status"] != R.CONVERGED:
                continue
            converged += 1
            cov = refine_covariance(r["H"])
            assert cov is not None, (resolution, k, r["H"])
            assert np.array_equal(cov, R9.covariance(r["H"]))
            sigma = np.sqrt(np.diag(cov))
            print("res %.2f job %2d: %d evals, sigma %.2f mm %.2f mm %.3f mrad" % (resolution, k, r["evals"], 1e3 * sigma[0],
                                                                                     1e3 * sigma[1], 1e3 * sigma[2]))
            assert np.all(sigma > 0.0) and np.all(sigma[:2] < 0.05) and sigma[2] < 0.01
    assert converged >= 12, converged


def test_covariance_header_under_the_sanitizers(tmp_path):
    """tests/cpp/refine_covariance_check.cpp: a program of its own over the plain-C++ header, built
    with the host compiler and -fsanitize=address,undefined (the sanitizer's runtime linked into
    the program), run directly.  Its inverses, printed in hexadecimal, have the restatement's bits."""
    exe = os.path.join(str(tmp_path), "refine_covariance_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-I",
                           os.path.join(ROOT, "ndt_2d_amd", "csrc", "refine"),
                           os.path.join(ROOT, "tests", "cpp", "refine_covariance_check.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.rstrip().endswith("OK") and "FAILED" not in done.stdout and not done.stderr, done.stdout + done.stderr
    lines = [ln for ln in done.stdout.split("\n") if ln.startswith("cov ")]
    assert len(lines) == 5
    for ln in lines:
        left, right = ln[len("cov "):].split(" -> ")
        H = [float.fromhex(v) for v in left.split()]
        got = np.array([float.fromhex(v) for v in right.split()]).reshape(3, 3)
        want = R9.covariance(H)
        assert want is not None and np.array_equal(got, want), ln
    # the step header stays plain C++
    step = open(os.path.join(ROOT, "ndt_2d_amd", "csrc", "refine", "ndt2d_refine_step.h")).read()
    assert "hip_runtime" not in step and "inline bool covariance(" in step


def test_plugin_members_compile():
    src = os.path.join(ROOT, "tests", "stubs", "refine_neighbours_instantiation.cpp")
    done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "stubs"), src],
                          capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr
    text = open(os.path.join(ROOT, "ndt_2d_amd", "plugin", "refine_hip.hpp")).read()
    for member in ("setNeighbourhood(", "double covariance[9];", "bool has_covariance;"):
        assert member in text, member
    assert "Eigen" not in re.sub(r"//[^\n]*", "", text) and "rclcpp" not in text


def test_kernel_keeps_one_cell_apart_and_clips_on_the_cell():
    refine = os.path.join(ROOT, "ndt_2d_amd", "csrc", "refine")
    code = re.sub(r"//[^\n]*", "", open(os.path.join(refine, "ndt2d_refine.hip")).read())
    kernel = re.sub(r"//[^\n]*", "", open(os.path.join(refine, "ndt2d_refine_kernel.h")).read())
    # the kernel's own head, in its header
    assert "template <bool POW2, uint32_t CELLS, class SOURCE>\n__global__" in kernel and "if constexpr (CELLS == 1)" in kernel
    assert "(nx < g.size_x) & (ny < g.size_y)" in kernel and "wave_any(" in kernel and kernel.count("__global__") == 1
    # the unit instantiates both neighbourhoods of it, by name
    assert "launch_refine<9>(" in code and "launch_refine<1>(" in code
    assert "refine_kernel<true, CELLS, InstalledSource>" in code and "refine_kernel<false, CELLS, InstalledSource>" in code
    assert "installed_kernel" not in code and "installed_kernel" not in kernel
