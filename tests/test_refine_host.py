"""Host side of the Newton NDT registration (csrc/refine/): the symbols, the plugin header, the
step header under the sanitizers and against the restatement's Cholesky, the restatement pinned
to the oracle, the C entry points' refusals that need no device, refine_matches() against a
stand-in matcher, and the build lists.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import refine_cases
import refine_restatement as R
from test_gpu_match_starts import NEAR, STARTS, fixture  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_INDEX = 2 ** 64 - 1
NEW_SYMBOLS = ("ndt2d_refine_create", "ndt2d_refine_destroy", "ndt2d_refine_last_error", "ndt2d_refine_run",
               "ndt2d_refine_set_timing", "ndt2d_refine_last_ms", "ndt2d_matcher_refine_scans", "ndt2d_matcher_refine")


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
    assert "typedef struct ndt2d_refine ndt2d_refine;" in text
    assert sorted(_capi.SIGNATURES) == sorted(declared)            # the bindings keep covering the header
    assert _capi.lib().ndt2d_abi_version() == 4
    # the status constants and the record: header, bindings and restatement agree
    values = dict(re.findall(r"#define NDT2D_REFINE_([A-Z_]+) (\d+)", text))
    assert values == {"RECORD_DOUBLES": "18", "CONVERGED": "0", "MAX_EVALS": "1", "STALLED": "2", "NO_OVERLAP": "3",
                      "NOT_FINITE": "4"}
    assert (_capi.REFINE_CONVERGED, _capi.REFINE_MAX_EVALS, _capi.REFINE_STALLED, _capi.REFINE_NO_OVERLAP,
            _capi.REFINE_NOT_FINITE) == (R.CONVERGED, R.MAX_EVALS, R.STALLED, R.NO_OVERLAP, R.NOT_FINITE) == (0, 1, 2, 3, 4)
    # the contract is in the header
    for phrase in ("Newton NDT registration", "H_jk", "lambda = max(10 lambda, 1e-3)", "NDT2D_REFINE_RECORD_DOUBLES"):
        assert phrase in raw, phrase


def test_refine_hip_header_compiles():
    src = os.path.join(ROOT, "tests", "stubs", "refine_instantiation.cpp")
    done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "stubs"), src],
                          capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr
    cmake = open(os.path.join(ROOT, "ndt_2d_amd", "plugin", "CMakeLists.txt")).read()
    assert "refine_hip.hpp" in cmake


def test_build_lists_and_the_unit_keeps_no_copy():
    from ndt_2d_amd import build
    csrc = os.path.join(ROOT, "ndt_2d_amd", "csrc")
    assert "refine/ndt2d_refine.hip" in build.SOURCES
    assert os.path.join(csrc, "refine", "ndt2d_refine_step.h") in build.HEADERS
    for name in os.listdir(os.path.join(csrc, "batch")):
        assert os.path.join(csrc, "batch", name) in build.HEADERS, name
    assert os.path.join(csrc, "refine", "ndt2d_refine_kernel.h") in build.HEADERS
    text = open(os.path.join(csrc, "refine", "ndt2d_refine.hip")).read()
    kernel_text = open(os.path.join(csrc, "refine", "ndt2d_refine_kernel.h")).read()
    code, kernel = re.sub(r"//[^\n]*", "", text), re.sub(r"//[^\n]*", "", kernel_text)
    # the shared device functions, the batch host and the stage layout are used, not copied: the
    # host's words in the unit, the kernel's in its header, which the unit includes
    assert '#include "batch/ndt2d_batch_state.h"\n' in text and '#include "refine/ndt2d_refine_kernel.h"\n' in text
    assert '#include "refine/ndt2d_refine_step.h"\n' in kernel_text and '#include "batch/ndt2d_installed_map.h"\n' in kernel_text
    # neither takes the search kernels' header, directly or through the search engine's: the unit compiles its own kernel only
    for header in ("ndt2d_batch_search.h", "ndt2d_batch_host.h"):
        assert header not in code and header not in kernel, header
    for used in ("BatchHost", "installed_grid(", "InstalledSource", "stage_layout(", "batch_round_trip("):
        assert used in code, used
    for used in ("cell_index<POW2>(", "record_exponent(", "exp_score(", "wave_sum_to_last_lane(", "refine::begin(", "refine::take("):
        assert used in kernel and used not in code, used
    # the installed grid's source is the shared one, beside InstalledMap, which it reads through
    installed = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "batch", "ndt2d_installed_map.h")).read())
    assert installed.count("struct InstalledSource") == 1 and "InstalledMap map(uint32_t) const" in installed
    assert "__global__" not in installed and "struct InstalledSource" not in open(os.path.join(csrc, "batch", "ndt2d_batch_search.h")).read()
    for absent in ("hipHostMalloc", "hipEventCreate", "hipEventRecord", "atomic", "__threadfence", "struct InstalledMap", "v_fma_f64",
                   "struct InstalledSource"):
        assert absent not in code and absent not in kernel, absent
    # one kernel, in the header; launched from the unit: pow2 / divide
    assert kernel.count("__global__") == 1 and code.count("__global__") == 0
    assert code.count("hipLaunchKernelGGL") == 2 and kernel.count("hipLaunchKernelGGL") == 0
    # the step is plain C++: no HIP header, no HIP type
    step = open(os.path.join(csrc, "refine", "ndt2d_refine_step.h")).read()
    assert "hip_runtime" not in step and "double2" not in step and "__host__ __device__" in step


def test_step_under_the_sanitizers_and_the_bits_of_its_cholesky(tmp_path):
    """tests/cpp/refine_step_check.cpp: a program of its own, built with the host compiler and
    -fsanitize=address,undefined (the sanitizer's runtime linked into the program), run directly.
    Its positive-definite solves, printed in hexadecimal, have the bits of the restatement's."""
    exe = os.path.join(str(tmp_path), "refine_step_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-I",
                           os.path.join(ROOT, "ndt_2d_amd", "csrc", "refine"),
                           os.path.join(ROOT, "tests", "cpp", "refine_step_check.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.rstrip().endswith("OK") and "FAILED" not in done.stdout and not done.stderr, done.stdout + done.stderr
    assert re.search(r"ladder: 1[67] rungs", done.stdout)
    solves = [ln for ln in done.stdout.split("\n") if ln.startswith("solve ")]
    assert len(solves) == 12
    for ln in solves:
        left, right = ln[len("solve "):].split(" -> ")
        H, g, lam = (part.split() for part in left.split(" | "))
        H, g, lam = [float.fromhex(v) for v in H], [float.fromhex(v) for v in g], float.fromhex(lam[0])
        want = R.cholesky_solve(H, g, lam)
        got = [float.fromhex(v) for v in right.split()]
        assert want is not None and got == want, ln
    # ... and the restatement refuses what the header refuses
    assert R.cholesky_solve([-1.0, 0.0, 0.0, 2.0, 0.0, 3.0], [1.0, 1.0, 1.0], 0.0) is None
    assert R.cholesky_solve([1.0, 1.0, 0.0, 1.0, 0.0, 1.0], [1.0, 0.0, 0.0], 0.0) is None
    assert R.cholesky_solve([float("nan"), 0.0, 0.0, 1.0, 0.0, 1.0], [1.0, 1.0, 1.0], 1e13) is None


def _poses(fixture):
    """The fixture's starts beside the truth and the six near starts of the path test."""
    return np.vstack([STARTS[list(NEAR)], refine_cases.NEAR6])


def test_restated_f_has_the_bits_of_the_oracles_score_points(fixture):
    """Sequential summation: f / N is bit for bit what the oracle's scorePoints returns -- at the
    near poses, at every start of the fixture (off the map, rotated away: f == 0 or tiny), for 100
    and 720 beams and both ways of indexing.  (f == scorePoints x N holds too wherever that
    product is exact; at a few poses it rounds, so the division is what is asserted.)"""
    for resolution in (0.25, 0.3):
        for beams in (100, 720):
            c = refine_cases.case(fixture, resolution, beams)
            assert c["n"] == beams
            for pose in np.vstack([STARTS, refine_cases.NEAR6, c["winners"]]):
                (f, _, _), _ = R.evaluate(c["grid"], c["beams"], pose)
                want = c["ref"].scorePoints(fixture["query"], pose)
                assert f / c["n"] == want, (resolution, beams, tuple(pose), f / c["n"], want)
    # the strided order adds the same terms: the same value to a few units in the last place
    c = refine_cases.case(fixture, 0.25, 720)
    (f, g, H), mag = R.evaluate(c["grid"], c["beams"], STARTS[0])
    (f2, g2, H2), _ = R.evaluate(c["grid"], c["beams"], STARTS[0], order="strided")
    got, want = np.array([-f2] + list(g2) + list(H2)), np.array([-f] + list(g) + list(H))
    assert np.all(np.abs(got - want) <= 720 * 2.0 ** -53 * mag) and f < -10.0


def test_restated_gradient_and_hessian_agree_with_central_differences(fixture):
    """g against central differences (step 1e-6) of the oracle's scorePoints, H against central
    differences of the restated g, to 1e-5 relative -- relative to the sum of the magnitudes of
    the terms, sum_i |e_i a_j|: that is the scale both the sum and the difference quotient are
    computed on.  Near an optimum g is a cancelling sum and the quotient's own truncation error,
    h^2 f''' / 6, is not small against |g|: at the fixture's start 1 (the true pose) and resolution
    0.25 it is 2.4e-5 of max |g| and falls a hundredfold per decade of h; against the magnitudes
    the largest deviation seen here is 6.4e-7.  Printed both ways."""
    h = 1e-6
    worst = 0.0
    for resolution in (0.25, 0.3):
        c = refine_cases.case(fixture, resolution, 100)
        n, ref, query = c["n"], c["ref"], fixture["query"]
        for k, pose in enumerate(_poses(fixture)):
            (f, g, H), mag = R.evaluate(c["grid"], c["beams"], pose)
            assert f / n < -0.05, (resolution, k)                       # the scan overlaps the map here
            g, H = np.array(g), np.array(H)
            full = np.array([[H[0], H[1], H[2]], [H[1], H[3], H[4]], [H[2], H[4], H[5]]])
            hmag = np.array([[mag[4], mag[5], mag[6]], [mag[5], mag[7], mag[8]], [mag[6], mag[8], mag[9]]])
            for j in range(3):
                up, down = np.array(pose), np.array(pose)
                up[j] += h
                down[j] -= h
                quotient = (ref.scorePoints(query, up) - ref.scorePoints(query, down)) / (2 * h) * n
                dev = abs(quotient - g[j])
                print("res %.2f pose %d g[%d] %.6e quotient %.6e: %.2e of |g|max, %.2e of the magnitude" % (
                    resolution, k, j, g[j], quotient, dev / np.max(np.abs(g)), dev / mag[1 + j]))
                assert dev <= 1e-5 * mag[1 + j], (resolution, k, j)
                worst = max(worst, dev / mag[1 + j])
                (_, g_up, _), _ = R.evaluate(c["grid"], c["beams"], up)
                (_, g_down, _), _ = R.evaluate(c["grid"], c["beams"], down)
                column = (np.array(g_up) - np.array(g_down)) / (2 * h)
                assert np.all(np.abs(column - full[:, j]) <= 1e-5 * hmag[:, j]), (resolution, k, j, column, full[:, j])
    print("largest deviation of g: %.2e of the magnitude" % worst)


def test_restated_iteration_descends_and_its_probes_agree(fixture):
    """The path test's qualification on the CPU: per setting at least 8 of the 12 jobs take the
    same path (status, evals, pose to 1e-9) under sequential sums, strided sums and a start nudged
    by 1e-13; every run obeys the contract."""
    c = refine_cases.case(fixture, 0.25, 100)
    qualified = 0
    for k, pose in enumerate(c["jobs"]):
        runs = [R.refine(c["grid"], c["beams"], pose), R.refine(c["grid"], c["beams"], pose, order="strided"),
                R.refine(c["grid"], c["beams"], pose + 1e-13)]
        for r in runs:
            assert r["f"] <= r["f_start"] < 0.0 and 1 <= r["evals"] <= 32 and r["steps"] <= r["evals"] - 1
            assert r["status"] in (R.CONVERGED, R.MAX_EVALS, R.STALLED)
            assert (r["status"] != R.CONVERGED or r["evals"] < 32) and (r["status"] != R.MAX_EVALS or r["evals"] == 32)
            (f, _, _), _ = R.evaluate(c["grid"], c["beams"], r["pose"])
            assert abs(f - r["f"]) <= 1e-9 * c["n"]
        same = all(r["status"] == runs[0]["status"] and r["evals"] == runs[0]["evals"] for r in runs)
        spread = max(float(np.max(np.abs(r["pose"] - runs[0]["pose"]))) for r in runs)
        qualified += bool(same and spread <= 1e-9)
        if k >= 6:   # from a lattice winner the refined pose scores strictly below it
            assert runs[0]["f"] < runs[0]["f_start"] and runs[0]["steps"] >= 1, k
    assert qualified >= 8, qualified
    # max_evals = 1 is the evaluation alone; off the map nothing scores
    one = R.refine(c["grid"], c["beams"], c["jobs"][0], max_evals=1)
    assert one["status"] == R.MAX_EVALS and one["evals"] == 1 and one["f"] == one["f_start"]
    off = R.refine(c["grid"], c["beams"], (40.0, 40.0, 0.0))
    assert off["status"] == R.NO_OVERLAP and off["evals"] == 1 and off["f"] == 0.0
    assert np.array_equal(off["pose"], [40.0, 40.0, 0.0])


def test_entry_points_refuse_null_arguments_without_a_device():
    from ndt_2d_amd import _capi
    L = _capi.lib()
    out = C.c_void_p(0x1)
    assert L.ndt2d_refine_create(None, 4, C.byref(out)) == _capi.ERR_INVALID and not out.value
    assert L.ndt2d_refine_create(None, 4, None) == _capi.ERR_INVALID
    assert L.ndt2d_refine_destroy(None) == _capi.ERR_INVALID
    assert L.ndt2d_refine_last_error(None) == b"null refine"
    assert L.ndt2d_refine_set_timing(None, 1) == _capi.ERR_INVALID
    assert L.ndt2d_refine_last_ms(None, None, None) == _capi.ERR_INVALID
    z = np.zeros(18)
    off = np.array([0, 1], dtype=np.uintp)
    offp = off.ctypes.data_as(C.POINTER(C.c_size_t))
    assert L.ndt2d_refine_run(None, _capi.dptr(z), None, 1, _capi.dptr(z), offp, 1, 32, 1e-6, 1e-6,
                              _capi.dptr(z)) == _capi.ERR_INVALID
    status = np.zeros(1, dtype=np.int32)
    assert L.ndt2d_matcher_refine_scans(None, _capi.dptr(z), None, 1, _capi.dptr(z), offp, 1, 32, 1e-6, 1e-6, _capi.dptr(z),
                                        _capi.dptr(z), None, None, None, status.ctypes.data_as(C.POINTER(C.c_int32)),
                                        None) == _capi.ERR_INVALID
    assert not L.ndt2d_matcher_refine(None)


class StandInMatcher:
    """matchScans with canned (score, correction, best_index) per job; refineScans records the
    poses it is started from."""

    def __init__(self, canned):
        self.canned = canned
        self.calls = []

    def matchScans(self, jobs, scans, job_scan=None, want_scores=False):
        self.calls.append(("matchScans", np.array(jobs, dtype=np.float64).copy(), len(scans),
                           None if job_scan is None else list(job_scan)))
        assert len(jobs) == len(self.canned)
        return [dict(score=s, pose=np.array(p, dtype=np.float64), covariance=np.eye(3) * (k + 1), n_candidates=245,
                     best_index=b, scores=None) for k, (s, p, b) in enumerate(self.canned)]

    def refineScans(self, jobs, scans, job_scan=None, max_evals=32, tol_lin=1e-6, tol_ang=1e-6):
        jobs = np.array(jobs, dtype=np.float64)
        self.calls.append(("refineScans", jobs.copy(), len(scans), None if job_scan is None else list(job_scan),
                           (max_evals, tol_lin, tol_ang)))
        return [dict(pose=j + 0.001, score=-0.5 - k, start_score=-0.25, gradient=np.zeros(3), hessian=np.eye(3), evals=7,
                     steps=5, status=0) for k, j in enumerate(jobs)]


def test_refine_matches_starts_from_the_winners_and_keeps_the_job_order():
    from ndt_2d_amd import refine_matches
    canned = [(-0.10, (0.01, 0.0, 0.0), 7),
              (-0.30, (0.02, -0.03, 0.004), 9),
              (0.0, (0.0, 0.0, 0.0), NO_INDEX),     # no winner: refined from the job's own pose
              (-0.45, (0.05, 0.0, -0.01), 11)]
    jobs = np.array([[1.0 * k + 0.5, 2.0 * k, 0.1 * k] for k in range(len(canned))])
    scans = [np.zeros((4, 2)), np.ones((3, 2)), np.zeros((5, 2))]
    job_scan = [2, 0, 0, 1]
    stub = StandInMatcher(canned)
    out = refine_matches(stub, jobs, scans, job_scan=job_scan, max_evals=12, tol_ang=1e-7)
    assert [c[0] for c in stub.calls] == ["matchScans", "refineScans"]            # one call of each
    assert np.array_equal(stub.calls[0][1], jobs) and stub.calls[0][2] == 3 and stub.calls[0][3] == job_scan
    starts = stub.calls[1][1]
    for k in range(4):
        # job pose + correction, as src/ndt_mapper.cpp:557-561 adds it
        assert np.array_equal(starts[k], np.array(canned[k][1]) + jobs[k])
    assert np.array_equal(starts[2], jobs[2])
    assert stub.calls[1][2] == 3 and stub.calls[1][3] == job_scan and stub.calls[1][4] == (12, 1e-6, 1e-7)
    assert [r["job"] for r in out] == [0, 1, 2, 3] and [r["scan"] for r in out] == job_scan
    for k, r in enumerate(out):
        assert sorted(r) == ["job", "match", "pose", "refined", "scan", "score", "start"]
        assert r["match"]["score"] == canned[k][0] and np.array_equal(r["start"], starts[k])
        assert np.array_equal(r["pose"], starts[k] + 0.001) and r["score"] == -0.5 - k       # the refined ones: absolute
        assert r["refined"]["evals"] == 7
    assert np.array_equal(jobs[1], [1.5, 2.0, 0.1])                     # the caller's poses are not written through
    # no job_scan: job k uses scan k
    stub = StandInMatcher(canned[:3])
    out = refine_matches(stub, jobs[:3], scans)
    assert stub.calls[0][3] is None and stub.calls[1][3] is None and [r["scan"] for r in out] == [0, 1, 2]
    # without jobs no call is made
    stub = StandInMatcher([])
    assert refine_matches(stub, np.zeros((0, 3)), []) == [] and stub.calls == []
