"""Host side of the batched scan tracking (csrc/scans/): the symbols, the plugin header,
track_scans() against a stand-in matcher, the C entry points' refusals that need no device, and
the grouping of a chunk's jobs by their number of partial sums.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_INDEX = 2 ** 64 - 1
NEW_SYMBOLS = ("ndt2d_scans_create", "ndt2d_scans_destroy", "ndt2d_scans_last_error", "ndt2d_scans_match",
               "ndt2d_scans_set_timing", "ndt2d_scans_last_ms", "ndt2d_matcher_match_scans", "ndt2d_matcher_scans")


def test_header_declares_and_library_exports_the_new_symbols():
    from ndt_2d_amd import _capi
    text = open(os.path.join(ROOT, "include", "ndt2d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ndt2d_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "typedef struct ndt2d_scans ndt2d_scans;" in text
    assert _capi.lib().ndt2d_abi_version() == 4


def test_track_scans_hip_header_compiles():
    src = os.path.join(ROOT, "tests", "stubs", "track_scans_instantiation.cpp")
    done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "stubs"), src],
                          capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr
    cmake = open(os.path.join(ROOT, "ndt_2d_amd", "plugin", "CMakeLists.txt")).read()
    assert "track_scans_hip.hpp" in cmake


def test_job_groups_under_the_sanitizers(tmp_path):
    """tests/cpp/job_groups_check.cpp: a program of its own, built with the host compiler and
    -fsanitize=address,undefined (the sanitizer's runtime linked into the program), run directly."""
    exe = os.path.join(str(tmp_path), "job_groups_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-I",
                           os.path.join(ROOT, "ndt_2d_amd", "csrc", "batch"),
                           os.path.join(ROOT, "tests", "cpp", "job_groups_check.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.rstrip().endswith("OK") and "FAILED" not in done.stdout and not done.stderr, done.stdout + done.stderr
    for beams, chunks in ((1, 1), (20, 1), (21, 2), (60, 3), (80, 4), (100, 5), (120, 6), (140, 7), (160, 8), (720, 8)):
        assert "beams %d: C %d (expected %d)" % (beams, chunks, chunks) in done.stdout
    # the search takes the plan, the walk, the kernel and the grouping from the shared headers and keeps
    # no copy (tests/test_starts_host.py looks at what the three units must not contain)
    csrc = os.path.join(ROOT, "ndt_2d_amd", "csrc")
    text = open(os.path.join(csrc, "scans", "ndt2d_scans.hip")).read()
    assert '#include "batch/ndt2d_batch_search.h"\n' in text and '#include "batch/ndt2d_batch_host.h"\n' in text
    assert "group_jobs(" in text and "launch_batch_search(" in text and "stage_layout(" in text
    assert "uint32_t sum_chunks" not in text and "void add_beam" not in text
    kernel = open(os.path.join(csrc, "batch", "ndt2d_batch_search.h")).read()
    assert '#include "ndt2d_walk_fn.h"\n' in kernel and "lane_walk<C, POW2>(" in kernel
    host = open(os.path.join(csrc, "batch", "ndt2d_batch_host.h")).read()
    assert '#include "ndt2d_job_groups.h"\n' in host
    from ndt_2d_amd import build
    assert "scans/ndt2d_scans.hip" in build.SOURCES
    for name in os.listdir(os.path.join(csrc, "batch")):
        assert os.path.join(csrc, "batch", name) in build.HEADERS, name


def test_stage_layout_under_the_sanitizers(tmp_path):
    """tests/cpp/stage_layout_check.cpp: a program of its own, built with the host compiler and
    -fsanitize=address,undefined (the sanitizer's runtime linked into the program), run directly."""
    exe = os.path.join(str(tmp_path), "stage_layout_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-I",
                           os.path.join(ROOT, "ndt_2d_amd", "csrc", "batch"),
                           os.path.join(ROOT, "tests", "cpp", "stage_layout_check.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.rstrip().endswith("OK") and "FAILED" not in done.stdout and not done.stderr, done.stdout + done.stderr
    assert "144 cases" in done.stdout
    # the engine takes its offsets from there and computes none itself
    text = open(os.path.join(ROOT, "ndt_2d_amd", "csrc", "scans", "ndt2d_scans.hip")).read()
    assert "stage_layout(" in text and "off_beams" not in text and "& ~size_t(1)" not in text


def test_entry_points_refuse_null_arguments_without_a_device():
    from ndt_2d_amd import _capi
    L = _capi.lib()
    out = C.c_void_p(0x1)
    assert L.ndt2d_scans_create(None, 4, C.byref(out)) == _capi.ERR_INVALID and not out.value
    assert L.ndt2d_scans_create(None, 4, None) == _capi.ERR_INVALID
    assert L.ndt2d_scans_destroy(None) == _capi.ERR_INVALID
    assert L.ndt2d_scans_last_error(None) == b"null scans"
    assert L.ndt2d_scans_set_timing(None, 1) == _capi.ERR_INVALID
    assert L.ndt2d_scans_last_ms(None, None, None) == _capi.ERR_INVALID
    z = np.zeros(12)
    off = np.array([0, 1], dtype=np.uintp)
    offp = off.ctypes.data_as(C.POINTER(C.c_size_t))
    assert L.ndt2d_scans_match(None, _capi.dptr(z), None, 1, _capi.dptr(z), offp, 1, _capi.dptr(z), 1, _capi.dptr(z), 1,
                               _capi.dptr(z), None) == _capi.ERR_INVALID
    assert L.ndt2d_matcher_match_scans(None, _capi.dptr(z), None, 1, _capi.dptr(z), offp, 1, None, None, _capi.dptr(z),
                                       None, None, 0, None) == _capi.ERR_INVALID
    assert not L.ndt2d_matcher_scans(None)


class StandInMatcher:
    """matchScans with canned (score, correction, best_index) per job."""

    def __init__(self, canned):
        self.canned = canned
        self.calls = []

    def matchScans(self, jobs, scans, job_scan=None, want_scores=False):
        self.calls.append((np.array(jobs, dtype=np.float64).copy(), len(scans),
                           None if job_scan is None else list(job_scan)))
        assert len(jobs) == len(self.canned)
        return [dict(score=s, pose=np.array(p, dtype=np.float64), covariance=np.eye(3) * (k + 1), n_candidates=245,
                     best_index=b, scores=None) for k, (s, p, b) in enumerate(self.canned)]


def test_track_scans_keeps_the_job_order_and_adds_the_correction():
    from ndt_2d_amd import track_scans
    canned = [(-0.10, (0.01, 0.0, 0.0), 7),
              (-0.30, (0.02, -0.03, 0.004), 9),
              (0.0, (0.0, 0.0, 0.0), NO_INDEX),     # no winner: the job keeps its pose
              (-0.45, (0.05, 0.0, -0.01), 11)]
    jobs = np.array([[1.0 * k + 0.5, 2.0 * k, 0.1 * k] for k in range(len(canned))])
    scans = [np.zeros((4, 2)), np.ones((3, 2)), np.zeros((5, 2))]
    job_scan = [2, 0, 0, 1]
    stub = StandInMatcher(canned)
    out = track_scans(stub, jobs, scans, job_scan=job_scan)
    assert len(stub.calls) == 1                                         # one batched call
    assert np.array_equal(stub.calls[0][0], jobs) and stub.calls[0][1] == 3 and stub.calls[0][2] == job_scan
    # job order, not score order
    assert [r["job"] for r in out] == [0, 1, 2, 3] and [r["scan"] for r in out] == job_scan
    assert [r["score"] for r in out] == [-0.10, -0.30, 0.0, -0.45]
    for k, r in enumerate(out):
        assert sorted(r) == ["correction", "covariance", "job", "pose", "scan", "score"]
        assert np.array_equal(r["correction"], canned[k][1])
        # pose = job pose + correction, as src/ndt_mapper.cpp:557-561 adds it
        assert np.array_equal(r["pose"], np.array(canned[k][1]) + jobs[k])
        assert np.array_equal(r["covariance"], np.eye(3) * (k + 1))
    assert np.array_equal(out[2]["pose"], jobs[2])
    # the caller's poses are not written through
    assert np.array_equal(jobs[1], [1.5, 2.0, 0.1])
    # no job_scan: job k uses scan k
    stub = StandInMatcher(canned[:3])
    out = track_scans(stub, jobs[:3], scans)
    assert stub.calls[0][2] is None and [r["scan"] for r in out] == [0, 1, 2]


def test_track_scans_without_jobs_makes_no_call():
    from ndt_2d_amd import track_scans
    stub = StandInMatcher([])
    assert track_scans(stub, np.zeros((0, 3)), []) == [] and stub.calls == []
    assert track_scans(stub, [], [np.zeros((4, 2))], job_scan=[]) == [] and stub.calls == []
