"""Host side of the (scan, pose) job list the five batched calls take (match_scans, refine_scans,
verify_scans, refine_candidates, verify_candidates): the C++ mirrors on stand-ins for the C entry
points and the matcher's job batch, both under the sanitizers; that every layer has one owner of the
list; the Python packing.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ndt_2d_amd import scan_matcher as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ndt_2d_amd", "csrc")
PLUGIN = os.path.join(ROOT, "ndt_2d_amd", "plugin")
SANITIZED = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all", "-static-libasan"]


def _run(exe):
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip() == "OK" and not done.stderr, done.stdout + done.stderr


def test_mirrors_on_stand_ins_under_the_sanitizers(tmp_path):
    """tests/cpp/job_mirrors_check.cpp: the five matcher mirrors of the plugin directory run, each on
    the one designed list (5 jobs over 4 scans: a shared scan, an empty one, one below and one above
    the beam limit), against stand-ins that record what they are given: the exact arrays of every C
    call, the result structs, last_error() after a refusal, and one loop-closure round with refine
    and verify on.  Built with -fsanitize=address,undefined (the runtime linked into the program),
    run directly."""
    exe = os.path.join(str(tmp_path), "job_mirrors_check")
    subprocess.check_call(SANITIZED + ["-I", os.path.join(ROOT, "include"), "-I", PLUGIN, "-I", os.path.join(CSRC, "refine"),
                                       os.path.join(ROOT, "tests", "cpp", "job_mirrors_check.cpp"), "-o", exe])
    _run(exe)


def test_job_batch_under_the_sanitizers(tmp_path):
    """tests/cpp/job_batch_check.cpp over csrc/host/ndt2d_job_batch.h, linked with
    host/ndt2d_host_ndt.cpp for subsample_into: the designed list with limit 4 -- which jobs and scans
    enter the batch and in which order, with and without job_scan; each scan's beams once, equal to
    subsample_into of that scan alone; limit 0 under both zero rules; the verification's offsets
    table; the records' way back, the in-place move with the empty scan's job in the middle included;
    every refusal's text and which of two is given.  The header is plain C++ and knows no matcher."""
    exe = os.path.join(str(tmp_path), "job_batch_check")
    subprocess.check_call(SANITIZED + ["-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                                       os.path.join(ROOT, "tests", "cpp", "job_batch_check.cpp"),
                                       os.path.join(CSRC, "host", "ndt2d_host_ndt.cpp"), "-o", exe])
    _run(exe)
    code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "host", "ndt2d_job_batch.h")).read())
    assert "hip" not in code.lower() and "ndt2d_matcher" not in code and "mfail" not in code
    from ndt_2d_amd import build
    assert os.path.join(CSRC, "host", "ndt2d_job_batch.h") in build.HEADERS


def test_the_job_list_has_one_owner_in_every_layer():
    """Used from the shared header, not copied: the searches' unit takes its refusals, the plan of the
    scans a chunk sends and their copy from batch/ndt2d_refine_jobs.h; the four calls of the device
    objects are JobList plus their own fields; the matcher keeps no copy of the check or the
    collection; one plugin header collects scans and jobs."""
    scans = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "scans", "ndt2d_scans.hip")).read())
    for used in ("refine_jobs::refusal", "plan_sent_scans(", "copy_sent_scans("):
        assert used in scans, used
    for copied in ("kNotSent =", "kMaxScanBeams =", "beam_offsets decrease"):
        assert copied not in scans, copied
    jobs = open(os.path.join(CSRC, "batch", "ndt2d_refine_jobs.h")).read()
    assert jobs.count("struct JobList") == 1 and "namespace refine_jobs" in jobs and "hip" not in jobs.replace(".hip", "").lower().replace("no hip", "")
    for path, call in ((("batch", "ndt2d_batch_host.h"), "struct JobsCall : refine_jobs::JobList"),
                       (("refine", "ndt2d_refine.hip"), "struct RefineCall : refine_jobs::JobList"),
                       (("closure", "ndt2d_closure.hip"), "struct RefineCall : ndt2d::refine_jobs::JobList"),
                       (("verify", "ndt2d_verify_kernel.h"), "struct VerifyCall : refine_jobs::JobList")):
        text = open(os.path.join(CSRC, *path)).read()
        assert call in text, call
        assert "const uint32_t * job_scan;" not in text, path
    for unit in (("verify", "ndt2d_verify.hip"), ("closure", "ndt2d_closure.hip")):
        assert "1u, 0.0, 0.0" not in open(os.path.join(CSRC, *unit)).read(), unit
    batched = open(os.path.join(CSRC, "host", "ndt2d_batched.cpp")).read()
    assert '#include "host/ndt2d_job_batch.h"\n' in batched
    assert batched.count("point_offsets decrease") <= 1 and batched.count("the pose is not finite") <= 1
    assert "subsample_into(" not in batched and batched.count("ndt2d_closure_create(") == 1
    for used in ("job_list_refusal(", "collect_job_batch(", "deal_refine_records(", "deal_verify_records(", "move_match_records(",
                 "fill_verify_offsets(", "batch_beams("):
        assert used in batched, used
    defining = [n for n in sorted(os.listdir(PLUGIN)) if n.endswith(".hpp") and "std::size_t addScan(" in open(os.path.join(PLUGIN, n)).read()]
    assert defining == ["job_list.hpp"]
    with_ok = [n for n in sorted(os.listdir(PLUGIN)) if n.endswith(".hpp") and "ndt2d_matcher_last_error(m_)" in open(os.path.join(PLUGIN, n)).read()]
    assert with_ok == ["job_list.hpp"]
    assert "job_list.hpp" in open(os.path.join(PLUGIN, "CMakeLists.txt")).read()
    text = re.sub(r"//[^\n]*", "", open(os.path.join(PLUGIN, "job_list.hpp")).read())
    assert "Eigen" not in text and "rclcpp" not in text and "hip_runtime" not in text


LIST = dict(jobs=[[1.0, 2.0, 0.25], [3.0, 4.0, 0.5], [5.0, 6.0, 0.75], [7.0, 8.0, 1.0], [9.0, 10.0, 1.25]],
            scans=[np.arange(12.0).reshape(6, 2), np.zeros((0, 2)), 20.0 + np.arange(6.0).reshape(3, 2),
                   30.0 + np.arange(18.0).reshape(9, 2)],
            job_scan=[0, 1, 2, 0, 3])
CALLERS = ("matchScans", "refineScans", "verifyScans", "refineCandidates", "verifyCandidates")


def test_python_job_list_and_candidates():
    """scan_matcher._JobList and _pack_candidates, which need no matcher: shapes, dtypes, None for no
    job_scan, the two ValueError texts under each caller's name, and an empty list."""
    lst = S._JobList("matchScans", **LIST)
    assert lst.K == 5 and lst.jp.shape == (5, 3) and lst.jp.dtype == np.float64 and lst.jp.flags.c_contiguous
    assert len(lst.arrays) == 4 and [a.shape for a in lst.arrays] == [(6, 2), (0, 2), (3, 2), (9, 2)]
    assert lst.pts.shape == (18, 2) and lst.pts.dtype == np.float64 and lst.pts.flags.c_contiguous
    assert np.array_equal(lst.pts, np.concatenate(LIST["scans"]))
    assert lst.offsets.dtype == np.uintp and lst.offsets.tolist() == [0, 6, 6, 9, 18]
    assert lst.js.dtype == np.uint32 and lst.js.tolist() == [0, 1, 2, 0, 3]
    assert [lst.scan_of(k) for k in range(5)] == [0, 1, 2, 0, 3] and all(type(lst.scan_of(k)) is int for k in range(5))
    # the six C arguments: jobs_xyt, job_scan, n_jobs, points_xy, point_offsets, n_scans
    assert len(lst.args) == 6 and lst.args[2] == 5 and lst.args[5] == 4
    assert C.cast(lst.args[0], C.c_void_p).value == lst.jp.ctypes.data and C.cast(lst.args[1], C.c_void_p).value == lst.js.ctypes.data
    assert C.cast(lst.args[3], C.c_void_p).value == lst.pts.ctypes.data and C.cast(lst.args[4], C.c_void_p).value == lst.offsets.ctypes.data
    # no job_scan: None goes out, job k uses scan k (whether there is one per job is the call's to say)
    plain = S._JobList("refineScans", LIST["jobs"], LIST["scans"], None)
    assert plain.js is None and plain.args[1] is None and [plain.scan_of(k) for k in range(5)] == [0, 1, 2, 3, 4]
    for who in CALLERS:
        for bad in ([0, 1, 2, 0], [0, 1, 2, 0, 3, 3]):
            with pytest.raises(ValueError) as e:
                S._JobList(who, LIST["jobs"], LIST["scans"], bad)
            assert str(e.value) == who + ": job_scan must name one scan per job"
        for bad in ([0, 1, -1, 0, 3], [0, 1, 2 ** 32, 0, 3]):
            with pytest.raises(ValueError) as e:
                S._JobList(who, LIST["jobs"], LIST["scans"], bad)
            assert str(e.value) == who + ": job_scan must hold scan indices"
    empty = S._JobList("verifyScans", np.zeros((0, 3)), [], None)
    assert empty.K == 0 and empty.jp.shape == (0, 3) and empty.pts.shape == (0, 2) and empty.pts.dtype == np.float64
    assert empty.offsets.tolist() == [0] and empty.offsets.dtype == np.uintp and empty.js is None and empty.args[2] == 0 and empty.args[5] == 0
    assert S._JobList("verifyScans", [], [], []).js.shape == (0,)

    offsets, ids, poses = S._pack_candidates([[(3, [0.0, 1.0, 2.0]), (4, [3.0, 4.0, 5.0])], [], [(7, [6.0, 7.0, 8.0])]])
    assert offsets.dtype == np.uintp and offsets.tolist() == [0, 2, 2, 3]
    assert ids.dtype == np.uintp and ids.tolist() == [3, 4, 7]
    assert poses.dtype == np.float64 and poses.shape == (3, 3) and poses.tolist() == [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0], [6.0, 7.0, 8.0]]
    offsets, ids, poses = S._pack_candidates([])
    assert offsets.tolist() == [0] and offsets.dtype == np.uintp and ids.shape == (0,) and ids.dtype == np.uintp and poses.shape == (0, 3)
    # one owner: the three *Candidates methods and the three users of the list hold no packing of their own
    text = open(os.path.join(ROOT, "ndt_2d_amd", "scan_matcher.py")).read()
    assert text.count("_pack_candidates(candidates)") == 4 and text.count("_JobList(") == 3
    assert text.count("for c in candidates for entry in c") == 1 and text.count("must name one") == 1
