"""Host side of the Newton registration on each loop-closure candidate's own map
(ndt2d_closure_refine, ndt2d_matcher_refine_candidates, ScanMatcherNDT.refineCandidates,
close_loops(refine=...)): the symbols, the refusals that need no device, the plugin's members, the
chunk plan under the sanitizers, the shared cases' own assertions, and close_loops' walk on a canned
matcher.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import closure_refine_cases as CC
from ndt_2d_amd import _capi, close_loops, loop_closure_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ndt2d_closure_refine", "ndt2d_closure_set_neighbourhood", "ndt2d_closure_neighbourhood",
               "ndt2d_matcher_refine_candidates")


def test_header_declares_and_library_exports_and_binds_the_new_symbols():
    raw = open(os.path.join(ROOT, "include", "ndt2d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(ndt2d_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert sorted(_capi.SIGNATURES) == sorted(declared)
    assert _capi.lib().ndt2d_abi_version() == 4
    # the contract is in the header
    for phrase in ("job_candidate[k]", "a\n * candidate no job names is not built",
                   "has_ndt and the grid are the same before and after", "reports the last call of either kind"):
        assert phrase in raw, phrase


def test_null_arguments_are_refused_without_a_device():
    L = _capi.lib()
    z3, rec = np.zeros(3), np.zeros(18)
    off = np.zeros(2, dtype=np.uintp)
    off[1] = 1
    ids = np.zeros(1, dtype=np.uintp)
    szp = lambda a: a.ctypes.data_as(C.POINTER(C.c_size_t))   # noqa: E731
    out = C.c_uint32(77)
    for cells in (0, 5, 1, 9):
        assert L.ndt2d_closure_set_neighbourhood(None, cells) == _capi.ERR_INVALID
    assert L.ndt2d_closure_neighbourhood(None, C.byref(out)) == _capi.ERR_INVALID and out.value == 77
    # a null object, whatever else is given -- jobs or none
    for n_jobs in (0, 1):
        assert L.ndt2d_closure_refine(None, 1, szp(off), szp(ids), _capi.dptr(z3), 0.25, 4.75, _capi.dptr(z3), None, None, n_jobs,
                                      _capi.dptr(z3), szp(off), 1, 32, 1e-6, 1e-6, _capi.dptr(rec)) == _capi.ERR_INVALID
        status = np.zeros(1, dtype=np.int32)
        assert L.ndt2d_matcher_refine_candidates(
            None, szp(off), szp(ids), _capi.dptr(z3), 1, _capi.dptr(z3), None, None, n_jobs, _capi.dptr(z3), szp(off), 1, 32, 1e-6,
            1e-6, _capi.dptr(z3), _capi.dptr(z3), None, None, None, status.ctypes.data_as(C.POINTER(C.c_int32)), None) == _capi.ERR_INVALID
    assert not rec.any()


def test_plugin_members_compile():
    for stub in ("closure_refine_instantiation.cpp", "loop_closure_instantiation.cpp"):
        done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I",
                               os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "stubs"),
                               os.path.join(ROOT, "tests", "stubs", stub)], capture_output=True, text=True)
        assert done.returncode == 0 and not done.stderr, done.stderr
    text = open(os.path.join(ROOT, "ndt_2d_amd", "plugin", "loop_closure_hip.hpp")).read()
    for member in ("bool setRefine(", "ndt2d_matcher_refine_candidates(", "double refined_pose[3]", "bool has_refined_covariance"):
        assert member in text, member
    assert "Eigen" not in re.sub(r"//[^\n]*", "", text) and "rclcpp" not in text


def test_chunk_plan_under_the_sanitizers(tmp_path):
    """tests/cpp/closure_jobs_check.cpp: a program of its own over the plain-C++ header, built with
    the host compiler and -fsanitize=address,undefined (the sanitizer's runtime linked into the
    program), run directly: K = 1, unnamed candidates, a scrambled job list, 5 candidates through 2
    slots, 4,097 jobs on one candidate, and every plan returning each job exactly once; what a slot
    takes of a launch's arrays for (n_points, ncell) = (0, 1), (3, 65534), (2048, 7), (5, 6); the sent
    scans of a chunk and their copy into a stage of exactly the chunk's beams."""
    exe = os.path.join(str(tmp_path), "closure_jobs_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-I",
                           os.path.join(ROOT, "ndt_2d_amd", "csrc", "closure"), "-I",
                           os.path.join(ROOT, "ndt_2d_amd", "csrc", "batch"),
                           os.path.join(ROOT, "tests", "cpp", "closure_jobs_check.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip() == "OK" and not done.stderr, done.stdout + done.stderr
    # the plan's header stays plain C++, and the build hashes it
    from ndt_2d_amd import build
    path = os.path.join(ROOT, "ndt_2d_amd", "csrc", "closure", "ndt2d_closure_jobs.h")
    assert path in build.HEADERS
    code = re.sub(r"//[^\n]*", "", open(path).read())
    assert "hip" not in code.lower() and "__device__" not in code


def test_one_kernel_text_for_both_map_sources():
    """The closure instantiates the refinement's kernel from csrc/refine/ndt2d_refine_kernel.h, the
    header the installed grid's unit includes too -- it holds no copy of the evaluation -- reads
    nothing of the installed grid in its source, and launches a block per job."""
    csrc = os.path.join(ROOT, "ndt_2d_amd", "csrc")
    closure = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "closure", "ndt2d_closure.hip")).read())
    refine = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "refine", "ndt2d_refine.hip")).read())
    kernel = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "refine", "ndt2d_refine_kernel.h")).read())
    assert '#include "refine/ndt2d_refine_kernel.h"\n' in closure and '#include "refine/ndt2d_refine_kernel.h"\n' in refine
    assert "refine_kernel<true, CELLS, SlotSource>" in closure and "refine_kernel<false, CELLS, SlotSource>" in closure
    for absent in ("record_exponent(", "exp_score(", "wave_sum_to_last_lane(", "refine::begin(", "atomic", "__threadfence"):
        assert absent not in closure, absent
    source = closure[closure.index("struct SlotSource"):closure.index("using SlotRefineArgs")]
    assert "occ_bits" not in source and "cells_global" not in source
    assert "template <bool POW2, uint32_t CELLS, class SOURCE>\n__global__" in kernel
    assert "a.source.grid(jr.slot)" in kernel and "a.source.map(jr.slot)" in kernel
    # exactly one __global__ of either shared kernel under csrc/, neither macro of the old layout
    # anywhere, and no unit includes a .hip
    count = {"refine_kernel": 0, "verify_kernel": 0}
    for base, _, names in os.walk(csrc):
        for n in names:
            if n.endswith((".hip", ".h", ".cpp")):
                raw = open(os.path.join(base, n)).read()
                for name in count:
                    count[name] += len(re.findall(r"__global__[^;{]*\b%s\b" % name, re.sub(r"//[^\n]*", "", raw)))
                assert "NDT2D_REFINE_KERNEL_ONLY" not in raw and "NDT2D_VERIFY_KERNEL_ONLY" not in raw, n
                assert not re.search(r'#\s*include\s*["<][^">]*\.hip[">]', raw), n
    assert count == {"refine_kernel": 1, "verify_kernel": 1}
    assert closure.count("__global__") == 1 and closure.count("hipLaunchKernelGGL(ndt2d::closure_build_kernel") == 1
    # the refinement's chunk is the shared path with its job record, its launch and its scatter
    chunk = closure[closure.index("int refine_chunk("):closure.index("int verify_chunk(")]
    assert "job_chunk(" in chunk and "RefineJob{" in chunk and "launch_slot_refine<9>(" in chunk and "launch_slot_refine<1>(" in chunk
    assert "hipMemcpyAsync" not in chunk and "launch_build(" not in chunk
    # the kernel's header is hashed with the headers: an edit to the kernel makes the unit's and
    # the closure's object stale, so the library cannot come to hold two texts of it
    from ndt_2d_amd import build
    assert os.path.join(csrc, "refine", "ndt2d_refine_kernel.h") in build.HEADERS
    assert not [h for h in build.HEADERS if h.endswith(".hip")]
    assert os.path.join(csrc, "refine", "ndt2d_refine_step.h") in build.HEADERS
    # (an object's hash covers its source and every listed header: build._input_sha256)
    assert "HEADERS" in build._input_sha256.__code__.co_names

def test_both_objects_refuse_by_one_text():
    """What ndt2d_refine_run and ndt2d_closure_refine refuse about rules, scans and jobs, and which
    scans a chunk uploads, is batch/ndt2d_refine_jobs.h: plain C++, hashed by the build, used by both
    units, copied by neither."""
    from ndt_2d_amd import build
    csrc = os.path.join(ROOT, "ndt_2d_amd", "csrc")
    path = os.path.join(csrc, "batch", "ndt2d_refine_jobs.h")
    assert path in build.HEADERS
    code = re.sub(r"//[^\n]*", "", open(path).read())
    assert "hip" not in code.lower() and "inline std::string refusal(" in code and "plan_sent_scans(" in code
    assert "inline void copy_sent_scans(" in code
    for unit in ("closure/ndt2d_closure.hip", "refine/ndt2d_refine.hip", "verify/ndt2d_verify.hip"):
        text = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, unit)).read())
        assert '#include "batch/ndt2d_refine_jobs.h"' in text, unit
        assert "refine_jobs::refusal(" in text and "refine_jobs::plan_sent_scans(" in text, unit
        # the copy of the sent scans into the stage is the header's, once per chunk path
        assert text.count("refine_jobs::copy_sent_scans(") == 1 and "2 * (t.beam_offsets[" not in text and \
            "2 * (v.beam_offsets[" not in text, unit
        for copied in ("beam_offsets decrease", "the pose is not finite", "1 << 20", "kNotSent"):
            assert copied not in text, (unit, copied)


def test_the_shared_cases_hold_what_the_gpu_tests_rely_on():
    """closure_refine_cases.case() asserts it: slot grids of at least three sizes and both parities
    in a call, beams in column 0 and in the last row of the designed slot, cells of n < 5 beside
    scoring ones.  Both parities occur at either resolution."""
    for resolution in CC.RESOLUTIONS:
        c = CC.case(resolution)
        assert len(c["slots"]) == 6 and all(len(s["beams"]) <= CC.BEAMS for s in c["slots"])
        assert {n % 2 for n in c["ncells"]} == {0, 1}
        for s in c["slots"][:5]:
            assert np.array_equal(s["starts"][1], CC.graph()["guess"]) and not np.array_equal(s["starts"][0], s["starts"][1])
    assert CC.case(0.25)["ncells"] != CC.case(0.3)["ncells"]


class _Canned:
    """A matcher whose answers are written down: matchCandidates gives the scores of `rounds` in
    turn, refineCandidates moves each start by (1, 2, 3) mm and reports `status`."""

    def __init__(self, rounds, status, rise=False):
        self.rounds, self.status, self.rise = list(rounds), status, rise
        self.match_calls, self.refine_calls = [], []

    def matchCandidates(self, pose, points, batch):
        self.match_calls.append((np.array(pose, dtype=np.float64).copy(), [list(c) for c in batch]))
        scores = self.rounds.pop(0)
        assert len(scores) == len(batch)
        return [dict(score=s, pose=np.array([0.01 * (k + 1), -0.02, 0.005]), covariance=np.eye(3) * (k + 1))
                for k, s in enumerate(scores)]

    def refineCandidates(self, jobs, scans, candidates, job_candidate=None, job_scan=None, **kw):
        jobs = np.array(jobs, dtype=np.float64).reshape(-1, 3)
        self.refine_calls.append(dict(jobs=jobs.copy(), scans=scans, candidates=[list(c) for c in candidates],
                                      job_candidate=job_candidate, job_scan=job_scan, kw=dict(kw)))
        assert len(candidates) == len(jobs) and job_candidate is None and list(job_scan) == [0] * len(jobs)
        return [dict(pose=j + np.array([0.001, 0.002, 0.003]), score=-0.4 if self.rise else -0.6, start_score=-0.5,
                     status=self.status, covariance=np.eye(3) * 1e-6 if self.status == _capi.REFINE_CONVERGED else None)
                for j in jobs]


def _walk(status, refine, rise=False):
    graph_poses = np.arange(30, dtype=np.float64).reshape(10, 3) * 0.1
    points = np.ones((7, 2))
    # round 1: candidates 2, 4, 6, 8 -- 4 and 8 pass, 4 is consumed; round 2: 6, 8 -- 8 passes; done
    m = _Canned([[-0.1, -0.9, -0.2, -0.8], [-0.1, -0.7]], status, rise)
    pose, accepted = close_loops(m, [1.0, 2.0, 0.1], points, [2, 4, 6, 8], graph_poses, 8, -0.5, 4, refine=refine)
    return m, pose, accepted, graph_poses, points


def test_close_loops_refines_the_winners_of_every_round():
    rules = dict(max_evals=16, tol_lin=1e-7, tol_ang=1e-7, neighbourhood=9)
    m, pose, accepted, graph_poses, points = _walk(_capi.REFINE_CONVERGED, rules)
    assert [a["candidate"] for a in accepted] == [4, 8]
    assert len(m.match_calls) == 2 and len(m.refine_calls) == 2          # one refineCandidates per round
    start = np.array([1.0, 2.0, 0.1])
    first, second = m.refine_calls
    # round 1: every candidate that passes (4 and 8: results 1 and 3), each from pose + its correction
    assert first["kw"] == rules and first["scans"][0] is points and len(first["scans"]) == 1
    assert len(first["candidates"]) == 2
    for c, i in zip(first["candidates"], (4, 8)):
        assert [j for j, _ in c] == loop_closure_window(i, 8) and all(np.array_equal(p, graph_poses[j]) for j, p in c)
    assert np.array_equal(first["jobs"], [np.array([0.02, -0.02, 0.005]) + start, np.array([0.04, -0.02, 0.005]) + start])
    a = accepted[0]
    assert np.array_equal(a["pose"], np.array([0.02, -0.02, 0.005]) + start)         # the lattice pose, as before
    assert np.array_equal(a["refined_pose"], a["pose"] + np.array([0.001, 0.002, 0.003]))
    assert a["refine_status"] == _capi.REFINE_CONVERGED and np.array_equal(a["refined_covariance"], np.eye(3) * 1e-6)
    # round 2 starts from the REFINED pose
    assert np.array_equal(m.match_calls[1][0], a["refined_pose"])
    assert [[j for j, _ in c] for c in m.match_calls[1][1]] == [loop_closure_window(6, 8), loop_closure_window(8, 8)]
    assert np.array_equal(second["jobs"], [np.array([0.02, -0.02, 0.005]) + a["refined_pose"]])
    assert np.array_equal(pose, accepted[1]["refined_pose"])
    # MAX_EVALS counts as usable too
    m, pose, accepted, _, _ = _walk(_capi.REFINE_MAX_EVALS, rules)
    assert np.array_equal(m.match_calls[1][0], accepted[0]["refined_pose"]) and accepted[0]["refined_covariance"] is None


def test_close_loops_falls_back_to_the_lattice_pose():
    start = np.array([1.0, 2.0, 0.1])
    for status, rise in ((_capi.REFINE_NOT_FINITE, False), (_capi.REFINE_STALLED, False), (_capi.REFINE_NO_OVERLAP, False),
                         (_capi.REFINE_CONVERGED, True)):
        m, pose, accepted, _, _ = _walk(status, dict(neighbourhood=9), rise)
        a = accepted[0]
        assert a["refine_status"] == status and "refined_pose" in a
        assert np.array_equal(m.match_calls[1][0], np.array([0.02, -0.02, 0.005]) + start)   # the lattice pose
        assert np.array_equal(pose, accepted[1]["pose"])


def test_close_loops_without_refine_is_what_it_was():
    m, pose, accepted, _, _ = _walk(_capi.REFINE_CONVERGED, None)
    assert m.refine_calls == [] and len(m.match_calls) == 2
    start = np.array([1.0, 2.0, 0.1])
    assert [sorted(a) for a in accepted] == [["candidate", "correction", "covariance", "pose", "score"]] * 2
    assert [a["candidate"] for a in accepted] == [4, 8] and [a["score"] for a in accepted] == [-0.9, -0.7]
    p1 = np.array([0.02, -0.02, 0.005]) + start
    p2 = np.array([0.02, -0.02, 0.005]) + p1
    assert np.array_equal(accepted[0]["pose"], p1) and np.array_equal(accepted[1]["pose"], p2) and np.array_equal(pose, p2)
    assert np.array_equal(accepted[0]["covariance"], np.eye(3) * 2) and np.array_equal(accepted[1]["covariance"], np.eye(3) * 2)
    # no candidate passes: nothing is refined either
    m = _Canned([[-0.1, -0.2]], _capi.REFINE_CONVERGED)
    pose, accepted = close_loops(m, start, np.ones((3, 2)), [1, 2], np.zeros((5, 3)), 4, -0.5, 0, refine=dict(neighbourhood=9))
    assert accepted == [] and m.refine_calls == [] and np.array_equal(pose, start)
