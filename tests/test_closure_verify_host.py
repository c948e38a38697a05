"""Host side of the match verification on each loop-closure candidate's own map
(ndt2d_closure_verify, ndt2d_matcher_verify_candidates, ScanMatcherNDT.verifyCandidates,
close_loops(verify=...)): the symbols, the refusals that need no device, the plugin's members, the
shape of the units, the chunk plan under the sanitizers, the shared cases' own assertions on the
restatement, and close_loops' walk on a canned matcher.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import closure_refine_cases as CC
import closure_verify_cases as VC
import verify_restatement as V
from ndt_2d_amd import _capi, close_loops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ndt_2d_amd", "csrc")
NEW_SYMBOLS = ("ndt2d_closure_verify", "ndt2d_closure_set_verify_neighbourhood", "ndt2d_closure_verify_neighbourhood",
               "ndt2d_closure_set_verify_gates", "ndt2d_closure_verify_gates", "ndt2d_closure_set_verify_rays",
               "ndt2d_closure_verify_rays", "ndt2d_matcher_verify_candidates")


def _code(*parts):
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, *parts)).read())


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
    assert _capi.lib().ndt2d_abi_version() == 4                    # additions only
    # the contract is in the header
    for phrase in ("Match verification on each loop-closure candidate's own map", "no installed grid is no error here",
                   "on the grid ndt2d_scanstore_build installs for that\n *                candidate",
                   "a job depends on nothing but its scan, its pose, its candidate", "per-beam results pass 2^24",
                   "the build and the verify launch of its last chunk", "no NDT in place is no error"):
        assert phrase in raw, phrase


def test_null_arguments_are_refused_without_a_device():
    L = _capi.lib()
    z3 = np.zeros(3)
    rec = np.full(8, 7, dtype=np.uint32)
    recp = rec.ctypes.data_as(C.POINTER(C.c_uint32))
    off = np.array([0, 1], dtype=np.uintp)
    ids = np.zeros(1, dtype=np.uintp)
    szp = lambda a: a.ctypes.data_as(C.POINTER(C.c_size_t))   # noqa: E731
    out = C.c_uint32(77)
    for cells in (0, 5, 1, 9):
        assert L.ndt2d_closure_set_verify_neighbourhood(None, cells) == _capi.ERR_INVALID
    assert L.ndt2d_closure_verify_neighbourhood(None, C.byref(out)) == _capi.ERR_INVALID and out.value == 77
    assert L.ndt2d_closure_set_verify_gates(None, 9.0, 1.0) == _capi.ERR_INVALID
    assert L.ndt2d_closure_verify_gates(None, None, None) == _capi.ERR_INVALID
    assert L.ndt2d_closure_set_verify_rays(None, 1) == _capi.ERR_INVALID
    assert L.ndt2d_closure_verify_rays(None, None) == _capi.ERR_INVALID
    # a null object, whatever else is given -- jobs or none
    for n_jobs in (0, 1):
        assert L.ndt2d_closure_verify(None, 1, szp(off), szp(ids), _capi.dptr(z3), 0.25, 4.75, _capi.dptr(z3), None, None, n_jobs,
                                      _capi.dptr(z3), szp(off), 1, recp, None, None, None) == _capi.ERR_INVALID
        assert L.ndt2d_matcher_verify_candidates(None, szp(off), szp(ids), _capi.dptr(z3), 1, _capi.dptr(z3), None, None, n_jobs,
                                                 _capi.dptr(z3), szp(off), 1, 0, recp, None, None, None, None, 0) == _capi.ERR_INVALID
    assert np.all(rec == 7)


def test_plugin_members_compile():
    for stub in ("closure_verify_instantiation.cpp", "closure_refine_instantiation.cpp", "loop_closure_instantiation.cpp"):
        done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I",
                               os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "stubs"),
                               os.path.join(ROOT, "tests", "stubs", stub)], capture_output=True, text=True)
        assert done.returncode == 0 and not done.stderr, done.stderr
    text = open(os.path.join(ROOT, "ndt_2d_amd", "plugin", "loop_closure_hip.hpp")).read()
    for member in ("bool setVerify(", "void clearVerify()", "ndt2d_matcher_verify_candidates(", "double verified_pose[3]",
                   "std::uint32_t verify[NDT2D_VERIFY_RECORD_U32]"):
        assert member in text, member
    assert "Eigen" not in re.sub(r"//[^\n]*", "", text) and "rclcpp" not in text


def test_one_kernel_text_for_both_map_sources():
    """The closure instantiates the verification's kernel from csrc/verify/ndt2d_verify_kernel.h,
    the header the installed grid's unit includes too -- it holds no copy of the evaluation or of the
    ray walk -- reads nothing of the installed grid in its source, refuses by the shared text, runs
    its chunks through the one path it shares with the refinement, and nothing new sits at the top
    level of csrc/."""
    closure, verify = _code("closure", "ndt2d_closure.hip"), _code("verify", "ndt2d_verify.hip")
    kernel = _code("verify", "ndt2d_verify_kernel.h")
    assert '#include "verify/ndt2d_verify_kernel.h"\n' in closure and '#include "verify/ndt2d_verify_kernel.h"\n' in verify
    assert "verify_kernel<true, CELLS, SlotSource>" in closure and "verify_kernel<false, CELLS, SlotSource>" in closure
    for absent in ("record_exponent(", "record_m2(", "verify::line_begin(", "verify::line_next(", "verify::approach(",
                   "verify::pierces(", "__builtin_amdgcn_ballot_w64(", "atomic", "__threadfence"):
        assert absent not in closure, absent
    assert "a.source.grid(jr.slot)" in kernel and "a.source.map(jr.slot)" in kernel
    # the kernel in the header; the object, the entry points and the launches in the unit; the
    # installed grid's source in neither
    assert "verify_kernel(const VerifyArgs<SOURCE> a)" in kernel and "verify_kernel(const VerifyArgs<SOURCE> a)" not in verify
    for host_side in ("struct ndt2d_verify", 'extern "C"', "hipLaunchKernelGGL"):
        assert host_side in verify and host_side not in kernel, host_side
    assert "struct InstalledSource" not in verify and "struct InstalledSource" not in kernel
    # one __global__ of either name in the tree, neither macro anywhere, no .hip included
    count = {"refine_kernel": 0, "verify_kernel": 0}
    for base, _, names in os.walk(CSRC):
        for n in names:
            if n.endswith((".hip", ".h", ".cpp")):
                raw = open(os.path.join(base, n)).read()
                for name in count:
                    count[name] += len(re.findall(r"__global__[^;{]*\b%s\b" % name, _code(base, n)))
                assert "NDT2D_VERIFY_KERNEL_ONLY" not in raw and "NDT2D_REFINE_KERNEL_ONLY" not in raw, n
                assert not re.search(r'#\s*include\s*["<][^">]*\.hip[">]', raw), n
    assert count == {"refine_kernel": 1, "verify_kernel": 1}
    # one closure_build_kernel, launched by one launch_build, which the one path of a chunk calls:
    # there the upload, the read-back and the wait; none in what the verification adds to it
    assert closure.count("__global__") == 1 and closure.count("hipLaunchKernelGGL(ndt2d::closure_build_kernel") == 1
    shared = closure[closure.index("int job_chunk("):closure.index("struct RefineCall")]
    assert "launch_build(" in shared and shared.count("hipMemcpyAsync") == 2 and shared.count("hipStreamSynchronize") == 1
    assert "place_chunk_slots(" in shared and "fill_scan_table(" in shared and "refine_jobs::copy_sent_scans(" in shared
    per_path = closure[closure.index("struct RefineCall"):closure.index("int check_job_call(")]
    assert "int refine_chunk(" in per_path and "int verify_chunk(" in per_path and per_path.count("job_chunk(") == 2
    for absent in ("hipMemcpyAsync", "hipStreamSynchronize", "hipEventRecord", "launch_build(", "grow_pair(", "grow_device("):
        assert absent not in per_path, absent
    # the slots' offsets and the scan table exist once, for the match too
    assert closure.count("s.lookup_off = ") == 1 and closure.count("sc.pool_offset = ") == 1 and closure.count("slot_extent(") == 1
    assert closure.count("grow_device(&c->d_lookup") == 1 and "int match_chunk(" in closure
    match = closure[closure.index("int match_chunk("):closure.index("struct ChunkOnDevice")]
    assert "place_chunk_slots(" in match and "fill_scan_table(" in match
    source = closure[closure.index("struct SlotSource"):closure.index("using SlotRefineArgs")]
    assert "occ_bits" not in source and "cells_global" not in source and "installed_grid(" not in closure
    # what it refuses about jobs and scans is the shared text, through the check both entries share;
    # the chunks are the plan's
    entry = closure[closure.index("int ndt2d_closure_verify("):]
    assert 'check_job_call(c, "ndt2d_closure_verify"' in entry and "plan_closure_jobs(" in entry
    assert 'check_job_call(c, "ndt2d_closure_refine"' in closure
    check = closure[closure.index("int check_job_call("):closure.index('extern "C"')]
    assert "refine_jobs::refusal(entry" in check and "check_candidates(c, entry" in check
    assert check.index("null argument") < check.index("bad resolution or range_max") < check.index("bad argument (n_candidates)") \
        < check.index("no job_candidate") < check.index("refine_jobs::refusal(") < check.index("check_candidates(") \
        < check.index('": candidate "')
    for copied in ("beam_offsets decrease", "the pose is not finite", "1 << 20", "kNotSent"):
        assert copied not in closure, copied
    # the settings and what they refuse are the header's, held once by either object
    assert "ndt2d::VerifySettings verify;" in closure and "ndt2d::VerifySettings set;" in verify
    for copied in ("cells (1 or 9)\"", "a gate is negative", "(0 or 1)"):
        assert copied not in verify and closure.count(copied) == (1 if copied.startswith("cells") else 0), copied
    # the kernel's header is hashed with the headers: an edit to the kernel makes the closure's object stale too
    from ndt_2d_amd import build
    assert os.path.join(CSRC, "verify", "ndt2d_verify_kernel.h") in build.HEADERS and "verify/ndt2d_verify.hip" in build.SOURCES
    assert not [h for h in build.HEADERS if h.endswith(".hip")]
    top = sorted(n for n in os.listdir(CSRC) if os.path.isfile(os.path.join(CSRC, n)))
    assert not [n for n in top if "verify" in n or "closure" in n]


def test_chunk_plan_under_the_sanitizers(tmp_path):
    """tests/cpp/closure_verify_jobs_check.cpp: a program of its own over the plain-C++ header, built
    with the host compiler and -fsanitize=address,undefined (the sanitizer's runtime linked into the
    program), run directly: candidates ascending among those named, unnamed ones not built, the 2^24
    beam cap, a candidate heavier than a chunk and one with 4,097 jobs, a job heavier than the cap,
    records in job order, and the refinement's plan unchanged for the same inputs."""
    exe = os.path.join(str(tmp_path), "closure_verify_jobs_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-I", os.path.join(CSRC, "closure"),
                           os.path.join(ROOT, "tests", "cpp", "closure_verify_jobs_check.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip() == "OK" and not done.stderr, done.stdout + done.stderr
    code = _code("closure", "ndt2d_closure_jobs.h")
    assert "hip" not in code.lower() and "__device__" not in code


def test_the_cases_hold_what_the_gpu_tests_rely_on():
    """All 120 combinations (2 resolutions x 6 slots x 5 poses x 2 neighbourhoods): no m2 or tested
    r^T I r within 1e-8 (relative) of its gate, no NaN m2; every class occurs, and pierced beams
    occur at each of the three displaced poses.  The counts are printed."""
    seen = set()
    pierced_at = {p: 0 for p in VC.DISPLACED}
    n = 0
    for resolution in CC.RESOLUTIONS:
        xyt, scans, cands, jc, js = VC.jobs(resolution)
        assert len(xyt) == 30 and len(cands) == 6 and len(scans) == 2
        for cells in VC.NEIGHBOURHOODS:
            for k, res in enumerate(VC.restated(resolution, cells)):
                assert V.near_gate(res, VC.GATE_INLIER, VC.GATE_PIERCE, rel=1e-8) == [], (resolution, cells, k)
                assert not np.isnan(res["m2"]).any(), (resolution, cells, k)
                r = [int(v) for v in res["record"]]
                assert r[0] == CC.BEAMS and sum(r[1:5]) == r[0] and r[5] <= r[6] <= r[0]
                print("res %.2f cells %d slot %d pose %d: record %s" % (resolution, cells, jc[k], k % 5, r))
                seen.update(int(c) for c in np.unique(res["classes"]))
                if k % 5 in pierced_at:
                    pierced_at[k % 5] += r[5]
                n += 1
    assert n == 120 and seen == {V.OFF, V.UNSEEN, V.OUTLIER, V.INLIER}
    assert all(v > 0 for v in pierced_at.values()), pierced_at
    # slot 0 at 0.25, + 1 m in x, nine cells: 22 beams off the grid, 41 unseen, 5 pierced
    r = VC.restated(0.25, 9)[2]["record"]
    assert (int(r[1]), int(r[2]), int(r[5])) == (22, 41, 5)


class _Canned:
    """A matcher whose answers are written down (tests/test_closure_refine_host.py's), with a
    verifyCandidates that records what it is asked."""

    def __init__(self, rounds, status, rise=False):
        self.rounds, self.status, self.rise = list(rounds), status, rise
        self.match_calls, self.refine_calls, self.verify_calls = [], [], []

    def matchCandidates(self, pose, points, batch):
        self.match_calls.append((np.array(pose, dtype=np.float64).copy(), [list(c) for c in batch]))
        scores = self.rounds.pop(0)
        return [dict(score=s, pose=np.array([0.01 * (k + 1), -0.02, 0.005]), covariance=np.eye(3) * (k + 1))
                for k, s in enumerate(scores)]

    def refineCandidates(self, jobs, scans, candidates, job_candidate=None, job_scan=None, **kw):
        jobs = np.array(jobs, dtype=np.float64).reshape(-1, 3)
        self.refine_calls.append(jobs.copy())
        return [dict(pose=j + np.array([0.001, 0.002, 0.003]), score=-0.4 if self.rise else -0.6, start_score=-0.5,
                     status=self.status, covariance=None) for j in jobs]

    def verifyCandidates(self, jobs, scans, candidates, job_candidate=None, job_scan=None, **kw):
        jobs = np.array(jobs, dtype=np.float64).reshape(-1, 3)
        self.verify_calls.append(dict(jobs=jobs.copy(), scans=scans, candidates=[list(c) for c in candidates],
                                      job_candidate=job_candidate, job_scan=list(job_scan), kw=dict(kw)))
        return [dict(n_beams=10, off=0, unseen=1, outlier=2, inlier=7, pierced=k, walked=10) for k in range(len(jobs))]


def _walk(status, refine, verify, rise=False):
    graph_poses = np.arange(30, dtype=np.float64).reshape(10, 3) * 0.1
    points = np.ones((7, 2))
    # round 1: candidates 2, 4, 6, 8 -- 4 and 8 pass, 4 is consumed; round 2: 6, 8 -- 8 passes; done
    m = _Canned([[-0.1, -0.9, -0.2, -0.8], [-0.1, -0.7]], status, rise)
    pose, accepted = close_loops(m, [1.0, 2.0, 0.1], points, [2, 4, 6, 8], graph_poses, 8, -0.5, 4, refine=refine, verify=verify)
    return m, pose, accepted, points


def test_close_loops_verifies_the_passing_candidates_of_every_round_and_changes_nothing():
    rules = dict(max_beams=0, gate_pierce=0.5)
    for refine, status, rise in ((None, _capi.REFINE_CONVERGED, False), (dict(neighbourhood=9), _capi.REFINE_CONVERGED, False),
                                 (dict(neighbourhood=9), _capi.REFINE_MAX_EVALS, False), (dict(neighbourhood=9), _capi.REFINE_STALLED, False),
                                 (dict(neighbourhood=9), _capi.REFINE_CONVERGED, True)):
        plain_m, plain_pose, plain, _ = _walk(status, refine, None, rise)
        m, pose, accepted, points = _walk(status, refine, rules, rise)
        assert plain_m.verify_calls == [] and len(m.verify_calls) == len(m.match_calls) == 2      # ONE call per round
        # the walk, the accepted entries and the returned pose are what they are without verify
        assert np.array_equal(pose, plain_pose) and len(accepted) == len(plain) == 2
        for a, b in zip(m.match_calls, plain_m.match_calls):
            assert np.array_equal(a[0], b[0]) and [[j for j, _ in c] for c in a[1]] == [[j for j, _ in c] for c in b[1]]
        for a, p in zip(accepted, plain):
            assert sorted(a) == sorted(list(p) + ["verify", "verified_pose"])
            for key in p:
                assert np.array_equal(a[key], p[key]) if p[key] is not None else a[key] is None, key
        # round 1 verifies both passing candidates (4 and 8), round 2 the one; all on the one scan
        first, second = m.verify_calls
        assert first["kw"] == rules and first["scans"][0] is points and len(first["scans"]) == 1
        assert len(first["candidates"]) == 2 and first["job_scan"] == [0, 0] and first["job_candidate"] is None
        assert len(second["candidates"]) == 1 and second["job_scan"] == [0]
        usable = refine is not None and status in (_capi.REFINE_CONVERGED, _capi.REFINE_MAX_EVALS) and not rise
        for call, a, start in ((first, accepted[0], np.array([1.0, 2.0, 0.1])), (second, accepted[1], m.match_calls[1][0])):
            # each at the pose the walk would adopt for it: the refined pose where usable, else the lattice pose
            lattice = [np.array([0.01 * (k + 1), -0.02, 0.005]) + start for k in ((1, 3) if call is first else (1,))]
            want = [p + np.array([0.001, 0.002, 0.003]) for p in lattice] if usable else lattice
            assert np.array_equal(call["jobs"], want)
            assert np.array_equal(a["verified_pose"], want[0]) and a["verify"]["pierced"] == 0 and a["verify"]["inlier"] == 7
            assert np.array_equal(a["verified_pose"], a["refined_pose"] if usable else a["pose"])
    # no candidate passes: nothing is verified
    m = _Canned([[-0.1, -0.2]], _capi.REFINE_CONVERGED)
    pose, accepted = close_loops(m, [0.0, 0.0, 0.0], np.ones((3, 2)), [1, 2], np.zeros((5, 3)), 4, -0.5, 0, verify={})
    assert accepted == [] and m.verify_calls == []
