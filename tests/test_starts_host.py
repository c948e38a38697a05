"""Host side of the batched match from K start poses (csrc/starts/): the symbols, the plugin
header, relocalize() / heading_fan() against a stub matcher, the C entry points' refusals that
need no device, and the chunk plan the batched searches share.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_INDEX = 2 ** 64 - 1
NEW_SYMBOLS = ("ndt2d_grid_view_get", "ndt2d_starts_create", "ndt2d_starts_destroy", "ndt2d_starts_last_error",
               "ndt2d_starts_match", "ndt2d_starts_set_timing", "ndt2d_starts_last_ms",
               "ndt2d_matcher_match_starts", "ndt2d_matcher_starts")


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
    assert "ndt2d_grid_view" in text and _capi.lib().ndt2d_abi_version() == 4


def test_relocalize_hip_header_compiles():
    src = os.path.join(ROOT, "tests", "stubs", "relocalize_instantiation.cpp")
    done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "stubs"), src],
                          capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr
    cmake = open(os.path.join(ROOT, "ndt_2d_amd", "plugin", "CMakeLists.txt")).read()
    assert "relocalize_hip.hpp" in cmake


def test_shared_chunk_plan_gives_the_closure_plans_values(tmp_path):
    exe = os.path.join(str(tmp_path), "sum_chunks_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "ndt_2d_amd", "csrc", "batch"),
                           os.path.join(ROOT, "tests", "cpp", "sum_chunks_check.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    for beams, chunks in ((1, 1), (4, 1), (5, 1), (100, 5), (720, 8), (1500, 8)):
        assert "beams %d: chunks %d (expected %d)" % (beams, chunks, chunks) in done.stdout
    # the three batched searches take the plan, the walk, the kernels, the launch switch and the host
    # scaffolding from csrc/batch/; none keeps a copy of any of it
    csrc = os.path.join(ROOT, "ndt_2d_amd", "csrc")
    shared = "".join(open(os.path.join(csrc, "batch", name)).read() for name in
                     ("ndt2d_walk_fn.h", "ndt2d_sum_chunks.h", "ndt2d_installed_map.h", "ndt2d_batch_search.h", "ndt2d_batch_state.h",
                      "ndt2d_batch_host.h"))
    for once in ("uint32_t sum_chunks(", "void add_beam(", "void lane_take(", "void block_record(", "batch_search_kernel(",
                 "batch_reduce_kernel(", "switch (chunks)", "struct InstalledMap", "hipHostMalloc(", "hipEventCreate("):
        assert shared.count(once) == 1, once
    for unit in ("closure/ndt2d_closure.hip", "starts/ndt2d_starts.hip", "scans/ndt2d_scans.hip"):
        text = open(os.path.join(csrc, unit)).read()
        code = re.sub(r"//[^\n]*", "", text)
        assert '#include "batch/ndt2d_batch_search.h"\n' in text, unit
        assert "uint32_t sum_chunks" not in code and "void add_beam" not in code, unit
        for copied in ("lane_take(", "block_record<", "hipHostMalloc", "hipEventCreate", "switch (chunks)",
                       "struct InstalledMap"):
            assert copied not in code, (unit, copied)
        # no kernel of its own, save the loop closure's build
        own = code.count("__global__")
        assert own == (1 if unit.startswith("closure") else 0) and ("closure_build_kernel(" in code) == (own == 1), unit
    # the start poses run as jobs of the scan tracking's engine
    starts = open(os.path.join(csrc, "starts", "ndt2d_starts.hip")).read()
    assert "match_jobs(" in starts and "hipLaunchKernelGGL" not in starts and "hipMemcpyAsync" not in starts
    from ndt_2d_amd import build
    for name in os.listdir(os.path.join(csrc, "batch")):
        assert os.path.join(csrc, "batch", name) in build.HEADERS, name


def test_entry_points_refuse_null_arguments_without_a_device():
    from ndt_2d_amd import _capi
    L = _capi.lib()
    out = C.c_void_p(0x1)
    assert L.ndt2d_starts_create(None, 4, C.byref(out)) == _capi.ERR_INVALID and not out.value
    assert L.ndt2d_starts_create(None, 4, None) == _capi.ERR_INVALID
    assert L.ndt2d_starts_destroy(None) == _capi.ERR_INVALID
    assert L.ndt2d_starts_last_error(None) == b"null starts"
    assert L.ndt2d_starts_set_timing(None, 1) == _capi.ERR_INVALID
    assert L.ndt2d_starts_last_ms(None, None, None) == _capi.ERR_INVALID
    z = np.zeros(12)
    assert L.ndt2d_starts_match(None, _capi.dptr(z), 1, _capi.dptr(z), 1, _capi.dptr(z), 1, _capi.dptr(z), 1,
                                _capi.dptr(z), None) == _capi.ERR_INVALID
    assert L.ndt2d_matcher_match_starts(None, _capi.dptr(z), 1, _capi.dptr(z), 1, None, None, _capi.dptr(z), None,
                                        None, 0, None) == _capi.ERR_INVALID
    assert not L.ndt2d_matcher_starts(None)
    assert L.ndt2d_grid_view_get(None, None) == _capi.ERR_INVALID


class StubMatcher:
    """matchStarts with canned (score, correction, best_index) per start."""

    def __init__(self, canned):
        self.canned = canned
        self.calls = []

    def matchStarts(self, start_poses, points, want_scores=False):
        self.calls.append(np.array(start_poses, dtype=np.float64).copy())
        assert len(start_poses) == len(self.canned)
        return [dict(score=s, pose=np.array(p, dtype=np.float64), covariance=np.eye(3) * (k + 1), n_candidates=245,
                     best_index=b, scores=None) for k, (s, p, b) in enumerate(self.canned)]


def test_relocalize_ranks_by_score_with_ties_in_start_order():
    from ndt_2d_amd import relocalize
    nan = float("nan")
    canned = [(-0.10, (0.01, 0.0, 0.0), 7),        # 0
              (-0.30, (0.02, -0.03, 0.004), 9),    # 1: tie with 3, first in start order
              (nan, (0.0, 0.0, 0.0), 3),           # 2: not finite -> last
              (-0.30, (0.05, 0.0, 0.0), 11),       # 3
              (0.0, (0.0, 0.0, 0.0), NO_INDEX),    # 4: no winner -> behind every start with one
              (-0.001, (0.0, 0.02, 0.0), 1),       # 5
              (float("-inf"), (0.0, 0.0, 0.0), 2)]  # 6: not finite either, behind 2 (start order)
    starts = np.array([[1.0 * k, 2.0 * k, 0.1 * k] for k in range(len(canned))])
    stub = StubMatcher(canned)
    ranked = relocalize(stub, np.zeros((4, 2)), starts)
    assert len(stub.calls) == 1 and np.array_equal(stub.calls[0], starts)     # one batched call
    assert [r["start"] for r in ranked] == [1, 3, 0, 5, 4, 2, 6]
    first = ranked[0]
    assert first["score"] == -0.30 and np.array_equal(first["correction"], [0.02, -0.03, 0.004])
    # pose = start + correction, as src/ndt_mapper.cpp:557-561 adds it
    assert np.array_equal(first["pose"], np.array([0.02, -0.03, 0.004]) + starts[1])
    assert np.array_equal(first["covariance"], np.eye(3) * 2)
    no_winner = ranked[4]
    assert no_winner["score"] == 0.0 and np.array_equal(no_winner["pose"], starts[4])
    # the caller's poses are not written through
    assert np.array_equal(starts[1], [1.0, 2.0, 0.1])


def test_relocalize_accept_below_is_the_loop_closure_rule():
    from ndt_2d_amd import relocalize
    canned = [(-0.10, (0.0, 0.0, 0.0), 7), (-0.30, (0.0, 0.0, 0.0), 9), (float("nan"), (0.0, 0.0, 0.0), 3),
              (-0.2, (0.0, 0.0, 0.0), 4), (float("-inf"), (0.0, 0.0, 0.0), 2), (-0.25, (0.0, 0.0, 0.0), 5)]
    starts = np.zeros((len(canned), 3))
    ranked = relocalize(StubMatcher(canned), np.zeros((4, 2)), starts, accept_below=-0.2)
    # isfinite(score) && score < threshold: -0.2 itself, NaN and -inf are out
    assert [r["start"] for r in ranked] == [1, 5]
    assert relocalize(StubMatcher(canned), np.zeros((4, 2)), starts, accept_below=-1.0) == []


def test_relocalize_without_starts_makes_no_call():
    from ndt_2d_amd import relocalize
    stub = StubMatcher([])
    assert relocalize(stub, np.zeros((4, 2)), np.zeros((0, 3))) == [] and stub.calls == []
    assert relocalize(stub, np.zeros((4, 2)), []) == [] and stub.calls == []


def test_heading_fan():
    from ndt_2d_amd import heading_fan
    poses = np.array([[1.0, 2.0, 0.25], [-3.0, 0.5, -1.0]])
    fan = heading_fan(poses, 4)
    assert fan.shape == (8, 3)
    for k in range(2):
        for j in range(4):
            row = fan[4 * k + j]
            assert row[0] == poses[k, 0] and row[1] == poses[k, 1]
            assert row[2] == poses[k, 2] + j * (2.0 * np.pi / 4)
    assert np.array_equal(heading_fan(poses, 1), poses)          # the pose's own heading first
    assert heading_fan(np.zeros((0, 3)), 3).shape == (0, 3)
    assert heading_fan([0.0, 0.0, 0.5], 2).shape == (2, 3)       # a single pose
    assert np.array_equal(poses[:, 2], [0.25, -1.0])              # not written through
    with pytest.raises(ValueError):
        heading_fan(poses, 0)
