"""Host side of the batched loop-closure match: the candidate window, the walk of close_loops
(against a stub matcher: no GPU) and the plugin header."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_window(i, rolling):
    """src/ndt_mapper.cpp:628-631, transcribed literally (size_t arithmetic on the cases used)."""
    begin_idx = (i - 1) if (i > 0) else i
    end_idx = (i + 1) if (i < rolling) else i
    return begin_idx, end_idx


def test_loop_closure_window_is_the_reference_window():
    from ndt_2d_amd import loop_closure_window
    rolling = 7
    for i in (0, 1, rolling - 1, rolling):
        b, e = _reference_window(i, rolling)
        assert loop_closure_window(i, rolling) == list(range(b, e)), i
    assert loop_closure_window(0, rolling) == [0]
    assert loop_closure_window(1, rolling) == [0, 1]
    assert loop_closure_window(rolling - 1, rolling) == [rolling - 2, rolling - 1]
    # the quirk: the candidate at the start of the rolling window yields only the scan before it
    assert loop_closure_window(rolling, rolling) == [rolling - 1]


class StubMatcher:
    """matchCandidates with canned results: keyed by (graph index of the candidate, batch number)."""

    def __init__(self, canned):
        self.canned = canned
        self.calls = []

    def matchCandidates(self, scan_pose, points, candidates, want_scores=False):
        self.calls.append((np.array(scan_pose, dtype=np.float64).copy(), [list(c) for c in candidates]))
        batch = len(self.calls) - 1
        out = []
        for cand in candidates:
            centre = cand[-1][0]   # (the windows used here end with the candidate itself)
            score, pose = self.canned[(centre, batch)]
            out.append(dict(score=score, pose=np.array(pose, dtype=np.float64), covariance=np.eye(3) * (centre + 1),
                            n_candidates=0, best_index=0, scores=None))
        return out


def _graph_poses(n):
    return np.array([[0.5 * i, 0.25 * i, 0.01 * i] for i in range(n)])


def test_close_loops_reissues_the_rest_from_the_corrected_pose():
    from ndt_2d_amd import close_loops
    poses = _graph_poses(12)
    rolling = 10
    cands = [2, 5, 7, 9]
    # batch 0: 2 rejected, 5 accepted; batch 1 (from the corrected pose): 7 rejected (NaN), 9 rejected
    canned = {(2, 0): (-0.1, (0.01, 0.0, 0.0)), (5, 0): (-0.9, (0.02, -0.03, 0.004)),
              (7, 0): (-0.95, (9.0, 9.0, 9.0)), (9, 0): (-0.95, (9.0, 9.0, 9.0)),
              (7, 1): (float("nan"), (0.0, 0.0, 0.0)), (9, 1): (-0.2, (0.0, 0.0, 0.0))}
    stub = StubMatcher(canned)
    start = np.array([1.0, 2.0, 0.1])
    pose, accepted = close_loops(stub, start, np.zeros((4, 2)), cands, poses, rolling, -0.5, 10)
    assert len(stub.calls) == 2
    # first batch: every candidate, each with its window and the graph poses, from the scan's pose
    p0, c0 = stub.calls[0]
    assert np.array_equal(p0, start)
    assert [[j for j, _ in c] for c in c0] == [[1, 2], [4, 5], [6, 7], [8, 9]]
    assert all(np.array_equal(pp, poses[j]) for c in c0 for j, pp in c)
    # second batch: only what remained behind the accept, from the corrected pose
    p1, c1 = stub.calls[1]
    corrected = np.array([0.02, -0.03, 0.004]) + start
    assert np.array_equal(p1, corrected)
    assert [[j for j, _ in c] for c in c1] == [[6, 7], [8, 9]]
    assert [a["candidate"] for a in accepted] == [5]
    assert np.array_equal(accepted[0]["pose"], corrected) and np.array_equal(pose, corrected)
    assert np.array_equal(accepted[0]["correction"], [0.02, -0.03, 0.004])
    assert np.array_equal(accepted[0]["covariance"], np.eye(3) * 6)
    # the caller's pose is not written through
    assert np.array_equal(start, [1.0, 2.0, 0.1])


def test_close_loops_limit_counts_as_num_scans_to_check():
    from ndt_2d_amd import close_loops
    poses = _graph_poses(12)
    canned = {(i, b): (-0.1, (0.0, 0.0, 0.0)) for i in range(12) for b in range(3)}
    # limit 2: the first two non-empty candidates; the empty scan 3 is skipped and does not count
    stub = StubMatcher(canned)
    sizes = [90] * 12
    sizes[3] = 0
    pose, accepted = close_loops(stub, [0.0, 0.0, 0.0], np.zeros((4, 2)), [3, 4, 6, 8], poses, 10, -0.5, 2,
                                 scan_sizes=sizes)
    assert accepted == [] and len(stub.calls) == 1
    assert [[j for j, _ in c] for c in stub.calls[0][1]] == [[3, 4], [5, 6]]
    # limit 1 stops after the first; an accept there ends the walk without a second batch
    canned[(4, 0)] = (-0.8, (0.1, 0.0, 0.0))
    stub = StubMatcher(canned)
    pose, accepted = close_loops(stub, [0.0, 0.0, 0.0], np.zeros((4, 2)), [4, 6, 8], poses, 10, -0.5, 1)
    assert [a["candidate"] for a in accepted] == [4] and len(stub.calls) == 1
    assert np.array_equal(pose, [0.1, 0.0, 0.0])
    # limit 0: the reference's unsigned `--num_scans_to_check` never reaches zero -- every candidate
    stub = StubMatcher({(i, b): (-0.1, (0.0, 0.0, 0.0)) for i in range(12) for b in range(3)})
    close_loops(stub, [0.0, 0.0, 0.0], np.zeros((4, 2)), [4, 6, 8], poses, 10, -0.5, 0)
    assert len(stub.calls[0][1]) == 3
    # candidates 0 and `rolling` take their one-scan windows
    stub = StubMatcher({(i, b): (-0.1, (0.0, 0.0, 0.0)) for i in range(12) for b in range(3)})
    close_loops(stub, [0.0, 0.0, 0.0], np.zeros((4, 2)), [0], poses, 10, -0.5, 5)
    assert [[j for j, _ in c] for c in stub.calls[0][1]] == [[0]]
    # no candidates: no call
    stub = StubMatcher({})
    pose, accepted = close_loops(stub, [1.0, 0.0, 0.0], np.zeros((4, 2)), [], poses, 10, -0.5, 5)
    assert stub.calls == [] and accepted == [] and np.array_equal(pose, [1.0, 0.0, 0.0])


def test_loop_closure_hip_header_compiles():
    src = os.path.join(ROOT, "tests", "stubs", "loop_closure_instantiation.cpp")
    done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-I",
                           os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr


def test_closure_symbols_are_bound():
    from ndt_2d_amd import _capi
    for name in ("ndt2d_closure_create", "ndt2d_closure_destroy", "ndt2d_closure_last_error", "ndt2d_closure_match",
                 "ndt2d_matcher_match_candidates"):
        assert name in _capi.SIGNATURES
        assert hasattr(_capi.lib(), name)
