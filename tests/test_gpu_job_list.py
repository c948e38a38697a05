"""One (scan, pose) job list through the five batched calls that take one -- matchScans, refineScans,
verifyScans, refineCandidates, verifyCandidates: a job's answer does not depend on who shares the
batch.  Every job's result in the one call is, bit for bit, the result of the same method called
with that job alone.

The list: 5 jobs over scans of 20, 0, 33 and 90 points with laser_max_beams = 40 -- 1, 2 and 2
partial sums, one scan subsampled, one empty --, jobs 0 and 3 on one scan; given once with job_scan
and once as the equivalent list of 5 scans without.  The map is tests/test_gpu_match_scans.py's;
the lattice has 3 theta steps x 3 x 3."""
import numpy as np
import pytest

from ndt_2d_amd import synth
from test_gpu_match_scans import _cut
from test_gpu_match_starts import RANGE_MAX, TRUE_POSE, _matcher, fixture  # noqa: F401

pytestmark = pytest.mark.gpu

PARAMS = dict(search_angular_size=0.025, search_angular_resolution=0.02, search_linear_size=0.025, search_linear_resolution=0.02,
              laser_max_beams=40)
POINTS = [20, 0, 33, 90]
JOB_SCAN = [0, 1, 2, 0, 3]
JOB_CANDIDATE = [0, 1, 0, 1, 1]
JOBS = np.array([(2.21, -1.29, 0.405), (2.2, -1.3, 0.4), (2.18, -1.31, 0.39), (2.23, -1.32, 0.41), (2.19, -1.28, 0.395)])


def _same(a, b):
    """Two result dicts with the same keys and, entry by entry, the same bits."""
    assert sorted(a) == sorted(b)
    for key in a:
        x, y = a[key], b[key]
        if x is None or y is None:
            assert x is None and y is None, key
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), key
        elif isinstance(x, float):
            assert np.float64(x).tobytes() == np.float64(y).tobytes(), key
        else:
            assert type(x) is type(y) and x == y, key


@pytest.fixture(scope="module")
def case(fixture):  # noqa: F811
    """The matcher (the map's scans stored, the NDT in place), the list, two candidate maps of two
    stored scans each, and every job's result alone -- computed once and left unchanged."""
    m = _matcher(fixture, by_id=True, **PARAMS)
    whole = synth.scan(fixture["world"], TRUE_POSE, 9400)
    scans = [_cut(whole, n) if n else np.zeros((0, 2)) for n in POINTS]
    assert [len(s) for s in scans] == POINTS
    near = sorted(range(len(fixture["scans"])), key=lambda i: np.hypot(fixture["scans"][i][0][0] - TRUE_POSE[0],
                                                                       fixture["scans"][i][0][1] - TRUE_POSE[1]))
    candidates = [[(i, fixture["scans"][i][0]) for i in near[0:2]], [(i, fixture["scans"][i][0]) for i in near[2:4]]]
    alone = dict(match=[], refine=[], verify=[], refine_candidates=[], verify_candidates=[])
    for k, sc in enumerate(JOB_SCAN):
        job, scan, cand = [JOBS[k]], [scans[sc]], [candidates[JOB_CANDIDATE[k]]]
        alone["match"] += m.matchScans(job, scan, want_scores=True)
        alone["refine"] += m.refineScans(job, scan)
        alone["verify"] += m.verifyScans(job, scan, want_beams=True)
        alone["refine_candidates"] += m.refineCandidates(job, scan, cand)
        alone["verify_candidates"] += m.verifyCandidates(job, scan, cand, want_beams=True)
    assert m.has_ndt() == 1
    return dict(m=m, scans=scans, candidates=candidates, alone=alone)


@pytest.mark.parametrize("with_job_scan", [True, False])
def test_a_jobs_answer_does_not_depend_on_who_shares_the_batch(case, with_job_scan):
    m, alone = case["m"], case["alone"]
    if with_job_scan:
        scans, job_scan = case["scans"], JOB_SCAN
    else:
        scans, job_scan = [case["scans"][sc] for sc in JOB_SCAN], None
    got = dict(match=m.matchScans(JOBS, scans, job_scan=job_scan, want_scores=True),
               refine=m.refineScans(JOBS, scans, job_scan=job_scan),
               verify=m.verifyScans(JOBS, scans, job_scan=job_scan, want_beams=True),
               refine_candidates=m.refineCandidates(JOBS, scans, case["candidates"], job_candidate=JOB_CANDIDATE, job_scan=job_scan),
               verify_candidates=m.verifyCandidates(JOBS, scans, case["candidates"], job_candidate=JOB_CANDIDATE, job_scan=job_scan,
                                                    want_beams=True))
    assert m.has_ndt() == 1
    for call, results in got.items():
        assert len(results) == len(alone[call]) == 5, call
        for k, (g, a) in enumerate(zip(results, alone[call])):
            print("%s job %d: %s" % (call, k, {key: g[key] for key in ("score", "n_beams", "status") if key in g}))
            _same(g, a)
    # the list is what it is meant to be: 27 lattice candidates; 20, 0, 33, 20 and 40 of 90 beams in use
    assert [r["n_candidates"] for r in got["match"]] == [27] * 5 and all(r["scores"].shape == (27,) for r in got["match"])
    for call in ("verify", "verify_candidates"):
        assert [r["n_beams"] for r in got[call]] == [20, 0, 33, 20, 40], call
        assert [len(r["classes"]) for r in got[call]] == [20, 0, 33, 20, 40], call
    # ... and the jobs beside the truth find the installed map: a winner, and beams the map explains
    for k in (0, 2, 3, 4):
        assert got["match"][k]["score"] < 0.0 and got["refine"][k]["score"] < 0.0 and got["verify"][k]["inlier"] > 0, k
