"""The cases the Newton registration's tests share (tests/test_refine_host.py on the CPU,
tests/test_gpu_refine.py on the GPU): six start poses within 10 cm of the pose the 720-beam query
of tests/test_gpu_match_starts.py's fixture was taken at, the CPU oracle per (resolution, beams)
with the restatement's grid and subsampled beams, and the twelve jobs of the path test -- the six
starts and the oracle's lattice winners from them.  Computed once, left unchanged."""
import numpy as np

import oracle_lib as O
import refine_restatement as R
from test_gpu_match_starts import RANGE_MAX, SMALL, TRUE_POSE

# offsets of 2 .. 7 cm and 0.01 .. 0.03 rad from TRUE_POSE = (2.2, -1.3, 0.4), one per octant or so
NEAR6 = np.array([(2.18, -1.27, 0.41), (2.2, -1.3, 0.4), (2.25, -1.35, 0.37), (2.16, -1.33, 0.42),
                  (2.23, -1.26, 0.385), (2.21, -1.34, 0.415)])
assert all(np.hypot(p[0] - TRUE_POSE[0], p[1] - TRUE_POSE[1]) < 0.1 for p in NEAR6)

_CASES = {}


def case(fixture, resolution, beams=100):
    """dict(ref = the oracle's matcher with the fixture's map, grid, beams = the query as
    scorePoints subsamples it, n, winners[6] = start + the oracle's matchScan correction,
    jobs[12] = NEAR6 then the winners)."""
    key = (resolution, beams)
    if key not in _CASES:
        ref = O.ScanMatcherNDT()
        ref.initialize(**dict(SMALL, ndt_resolution=resolution, range_max=RANGE_MAX, laser_max_beams=beams))
        ref.addScans(fixture["scans"])
        sub = R.subsample(fixture["query"], beams)
        winners = []
        for s in NEAR6:
            got = ref.matchScan(s, fixture["query"])
            assert got["best_index"] != O.UINT64_MAX
            winners.append(s + got["pose"])
        winners = np.array(winners)
        _CASES[key] = dict(ref=ref, grid=R.Grid.of_oracle(ref), beams=sub, n=len(sub), winners=winners,
                           jobs=np.vstack([NEAR6, winners]))
    return _CASES[key]
