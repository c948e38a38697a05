"""The cases the loop-closure verification's tests share (tests/test_closure_verify_host.py on the
CPU, tests/test_gpu_closure_verify.py on the GPU): over tests/closure_refine_cases.py's six slots
(32 x 32 ... 46 x 41 cells, 100 beams) at both resolutions, every slot under five poses -- its two
starts, starts[0] + 1 m in x, starts[0] + 0.3 rad and starts[0] + (-1.5, 1.0, 2.0) -- with the
restatement's answer (tests/verify_restatement.py over the oracle's build of the candidate) for the
neighbourhoods 1 and 9 at the gates 9.0 / 1.0.  Computed once, left unchanged."""
import numpy as np

import closure_refine_cases as CC
import verify_restatement as V

GATE_INLIER, GATE_PIERCE = 9.0, 1.0
NEIGHBOURHOODS = (1, 9)
DISPLACEMENTS = (None, None, (1.0, 0.0, 0.0), (0.0, 0.0, 0.3), (-1.5, 1.0, 2.0))
DISPLACED = (2, 3, 4)            # the poses away from the match

_JOBS = {}
_RESTATED = {}


def poses_of(slot):
    """The five poses of a slot."""
    s0, s1 = slot["starts"]
    return [s0.copy(), s1.copy()] + [s0 + np.array(d) for d in DISPLACEMENTS[2:]]


def jobs(resolution):
    """(jobs[30, 3], scans, candidates, job_candidate, job_scan): slot after slot, pose after pose;
    scan 0 is the graph's query, scan 1 the designed one (closure_refine_cases)."""
    if resolution not in _JOBS:
        c = CC.case(resolution)
        xyt, jc, js = [], [], []
        for k, s in enumerate(c["slots"]):
            for p in poses_of(s):
                xyt.append(p)
                jc.append(k)
                js.append(1 if k == len(c["slots"]) - 1 else 0)
        _JOBS[resolution] = (np.array(xyt), [c["slots"][0]["query"], c["slots"][-1]["query"]],
                             [s["candidate"] for s in c["slots"]], jc, js)
    return _JOBS[resolution]


def restated(resolution, cells):
    """The restatement's results of the 30 jobs, in jobs()' order."""
    key = (resolution, cells)
    if key not in _RESTATED:
        c = CC.case(resolution)
        xyt, _, _, jc, _ = jobs(resolution)
        _RESTATED[key] = [V.verify(c["slots"][k]["grid"], c["slots"][k]["beams"], p, neighbourhood=cells, gate_inlier=GATE_INLIER,
                                   gate_pierce=GATE_PIERCE) for p, k in zip(xyt, jc)]
    return _RESTATED[key]
