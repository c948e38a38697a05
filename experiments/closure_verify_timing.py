"""Match verification on the loop closure's candidate maps (ScanMatcherNDT.verifyCandidates) against
the per-candidate sequence on the same tree -- reset(), addScansById(candidate), verifyScans([job])
per candidate -- and the verify launch on a slot against the same job's launch on the installed grid.

    python experiments/closure_verify_timing.py [OUT.json]

Rows: K = 1, 8, 16 candidates (one job each) x 100 / 720 beams in use x rays on / off, neighbourhood
9, per-beam outputs not wanted.  The graph, the query and the candidates are
tests/closure_refine_cases.py's (ten scans of 90 to 720 points; candidates of one or two scans,
39 x 39 cells at 0.25 m); job k's pose is the scan's guess displaced by up to 0.8 m and 0.3 rad, so
that the rows hold right and wrong poses alike.  Per row the median of REPS calls after WARM_UPS in
one process, with minimum and maximum: the call's wall time, the sequence's wall time, the build
and the verify launch of the call (ndt2d_closure_last_ms), and the sequence's K kernel launches
(ndt2d_verify_last_ms, summed).  A run without a GPU fails; nothing falls back."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KS = (1, 8, 16)
BEAMS = (100, 720)
WARM_UPS, REPS = 5, 20


def spread(values):
    return dict(median=float(np.median(values)), min=float(min(values)), max=float(max(values)))


def main():
    import closure_refine_cases as CC
    from ndt_2d_amd import ScanMatcherNDT
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "closure_verify_timing.json")
    g = CC.graph()
    cands = [[(i, g["poses"][i])] for i in range(10)] + [[(i, g["poses"][i]), (i + 1, g["poses"][i + 1])] for i in range(6)]
    jobs = np.array([g["guess"] + (0.05 * k, -0.03 * k, 0.02 * k) for k in range(16)])
    query = g["query"]
    rows = []
    for beams in BEAMS:
        m = ScanMatcherNDT(0)
        m.initialize("closure-verify-timing", **dict(CC.SMALL, ndt_resolution=0.25, range_max=CC.RANGE_MAX, laser_max_beams=beams))
        for i, pts in enumerate(g["points"]):
            assert m.storeScan(pts) == i
        for K in KS:
            for rays in (True, False):
                def call():
                    return m.verifyCandidates(jobs[:K], [query], cands[:K], job_scan=[0] * K, rays=rays)

                def sequence(kernel=None):
                    out = []
                    for k in range(K):
                        m.reset()
                        m.addScansById([p for _, p in cands[k]], [i for i, _ in cands[k]])
                        out.append(m.verifyScans([jobs[k]], [query], rays=rays)[0])
                        if kernel is not None:
                            kernel.append(m.verify_last_ms()[0])
                    return out

                counts = call()
                assert counts == sequence()                     # the same verdicts, before anything is timed
                m.reset()
                m.closure_set_timing(True)
                m.verify_set_timing(True)
                for _ in range(WARM_UPS):
                    call()
                    sequence()
                wall, seq_wall, build, launch, seq_kernel = [], [], [], [], []
                for _ in range(REPS):                           # alternating, in one process
                    t0 = time.perf_counter()
                    call()
                    wall.append(1e3 * (time.perf_counter() - t0))
                    a, b = m.closure_last_ms()
                    build.append(a)
                    launch.append(b)
                    kernel = []
                    t0 = time.perf_counter()
                    sequence(kernel)
                    seq_wall.append(1e3 * (time.perf_counter() - t0))
                    seq_kernel.append(sum(kernel))
                m.closure_set_timing(False)
                m.verify_set_timing(False)
                m.reset()
                n_all = sum(c["n_beams"] for c in counts)
                rows.append(dict(candidates=K, beams=beams, rays=rays, neighbourhood=9, call_wall_ms=spread(wall),
                                 sequence_wall_ms=spread(seq_wall), build_ms=spread(build), verify_launch_ms=spread(launch),
                                 sequence_kernels_ms=spread(seq_kernel), beams_all=int(n_all),
                                 pierced_share=sum(c["pierced"] for c in counts) / float(n_all),
                                 inlier_share=sum(c["inlier"] for c in counts) / float(n_all)))
                print(json.dumps(rows[-1]), flush=True)
        m.close()
    out = dict(what="verifyCandidates against reset + addScansById + verifyScans per candidate: wall times, "
                    "ndt2d_closure_last_ms (HIP events: build, verify launch) and the sequence's summed "
                    "ndt2d_verify_last_ms kernels, ms; K = 1: the slot launch against the installed-grid launch of the same job",
               warm_ups=WARM_UPS, reps=REPS, rows=rows)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
