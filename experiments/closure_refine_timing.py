"""Newton NDT registration on each loop-closure candidate's own map in one call
(ScanMatcherNDT.refineCandidates) against the way to the same result without it: reset() +
addScansById(candidate) + refineScans(job) per candidate.

    python experiments/closure_refine_timing.py [OUT.json]

A graph of 17 scans of 720 points along a path through the 8 m room of synth cfg-1, the candidates
the loop-closure windows of scans 1 .. K (two scans each), one query scan; job k starts where the
lattice search on candidate k ended (matchCandidates' winner).  Rows: K = 1, 8, 16 candidates x
100 / 720 beams in use x neighbourhood 1 / 9.  Per row, in one process: the wall time of
refineCandidates, the build and the refinement launch from the closure's HIP events, and the wall
time of the sequence -- each the median of REPS calls after WARM_UPS, with minimum and maximum --
and whether the two gave the same bits; the sequence once more with a clock between its steps
(sequence_builds_ms: the reset + addScansById round trips, sequence_refines_ms: the refineScans
calls, sequence_refine_kernels_ms: their launches) beside call_outside_launches_ms, the call's
wall time less its two launches.  build_share: the build launch's part of the call's wall
time, what reusing the build of the matchCandidates call in front would save at most."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (1, 8, 16)
BEAMS = (100, 720)
CELLS = (1, 9)
WARM_UPS, REPS = 5, 20
N_SCANS = 17
SEARCH = dict(search_angular_size=0.045, search_angular_resolution=0.02, search_linear_size=0.065, search_linear_resolution=0.02)


def timed(fn):
    for _ in range(WARM_UPS):
        fn()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t)))


def main():
    from ndt_2d_amd import ScanMatcherNDT, _capi, loop_closure_window, synth
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "closure_refine_timing.json")
    world = synth.world_of((4.0, 4.0, 0.25))
    poses = np.array([(-1.2 + 0.15 * i, 0.4 - 0.05 * i + (0.1 if i % 2 else 0.0), 0.03 * i - 0.2) for i in range(N_SCANS)])
    points = [synth.scan(world, p, 8000 + i, n_beams=720) for i, p in enumerate(poses)]
    query = synth.scan(world, (0.13, -0.07, 0.031), 8100)
    guess = np.array([0.1, -0.05, 0.02])
    keys = ("pose", "score", "start_score", "gradient", "hessian", "status", "evals", "steps")
    rows = []
    for beams in BEAMS:
        m = ScanMatcherNDT(0)
        m.initialize("closure-refine-timing", ndt_resolution=0.25, range_max=4.75, laser_max_beams=beams, **SEARCH)
        for pts in points:
            m.storeScan(pts)
        m.set_timing(False)
        for K in KS:
            cands = [[(j, poses[j]) for j in loop_closure_window(i, N_SCANS)] for i in range(1, K + 1)]
            won = m.matchCandidates(guess, query, cands)
            jobs = np.array([guess + (w["pose"] if w["best_index"] != _capi.NO_INDEX else 0.0) for w in won])
            for cells in CELLS:
                def batched():
                    return m.refineCandidates(jobs, [query], cands, job_scan=[0] * K, neighbourhood=cells)

                def sequence():
                    out = []
                    for c, job in zip(cands, jobs):
                        m.reset()
                        m.addScansById([p for _, p in c], [i for i, _ in c])
                        out.append(m.refineScans([job], [query], neighbourhood=cells)[0])
                    return out

                got, want = batched(), sequence()
                same = all(np.array_equal(g[k], w[k], equal_nan=True) for g, w in zip(got, want) for k in keys)
                m.closure_set_timing(True)
                build, refine = [], []

                def batched_timed():
                    batched()
                    b, r = m.closure_last_ms()
                    build.append(b)
                    refine.append(r)

                wall = timed(batched_timed)
                m.closure_set_timing(False)
                build, refine = build[WARM_UPS:], refine[WARM_UPS:]
                seq = timed(sequence)
                # where the sequence's time goes: the build round trips, the refinements, their launches
                m.refine_set_timing(True)
                parts = dict(build=[], refine=[], kernel=[])

                def sequence_split():
                    b = r = k = 0.0
                    for c, job in zip(cands, jobs):
                        t0 = time.perf_counter()
                        m.reset()
                        m.addScansById([p for _, p in c], [i for i, _ in c])
                        t1 = time.perf_counter()
                        m.refineScans([job], [query], neighbourhood=cells)
                        t2 = time.perf_counter()
                        b, r, k = b + 1e3 * (t1 - t0), r + 1e3 * (t2 - t1), k + m.refine_last_ms()[0]
                    parts["build"].append(b)
                    parts["refine"].append(r)
                    parts["kernel"].append(k)

                timed(sequence_split)
                m.refine_set_timing(False)
                split = {key: float(np.median(v[WARM_UPS:])) for key, v in parts.items()}
                st = [g["status"] for g in got]
                rows.append(dict(beams=beams, K=K, cells=cells, call_ms=wall, sequence_ms=seq,
                                 build_kernel_ms=float(np.median(build)), refine_kernel_ms=float(np.median(refine)),
                                 build_share=float(np.median(build)) / wall["median"], speedup=seq["median"] / wall["median"],
                                 call_outside_launches_ms=wall["median"] - float(np.median(build)) - float(np.median(refine)),
                                 sequence_builds_ms=split["build"], sequence_refines_ms=split["refine"],
                                 sequence_refine_kernels_ms=split["kernel"],
                                 same_bits=bool(same), mean_evals=float(np.mean([g["evals"] for g in got])),
                                 converged=st.count(_capi.REFINE_CONVERGED), at_limit=st.count(_capi.REFINE_MAX_EVALS),
                                 stalled=st.count(_capi.REFINE_STALLED)))
                print(json.dumps(rows[-1]), flush=True)
        m.close()
    out = dict(experiment="closure_refine_timing", graph="%d scans of 720 points, candidates of two scans, resolution 0.25, range_max 4.75" % N_SCANS,
               refine="max_evals 32, tol_lin 1e-6, tol_ang 1e-6", warm_ups=WARM_UPS, repetitions=REPS,
               note="ms; call and sequence: wall time in one process; build / refine kernel: HIP events of the call's last chunk",
               build_info=_capi.build_info(), rows=rows)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("beams K   cells  call_ms (min .. max)       sequence_ms (min .. max)    build  refine  share  x     same")
    for r in rows:
        print("%-5d %-3d %-5d %7.3f (%.3f .. %.3f) %9.3f (%.3f .. %.3f) %7.4f %7.4f %5.2f %5.1f %s" % (
            r["beams"], r["K"], r["cells"], r["call_ms"]["median"], r["call_ms"]["min"], r["call_ms"]["max"],
            r["sequence_ms"]["median"], r["sequence_ms"]["min"], r["sequence_ms"]["max"], r["build_kernel_ms"],
            r["refine_kernel_ms"], r["build_share"], r["speedup"], r["same_bits"]))
    print("wrote", path)


if __name__ == "__main__":
    main()
