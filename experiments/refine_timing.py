"""Newton NDT registration (refineScans) against the lattice search of the same jobs (matchScans
with the plugin's default lattice, 80 x 21 x 21: the way to a pose without it), and the two in a
row (refine_matches), on the 129 x 129 map of tests/test_gpu_match_starts.py.

    python experiments/refine_timing.py [OUT.json]     # prints the table; writes profiles/refine_timing.json or OUT.json

For 100 and 720 beams of 720-beam scans and K in {1, 8, 64, 512}: K distinct scans, each from its
own pose a few centimetres off where it was taken.  Medians of 20 wall times after 5 warm-ups, one
process, one matcher per beam count, HIP events off; then -- events on -- the registration's
kernel and read-back (ndt2d_refine_last_ms) and what the jobs did (evaluations, how they stopped)."""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ndt_2d_amd import ScanMatcherNDT, _capi, refine_matches, synth  # noqa: E402

KS = (1, 8, 64, 512)
BEAMS = (100, 720)
WARM_UPS, REPS = 5, 20


def median_us(fn):
    for _ in range(WARM_UPS):
        fn()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(t))


def fixture_map():
    """45 scans of 360 beams, 129 x 129 cells of 0.25 m."""
    w = synth.world_of((12.0, 4.0, 0.25))
    scans, index = [], 0
    for iy in range(7):
        for ix in range(7):
            x, y = (ix - 3) * 3.0, (iy - 3) * 3.0
            if not synth.pose_blocked(w, x, y):
                scans.append(((x, y, 0.0), synth.scan(w, (x, y, 0.0), 9000 + index, n_beams=360)))
            index += 1
    return w, scans


def query_poses(world, half, n, rng):
    poses = []
    while len(poses) < n:
        x, y = rng.uniform(-half, half, size=2)
        if not synth.pose_blocked(world, x, y):
            poses.append((x, y, rng.uniform(-math.pi, math.pi)))
    return poses


def run(world, scans, beams):
    m = ScanMatcherNDT(0)
    m.initialize("refine-timing", range_max=7.0, laser_max_beams=beams)      # otherwise the plugin's declared defaults
    m.addScans(scans)
    m.set_timing(False)
    rng = np.random.default_rng(20261019)
    truth = query_poses(world, 10.0, max(KS), rng)
    queries = [synth.scan(world, pose, 9900 + k) for k, pose in enumerate(truth)]
    off = rng.uniform(-0.03, 0.03, size=(len(truth), 3)) * np.array([1.0, 1.0, 0.5])
    jobs_all = np.array(truth) + off
    rows = []
    print("%d beams, map 129 x 129, %s" % (beams, m.last_build()))
    print("K     refine_us  match_us  both_us  kernel_ms  fetch_ms  mean_evals  converged  max_evals  stalled  no_overlap")
    for K in KS:
        jobs, qs = jobs_all[:K], queries[:K]
        t_refine = median_us(lambda: m.refineScans(jobs, qs))
        t_match = median_us(lambda: m.matchScans(jobs, qs))
        t_both = median_us(lambda: refine_matches(m, jobs, qs))
        m.refine_set_timing(True)
        got = m.refineScans(jobs, qs)
        kernel_ms, fetch_ms = m.refine_last_ms()
        m.refine_set_timing(False)
        status = [r["status"] for r in got]
        counts = [status.count(s) for s in (_capi.REFINE_CONVERGED, _capi.REFINE_MAX_EVALS, _capi.REFINE_STALLED,
                                            _capi.REFINE_NO_OVERLAP)]
        evals = float(np.mean([r["evals"] for r in got]))
        print("%-5d %9.1f %9.1f %8.1f %10.4f %9.4f %11.1f %10d %10d %8d %11d" % (
            K, t_refine, t_match, t_both, kernel_ms, fetch_ms, evals, *counts), flush=True)
        rows.append(dict(K=K, refine_us=t_refine, match_scans_us=t_match, refine_matches_us=t_both, kernel_ms=kernel_ms,
                         fetch_ms=fetch_ms, mean_evals=evals, converged=counts[0], max_evals=counts[1], stalled=counts[2],
                         no_overlap=counts[3]))
    return dict(beams=beams, build=m.last_build(), rows=rows)


def main():
    world, scans = fixture_map()
    out = dict(experiment="refine_timing", map="129 x 129", lattice_of_match_scans="80 x 21 x 21 (plugin defaults)",
               refine="max_evals 32, tol_lin 1e-6, tol_ang 1e-6", warm_ups=WARM_UPS, repetitions=REPS,
               note="median wall time per call, one process; refine_matches = matchScans, then refineScans from its winners",
               runs=[run(world, scans, b) for b in BEAMS])
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "refine_timing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
