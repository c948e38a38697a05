"""Batched scan tracking against the K sequential matchScan calls (plugin defaults: 80 x 21 x 21
lattice, 100 of 720 beams), on a 129 x 129 map and on the cfg-5 801 x 801 map (larger than LDS).

    python experiments/scans_batch_timing.py [OUT.json]     # prints the table; writes profiles/scans_batch_timing.json or OUT.json

For K in {1, 8, 64, 1024}: K distinct 720-beam scans, each matched from its own pose a few
centimetres off where it was taken.  The median wall time of ScanMatcherNDT.matchScans and of K
matchScan calls (the same process, the same matcher, HIP events off; 20 repetitions after two
warm-ups, 5 at K = 1,024), then -- events on -- the batched call's search and reduce launches
(ndt2d_scans_last_ms; the last chunk of the call).  Writes profiles/scans_batch_timing.json."""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ndt_2d_amd import ScanMatcherNDT, synth  # noqa: E402

KS = (1, 8, 64, 1024)


def median_us(fn, reps):
    fn()
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(t))


def fixture_map():
    """The map of tests/test_gpu_match_starts.py: 45 scans of 360 beams, 129 x 129 cells."""
    w = synth.world_of((12.0, 4.0, 0.25))
    scans, index = [], 0
    for iy in range(7):
        for ix in range(7):
            x, y = (ix - 3) * 3.0, (iy - 3) * 3.0
            if not synth.pose_blocked(w, x, y):
                scans.append(((x, y, 0.0), synth.scan(w, (x, y, 0.0), 9000 + index, n_beams=360)))
            index += 1
    return "129 x 129", w, scans, 7.0, 10.0


def cfg5_map():
    c = synth.CONFIGS[5]
    return "801 x 801 (cfg-5)", synth.world_of(5), synth.map_scans(5), c["range_max"], 80.0


def query_poses(world, half, n, rng):
    """n free poses uniform over the room, every heading."""
    poses = []
    while len(poses) < n:
        x, y = rng.uniform(-half, half, size=2)
        if not synth.pose_blocked(world, x, y):
            poses.append((x, y, rng.uniform(-math.pi, math.pi)))
    return poses


def run(name, world, scans, range_max, half):
    m = ScanMatcherNDT(0)
    m.initialize("scans-timing", range_max=range_max)      # the plugin's declared defaults
    m.addScans(scans)
    m.set_timing(False)
    rng = np.random.default_rng(20261018)
    truth = query_poses(world, half, max(KS), rng)
    queries = [synth.scan(world, pose, 9900 + k) for k, pose in enumerate(truth)]
    off = rng.uniform(-0.03, 0.03, size=(len(truth), 3)) * np.array([1.0, 1.0, 0.5])
    jobs_all = np.array(truth) + off
    rows = []
    print("map %s, %s" % (name, m.last_build()))
    print("K     batched_us  sequential_us  ratio  search_ms  reduce_ms")
    for K in KS:
        jobs, qs = jobs_all[:K], queries[:K]
        reps = 20 if K < 1024 else 5

        def batched():
            m.matchScans(jobs, qs)

        def sequential():
            for j, q in zip(jobs, qs):
                m.matchScan(j, q)

        batched()
        m.scans_set_timing(False)
        t_bat = median_us(batched, reps)
        t_seq = median_us(sequential, reps)
        m.scans_set_timing(True)
        batched()
        search_ms, reduce_ms = m.scans_last_ms()
        m.scans_set_timing(False)
        print("%-5d %10.1f %14.1f %6.2f %10.4f %10.4f" % (K, t_bat, t_seq, t_seq / t_bat, search_ms, reduce_ms), flush=True)
        rows.append(dict(K=K, batched_us=t_bat, sequential_us=t_seq, repetitions=reps, search_ms=search_ms,
                         reduce_ms=reduce_ms))
    return dict(map=name, build=m.last_build(), rows=rows)


def main():
    out = dict(experiment="scans_batch_timing", lattice="80 x 21 x 21", beams="100 of 720",
               note="median wall time of one matchScans call against K matchScan calls, same process and matcher",
               maps=[run(*fixture_map()), run(*cfg5_map())])
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "scans_batch_timing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
