"""Batched loop-closure match against the sequential calls (plugin defaults: 80 x 21 x 21
lattice, 100 of 720 beams), K candidate maps of two scans each.

    python experiments/closure_batch_timing.py [OUT.json]     # prints the table; writes profiles/closure_batch_timing.json or OUT.json

For K in {1, 2, 4, 8, 16}: the median wall time of ScanMatcherNDT.matchCandidates and of K
reset() / addScansById() / matchScan() triples (20 repetitions each after a warm-up, the same
process, HIP events off), then -- events on -- the batched call's build and search launches
(ndt2d_closure_last_ms) and one sequential search kernel (ndt2d_last_launch_ms)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ndt_2d_amd import ScanMatcherNDT, loop_closure_window, synth  # noqa: E402

REPS = 20


def median_us(fn):
    fn()
    fn()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(t))


def main():
    w = synth.world_of((4.0, 4.0, 0.25))
    n_scans = 18
    poses = [(-0.9 + 0.1 * i, 0.35 - 0.04 * i + (0.11 if i % 2 else 0.0), 0.03 * i - 0.2) for i in range(n_scans)]
    m = ScanMatcherNDT(0)
    m.initialize("closure-timing", range_max=4.75)
    for i, p in enumerate(poses):
        m.storeScan(synth.scan(w, p, 7000 + i))
    query = synth.scan(w, (0.13, -0.07, 0.031), 7100)
    guess = np.array([0.1, -0.05, 0.02])
    print("K  batched_us  sequential_us  ratio  build_ms  search_ms  one_sequential_search_ms")
    rows = []
    for K in (1, 2, 4, 8, 16):
        cands = [[(j, poses[j]) for j in loop_closure_window(i, n_scans)] for i in range(1, K + 1)]

        def batched():
            m.matchCandidates(guess, query, cands)

        def sequential():
            for c in cands:
                m.reset()
                m.addScansById([p for _, p in c], [i for i, _ in c])
                m.matchScan(guess, query)

        m.set_timing(False)
        batched()
        m.closure_set_timing(False)
        t_bat = median_us(batched)
        t_seq = median_us(sequential)
        m.closure_set_timing(True)
        batched()
        build_ms, search_ms = m.closure_last_ms()
        m.closure_set_timing(False)
        m.set_timing(True)
        sequential()
        seq_ms = m.last_launch_ms()[0]
        m.set_timing(False)
        print("%-2d %10.1f %14.1f %6.2f %9.4f %10.4f %12.4f" % (K, t_bat, t_seq, t_seq / t_bat, build_ms, search_ms, seq_ms),
              flush=True)
        rows.append(dict(K=K, batched_us=t_bat, sequential_us=t_seq, repetitions=REPS, build_ms=build_ms, search_ms=search_ms,
                         one_sequential_search_ms=seq_ms))
    out = dict(experiment="closure_batch_timing", lattice="80 x 21 x 21", beams="100 of 720",
               note="median wall time of one matchCandidates call against K reset / addScansById / matchScan triples, "
                    "candidate maps of two scans each, same process and matcher", rows=rows)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "closure_batch_timing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
