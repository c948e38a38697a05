"""Match verification (ScanMatcherNDT.verifyScans): the kernel and the read-back of one call from
the object's HIP events (ndt2d_verify_last_ms), and the call's wall time.

    python experiments/verify_timing.py [OUT.json]

Rows: the 41 x 41 map of synth cfg-1 and the 201 x 201 map of cfg-3 x K = 1, 64, 1,024 jobs x 100 /
720 beams in use x rays on / off, neighbourhood 9, per-beam outputs not wanted.  The jobs share the
config's query scan; job k's pose is the true pose displaced along a spiral of up to 1 m and turned
by up to 0.3 rad, so that the rows hold right and wrong poses alike (pierced_share: the part of all
beams whose ray was pierced).  Per row the median of REPS calls after WARM_UPS, with minimum and
maximum.  A run without a GPU fails; nothing falls back."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (1, 64, 1024)
BEAMS = (100, 720)
MAPS = (1, 3)            # synth configs: 41 x 41 and 201 x 201 cells
WARM_UPS, REPS = 5, 30


def spread(values):
    return dict(median=float(np.median(values)), min=float(min(values)), max=float(max(values)))


def main():
    from ndt_2d_amd import ScanMatcherNDT, synth
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "verify_timing.json")
    rows = []
    for cfg in MAPS:
        scans = synth.map_scans(cfg)
        _, query, true_pose = synth.query_scan(cfg)
        for beams in BEAMS:
            m = ScanMatcherNDT(0)
            m.initialize("verify-timing", **synth.matcher_params(cfg, laser_max_beams=beams))
            m.addScans(scans)
            grid = m.grid()
            for K in KS:
                k = np.arange(K, dtype=np.float64)
                radius = k / max(K - 1, 1)
                jobs = np.column_stack([true_pose[0] + radius * np.cos(2.4 * k), true_pose[1] + radius * np.sin(2.4 * k),
                                        true_pose[2] + 0.3 * radius * np.cos(1.7 * k)])
                for rays in (True, False):
                    call = lambda: m.verifyScans(jobs, [query], job_scan=[0] * K, rays=rays)   # noqa: E731
                    counts = call()
                    m.verify_set_timing(True)
                    for _ in range(WARM_UPS):
                        call()
                    kernel, fetch, wall = [], [], []
                    for _ in range(REPS):
                        t0 = time.perf_counter()
                        call()
                        wall.append(1e3 * (time.perf_counter() - t0))
                        a, b = m.verify_last_ms()
                        kernel.append(a)
                        fetch.append(b)
                    m.verify_set_timing(False)
                    n_all = sum(c["n_beams"] for c in counts)
                    rows.append(dict(map_cells=[int(grid[1]), int(grid[2])], jobs=K, beams=beams, rays=rays,
                                     neighbourhood=9, kernel_ms=spread(kernel), fetch_ms=spread(fetch), call_wall_ms=spread(wall),
                                     beams_all=int(n_all), pierced_share=sum(c["pierced"] for c in counts) / float(n_all),
                                     inlier_share=sum(c["inlier"] for c in counts) / float(n_all)))
                    print(json.dumps(rows[-1]))
    out = dict(what="verifyScans: ndt2d_verify_last_ms (HIP events: kernel, read-back) and the call's wall time, ms",
               warm_ups=WARM_UPS, reps=REPS, rows=rows)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
