"""Wall time of one map publish: OccupancyGrid.getMsg (every scan uploaded twice, every ray traced
again, the whole map read back) against OccupancyMap.getMsg (resident scans and counts), for the
map scans of cfg-3 and cfg-5 fed one at a time.

    python experiments/occupancy_map_timing.py [--out profiles/occupancy_map_timing.json]
                                               [--cfgs 3,5] [--resolution 0.05]

What is timed is a host clock around one getMsg; both forms end in a blocking device-to-host copy,
so the clock covers the device work.  Needs a GPU; there is no fallback.

  feed        OccupancyMap.getMsg(scans[:k], copy=False) for k = 1 .. N, every step timed once
              and kept with its mode, beams traced, dirty rectangle and bytes moved; per
              checkpoint the median / quartiles / extremes of the INCREMENTAL steps in a window
              of steps around it (a step cannot be repeated without changing the object)
  baseline    OccupancyGrid.getMsg(scans[:k]) on a generator that has seen scans[:k - 1], at
              the checkpoints: 1 warm-up and `reps` timed repetitions, each on a fresh generator
  full        at the final length: OccupancyMap forced to FULL (one pose moved by one ulp each
              time) against OccupancyGrid on the same inputs, alternating
"""
import argparse
import json
import os
import sys
import time

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)

from ndt_2d_amd import OccupancyMap, ScanMatcherNDT, synth  # noqa: E402
from ndt_2d_amd.occupancy_grid import OccupancyGrid  # noqa: E402


def spread(values):
    v = np.sort(np.asarray(values, dtype=np.float64))
    if len(v) == 0:
        return None
    return dict(n=int(len(v)), median_ms=float(np.median(v)), q1_ms=float(np.percentile(v, 25)),
                q3_ms=float(np.percentile(v, 75)), min_ms=float(v[0]), max_ms=float(v[-1]))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def baseline_bytes(scans, msg):
    n_points = sum(len(s[1]) for s in scans)
    once = 16 * n_points + 32 * len(scans) + 4 * (len(scans) + 1)
    return dict(up=2 * once, down=32 + msg["width"] * msg["height"])


def run_cfg(device, cfg, resolution, occ_thresh, reps, window):
    scans = synth.map_scans(cfg)
    n = len(scans)
    checkpoints = sorted({k for k in (1, n // 16, n // 8, n // 4, n // 2, 3 * n // 4, n) if k >= 1})

    # warm-up: code objects, allocator, the first imports of both paths
    warm = OccupancyMap(resolution, occ_thresh, device)
    for k in range(1, min(n, 12) + 1):
        warm.getMsg(scans[:k], copy=False)
    warm.close()
    OccupancyGrid(resolution, occ_thresh, device).getMsg(scans[:min(n, 12)])

    om = OccupancyMap(resolution, occ_thresh, device)
    steps = []
    base = {}
    for k in range(1, n + 1):
        ms, msg = timed(lambda: om.getMsg(scans[:k], copy=False))
        x0, y0, w, h = om.last_rect
        steps.append(dict(k=k, ms=ms, mode=om.last_mode, beams_traced=om.last_beams_traced,
                          rect_cells=w * h, map_cells=msg["width"] * msg["height"],
                          bytes_up=om.last_bytes_up, bytes_down=om.last_bytes_down))
        if k in checkpoints:
            times = []
            for rep in range(reps + 1):
                g = OccupancyGrid(resolution, occ_thresh, device)
                if k > 1:
                    g.getMsg(scans[:k - 1])
                t, ref = timed(lambda: g.getMsg(scans[:k]))
                if rep:
                    times.append(t)
            assert np.array_equal(ref["data"], msg["data"]), "the two renderers disagree at k=%d" % k
            base[k] = dict(spread(times), **baseline_bytes(scans[:k], ref))
    modes = [s["mode"] for s in steps]

    points = []
    for k in checkpoints:
        near = [s for s in steps if abs(s["k"] - k) <= window and s["mode"] == "INCREMENTAL"]
        at = steps[k - 1]
        points.append(dict(k=k, map_cells=at["map_cells"], baseline=base[k],
                           step=dict(mode=at["mode"], ms=at["ms"], beams_traced=at["beams_traced"],
                                     rect_cells=at["rect_cells"], bytes_up=at["bytes_up"],
                                     bytes_down=at["bytes_down"]),
                           incremental_near=dict(spread([s["ms"] for s in near]) or {},
                                                 window_steps=window,
                                                 median_rect_cells=float(np.median([s["rect_cells"] for s in near])) if near else None,
                                                 median_bytes_up=float(np.median([s["bytes_up"] for s in near])) if near else None,
                                                 median_bytes_down=float(np.median([s["bytes_down"] for s in near])) if near else None)))

    # FULL at the final length against the baseline on the same inputs, alternating
    g = OccupancyGrid(resolution, occ_thresh, device)
    g.getMsg(scans)
    cur = list(scans)
    t_full, t_base, t_copy = [], [], []
    full_bytes = None
    for rep in range(reps + 1):
        (x, y, th), pts = cur[0]
        cur[0] = ((float(np.nextafter(x, np.inf)), y, th), pts)
        a, got = timed(lambda: om.getMsg(cur, copy=False))
        assert om.last_mode == "FULL", om.last_mode
        full_bytes = dict(up=om.last_bytes_up, down=om.last_bytes_down)
        b, ref = timed(lambda: g.getMsg(cur))
        assert np.array_equal(ref["data"], got["data"])
        c, _ = timed(lambda: got["data"].copy())
        if rep:
            t_full.append(a)
            t_base.append(b)
            t_copy.append(c)
    om.close()

    by_mode = {m: spread([s["ms"] for s in steps if s["mode"] == m]) for m in ("FULL", "INCREMENTAL", "UNCHANGED")}
    return dict(cfg=cfg, n_scans=n, n_points=int(sum(len(s[1]) for s in scans)), resolution=resolution,
                occ_thresh=occ_thresh, share_incremental=modes.count("INCREMENTAL") / float(n),
                mode_counts={m: modes.count(m) for m in ("FULL", "INCREMENTAL", "UNCHANGED")},
                feed_ms_by_mode=by_mode, checkpoints=points,
                full_at_final=dict(occupancy_map_full=dict(spread(t_full), **full_bytes),
                                   occupancy_grid=dict(spread(t_base), **baseline_bytes(cur, ref)),
                                   map_copy_on_host=spread(t_copy)),
                steps=["%d %s %.4f %d %d" % (s["k"], s["mode"][0], s["ms"], s["beams_traced"], s["rect_cells"])
                       for s in steps])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_ROOT, "profiles", "occupancy_map_timing.json"))
    ap.add_argument("--cfgs", default="3,5")
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--occ-thresh", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=int, default=15)
    args = ap.parse_args()

    import torch
    device = ScanMatcherNDT(0)
    device.initialize("occupancy_map_timing", **synth.matcher_params(1))
    out = dict(what="wall time (ms) of one map publish; host clock around getMsg, which ends in a blocking "
                    "device-to-host copy; OccupancyMap with copy=False (the array it keeps, patched in place)",
               device=torch.cuda.get_device_name(0), reps=args.reps,
               steps_columns="k mode(F/I/U) ms beams_traced rect_cells", runs=[])
    for cfg in [int(c) for c in args.cfgs.split(",")]:
        t0 = time.perf_counter()
        run = run_cfg(device, cfg, args.resolution, args.occ_thresh, args.reps, args.window)
        run["script_seconds"] = time.perf_counter() - t0
        out["runs"].append(run)
        print("cfg-%d: %d scans, share incremental %.3f, INCREMENTAL median %s ms, FULL at final %.3f ms, "
              "OccupancyGrid at final %.3f ms" %
              (cfg, run["n_scans"], run["share_incremental"],
               run["feed_ms_by_mode"]["INCREMENTAL"] and round(run["feed_ms_by_mode"]["INCREMENTAL"]["median_ms"], 4),
               run["full_at_final"]["occupancy_map_full"]["median_ms"],
               run["full_at_final"]["occupancy_grid"]["median_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
