"""The clearance map: what the transform, the mask and the table build that follows cost on the
benchmark's occupancy maps, and what the call replaces on the host.

    python experiments/clearance_timing.py [--out profiles/clearance_timing.json] [--cfgs 3,5]
                                           [--resolution 0.25] [--reps 20]

Needs a GPU; there is no fallback.  Every GPU step is a child process of its own under its own time
limit (`--step-seconds`), and the first step that fails or runs out of time ends the script: nothing
more is started on the GPU after it, and no JSON is written.

Per cfg: the map scans of the cfg rendered by OccupancyMap at `--resolution` (0.25 m: cfg-5's map is
the 801 x 801 class of the benchmark), then for the cap R = 0 (none) and the R that covers `--cover`
metres (0.5), `reps` times each after three warm-ups:

  transform          ClearanceMap.compute_occupancy_map (HIP events round its four launches; the host
                     clock round the call, which includes the copy of the map and the wait)
  mask               ClearanceMap.mask at `--clearance` metres (0.3) (HIP events)
  table              Seeder.set_map_device of the masked map (HIP events round its three launches)

and as what these serve and replace:

  init_global        Seeder.set_occupancy_map plus Seeder.launch of the cfg's particle count, without
                     a clearance (HIP events): if the uncapped transform takes longer than this, cap it
  host               scipy.ndimage.distance_transform_edt on the same map, the mask in numpy and the
                     upload of the masked map (host clock); left out if scipy does not import
  share              the share of the free cells that `--clearance` removes

The medians are of one process on one GPU; nothing is asserted about them.  The d2 of the uncapped
transform is compared with scipy's (squared, rounded) and the script fails if they differ.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)


def spread(values):
    v = np.sort(np.asarray(values, dtype=np.float64))
    return dict(n=int(len(v)), median_ms=float(np.median(v)), q1_ms=float(np.percentile(v, 25)),
                q3_ms=float(np.percentile(v, 75)), min_ms=float(v[0]), max_ms=float(v[-1]))


def step_timing(cfg, resolution, reps, clearance, cover):
    import torch
    from ndt_2d_amd import ClearanceMap, OccupancyMap, ScanMatcherNDT, Seeder, synth
    from ndt_2d_amd.clearance import min_d2_of
    device = ScanMatcherNDT(0)
    device.initialize("clearance_timing", **synth.matcher_params(1))
    occ = OccupancyMap(resolution, 0.25, device)
    msg = occ.getMsg(synth.map_scans(cfg))
    grid = msg["data"]
    width, height = msg["width"], msg["height"]
    geo = (msg["origin_x"], msg["origin_y"], msg["resolution"])
    n = synth.CONFIGS[cfg]["particles"]["n"]
    free = int((grid == 0).sum())
    threshold = min_d2_of(clearance, resolution)
    cover_cells = int(np.ceil(cover / resolution))
    cm = ClearanceMap(device)
    cm.set_timing(True)
    seeder = Seeder(device)
    seeder.set_timing(True)
    poses = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    out = dict(cfg=cfg, resolution=resolution, map_width=width, map_height=height, map_cells=width * height,
               free_cells=free, obstacle_cells=int(((grid != 0) & (grid != -1)).sum()), particles=n,
               clearance_m=clearance, min_d2=threshold, device=torch.cuda.get_device_name(0), caps=[])
    exact = None
    for cap in (0, cover_cells):
        transform_ms, transform_wall_ms, mask_ms, table_ms = [], [], [], []
        kept = 0
        for rep in range(reps + 3):                               # three warm-ups
            t0 = time.perf_counter()
            cm.compute_occupancy_map(occ, max_cells=cap)
            wall = (time.perf_counter() - t0) * 1e3
            ptr = cm.mask(min_d2=threshold)
            a, b = cm.last_ms()
            kept = seeder.set_map_device(ptr, width, height, *geo)
            c, _ = seeder.last_ms()
            if rep >= 3:
                transform_ms.append(a)
                transform_wall_ms.append(wall)
                mask_ms.append(b)
                table_ms.append(c)
        d2 = cm.d2()
        if cap == 0:
            exact = d2
        within = d2 != 0xFFFFFFFF
        out["caps"].append(dict(max_cells=cap, transform_events=spread(transform_ms),
                                transform_host_clock=spread(transform_wall_ms), mask_events=spread(mask_ms),
                                table_build_events=spread(table_ms), cells_kept=kept,
                                share_of_free_cells_removed=1.0 - kept / max(free, 1),
                                largest_d2_reported=int(d2[within].max()) if within.any() else None))
    # what the clearance serves: the init_global without it
    table_ms, sample_ms = [], []
    for rep in range(reps + 3):
        seeder.set_occupancy_map(occ)
        seeder.launch(poses.data_ptr(), n, 1, 2 * rep + 1)
        torch.cuda.synchronize()
        a, b = seeder.last_ms()
        if rep >= 3:
            table_ms.append(a)
            sample_ms.append(b)
    out["init_global_without_clearance"] = dict(table_build_events=spread(table_ms), seed_events=spread(sample_ms),
                                                total_median_ms=float(np.median(table_ms) + np.median(sample_ms)))
    # what the call replaces on the host
    try:
        from scipy import ndimage
    except ImportError:
        out["host"] = None
        return out
    obstacles = (grid != 0) & (grid != -1)
    edt_ms, mask_np_ms, upload_ms = [], [], []
    masked = grid
    for rep in range(5):
        t0 = time.perf_counter()
        edt = ndimage.distance_transform_edt(~obstacles)
        t1 = time.perf_counter()
        host_d2 = np.rint(edt * edt)
        masked = grid.copy()
        masked[(grid == 0) & (host_d2 < threshold)] = 99
        t2 = time.perf_counter()
        d = torch.from_numpy(masked).cuda()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        del d
        edt_ms.append((t1 - t0) * 1e3)
        mask_np_ms.append((t2 - t1) * 1e3)
        upload_ms.append((t3 - t2) * 1e3)
    if obstacles.any():
        assert np.array_equal(host_d2.astype(np.uint32), exact), "the device d2 differs from scipy's"
    if threshold <= cover_cells * cover_cells:                     # (the capped transform then masks the same cells)
        assert np.array_equal(cm.inflated(), masked), "the device mask differs from the host's"
    out["host"] = dict(scipy_edt_host_clock=spread(edt_ms), numpy_mask_host_clock=spread(mask_np_ms),
                       upload_host_clock=spread(upload_ms), d2_equals_scipy=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_ROOT, "profiles", "clearance_timing.json"))
    ap.add_argument("--cfgs", default="3,5")
    ap.add_argument("--resolution", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--clearance", type=float, default=0.3)
    ap.add_argument("--cover", type=float, default=0.5)
    ap.add_argument("--step-seconds", type=int, default=240)
    ap.add_argument("--cfg", type=int, help="(internal) run one cfg's GPU step in this process")
    ap.add_argument("--piece")
    args = ap.parse_args()
    if args.cfg is not None:
        with open(args.piece, "w") as f:
            json.dump(step_timing(args.cfg, args.resolution, args.reps, args.clearance, args.cover), f)
        return 0

    common = ["--resolution", str(args.resolution), "--reps", str(args.reps), "--clearance", str(args.clearance),
              "--cover", str(args.cover)]
    pieces, seconds = [], {}
    for k, cfg in enumerate(c for c in args.cfgs.split(",") if c):
        piece = args.out + ".piece%d" % k
        t0 = time.perf_counter()
        try:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--cfg", cfg, "--piece", piece] + common,
                                  timeout=args.step_seconds)
            status = done.returncode
        except subprocess.TimeoutExpired:
            status = "time limit of %d s" % args.step_seconds
        if status != 0:
            # nothing more is started on the GPU after a step that failed
            print("step 'cfg-%s' failed (%s): stopping" % (cfg, status), file=sys.stderr)
            return 1
        with open(piece) as f:
            pieces.append(json.load(f))
        os.remove(piece)
        seconds["cfg-%s" % cfg] = time.perf_counter() - t0
        print("step 'cfg-%s' done in %.1f s" % (cfg, seconds["cfg-%s" % cfg]), flush=True)
    out = dict(what="clearance map: transform, mask and the seeder's table build that follows (HIP events round the "
                    "kernels, ms) on the benchmark's occupancy maps, uncapped and capped at the radius that covers "
                    "--cover metres; the init_global they serve; scipy's transform, a numpy mask and the upload "
                    "on the host clock",
               timing=pieces, step_seconds=seconds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
