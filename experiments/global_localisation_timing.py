"""Global localisation: what the free table and the seeding cost at the benchmark's sizes, and a
kidnapped-robot run with and without ParticleFilter.inject.

    python experiments/global_localisation_timing.py [--out profiles/global_localisation_timing.json]
                                                     [--cfgs 3,5] [--resolution 0.25] [--reps 20]

Needs a GPU; there is no fallback.  Every GPU step is a child process of its own under its own time
limit (`--step-seconds`), and the first step that fails or runs out of time ends the script: nothing
more is started on the GPU after it, and no JSON is written.

  timing (per cfg)   the map scans of the cfg rendered by OccupancyMap at `--resolution` (0.25 m: the
                     NDT's cell, so cfg-5's map is the 801 x 801 class of the benchmark), then, `reps`
                     times each: Seeder.set_occupancy_map (HIP events round its three launches, and the
                     host clock round the call, which includes its two waits), Seeder.launch of the cfg's
                     particle count and Seeder.inject_launch at probability 0.1 (HIP events)
  kidnapped          the generator's smallest world with a map of one corner (three scans on an L,
                     range_max 2.5 m); a filter seeded by init_global follows the truth for `--before`
                     steps, the truth is carried to another place in the mapped corner, and the run
                     goes on for `--after` steps: once without inject, once with inject(share) after
                     every measure, share from RecoveryAverages.  The position error of every step is
                     recorded; nothing is asserted.
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

LATTICE = ((-3.0, -3.0), (-3.0, -1.0), (-1.0, -3.0))
RANGE_MAX = 2.5
ALPHAS = (0.05, 0.05, 0.05, 0.05, 0.05)
MOTION = (0.15, 0.0, 0.03)
START = (-3.4, -3.1, 0.1)
CARRIED_TO = (-3.5, -0.3, -1.55)


def spread(values):
    v = np.sort(np.asarray(values, dtype=np.float64))
    return dict(n=int(len(v)), median_ms=float(np.median(v)), q1_ms=float(np.percentile(v, 25)),
                q3_ms=float(np.percentile(v, 75)), min_ms=float(v[0]), max_ms=float(v[-1]))


def step_timing(cfg, resolution, reps):
    import torch
    from ndt_2d_amd import OccupancyMap, ScanMatcherNDT, Seeder, synth
    device = ScanMatcherNDT(0)
    device.initialize("global_localisation_timing", **synth.matcher_params(1))
    scans = synth.map_scans(cfg)
    occ = OccupancyMap(resolution, 0.25, device)
    msg = occ.getMsg(scans, copy=False)
    n = synth.CONFIGS[cfg]["particles"]["n"]
    seeder = Seeder(device)
    seeder.set_timing(True)
    poses = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    count = torch.zeros((1,), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    table_ms, table_wall_ms, sample_ms, inject_ms = [], [], [], []
    free = 0
    for rep in range(reps + 3):                                   # three warm-ups
        t0 = time.perf_counter()
        free = seeder.set_occupancy_map(occ)
        wall = (time.perf_counter() - t0) * 1e3
        seeder.launch(poses.data_ptr(), n, 1, 2 * rep + 1)
        torch.cuda.synchronize()
        a, b = seeder.last_ms()
        seeder.inject_launch(poses.data_ptr(), n, 0.1, 1, 2 * rep + 1, 0, count.data_ptr())
        torch.cuda.synchronize()
        _, c = seeder.last_ms()
        if rep >= 3:
            table_ms.append(a)
            table_wall_ms.append(wall)
            sample_ms.append(b)
            inject_ms.append(c)
    assert free == int((msg["data"] == 0).sum())
    return dict(cfg=cfg, resolution=resolution, map_width=msg["width"], map_height=msg["height"],
                map_cells=msg["width"] * msg["height"], free_cells=free, particles=n,
                table_build_events=spread(table_ms), table_build_host_clock=spread(table_wall_ms),
                seed_events=spread(sample_ms), inject_p01_events=spread(inject_ms),
                replaced_last=int(count.item()), device=torch.cuda.get_device_name(0))


def step_kidnapped(before, after, particles, seed):
    import ctypes as C
    from ndt_2d_amd import MotionModel, OccupancyMap, ParticleFilter, RecoveryAverages, ScanMatcherNDT, _capi, synth
    world = synth.world_of(1)
    params = synth.matcher_params(1)
    params["range_max"] = RANGE_MAX
    scans = [((x, y, 0.0), synth.scan(world, (x, y, 0.0), 1000003 + k)) for k, (x, y) in enumerate(LATTICE)]
    clipped = [(p, pts[np.hypot(pts[:, 0], pts[:, 1]) <= RANGE_MAX]) for p, pts in scans]
    L = _capi.lib()

    def moved(pose):
        # the odometry model without noise: rotate by atan2(dy, dx), advance, rotate the rest
        x, y, th = pose
        dx, dy, dth = MOTION
        trans = float(np.hypot(dx, dy))
        rot1 = float(np.arctan2(dy, dx)) if trans > 0.01 else 0.0
        return (x + trans * np.cos(th + rot1), y + trans * np.sin(th + rot1), th + dth)

    runs = {}
    for name in ("without_inject", "with_inject"):
        m = ScanMatcherNDT(0)
        m.initialize("kidnapped", **params)
        m.addScans(scans)
        occ = OccupancyMap(0.05, 0.25, m)
        occ.getMsg(clipped)
        f = ParticleFilter(500, particles, MotionModel(*ALPHAS), m, seed=seed, resample_on="device")
        f.init_global(occ)
        averages = RecoveryAverages(0.05, 0.5)
        truth = START
        rows = []
        for t in range(before + after):
            truth = CARRIED_TO if t == before else moved(truth)
            assert not L.ndt2d_synth_pose_blocked(C.byref(world), truth[0], truth[1], 0.25)
            points = synth.scan(world, truth, 777 + t)
            f.update(*MOTION)
            f.measure(m, points)
            mean = f.getMean()
            share = averages.update(f.mean_measure_weight())
            replaced = 0
            f.resample(0.01, 2.3)
            if name == "with_inject" and share > 0.0:
                replaced = f.inject(min(share, 1.0))
            rows.append(dict(step=t, carried=t >= before, error_m=float(np.hypot(mean[0] - truth[0], mean[1] - truth[1])),
                             particles=len(f.particles), share=share, replaced=replaced,
                             mean_weight=f.mean_measure_weight()))
        runs[name] = rows
        m.close()
    return dict(world="cfg-1 room, map of one corner (three scans on an L, range_max 2.5 m)", particles=particles,
                seed=seed, steps_before=before, steps_after=after, start=START, carried_to=CARRIED_TO,
                alpha_slow=0.05, alpha_fast=0.5, runs=runs)


def child(args):
    if args.step == "timing":
        out = step_timing(args.cfg, args.resolution, args.reps)
    else:
        out = step_kidnapped(args.before, args.after, args.particles, args.seed)
    with open(args.piece, "w") as f:
        json.dump(out, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_ROOT, "profiles", "global_localisation_timing.json"))
    ap.add_argument("--cfgs", default="3,5")
    ap.add_argument("--resolution", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--before", type=int, default=10)
    ap.add_argument("--after", type=int, default=20)
    ap.add_argument("--particles", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--step-seconds", type=int, default=240)
    ap.add_argument("--step", choices=("timing", "kidnapped"), help="(internal) run one GPU step in this process")
    ap.add_argument("--cfg", type=int)
    ap.add_argument("--piece")
    args = ap.parse_args()
    if args.step:
        child(args)
        return 0

    steps = [("timing cfg-%s" % c, ["--step", "timing", "--cfg", c]) for c in args.cfgs.split(",") if c]
    steps.append(("kidnapped", ["--step", "kidnapped"]))
    common = ["--resolution", str(args.resolution), "--reps", str(args.reps), "--before", str(args.before),
              "--after", str(args.after), "--particles", str(args.particles), "--seed", str(args.seed)]
    pieces = []
    for k, (name, extra) in enumerate(steps):
        piece = args.out + ".piece%d" % k
        t0 = time.perf_counter()
        try:
            done = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra + common + ["--piece", piece],
                                  timeout=args.step_seconds)
            status = done.returncode
        except subprocess.TimeoutExpired:
            status = "time limit of %d s" % args.step_seconds
        if status != 0:
            # nothing more is started on the GPU after a step that failed
            print("step '%s' failed (%s): stopping" % (name, status), file=sys.stderr)
            return 1
        with open(piece) as f:
            pieces.append((name, json.load(f), time.perf_counter() - t0))
        os.remove(piece)
        print("step '%s' done in %.1f s" % (name, pieces[-1][2]), flush=True)
    out = dict(what="global localisation: table build and seeding (HIP events round the kernels, ms) at the "
                    "benchmark's map and particle counts, and a kidnapped-robot run with and without inject",
               timing=[p for name, p, _ in pieces if name.startswith("timing")],
               kidnapped=[p for name, p, _ in pieces if name == "kidnapped"][0],
               step_seconds={name: s for name, _, s in pieces})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
