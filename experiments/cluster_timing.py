"""Pose clusters: what a Clusterer call costs, per call and per phase, beside the `measure` step it
would accompany and beside the host alternative.

    python experiments/cluster_timing.py [--out profiles/cluster_timing.json] [--sizes 500,100000,1000000]
                                         [--reps 20]

Needs a GPU; there is no fallback.  Every size is a child process of its own under its own time
limit (`--step-seconds`), and the first step that fails or runs out of time ends the script: nothing
more is started on the GPU after it, and no JSON is written.

  per size n, three set shapes:
    seeded      fresh from Seeder.launch over the free cells of the cfg-5 map rendered by OccupancyMap
                at `--resolution` (many bins, many clusters), weights 1 / n
    two_blobs   shares 0.6 / 0.4 round two poses 6 m apart, sigma 0.15 m and 0.1 rad, random weights
    converged   every particle in one or two adjacent bins (sigma 0.05 m, 0.02 rad), random weights
  per shape, `reps` times after three warm-ups: the host clock round launch() + fetch() (what a caller
  waits for: it holds the waits between the label rounds), and the five phases' HIP events
  (Clusterer.last_ms: table, bins, labels, select, statistics), with the header of the last call.
  Once per shape: the host alternative, particles.cpu() + weights.cpu() + tests/cluster_restatement.py.
  Per size, for scale: the `measure` step, ScanMatcherNDT.score_poses_launch of n of the cfg's particles
  on the cfg's map and scan (cfg-5 for 1,000,000, cfg-3 otherwise), its kernel time from last_launch_ms.
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
sys.path.insert(0, os.path.join(_ROOT, "tests"))


def spread(values):
    v = np.sort(np.asarray(values, dtype=np.float64))
    return dict(n=int(len(v)), median_ms=float(np.median(v)), q1_ms=float(np.percentile(v, 25)),
                q3_ms=float(np.percentile(v, 75)), min_ms=float(v[0]), max_ms=float(v[-1]))


def blobs(rng, n, centres, shares, sigma):
    which = rng.choice(len(centres), size=n, p=shares)
    poses = np.asarray(centres, dtype=np.float64)[which] + rng.normal(size=(n, 3)) * np.asarray(sigma)
    w = rng.random(n) + 0.1
    for k, share in enumerate(shares):
        if (which == k).any():
            w[which == k] *= share / w[which == k].sum()
    return poses, w / w.sum()


def step_size(n, resolution, reps):
    import torch
    import cluster_restatement as R
    from ndt_2d_amd import Clusterer, OccupancyMap, ScanMatcherNDT, Seeder, synth
    measure_cfg = 5 if n >= 1000000 else 3
    device = ScanMatcherNDT(0)
    device.initialize("cluster_timing", **synth.matcher_params(measure_cfg))
    device.addScans(synth.map_scans(measure_cfg))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    device.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(n)
    shapes = {}

    # the seeded set, on the device
    occ = OccupancyMap(resolution, 0.25, device)
    msg = occ.getMsg(synth.map_scans(5), copy=False)
    seeder = Seeder(device)
    seeder.set_occupancy_map(occ)
    with torch.cuda.stream(stream):
        seeded = torch.empty((n, 3), dtype=torch.float64, device="cuda")
        seeder.launch(seeded.data_ptr(), n, 1, 1)
        shapes["seeded"] = (seeded, None)
        p, w = blobs(rng, n, [(-2.0, 1.0, 0.5), (4.0, 1.0, -2.0)], [0.6, 0.4], (0.15, 0.15, 0.1))
        shapes["two_blobs"] = (torch.from_numpy(p).cuda(), torch.from_numpy(w).cuda())
        p, w = blobs(rng, n, [(1.49, 0.77, 0.3)], [1.0], (0.05, 0.05, 0.02))
        shapes["converged"] = (torch.from_numpy(p).cuda(), torch.from_numpy(w).cuda())
    stream.synchronize()

    c = Clusterer(device, n)
    c.set_timing(True)
    rows = {}
    for name, (d_p, d_w) in shapes.items():
        wall, phases = [], []
        head = None
        for rep in range(reps + 3):                                   # three warm-ups
            t0 = time.perf_counter()
            c.launch(d_p.data_ptr(), d_w.data_ptr() if d_w is not None else None, n)
            head, found = c.fetch()
            took = (time.perf_counter() - t0) * 1e3
            if rep >= 3:
                wall.append(took)
                phases.append(c.last_ms())
        t0 = time.perf_counter()
        host_p = d_p.cpu().numpy()
        host_w = d_w.cpu().numpy() if d_w is not None else None
        copied = (time.perf_counter() - t0) * 1e3
        want = R.cluster(host_p, host_w)
        restated = (time.perf_counter() - t0) * 1e3
        assert want["header"]["n_clusters"] == head.n_clusters and want["header"]["n_bins"] == head.n_bins
        assert [r["label"] for r in want["records"]] == [f.label for f in found]
        rows[name] = dict(call_host_clock=spread(wall),
                          phases_events={k: spread([ph[k] for ph in phases]) for k in phases[0]},
                          events_total=spread([sum(ph.values()) for ph in phases]),
                          header=dict(head._asdict()), best_share=found[0].share if found else None,
                          host_alternative=dict(copy_ms=copied, copy_and_restatement_ms=restated))
    c.close()

    # the measure step this call would accompany
    _, pts, _ = synth.query_scan(measure_cfg)
    device.prepare_beams(pts)
    parts = synth.particles(measure_cfg, n)
    with torch.cuda.stream(stream):
        d_parts = torch.from_numpy(np.ascontiguousarray(parts)).cuda()
        d_scores = torch.zeros(len(parts), dtype=torch.float64, device="cuda")
        d_stats = torch.zeros(8, dtype=torch.float64, device="cuda")
    stream.synchronize()
    ms = []
    for rep in range(reps + 3):
        device.score_poses_launch(d_parts.data_ptr(), len(parts), d_scores.data_ptr(), d_stats.data_ptr())
        t, _ = device.last_launch_ms()
        if rep >= 3:
            ms.append(t)
    device.set_stream(None)
    return dict(n=n, shapes=rows, seeded_map=dict(width=msg["width"], height=msg["height"], resolution=resolution),
                measure=dict(cfg=measure_cfg, particles=len(parts), kernel_events=spread(ms)),
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_ROOT, "profiles", "cluster_timing.json"))
    ap.add_argument("--sizes", default="500,100000,1000000")
    ap.add_argument("--resolution", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-seconds", type=int, default=240)
    ap.add_argument("--step", type=int, help="(internal) run one size in this process")
    ap.add_argument("--piece")
    args = ap.parse_args()
    if args.step is not None:
        with open(args.piece, "w") as f:
            json.dump(step_size(args.step, args.resolution, args.reps), f)
        return 0

    pieces, seconds = [], {}
    for k, n in enumerate(int(s) for s in args.sizes.split(",") if s):
        piece = args.out + ".piece%d" % k
        t0 = time.perf_counter()
        try:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(n), "--resolution",
                                   str(args.resolution), "--reps", str(args.reps), "--piece", piece],
                                  timeout=args.step_seconds)
            status = done.returncode
        except subprocess.TimeoutExpired:
            status = "time limit of %d s" % args.step_seconds
        if status != 0:
            # nothing more is started on the GPU after a step that failed
            print("size %d failed (%s): stopping" % (n, status), file=sys.stderr)
            return 1
        with open(piece) as f:
            pieces.append(json.load(f))
        os.remove(piece)
        seconds[str(n)] = time.perf_counter() - t0
        print("size %d done in %.1f s" % (n, seconds[str(n)]), flush=True)
    out = dict(what="pose clusters: one Clusterer call (launch + fetch) per set shape and size: the host clock round "
                    "the call, HIP events round its five phases (ms), the measure step of the same run for scale, "
                    "and the host alternative (copy to the host + the numpy/Python restatement)",
               sizes=pieces, step_seconds=seconds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
