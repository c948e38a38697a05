"""Timing of the pose-graph solve (csrc/posegraph/) on synthetic graphs -> profiles/posegraph_timing.json.

A measurement script, not a test.  The graphs: an odometry chain along two laps of a loop, 0.25 m
between poses, noisy odometry integrated into the start poses, and a switchable closure every 50
nodes of the second lap back to the pose one lap earlier.  N = 100, 1,000 and 10,000 poses; K = 1,
64 and 256 masks, the first with every constraint on, the others random over the closures (each
closure off with probability 1/2).  Per (N, K): the median over 30 calls after 5 warm-ups of the
kernel time from HIP events (the solver launch and the two chi2 launches round it) and of the
call's wall time, with the LM and CG iterations of the jobs.  Ceres's default tolerances.  As
context, not as a rival: the wall time of the numpy restatement's dense solve of job 0 up to
N = 1,000.  No speed against Ceres is claimed: it is not built here.

    python experiments/posegraph_timing.py [--calls 30] [--warmup 5] [--sizes 100,1000,10000]

--preconditioner jacobi,chain runs every (N, K) with one preconditioner after the other on the same
object, masks and session (a row's "preconditioner" says which; "us_per_cg_slowest_job" is the kernel
time over the CG iterations of the job that made most: a launch lasts as long as its slowest job).
profiles/posegraph_chain_timing.json is such a run.

--loss trivial,huber,cauchy runs every (N, K, preconditioner) under one loss after the other (at
--loss-scale, on the constraints --loss-on says: "all" or "switchable", the closures), again on the
same object, masks and session; a row's "loss" says which, and its costs are the robust ones.  The
closures of these graphs are true ones that the start poses' drift has carried out of the loss's
quadratic part: the robust rows make more LM iterations, not another kind of step.
profiles/posegraph_robust_timing.json is put together from such runs ("jacobi" at N = 100, "chain"
at N = 1,000), with the rows of the commit before the losses taken in the same session.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

INFORMATION = np.array([[100.0, 10.0, 5.0], [10.0, 80.0, -8.0], [5.0, -8.0, 400.0]])


def relative(a, b):
    c, s = math.cos(a[2]), math.sin(a[2])
    dx, dy = b[0] - a[0], b[1] - a[1]
    return np.array([c * dx + s * dy, c * dy - s * dx, b[2] - a[2]])


def compose(a, t):
    c, s = math.cos(a[2]), math.sin(a[2])
    return np.array([a[0] + c * t[0] - s * t[1], a[1] + s * t[0] + c * t[1], a[2] + t[2]])


def loop_graph(n, seed, every=50):
    rng = np.random.default_rng(seed)
    per_lap = n // 2
    step = 2.0 * math.pi / per_lap
    radius = 0.25 / step
    true = np.array([[radius * math.sin(step * i), radius * (1.0 - math.cos(step * i)), step * i] for i in range(n)])
    begin, end, transform, switchable = [], [], [], []
    start = [true[0].copy()]
    for i in range(n - 1):
        t = relative(true[i], true[i + 1]) + rng.normal(0.0, [0.004, 0.004, 0.001])
        begin.append(i)
        end.append(i + 1)
        transform.append(t)
        switchable.append(False)
        start.append(compose(start[-1], t))
    for j in sorted(set(range(per_lap, n, every)) | {n - 1}):
        i = j - per_lap
        t = relative(true[i], true[j]) + rng.normal(0.0, [0.002, 0.002, 0.0005])
        t[2] -= 2.0 * math.pi * math.floor((t[2] + math.pi) / (2.0 * math.pi))
        begin.append(i)
        end.append(j)
        transform.append(t)
        switchable.append(True)
    return dict(poses=np.array(start), begin=np.array(begin), end=np.array(end), transform=np.array(transform),
                information=np.tile(INFORMATION, (len(begin), 1, 1)), switchable=np.array(switchable))


def write(args, rows, dense):
    """The record so far (rewritten after every configuration: a long run leaves what it has)."""
    out = dict(what="posegraph_solve_kernel + the two chi2 launches, HIP events; default (Ceres) tolerances; calls and warm-ups per row",
               rows=rows, restatement=dense)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="100,1000,10000")
    ap.add_argument("--masks", default="1,64,256")
    ap.add_argument("--preconditioner", default="jacobi", help="\"jacobi\", \"chain\" or both with a comma: each (N, K) with one after the other")
    ap.add_argument("--loss", default="", help="\"trivial\", \"huber\", \"cauchy\" or several with commas: each configuration under one after the other")
    ap.add_argument("--loss-scale", type=float, default=1.0)
    ap.add_argument("--loss-on", default="all", choices=["all", "switchable"])
    ap.add_argument("--no-restatement", action="store_true", help="leave the numpy context rows out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph_timing.json"))
    args = ap.parse_args()
    from ndt_2d_amd import PoseGraph, ScanMatcherNDT, _capi
    matcher = ScanMatcherNDT(0)
    rows, dense = [], []
    for n in [int(v) for v in args.sizes.split(",")]:
        g = loop_graph(n, seed=n)
        m = len(g["begin"])
        closures = np.nonzero(g["switchable"])[0]
        pg = PoseGraph(matcher, max_nodes=n, max_constraints=m, max_jobs=256)
        pg.set_graph(g["poses"], begin=g["begin"], end=g["end"], transform=g["transform"], information=g["information"],
                     switchable=g["switchable"])
        pg.set_timing(True)
        losses = args.loss.split(",") if args.loss else [None]   # (None: an object no loss was ever set on)
        for preconditioner, K, loss in [(p, int(v), ls) for v in args.masks.split(",") for p in args.preconditioner.split(",") for ls in losses]:
            pg.set_preconditioner(preconditioner)
            if loss is not None:
                pg.set_loss(loss, args.loss_scale, args.loss_on)
            rng = np.random.default_rng(1000 * n + K)
            masks = np.ones((K, m), dtype=np.uint8)
            for k in range(1, K):
                masks[k, closures[rng.random(len(closures)) < 0.5]] = 0
            kernel, wall = [], []
            for call in range(args.warmup + args.calls):
                t0 = time.perf_counter()
                jobs = pg.optimize(masks)
                t1 = time.perf_counter()
                if call >= args.warmup:
                    kernel.append(pg.last_ms()[0])
                    wall.append((t1 - t0) * 1e3)
                if t1 - t0 > 1.0:   # (a long call says so at once: a 10,000-pose solve takes seconds)
                    print("n %d masks %d call %d: %.1f s" % (n, K, call, t1 - t0), file=sys.stderr, flush=True)
            lm = [j["iterations"] for j in jobs]
            cg = [j["cg_iterations"] for j in jobs]
            row = dict(preconditioner=pg.preconditioner(), loss=loss or "trivial", us_per_cg_slowest_job=float(np.median(kernel)) * 1e3 / max(1, max(cg)),
                       n=n, m=m, closures=int(len(closures)), masks=K, calls=args.calls, warmup=args.warmup, kernel_ms_median=float(np.median(kernel)),
                       kernel_ms_min=float(np.min(kernel)), kernel_ms_max=float(np.max(kernel)), wall_ms_median=float(np.median(wall)),
                       lm_iterations_job0=lm[0], lm_iterations_max=int(max(lm)), cg_iterations_job0=cg[0], cg_iterations_max=int(max(cg)),
                       cg_per_lm_job0=cg[0] / max(1, lm[0]), status_job0=_capi.POSEGRAPH_STATUS_NAMES[jobs[0]["status"]],
                       statuses=sorted({_capi.POSEGRAPH_STATUS_NAMES[j["status"]] for j in jobs}),
                       cost_job0=[jobs[0]["initial_cost"], jobs[0]["final_cost"]], gradient_job0=jobs[0]["gradient"])
            rows.append(row)
            print(json.dumps(row), flush=True)
            write(args, rows, dense)
        pg.close()
        if n <= 1000 and not args.no_restatement:
            import posegraph_restatement as R
            P = R.Problem(g["poses"], g["begin"], g["end"], g["transform"], g["information"])
            t0 = time.perf_counter()
            ref = P.solve()
            row = dict(n=n, m=m, dense_wall_ms=(time.perf_counter() - t0) * 1e3, iterations=ref["iterations"], gradient=ref["gradient"],
                       cost=ref["cost"], note="numpy float64, dense H, np.linalg.solve, run to its |g| floor: context, not a rival")
            dense.append(row)
            print(json.dumps(row), flush=True)
    matcher.close()
    write(args, rows, dense)


if __name__ == "__main__":
    main()
