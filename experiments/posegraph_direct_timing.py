"""Timing of the direct pose-graph solve (ndt2d_direct_solve, PoseGraph.optimize_direct) beside the CG
solver (ndt2d_posegraph_solve, PoseGraph.optimize under "jacobi" and "chain") on the synthetic loops
of experiments/posegraph_timing.py -> profiles/posegraph_direct_timing.json.

A measurement script, not a test.  The graphs: posegraph_timing.loop_graph at N = 100 and 1,000 with
its own few closures (2 and 11) and with N / 3 of them (posegraph_dense_timing.graph_with); K = 1 and
64 masks (the first with every constraint on, the others random over the closures); Ceres's default
tolerances.  The three solvers run one after the other on the same object, masks and session.  Per
row: medians over --calls calls after --warmup warm-ups of the call's wall time (a host clock round a
call that ends in a stream synchronise) and of the HIP-event time of the call's LAST chunk -- for the
direct solve that is its iterations with the read-backs between them -- with the jobs' LM
iterations, rejected steps and, for the CG rows, CG iterations.

    python experiments/posegraph_direct_timing.py [--calls 10] [--warmup 3] [--sizes 100,1000] [--masks 1,64]

--direct-only leaves the CG rows out (a run under rocprofv3 --kernel-trace for the per-kernel split of
a direct iteration); --workspace-gb sets optimize_direct's workspace (default: the package's 1 GiB)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "experiments"))

from posegraph_dense_timing import graph_with  # noqa: E402


def timed(call, calls, warmup, last_ms):
    kernel, wall = [], []
    for k in range(warmup + calls):
        t0 = time.perf_counter()
        got = call()
        t1 = time.perf_counter()
        if k >= warmup:
            kernel.append(last_ms()[0])
            wall.append((t1 - t0) * 1e3)
    return got, dict(wall_ms_median=float(np.median(wall)), wall_ms_min=float(np.min(wall)), wall_ms_max=float(np.max(wall)),
                     last_chunk_kernel_ms_median=float(np.median(kernel)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="100,1000")
    ap.add_argument("--masks", default="1,64")
    ap.add_argument("--direct-only", action="store_true")
    ap.add_argument("--workspace-gb", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph_direct_timing.json"))
    args = ap.parse_args()
    from ndt_2d_amd import PoseGraph, ScanMatcherNDT, _capi
    from ndt_2d_amd.pose_graph import DEFAULT_DIRECT_WORKSPACE
    workspace = int(args.workspace_gb * 2 ** 30) if args.workspace_gb > 0.0 else DEFAULT_DIRECT_WORKSPACE
    matcher = ScanMatcherNDT(0)
    rows = []

    def write():
        out = dict(what="PoseGraph.optimize_direct beside PoseGraph.optimize (\"jacobi\", \"chain\") on the same object, masks and session; "
                        "default (Ceres) tolerances; medians; wall: host clock round the call; kernel: HIP events round the last chunk",
                   calls=args.calls, warmup=args.warmup, direct_workspace_bytes=workspace, rows=rows)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    for n in [int(v) for v in args.sizes.split(",")]:
        for closures in (None, n // 3):
            g = graph_with(n, closures)
            m = len(g["begin"])
            at = np.nonzero(np.asarray(g["switchable"], dtype=bool))[0]
            pg = PoseGraph(matcher, max_nodes=n, max_constraints=m, max_jobs=64)
            pg.set_graph(g["poses"], begin=g["begin"], end=g["end"], transform=g["transform"], information=g["information"],
                         switchable=g["switchable"])
            pg.set_timing(True)
            for K in [int(v) for v in args.masks.split(",")]:
                rng = np.random.default_rng(1000 * n + K)
                masks = np.ones((K, m), dtype=np.uint8)
                for k in range(1, K):
                    masks[k, at[rng.random(len(at)) < 0.5]] = 0
                paths = [("direct", None)] + ([] if args.direct_only else [("CG jacobi", "jacobi"), ("CG chain", "chain")])
                for path, preconditioner in paths:
                    if preconditioner is None:
                        jobs, t = timed(lambda: pg.optimize_direct(masks, workspace_bytes=workspace), args.calls, args.warmup, pg.direct_last_ms)
                    else:
                        pg.set_preconditioner(preconditioner)
                        jobs, t = timed(lambda: pg.optimize(masks), args.calls, args.warmup, pg.last_ms)
                    lm = [j["iterations"] for j in jobs]
                    row = dict(n=n, m=m, closures=int(len(at)), masks=K, path=path, lm_iterations_job0=lm[0], lm_iterations_max=int(max(lm)),
                               status_job0=_capi.POSEGRAPH_STATUS_NAMES[jobs[0]["status"]],
                               statuses=sorted({_capi.POSEGRAPH_STATUS_NAMES[j["status"]] for j in jobs}),
                               cost_job0=[jobs[0]["initial_cost"], jobs[0]["final_cost"]], gradient_job0=jobs[0]["gradient"], **t)
                    if preconditioner is None:
                        row.update(rejected_job0=jobs[0]["rejected"], rejected_max=int(max(j["rejected"] for j in jobs)),
                                   not_positive_definite_max=int(max(j["not_positive_definite"] for j in jobs)))
                    else:
                        row.update(cg_iterations_job0=jobs[0]["cg_iterations"], cg_iterations_max=int(max(j["cg_iterations"] for j in jobs)))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    write()
            pg.close()
    matcher.close()
    write()


if __name__ == "__main__":
    main()
