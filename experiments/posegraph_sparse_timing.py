"""Timing of the sparse pose-graph solve (ndt2d_sparse_solve, PoseGraph.optimize_sparse) beside the
direct solve (PoseGraph.optimize_direct) and the CG solver under "chain" (PoseGraph.optimize) on the
synthetic loops of experiments/posegraph_timing.py -> profiles/posegraph_sparse_timing.json.

A measurement script, not a test.  The graphs: posegraph_timing.loop_graph at 1,000 poses with its own
11 closures and with 333 (posegraph_dense_timing.graph_with), and at 10,000 poses with its own 101,
where the direct solve's refusal is recorded as such; one mask, every constraint on; Ceres's default
tolerances.  The three solvers run one after the other on the same object, mask and session.  Per row:
medians over --calls calls after --warmup warm-ups of the call's wall time (a host clock round a call
that ends in a stream synchronise) and of the HIP-event time of the call's last chunk, the LM
iterations, the status, ms per LM iteration (the events' time over the iterations), and for the sparse
rows the separators s.

    python experiments/posegraph_sparse_timing.py [--calls 10] [--warmup 3] [--graphs 1000:,1000:333,10000:]

--sparse-only leaves the other two out: a run of its own under
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python experiments/posegraph_sparse_timing.py --sparse-only ...
after which --shares DIR (no GPU) reads the trace and adds each kernel's share of the traced kernel
time to the JSON."""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "experiments"))


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


def shares(trace_dir):
    """Each kernel's count, total microseconds and share of the traced kernel time, out of rocprofv3's kernel_trace.csv."""
    by = defaultdict(list)
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name") or row.get("Name") or ""
                found = re.search(r"(\w+_kernel)", name)
                short = found.group(1) if found else name[:60]
                if found and "<" in name:
                    short += "<" + name.split("<", 1)[1].split(">")[0] + ">"
                by[short].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0)
    total = sum(sum(v) for v in by.values())
    return [dict(kernel=k, launches=len(v), total_us=round(sum(v), 1), median_us=round(float(np.median(v)), 2), share=round(sum(v) / total, 4))
            for k, v in sorted(by.items(), key=lambda kv: -sum(kv[1]))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--graphs", default="1000:,1000:333,10000:")
    ap.add_argument("--sparse-only", action="store_true")
    ap.add_argument("--shares", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph_sparse_timing.json"))
    args = ap.parse_args()
    if args.shares:
        with open(args.out) as f:
            out = json.load(f)
        out["kernel_shares"] = dict(what="one run of its own under rocprofv3 --kernel-trace, --sparse-only: every kernel of the process",
                                    kernels=shares(args.shares))
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        return
    from posegraph_dense_timing import graph_with
    from ndt_2d_amd import Ndt2dError, PoseGraph, ScanMatcherNDT, _capi
    matcher = ScanMatcherNDT(0)
    rows = []

    def write():
        out = dict(what="PoseGraph.optimize_sparse beside optimize_direct and optimize (\"chain\") on the same object, mask and session; "
                        "default (Ceres) tolerances; medians; wall: host clock round the call; kernel: HIP events round the last chunk",
                   calls=args.calls, warmup=args.warmup, rows=rows)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    for spec in args.graphs.split(","):
        n, closures = spec.split(":")
        n, closures = int(n), int(closures) if closures else None
        g = graph_with(n, closures)
        m = len(g["begin"])
        pg = PoseGraph(matcher, max_nodes=n, max_constraints=m, max_jobs=1)
        pg.set_graph(g["poses"], begin=g["begin"], end=g["end"], transform=g["transform"], information=g["information"], switchable=g["switchable"])
        pg.set_timing(True)
        pg.set_preconditioner("chain")
        layout = pg.sparse_layout()
        paths = [("sparse", pg.optimize_sparse, pg.sparse_last_ms)]
        if not args.sparse_only:
            paths += [("direct", pg.optimize_direct, pg.direct_last_ms), ("CG chain", pg.optimize, pg.last_ms)]
        for path, call, last_ms in paths:
            row = dict(n=n, m=m, closures=int(np.count_nonzero(g["switchable"])), path=path)
            try:
                jobs, t = timed(call, args.calls, args.warmup, last_ms)
            except Ndt2dError as e:
                row.update(refused=str(e))
            else:
                job = jobs[0]
                row.update(lm_iterations=job["iterations"], status=_capi.POSEGRAPH_STATUS_NAMES[job["status"]],
                           cost=[job["initial_cost"], job["final_cost"]], gradient=job["gradient"],
                           ms_per_lm_iteration=t["last_chunk_kernel_ms_median"] / max(1, job["iterations"]), **t)
                if path == "CG chain":
                    row.update(cg_iterations=job["cg_iterations"])
                else:
                    row.update(rejected=job["rejected"], not_positive_definite=job["not_positive_definite"], pivot_ratio=job["pivot_ratio"])
                if path == "sparse":
                    row.update(separators=layout["separators"], interior=layout["interior"])
            rows.append(row)
            print(json.dumps(row), flush=True)
            write()
        pg.close()
    matcher.close()
    write()


if __name__ == "__main__":
    main()
