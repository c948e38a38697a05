"""Timing of the sparse covariance (ndt2d_sparsecov_compute, PoseGraph.covariances_sparse) beside the dense
covariance (PoseGraph.covariances) and the CG marginals under "chain" (PoseGraph.marginals) on the
synthetic loops of experiments/posegraph_sparse_timing.py -> profiles/posegraph_sparsecov_timing.json.

A measurement script, not a test.  The graphs: posegraph_timing.loop_graph at 1,000 poses with its own
11 closures and with 333 (posegraph_dense_timing.graph_with), and at 10,000 poses with its own 101; one
mask, every constraint on, at the graph's poses, damping 0.  The paths run one after the other on the same
object and session: covariances_sparse for the diagonal alone and for the diagonal with 16 pairs (8 nodes
spread over the graph: for four of them (a, a + 2) and (a + 2, a), two nodes of one segment wherever neither
is a separator, each a column pass of its own; for the others a far node, both ways round), covariances
(dense) with the same pairs, marginals for 16 nodes.  A refusal
is a row.  Per row: medians over --calls calls after --warmup warm-ups of the call's wall time (a host
clock round a call that ends in a stream synchronise) and of the HIP-event time of the call's last chunk.

    python experiments/posegraph_sparsecov_timing.py [--calls 10] [--warmup 3] [--graphs 1000:,1000:333,10000:]

--sparse-only leaves the other paths out: a run of its own under
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python experiments/posegraph_sparsecov_timing.py --sparse-only ...
after which --shares DIR (no GPU) reads the trace and adds each kernel's share of the traced kernel
time to the JSON."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "experiments"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--graphs", default="1000:,1000:333,10000:")
    ap.add_argument("--sparse-only", action="store_true")
    ap.add_argument("--shares", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph_sparsecov_timing.json"))
    args = ap.parse_args()
    from posegraph_sparse_timing import shares, timed
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
    from ndt_2d_amd import Ndt2dError, PoseGraph, ScanMatcherNDT
    matcher = ScanMatcherNDT(0)
    rows = []

    def write():
        out = dict(what="PoseGraph.covariances_sparse beside covariances (dense) and marginals (\"chain\") on the same object and session; "
                        "one mask, the graph's poses, damping 0; medians; wall: host clock round the call; kernel: HIP events round the last chunk",
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
        nodes = [int(v) for v in np.linspace(1, n - 1, 8)]
        pairs = [p for a in nodes[:4] for p in ((a, a + 2), (a + 2, a))] + [p for a, b in zip(nodes[4:], nodes[:4]) for p in ((a, b), (b, a))]
        queries = [int(v) for v in np.linspace(1, n - 1, 16)]
        paths = [("sparse, the diagonal", lambda: pg.covariances_sparse(), pg.sparsecov_last_ms),
                 ("sparse, the diagonal and 16 pairs", lambda: pg.covariances_sparse(pairs=pairs), pg.sparsecov_last_ms)]
        if not args.sparse_only:
            paths += [("dense, the diagonal and 16 pairs", lambda: pg.covariances(pairs=pairs), pg.covariance_last_ms),
                      ("CG chain, 16 nodes", lambda: pg.marginals(queries), pg.last_ms)]
        for path, call, last_ms in paths:
            row = dict(n=n, m=m, closures=int(np.count_nonzero(g["switchable"])), separators=layout["separators"], path=path)
            try:
                got, t = timed(call, args.calls, args.warmup, last_ms)
            except Ndt2dError as e:
                row.update(refused=str(e))
            else:
                row.update(**t)
                if isinstance(got, dict):
                    row.update(status=int(got["status"][0]), pivot_ratio=float(got["pivot_ratio"][0]))
                else:
                    row.update(cg_iterations_median=float(np.median(got[0]["cg_iterations"])), cg_iterations_max=int(np.max(got[0]["cg_iterations"])))
            rows.append(row)
            print(json.dumps(row), flush=True)
            write()
        pg.close()
    matcher.close()
    write()


if __name__ == "__main__":
    main()
