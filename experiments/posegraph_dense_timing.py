"""Timing of the dense covariance (csrc/covariance/, ndt2d_covariance_compute) beside the CG marginals
of every node (ndt2d_marginals_columns under "jacobi" and "chain") on the synthetic loops of
experiments/posegraph_timing.py -> profiles/posegraph_dense_timing.json.

A measurement script, not a test.  The graphs: posegraph_timing.loop_graph at N = 100 and 1,000 with
its own few closures (2 and 11) and with N / 3 of them (every lap-back closure the loop offers, thinned
evenly), solved once with the default tolerances; the solved poses are given to set_graph and both
paths run there, on one object, one after the other, in one session.  K = 1 and 64 masks (the first
with every constraint on, the others random over the closures).  Per row: medians over --calls calls
after --warmup warm-ups of the call's wall time (a host clock round a call that ends in a stream
synchronise) and of the HIP events round the launches of the call's LAST chunk, with the number of
chunks beside it.  One more row, dense only: the largest N whose job fits the default workspace.

The operations of the two update kernels (v_mfma_f64_16x16x4_f64) are counted from the plan as the
kernels run it -- 2 x 48^3 a block and panel -- and written into the record; their time comes from a
run of its own under a kernel trace (--dense-only --sizes 1000), never from
these rows.

    python experiments/posegraph_dense_timing.py [--calls 10] [--warmup 3] [--sizes 100,1000] [--masks 1,64] [--dense-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "experiments"))

from posegraph_timing import loop_graph  # noqa: E402

PANEL = 48


def graph_with(n, closures):
    """loop_graph(n) with its own closures (closures None) or with `closures` of the n / 2 it can have."""
    if closures is None:
        return loop_graph(n, seed=n)
    g = loop_graph(n, seed=n, every=1)
    sw = np.asarray(g["switchable"], dtype=bool)
    at = np.nonzero(sw)[0]
    keep = np.ones(len(sw), dtype=bool)
    keep[at] = False
    keep[at[np.unique(np.linspace(0, len(at) - 1, closures).astype(int))]] = True
    out = dict(g)
    for key in ("begin", "end", "transform", "information", "switchable"):
        out[key] = [v for v, k in zip(g[key], keep) if k]
    return out


def update_operations(n):
    """Floating-point operations of the two update kernels for n poses: blocks x 2 x 48^3."""
    np_ = -(-3 * n // PANEL)
    lower = sum((np_ - p - 1) * (np_ - p) // 2 for p in range(np_))
    rect = sum((np_ - p - 1) * (p + 1) for p in range(np_))
    return dict(panels=np_, update_blocks=lower, update_rect_blocks=rect, operations=2.0 * PANEL ** 3 * (lower + rect))


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
    ap.add_argument("--dense-only", action="store_true", help="leave the CG marginals out (a run under a kernel trace)")
    ap.add_argument("--no-largest", action="store_true")
    ap.add_argument("--masks", default="1,64", help="the K of the rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph_dense_timing.json"))
    args = ap.parse_args()
    from ndt_2d_amd import PoseGraph, ScanMatcherNDT, _capi
    from ndt_2d_amd.pose_graph import DEFAULT_COVARIANCE_WORKSPACE
    matcher = ScanMatcherNDT(0)
    rows, not_measured = [], []

    def write():
        out = dict(what="ndt2d_covariance_compute (every node's diagonal block, no pairs) beside ndt2d_marginals_columns (nodes = every free node, "
                        "tolerance 1e-10), damping 0; medians of the calls after the warm-ups; wall: a host clock round the call",
                   default_workspace_bytes=DEFAULT_COVARIANCE_WORKSPACE, rows=rows, not_measured=not_measured)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    def job_bytes(n):
        ld = -(-3 * n // PANEL) * PANEL
        return 8 * (2 * ld * ld + ld + 3 * n)

    def run(n, closures, Ks, dense_only, label):
        g = graph_with(n, closures)
        m = len(g["begin"])
        sw = np.nonzero(g["switchable"])[0]
        pg = PoseGraph(matcher, max_nodes=n, max_constraints=m, max_jobs=1024)
        pg.set_graph(g["poses"], begin=g["begin"], end=g["end"], transform=g["transform"], information=g["information"], switchable=g["switchable"])
        solved = pg.optimize()[0]["poses"]
        pg.set_graph(solved, begin=g["begin"], end=g["end"], transform=g["transform"], information=g["information"], switchable=g["switchable"])
        pg.set_timing(True)
        for K in Ks:
            rng = np.random.default_rng(1000 * n + K)
            masks = np.ones((K, m), dtype=np.uint8)
            for k in range(1, K):
                masks[k, sw[rng.random(len(sw)) < 0.5]] = 0
            base = dict(graph=label, n=n, m=m, closures=int(len(sw)), masks=K, calls=args.calls, warmup=args.warmup)
            workspaces = [DEFAULT_COVARIANCE_WORKSPACE]
            if K * job_bytes(n) > DEFAULT_COVARIANCE_WORKSPACE:
                workspaces.append(K * job_bytes(n))                                  # every job in one chunk
            for workspace in workspaces:
                got, t = timed(lambda: pg.covariances(masks=masks, workspace_bytes=workspace), args.calls, args.warmup, pg.covariance_last_ms)
                chunk = min(K, workspace // job_bytes(n))
                rows.append(dict(base, path="dense", workspace_bytes=int(workspace), job_bytes=job_bytes(n), chunks=-(-K // chunk),
                                 statuses=sorted({_capi.COVARIANCE_STATUS_NAMES[int(s)] for s in got["status"]}),
                                 pivot_ratio_min=float(np.min(got["pivot_ratio"])), **update_operations(n), **t))
                print(json.dumps(rows[-1]), flush=True)
                write()
            if dense_only:
                continue
            nodes = np.arange(1, n)
            if K * len(nodes) ** 2 * 72 > 2 << 30:
                not_measured.append("%s, K = %d: the CG marginals of every node (blocks_out alone is %.1f GB)" % (label, K, K * len(nodes) ** 2 * 72 / 1e9))
                continue
            for preconditioner in ("jacobi", "chain"):
                pg.set_preconditioner(preconditioner)
                jobs, t = timed(lambda: pg.marginals(nodes, masks=masks), args.calls, args.warmup, pg.last_ms)
                rows.append(dict(base, path="cg " + preconditioner, chunks=-(-K * len(nodes) // 1024),
                                 statuses=sorted({_capi.MARGINALS_STATUS_NAMES[int(s)] for j in jobs for s in j["status"]}),
                                 lockstep_cg_iterations_max=max(int(np.max(j["cg_iterations"])) for j in jobs), **t))
                print(json.dumps(rows[-1]), flush=True)
                write()
        pg.close()

    for n in [int(v) for v in args.sizes.split(",")]:
        Ks = tuple(int(v) for v in args.masks.split(","))
        run(n, None, Ks, args.dense_only, "loop_%d" % n)
        run(n, n // 3, Ks, args.dense_only, "loop_%d_third" % n)
    if not args.no_largest:
        largest = 1
        while job_bytes(largest + 1) <= DEFAULT_COVARIANCE_WORKSPACE:
            largest += 1
        run(largest, None, (1,), True, "loop_%d_largest" % largest)
    matcher.close()
    write()


if __name__ == "__main__":
    main()
