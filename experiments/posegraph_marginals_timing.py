"""Timing of the pose graph's marginal covariances (csrc/posegraph/, ndt2d_marginals_columns) on the
synthetic loops of experiments/posegraph_timing.py -> profiles/posegraph_marginals_timing.json.

A measurement script, not a test.  The graphs: posegraph_timing.loop_graph at N = 100 and 1,000,
solved once with the default tolerances; the solved poses are given to set_graph and the columns are
taken there.  K = 1 and 64 masks (the first with every constraint on, the others random over the
closures), Q = 1 and 16 query nodes spread over the free nodes, and at N = 1,000 with K = 1 every
node; both preconditioners, one after the other on the same object and session.  The object has
max_jobs = 1,024, so every row is one chunk and the HIP events (round the linearize and the columns
launch) cover the whole call.  Per row: the median over --calls calls after --warmup warm-ups of the
kernel time and of the call's wall time, the lockstep CG iterations (the largest over the queries)
and kernel time over them, and the statuses.  As context, not as a rival: the wall time of numpy's
dense inverse of H_FF on this machine's CPU at the same N.  No speed against the commit before is
claimed: it has nothing to compare.

    python experiments/posegraph_marginals_timing.py [--calls 10] [--warmup 3] [--sizes 100,1000]

The design's one unmeasured claim, three columns in lockstep in one workgroup against one column per
workgroup with three times the workgroups.  The library takes one or the other by the size of a
chunk (pg_marginals_form); --build-forms compiles the marginals unit twice more, with
-DNDT2D_MARGINALS_LOCKSTEP and -DNDT2D_MARGINALS_ONE_COLUMN, which force a form, and links
experiments/bin/libndt2d_hip_lockstep.so and libndt2d_hip_onecol.so from the library's other objects
(no GPU needed); --ab LABEL runs N = 1,000, K = 1 with --ab-queries query nodes and both
preconditioners on whichever library NDT2D_HIP_LIB names and puts the rows under "ab"[LABEL] of the
record, beside the rows above:

    python experiments/posegraph_marginals_timing.py --build-forms
    python experiments/posegraph_marginals_timing.py
    NDT2D_HIP_LIB=experiments/bin/libndt2d_hip_lockstep.so python experiments/posegraph_marginals_timing.py --ab lockstep --ab-queries 16,85,256,999
    NDT2D_HIP_LIB=experiments/bin/libndt2d_hip_onecol.so python experiments/posegraph_marginals_timing.py --ab one_column --ab-queries 16,85,256,999

The record's "ab"["lockstep_together"] and "ab"["one_column_together"] rows are of a third form, the
chain's factors applied to the live columns in one pass over the levels: measured once, decided
against and removed from the unit (DESIGN.md 3.18.3 names the commit that has it).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "experiments"))

from posegraph_timing import loop_graph  # noqa: E402


FORMS = {"lockstep": ["NDT2D_MARGINALS_LOCKSTEP"], "onecol": ["NDT2D_MARGINALS_ONE_COLUMN"]}


def build_forms():
    """The library with marginals_columns_kernel's form forced, once each way: the marginals unit
    compiled anew with the macro, every other object as the library's own build left it."""
    from concurrent.futures import ThreadPoolExecutor
    from ndt_2d_amd import build
    out_dir = os.path.join(ROOT, "experiments", "bin")
    os.makedirs(out_dir, exist_ok=True)
    unit = "posegraph/ndt2d_posegraph_marginals.hip"

    def compile_form(name):
        obj = os.path.join(out_dir, "ndt2d_posegraph_marginals_%s.o" % name)
        subprocess.check_call([build.hipcc(), "--offload-arch=" + build.ARCH] + build.FLAGS + ["-D" + v for v in FORMS[name]] +
                              ["-I", os.path.join(ROOT, "include"), "-I", build._CSRC, "-c", os.path.join(build._CSRC, unit), "-o", obj])
        return obj

    with ThreadPoolExecutor(max_workers=len(FORMS) + 1) as pool:
        main = pool.submit(build.build_all)
        objects = dict(zip(FORMS, pool.map(compile_form, FORMS)))
        main.result()
    if any(not os.path.exists(build._obj(s)) for s in build.SOURCES):
        build.build_all(force=True)
    libs = []
    for name, obj in objects.items():
        lib = os.path.join(out_dir, "libndt2d_hip_%s.so" % name)
        objs = [obj if s == unit else build._obj(s) for s in build.SOURCES + [build.BUILD_INFO_SOURCE]]
        subprocess.check_call([build.hipcc(), "--offload-arch=" + build.ARCH, "-shared", "-fPIC"] + objs + ["-ldl", "-lpthread", "-o", lib])
        libs.append(lib)
    return libs


def write(args, rows, dense):
    ab = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            ab = json.load(f).get("ab", {})
    if args.ab:
        with open(args.out) as f:
            out = json.load(f)
        out.setdefault("ab", {})[args.ab] = rows
        out["not_measured"] = [v for v in out["not_measured"] if not v.startswith("three columns in lockstep")]
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        return
    out = dict(ab=ab, what="marginals_linearize_kernel + marginals_columns_kernel, HIP events round the two launches; tolerance 1e-10, damping 0; "
                    "calls and warm-ups per row; one chunk per call",
               rows=rows, numpy_dense_inverse=dense,
               not_measured=([] if len(ab) >= 2 else ["three columns in lockstep against one column per workgroup (--ab was not run with both libraries)"]) +
                            ["every node at N = 1,000 with K = 64 (64,000 pairs: 4.6 GB of blocks alone)"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="100,1000")
    ap.add_argument("--no-dense", action="store_true", help="leave the numpy context rows out")
    ap.add_argument("--build-forms", action="store_true", help="build experiments/bin/libndt2d_hip_lockstep.so and libndt2d_hip_onecol.so and stop")
    ap.add_argument("--ab", default="", help="a label: run the A/B configuration only, on the library NDT2D_HIP_LIB names, into \"ab\"[label]")
    ap.add_argument("--ab-queries", default="16", help="the Q of the A/B rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph_marginals_timing.json"))
    args = ap.parse_args()
    if args.build_forms:
        print("\n".join(build_forms()))
        return
    if args.ab:
        args.sizes, args.no_dense = "1000", True
    from ndt_2d_amd import PoseGraph, ScanMatcherNDT, _capi
    matcher = ScanMatcherNDT(0)
    rows, dense = [], []
    for n in [int(v) for v in args.sizes.split(",")]:
        g = loop_graph(n, seed=n)
        m = len(g["begin"])
        closures = np.nonzero(g["switchable"])[0]
        pg = PoseGraph(matcher, max_nodes=n, max_constraints=m, max_jobs=1024)
        pg.set_graph(g["poses"], begin=g["begin"], end=g["end"], transform=g["transform"], information=g["information"], switchable=g["switchable"])
        solved = pg.optimize()[0]["poses"]
        pg.set_graph(solved, begin=g["begin"], end=g["end"], transform=g["transform"], information=g["information"], switchable=g["switchable"])
        pg.set_timing(True)
        configs = [(K, Q) for K in (1, 64) for Q in (1, 16)] + ([(1, n - 1)] if n >= 1000 else [])
        if args.ab:
            configs = [(1, int(v)) for v in args.ab_queries.split(",")]
        for K, Q in configs:
            nodes = np.unique(np.linspace(1, n - 1, Q).astype(int)) if Q < n - 1 else np.arange(1, n)
            rng = np.random.default_rng(1000 * n + K)
            masks = np.ones((K, m), dtype=np.uint8)
            for k in range(1, K):
                masks[k, closures[rng.random(len(closures)) < 0.5]] = 0
            for preconditioner in ("jacobi", "chain"):
                pg.set_preconditioner(preconditioner)
                kernel, wall = [], []
                for call in range(args.warmup + args.calls):
                    t0 = time.perf_counter()
                    jobs = pg.marginals(nodes, masks=masks)
                    t1 = time.perf_counter()
                    if call >= args.warmup:
                        kernel.append(pg.last_ms()[0])
                        wall.append((t1 - t0) * 1e3)
                its = max(int(np.max(j["cg_iterations"])) for j in jobs)
                row = dict(library=os.path.basename(_capi.LIB_PATH), n=n, m=m, masks=K, queries=int(len(nodes)), pairs=int(K * len(nodes)), preconditioner=pg.preconditioner(), calls=args.calls,
                           warmup=args.warmup, kernel_ms_median=float(np.median(kernel)), kernel_ms_min=float(np.min(kernel)),
                           kernel_ms_max=float(np.max(kernel)), wall_ms_median=float(np.median(wall)), lockstep_cg_iterations_max=its,
                           us_per_iteration=float(np.median(kernel)) * 1e3 / max(1, its),
                           statuses=sorted({_capi.MARGINALS_STATUS_NAMES[int(s)] for j in jobs for s in j["status"]}),
                           residual_max=float(max(np.max(j["residuals"]) for j in jobs)))
                rows.append(row)
                print(json.dumps(row), flush=True)
                write(args, rows, dense)
        pg.close()
        if not args.no_dense:
            import posegraph_marginals_restatement as MR
            import posegraph_restatement as R
            P = R.Problem(solved, g["begin"], g["end"], g["transform"], g["information"])
            S = MR.System(P, solved)
            t0 = time.perf_counter()
            inverse = np.linalg.inv(S.A)
            row = dict(n=n, unknowns=int(len(S.A)), dense_inverse_wall_ms=(time.perf_counter() - t0) * 1e3,
                       inverse_norm=float(np.max(np.sum(np.abs(inverse), axis=1))),
                       note="numpy float64, np.linalg.inv of the dense H_FF (every column at once), this machine's CPU: context, not a rival")
            dense.append(row)
            print(json.dumps(row), flush=True)
    matcher.close()
    write(args, rows, dense)


if __name__ == "__main__":
    main()
