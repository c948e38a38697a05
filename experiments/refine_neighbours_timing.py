"""Newton NDT registration with one cell per point against the 3 x 3 cells round it
(ndt2d_refine_set_neighbourhood), on the map and jobs of experiments/refine_timing.py: the 129 x 129
map, K in {1, 8, 64, 512} distinct 720-beam scans, 100 and 720 beams in use, each job from its own
pose a few centimetres off where its scan was taken.

    python experiments/refine_neighbours_timing.py [--parent-lib LIB.so] [OUT.json]

Every measurement runs in a child process of its own (one matcher per beam count, HIP events on):
per (beams, K, neighbourhood) the kernel time of REPS timed calls after WARM_UPS (median, minimum,
maximum), the mean evaluations, how the jobs stopped, and the refined poses' distance to the pose
the scan was taken at.  Both neighbourhoods are measured in the same child.

--parent-lib: a libndt2d_hip.so built from the parent commit.  Its one-cell kernel is then timed
against this tree's in alternating child processes (parent, this, parent, this, ...: ROUNDS each),
and the difference of the medians is set beside the spread of each library's own repeated rounds.
The parent library has no neighbourhood entry points: the children call ndt2d_matcher_refine_scans
itself, the same way for both libraries."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "experiments"))

KS = (1, 8, 64, 512)
BEAMS = (100, 720)
WARM_UPS, REPS, ROUNDS = 5, 20, 5
NEW_SYMBOLS = ("ndt2d_refine_set_neighbourhood", "ndt2d_refine_neighbourhood", "ndt2d_refine_covariance",
               "ndt2d_matcher_set_refine_neighbourhood", "ndt2d_matcher_refine_neighbourhood")


def child(out_path, cells_list):
    from ndt_2d_amd import _capi
    has_cells = hasattr(C.CDLL(_capi.LIB_PATH), NEW_SYMBOLS[0])
    if not has_cells:       # the parent's library: bind what it has
        for name in NEW_SYMBOLS:
            _capi.SIGNATURES.pop(name, None)
        assert cells_list == [1]
    import refine_timing as T
    from ndt_2d_amd import ScanMatcherNDT, synth

    world, scans = T.fixture_map()
    L = _capi.lib()
    f32 = C.c_float
    rows = []
    for beams in BEAMS:
        m = ScanMatcherNDT(0)
        m.initialize("refine-neighbours-timing", range_max=7.0, laser_max_beams=beams)
        m.addScans(scans)
        m.set_timing(False)
        rng = np.random.default_rng(20261019)
        truth = np.array(T.query_poses(world, 10.0, max(KS), rng))
        queries = [synth.scan(world, pose, 9900 + k) for k, pose in enumerate(truth)]
        off = rng.uniform(-0.03, 0.03, size=(len(truth), 3)) * np.array([1.0, 1.0, 0.5])
        jobs_all = truth + off
        for K in KS:
            jp = np.ascontiguousarray(jobs_all[:K])
            arrays = [np.ascontiguousarray(q, dtype=np.float64) for q in queries[:K]]
            offsets = np.zeros(K + 1, dtype=np.uintp)
            offsets[1:] = np.cumsum([len(a) for a in arrays])
            pts = np.ascontiguousarray(np.concatenate(arrays))
            poses, scores = np.zeros((K, 3)), np.zeros(K)
            status, evals = np.zeros(K, dtype=np.int32), np.zeros((K, 2), dtype=np.uint32)

            def call():
                rc = L.ndt2d_matcher_refine_scans(m._m, _capi.dptr(jp), None, K, _capi.dptr(pts),
                                                  offsets.ctypes.data_as(C.POINTER(C.c_size_t)), K, 32, 1e-6, 1e-6, _capi.dptr(poses),
                                                  _capi.dptr(scores), None, None, None, status.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  evals.ctypes.data_as(C.POINTER(C.c_uint32)))
                assert rc == _capi.OK, rc

            for cells in cells_list:
                if has_cells:
                    assert L.ndt2d_matcher_set_refine_neighbourhood(m._m, cells) == _capi.OK
                call()       # (makes the object)
                assert L.ndt2d_refine_set_timing(L.ndt2d_matcher_refine(m._m), 1) == _capi.OK
                for _ in range(WARM_UPS):
                    call()
                kernel = []
                for _ in range(REPS):
                    call()
                    k_ms, f_ms = f32(0), f32(0)
                    assert L.ndt2d_refine_last_ms(L.ndt2d_matcher_refine(m._m), C.byref(k_ms), C.byref(f_ms)) == _capi.OK
                    kernel.append(float(k_ms.value))
                dist = 1e3 * np.hypot(poses[:, 0] - truth[:K, 0], poses[:, 1] - truth[:K, 1])
                start = 1e3 * np.hypot(jp[:, 0] - truth[:K, 0], jp[:, 1] - truth[:K, 1])
                st = status.tolist()
                rows.append(dict(beams=beams, K=K, cells=cells, kernel_ms_median=float(np.median(kernel)), kernel_ms_min=min(kernel),
                                 kernel_ms_max=max(kernel), mean_evals=float(np.mean(evals[:, 0])),
                                 converged=st.count(_capi.REFINE_CONVERGED), max_evals=st.count(_capi.REFINE_MAX_EVALS),
                                 stalled=st.count(_capi.REFINE_STALLED), no_overlap=st.count(_capi.REFINE_NO_OVERLAP),
                                 start_mm_median=float(np.median(start)), refined_mm_median=float(np.median(dist)),
                                 refined_mm_max=float(np.max(dist))))
                print(json.dumps(rows[-1]), flush=True)
    with open(out_path, "w") as f:
        json.dump(dict(library=_capi.LIB_PATH, build_info=_capi.build_info(), rows=rows), f)


def run_child(tmp, tag, cells, lib=None):
    out = os.path.join(tmp, tag + ".json")
    env = dict(os.environ)
    env.pop("NDT2D_HIP_LIB", None)
    if lib:
        env["NDT2D_HIP_LIB"] = lib
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out, cells], check=True, env=env, timeout=400)
    with open(out) as f:
        return json.load(f)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        child(args[1], [int(v) for v in args[2].split(",")])
        return
    parent_lib = None
    if args and args[0] == "--parent-lib":
        parent_lib, args = os.path.abspath(args[1]), args[2:]
    path = args[0] if args else os.path.join(ROOT, "profiles", "refine_neighbours_timing.json")
    tmp = tempfile.mkdtemp(prefix="refine_neighbours_timing.")
    both = run_child(tmp, "both", "1,9")
    out = dict(experiment="refine_neighbours_timing", map="129 x 129", refine="max_evals 32, tol_lin 1e-6, tol_ang 1e-6",
               warm_ups=WARM_UPS, repetitions=REPS,
               note="kernel ms: HIP events round the one launch of a call; both neighbourhoods in one process",
               rows=both["rows"])
    print("beams K     cells kernel_ms (min .. max)        evals  converged  at_limit  start_mm  refined_mm (max)")
    for r in both["rows"]:
        print("%-5d %-5d %-5d %8.4f (%.4f .. %.4f) %8.1f %10d %9d %9.1f %11.1f (%.1f)" % (
            r["beams"], r["K"], r["cells"], r["kernel_ms_median"], r["kernel_ms_min"], r["kernel_ms_max"], r["mean_evals"],
            r["converged"], r["max_evals"], r["start_mm_median"], r["refined_mm_median"], r["refined_mm_max"]))
    if parent_lib:
        rounds = {"parent": [], "this": []}
        for k in range(ROUNDS):
            rounds["parent"].append(run_child(tmp, "parent%d" % k, "1", parent_lib)["rows"])
            rounds["this"].append(run_child(tmp, "this%d" % k, "1")["rows"])
        table = []
        print("one cell, parent against this tree: median kernel ms of each round")
        for i, r in enumerate(rounds["this"][0]):
            p = [rows[i]["kernel_ms_median"] for rows in rounds["parent"]]
            t = [rows[i]["kernel_ms_median"] for rows in rounds["this"]]
            same = all(rows[i]["mean_evals"] == r["mean_evals"] and rows[i]["converged"] == r["converged"]
                       for rows in rounds["parent"] + rounds["this"])
            spread = max(max(p) - min(p), max(t) - min(t))
            table.append(dict(beams=r["beams"], K=r["K"], parent_ms=p, this_ms=t, spread_ms=spread,
                              slower_by_ms=float(np.median(t) - np.median(p)), same_work=same))
            print("%-5d %-5d parent %s  this %s  spread %.4f  this - parent %+.4f %s" % (
                r["beams"], r["K"], " ".join("%.4f" % v for v in p), " ".join("%.4f" % v for v in t), spread,
                table[-1]["slower_by_ms"], "" if same else "(the jobs did not do the same work)"))
        out["one_cell_against_parent"] = dict(rounds=ROUNDS, order="parent, this, parent, this, ...", rows=table)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
