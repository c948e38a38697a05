#!/usr/bin/env python3
"""The mapper's per-scan NDT build, four ways, in one session on one GPU: build modes "host",
"device" and "fused" of addScans, and addScansById on resident scans -- wall time of the whole
add_scans call and of the per-scan cycle (reset + addScans + scoreScan + matchScan, reference
src/ndt_mapper.cpp:508-515), on the 41 x 41 map (cfg-1) and on a 30 m lidar's 245 x 245 map, both
of 6,480 points.  The C entry points are called with arrays packed once, event timing off, as the
pluginlib shim calls them.  Medians over --iters calls after --warmup.

    python experiments/fused_build_timing.py [--iters 400] [--warmup 40] [--out profiles/fused_build_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ndt_2d_amd import ScanMatcherNDT, _capi, synth  # noqa: E402
from ndt_2d_amd.scan_matcher import _pack_scans  # noqa: E402

DEFAULT_SEARCH = dict(search_linear_size=0.05, search_linear_resolution=0.005, search_angular_size=0.1,
                      search_angular_resolution=0.0025, laser_max_beams=100)


def maps():
    guess, pts, _ = synth.query_scan(1)
    yield "41x41", synth.map_scans(1), synth.matcher_params(1, **DEFAULT_SEARCH), guess, pts
    w = synth.world_of(5)
    true = synth.query_scan(5)[2]
    scans = []
    for j in range(3):
        for i in range(3):
            x, y = true[0] + (i - 1) * 0.5, true[1] + (j - 1) * 0.5
            scans.append(((x, y, 0.0), synth.scan(w, (x, y, 0.0), 77 + 10 * j + i)))
    params = dict(synth.matcher_params(5, **DEFAULT_SEARCH), range_max=30.0)
    yield "245x245", scans, params, true + np.array([0.02, -0.02, 0.01]), synth.query_scan(5)[1]


def stats(us):
    us = np.sort(np.asarray(us))
    return dict(median_us=round(float(np.median(us)), 2), p10_us=round(float(us[len(us) // 10]), 2),
                p90_us=round(float(us[(9 * len(us)) // 10]), 2))


def measure(name, scans, params, guess, pts, way, iters, warmup):
    L = _capi.lib()
    m = ScanMatcherNDT(0)
    m.initialize(name, **params)
    m.set_timing(False)
    m.set_build_mode("fused" if way == "fused-by-id" else way)
    poses, allpts, offsets = _pack_scans(scans)
    off_p = offsets.ctypes.data_as(C.POINTER(C.c_size_t))
    ids = np.arange(len(scans), dtype=np.uint64)
    ids_p = ids.ctypes.data_as(C.POINTER(C.c_size_t))
    if way == "fused-by-id":
        for s in scans:
            m.storeScan(s[1])
    sp = np.ascontiguousarray(guess, dtype=np.float64)
    qp = np.ascontiguousarray(pts, dtype=np.float64)
    pose_io, cov = np.zeros(3), np.zeros(9)
    score = C.c_double(0.0)

    def add():
        if way == "fused-by-id":
            rc = L.ndt2d_matcher_add_scans_by_id(m._m, _capi.dptr(poses), ids_p, len(scans))
        else:
            rc = L.ndt2d_matcher_add_scans(m._m, _capi.dptr(poses), _capi.dptr(allpts), off_p, len(scans))
        assert rc == 0, L.ndt2d_matcher_last_error(m._m)

    t_add, t_cycle = [], []
    for it in range(warmup + iters):
        L.ndt2d_matcher_reset(m._m)
        t0 = time.perf_counter()
        add()
        t1 = time.perf_counter()
        if it >= warmup:
            t_add.append((t1 - t0) * 1e6)
    build_variant = m.last_variant()
    for it in range(warmup + iters):
        t0 = time.perf_counter()
        L.ndt2d_matcher_reset(m._m)
        add()
        assert L.ndt2d_matcher_score_scan(m._m, _capi.dptr(sp), _capi.dptr(qp), len(qp), C.byref(score)) == 0
        assert L.ndt2d_matcher_match_scan(m._m, _capi.dptr(sp), _capi.dptr(qp), len(qp), _capi.dptr(pose_io),
                                          _capi.dptr(cov), C.byref(score)) == 0
        t1 = time.perf_counter()
        if it >= warmup:
            t_cycle.append((t1 - t0) * 1e6)
    out = dict(add_scans=stats(t_add), cycle=stats(t_cycle), build_variant=build_variant, match_score=score.value,
               match_pose=[float(v) for v in pose_io])
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_build_timing.json"))
    a = ap.parse_args()
    result = dict(build=_capi.build_info(), iters=a.iters, warmup=a.warmup, maps={})
    for name, scans, params, guess, pts in maps():
        n_points = int(sum(len(s[1]) for s in scans))
        entry = dict(n_scans=len(scans), n_points=n_points, ways={})
        for way in ("host", "device", "fused", "fused-by-id"):
            entry["ways"][way] = measure(name, scans, params, guess, pts, way, a.iters, a.warmup)
            r = entry["ways"][way]
            print("%-8s %-12s add_scans %7.1f us   cycle %7.1f us   (%s)" %
                  (name, way, r["add_scans"]["median_us"], r["cycle"]["median_us"], r["build_variant"]), flush=True)
        poses = {tuple(w["match_pose"]) for w in entry["ways"].values()}
        assert len(poses) == 1, poses        # the four ways match the scan to the same pose
        result["maps"][name] = entry
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
