"""Wide search against the existing large search on the same lattice, same machine, same run.

    python experiments/wide_search_timing.py [--reps 5] [--out profiles/wide_search_timing.json]

Cases: cfg-4's lattice (+-5 m / 0.02 m, +-pi / 0.005 rad on the cfg-1 map) and a +-2 m / 0.02 m,
+-0.5 rad / 0.005 rad lattice on the cfg-1 and cfg-3 maps at 100 and 720 beams.  Per case: the
existing search (ScanMatcherNDT.matchScan, whole call, wall clock) and, for tile steps T in
{4, 8, 16} x pixels per tile in {1, 2, 4}, the wide search (WideSearch.match on the matcher's
context with the same subsampled beams, whole call, wall clock: once with the bound image kept and
once with it made in every call) with its stages from the HIP events and the share of tiles scored.
same_winner: the winner is the existing search's.  same_score compares the score's bits with the
EXISTING LARGE search's, which sums a candidate's beams in another order than the batched searches'
lane: false is the expected answer there (the bit-for-bit yardstick is ndt2d_starts_match,
tests/test_gpu_wide.py).  Medians over --reps calls."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ndt_2d_amd import Ndt2dError, ScanMatcherNDT, WideSearch, search_offsets, synth  # noqa: E402


def median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def subsample(points, n):
    step = len(points) / n
    return np.ascontiguousarray([points[int(i * step)] for i in range(n)])


def run_case(name, cfg, lattice, n_beams, reps, out):
    lin_size, lin_res, ang_size, ang_res = lattice
    pose, points = synth.query_scan(cfg)[:2]
    m = ScanMatcherNDT(0)
    m.initialize(name, **synth.matcher_params(cfg, search_linear_size=lin_size, search_linear_resolution=lin_res,
                                              search_angular_size=ang_size, search_angular_resolution=ang_res,
                                              laser_max_beams=n_beams))
    m.addScans(synth.map_scans(cfg))
    dth, dlin = search_offsets(ang_size, ang_res), search_offsets(lin_size, lin_res)
    beams = subsample(points, min(n_beams, len(points)))
    want = m.matchScan(pose, points)
    variant = m.last_variant()
    exhaustive_ms = median_ms(lambda: m.matchScan(pose, points), reps)
    base = dict(case=name, cfg=cfg, grid=list(m.grid()[1:3]), n_beams=len(beams), n_th=len(dth), n_lin=len(dlin),
                candidates=len(dth) * len(dlin) ** 2, exhaustive_ms=exhaustive_ms, exhaustive_variant=variant)
    print(json.dumps(base), flush=True)
    out.append(base)
    wide = WideSearch(m)
    for tile_steps in (4, 8, 16):
        for pixels in (1, 2, 4):
            row = dict(case=name, tile_steps=tile_steps, pixels_per_tile=pixels)
            wide.set_tile(tile_steps, pixels)
            try:
                wide.set_timing(True)
                first = wide.match(pose, beams, dth, dlin)             # makes the image
                image_ms = wide.last_ms()[0]
                wide.match(pose, beams, dth, dlin, reuse_image=True)
                stages = wide.last_ms()
                wide.set_timing(False)
                kept_ms = median_ms(lambda: wide.match(pose, beams, dth, dlin, reuse_image=True), reps)
                rebuilt_ms = median_ms(lambda: wide.match(pose, beams, dth, dlin), reps)
            except Ndt2dError as e:
                row["refused"] = str(e)
                print(json.dumps(row), flush=True)
                out.append(row)
                continue
            row.update(wide_ms_image_kept=kept_ms, wide_ms_image_rebuilt=rebuilt_ms, image_ms=image_ms, bounds_ms=stages[1],
                       sort_ms=stages[2], rounds_ms=stages[3], tiles_scored=first["tiles_scored"], tiles_total=first["tiles_total"],
                       share_scored=first["tiles_scored"] / first["tiles_total"],
                       same_winner=bool(first["best_index"] == want["best_index"]),
                       same_score=bool(first["best_score"] / len(beams) == want["score"]),
                       near_tie=first["near_tie"], exhaustive_over_wide=exhaustive_ms / kept_ms)
            print(json.dumps(row), flush=True)
            out.append(row)
    wide.close()
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "wide_search_timing.json"))
    ap.add_argument("--cases", default="cfg4,cfg1-100,cfg1-720,cfg3-100,cfg3-720")
    a = ap.parse_args()
    c4 = synth.CONFIGS[4]["search"]
    mid = (2.0, 0.02, 0.5, 0.005)
    cases = {"cfg4": (4, (c4["search_linear_size"], c4["search_linear_resolution"], c4["search_angular_size"],
                          c4["search_angular_resolution"]), synth.matcher_params(4)["laser_max_beams"]),
             "cfg1-100": (1, mid, 100), "cfg1-720": (1, mid, 720), "cfg3-100": (3, mid, 100), "cfg3-720": (3, mid, 720)}
    out = []
    for name in a.cases.split(","):
        cfg, lattice, n_beams = cases[name]
        run_case(name, cfg, lattice, n_beams, a.reps, out)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device="MI355X", reps=a.reps, rows=out), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
