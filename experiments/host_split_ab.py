"""profiles/<NAME>.json (NAME: host_split_ab unless given): ndt_2d_amd/tools/latency_probe.c linked against the parent commit's library
and against the tree's, run in turn in one session (parent1, branch1, parent2, ...), each run's JSON
line kept as DIR/probe_<run>.json.

    python experiments/host_split_ab.py DIR [NAME] > profiles/NAME.json

The margin of a figure is the spread the parent shows against itself; a branch figure above the
parent's highest on a majority of the branch runs is a regression."""
import json
import os
import sys

COLUMNS = [("match_scan_us", None), ("mapper_cycle_us", None), ("mapper_cycle_p99_us", None),
           ("measure_500_particles_unchanged_loop_us", None), ("pf_measure_500_particles_us", None),
           ("add_scans_us", None), ("add_scans_us", "real_lidar_map"), ("match_scan_us", "real_lidar_map"),
           ("mapper_cycle_us", "real_lidar_map")]


def main(where, experiment="host_split_ab"):
    runs = {}
    for name in sorted(os.listdir(where)):
        if name.startswith("probe_") and name.endswith(".json"):
            with open(os.path.join(where, name)) as f:
                runs[name[len("probe_"):-len(".json")]] = json.loads(f.read().strip().splitlines()[-1])
    parents = sorted(k for k in runs if k.startswith("parent"))
    branches = sorted(k for k in runs if k.startswith("branch"))
    rows = []
    for col, sub in COLUMNS:
        vals = {k: (v[sub][col] if sub else v[col]) for k, v in runs.items()}
        lo, hi = min(vals[k] for k in parents), max(vals[k] for k in parents)
        slow = [k for k in branches if vals[k] > hi]
        rows.append({"column": (sub + "." if sub else "") + col, "values": vals, "parent_lo": lo, "parent_hi": hi,
                     "branch_runs_above_every_parent_run": slow,
                     "verdict": "regression" if 2 * len(slow) > len(branches) else "within the parent's own spread"})
    json.dump({"experiment": experiment,
               "what": "latency_probe.c (bench.py's default-search settings) against the parent's library and the tree's, "
                       "in turn, one session, one MI355X; microseconds",
               "rule": "margin = the spread of the parent's own runs; a branch figure above the parent's highest on a "
                       "majority of the branch runs is a regression",
               "runs": sorted(runs), "rows": rows}, sys.stdout, indent=1)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main(*sys.argv[1:3])
