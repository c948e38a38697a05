"""A/B of the batched calls between two builds of the library, from the JSON files the timing
scripts write: the parent and the branch in turn, in one session on one GPU.

    for tag in parent1 branch1 parent2 branch2 parent3; do      # NDT2D_HIP_LIB: the parent's library
        for s in starts scans closure; do
            NDT2D_HIP_LIB=... python experiments/${s}_batch_timing.py DIR/$tag.$s.json
        done
        for s in refine verify closure_refine closure_verify; do
            NDT2D_HIP_LIB=... python experiments/${s}_timing.py DIR/$tag.$s.json
        done
    done
    python experiments/batch_ab_summary.py DIR [OUT.json [NOTE]]    # default: profiles/batch_refactor_ab.json

The yardsticks are each script's wall time per call and its kernel time (COLUMNS; the scripts whose
files are in DIR are judged).  The rule: a value passes where it lies within the
range of parent1 and parent2 widened by that same range on either side -- two parent runs are
the only margin.  It is applied to every branch run, and, as a control of what the rule makes of
run-to-run spread alone, to every further PARENT run (parent3, ...) in the same way: a parent
judged against two other runs of itself.  Every row names all the runs."""
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# script -> the columns judged: kernel (or launch) time in ms, wall time per call.  A column that
# holds a spread {median, min, max} is judged by its median.
COLUMNS = {"starts": ("search_ms", "batched_us"), "scans": ("search_ms", "batched_us"), "closure": ("search_ms", "batched_us"),
           "refine": ("kernel_ms", "refine_us"), "verify": ("kernel_ms", "call_wall_ms"),
           "closure_refine": ("refine_kernel_ms", "call_ms"), "closure_verify": ("verify_launch_ms", "call_wall_ms")}
# what names a row within its table
ROW_KEYS = ("map_cells", "beams", "cells", "rays", "K", "jobs", "candidates")


def tables(path, unnamed=""):
    """[(table name, rows)] of one timing file; unnamed: the name of a file's one table."""
    with open(path) as f:
        doc = json.load(f)
    if "maps" in doc:
        return [(m["map"], m["rows"]) for m in doc["maps"]]
    if "runs" in doc:
        return [("%d beams" % r["beams"], r["rows"]) for r in doc["runs"]]
    return [(unnamed, doc["rows"])]


def figure(value):
    return value["median"] if isinstance(value, dict) else value


def verdict(value, lo, hi):
    return "within" if lo - (hi - lo) <= value <= hi + (hi - lo) else "slower" if value > hi else "faster"


def main(directory, path=None, note=None):
    tags = sorted({os.path.basename(p).split(".")[0] for p in glob.glob(os.path.join(directory, "*.starts.json"))})
    judged = [t for t in tags if t not in ("parent1", "parent2")]
    path = path or os.path.join(ROOT, "profiles", "batch_refactor_ab.json")
    out = dict(experiment=os.path.splitext(os.path.basename(path))[0], runs=tags, session="the runs in turn, one session, one MI355X",
               rule="within: lo - (hi - lo) <= value <= hi + (hi - lo), lo / hi of parent1 and parent2; "
                    "applied to the branch runs and, as the control, to the further parent runs", rows=[])
    if note:
        out["note"] = note
    count = {t: dict(within=0, slower=0, faster=0) for t in judged}
    for script, columns in COLUMNS.items():
        if not os.path.exists(os.path.join(directory, "parent1.%s.json" % script)):
            continue
        runs = {t: tables(os.path.join(directory, "%s.%s.json" % (t, script)), "two-scan candidate maps" if script == "closure" else "")
                for t in tags}
        for i, (name, rows) in enumerate(runs["parent1"]):
            for j, row in enumerate(rows):
                K = row.get("K", row.get("jobs", row.get("candidates")))
                label = {key: row[key] for key in ROW_KEYS if key in row}
                for column in columns:
                    values = {t: figure(runs[t][i][1][j][column]) for t in tags}
                    lo, hi = sorted((values["parent1"], values["parent2"]))
                    verdicts = {t: verdict(values[t], lo, hi) for t in judged}
                    for t in judged:
                        count[t][verdicts[t]] += 1
                    out["rows"].append(dict(script=script, map=name, K=K, row=label, column=column, values=values, verdicts=verdicts))
                    print("%-14s %-24s %-40s %-16s %s" % (script, name, json.dumps(label), column, "  ".join(
                        "%s %.4f%s" % (t, values[t], " (" + verdicts[t] + ")" if t in verdicts else "") for t in tags)))
    out["counts"] = count
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote %s: %s" % (path, json.dumps(count)))


if __name__ == "__main__":
    main(*sys.argv[1:4])
