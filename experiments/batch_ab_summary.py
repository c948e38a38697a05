"""A/B of the three batched matches between two builds of the library, from the JSON files the
timing scripts write: the parent and the branch in turn, in one session on one GPU.

    for tag in parent1 branch1 parent2 branch2 parent3; do      # NDT2D_HIP_LIB: the parent's library
        for s in starts scans closure; do
            NDT2D_HIP_LIB=... python experiments/${s}_batch_timing.py DIR/$tag.$s.json
        done
    done
    python experiments/batch_ab_summary.py DIR [OUT.json [NOTE]]    # default: profiles/batch_refactor_ab.json

The yardsticks are search_ms and batched_us.  The rule: a value passes where it lies within the
range of parent1 and parent2 widened by that same range on either side -- two parent runs are
the only margin.  It is applied to every branch run, and, as a control of what the rule makes of
run-to-run spread alone, to every further PARENT run (parent3, ...) in the same way: a parent
judged against two other runs of itself.  Every row names all the runs."""
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tables(path):
    """[(map name, rows)] of one timing file."""
    with open(path) as f:
        doc = json.load(f)
    if "maps" in doc:
        return [(m["map"], m["rows"]) for m in doc["maps"]]
    return [("two-scan candidate maps", doc["rows"])]


def verdict(value, lo, hi):
    return "within" if lo - (hi - lo) <= value <= hi + (hi - lo) else "slower" if value > hi else "faster"


def main(directory, path=None, note=None):
    tags = sorted({os.path.basename(p).split(".")[0] for p in glob.glob(os.path.join(directory, "*.starts.json"))})
    judged = [t for t in tags if t not in ("parent1", "parent2")]
    out = dict(experiment="batch_refactor_ab", runs=tags, session="the runs in turn, one session, one MI355X",
               rule="within: lo - (hi - lo) <= value <= hi + (hi - lo), lo / hi of parent1 and parent2; "
                    "applied to the branch runs and, as the control, to the further parent runs", rows=[])
    if note:
        out["note"] = note
    count = {t: dict(within=0, slower=0, faster=0) for t in judged}
    for script in ("starts", "scans", "closure"):
        runs = {t: tables(os.path.join(directory, "%s.%s.json" % (t, script))) for t in tags}
        for i, (name, rows) in enumerate(runs["parent1"]):
            for j, row in enumerate(rows):
                for column in ("search_ms", "batched_us"):
                    values = {t: runs[t][i][1][j][column] for t in tags}
                    lo, hi = sorted((values["parent1"], values["parent2"]))
                    verdicts = {t: verdict(values[t], lo, hi) for t in judged}
                    for t in judged:
                        count[t][verdicts[t]] += 1
                    out["rows"].append(dict(script=script, map=name, K=row["K"], column=column, values=values, verdicts=verdicts))
                    print("%-8s %-24s K %-5d %-10s %s" % (script, name, row["K"], column, "  ".join(
                        "%s %.4f%s" % (t, values[t], " (" + verdicts[t] + ")" if t in verdicts else "") for t in tags)))
    out["counts"] = count
    path = path or os.path.join(ROOT, "profiles", "batch_refactor_ab.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote %s: %s" % (path, json.dumps(count)))


if __name__ == "__main__":
    main(*sys.argv[1:4])
