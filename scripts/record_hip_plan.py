"""Record tests/golden/hip_plan_snapshot.json: the HIP evaluator's plan (allocated bytes, table arenas, op names,
launch log) for every case of tests/test_gpu_plan_snapshot.py, on an MI355X.

The fixture is the expectation of a planner refactor, so it is recorded from the tree whose dash_amd/csrc is the
commit *before* the change and committed unchanged; to check it, run this on that commit and diff:

    python scripts/record_hip_plan.py --commit $(git rev-parse HEAD) [--out PATH]
"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", required=True, help="full hash of the commit whose dash_amd/csrc is being recorded")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "hip_plan_snapshot.json"))
    args = ap.parse_args()
    if not re.fullmatch(r"[0-9a-f]{40}", args.commit):
        ap.error("--commit takes the full 40-digit hash")

    import test_gpu_plan_snapshot as snap
    from dash_amd.native import native

    n = native()
    cases = {}
    for name in snap.CASES:
        cases[name] = snap.snapshot(n, name)  # raises unless the run's labels equal the host evaluator's
        print("%-28s %3d ops %3d launches %12d B" % (name, len(cases[name]["ops"]), len(cases[name]["launches"]),
                                                      cases[name]["device_bytes"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"recorded_from": args.commit, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    seen = set().union(*(snap.op_suffixes(c["ops"]) for c in cases.values()))
    print("suffixes not reached:", sorted(snap.SUFFIXES - seen), "unknown:", sorted(seen - snap.SUFFIXES))


if __name__ == "__main__":
    main()
