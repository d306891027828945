#!/usr/bin/env python3
"""tools/fringe_timing.py and tools/tec_timing.py on a previous build of the library (tools/ab/libgridhip_prev.so, built as
README.md here says) and on the tree's, in the order previous, tree, tree, previous, in one job on one box.  Every row the
two tools write goes to --out with three fields added: `library` ("parent" or "tree"), `run` (1..4) and `tool`.
Then the band test, row by row (a row: one `what` and `case` of a tool; the torch rows are not judged): the tree's median
of either run must lie within the parent's median - of its two runs' medians, so their midpoint - plus or minus the
distance between those two medians, or, where that is smaller, the larger max_ms - min_ms of the parent's two runs.
A tool that fails ends the job at once: nothing more is started on the device.  Exit status 1: a row lies outside.
usage: python tools/ab/delay_ab.py [--out profiles/delay_common_ab.jsonl] [--reps 5]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PREV = os.path.join(HERE, "libgridhip_prev.so")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delay_common_ab.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not os.path.exists(PREV):
        sys.exit(f"{PREV} is missing: build the previous commit's library first (tools/ab/README.md)")
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for run, lib in enumerate(("parent", "tree", "tree", "parent"), 1):
            for tool in ("fringe_timing.py", "tec_timing.py"):
                env = dict(os.environ)
                env.pop("GRIDHIP_LIB", None)
                if lib == "parent":
                    env["GRIDHIP_LIB"] = PREV
                part = os.path.join(tmp, f"{run}_{tool}.jsonl")
                print(f"== run {run}: {tool} on the {lib}'s library", flush=True)
                r = subprocess.run(["timeout", "-k", "10", "900", sys.executable, os.path.join(ROOT, "tools", tool), "--reps",
                                    str(args.reps), "--out", part], env=env, stdout=subprocess.DEVNULL)
                if r.returncode != 0:
                    sys.exit(f"{tool} ended with status {r.returncode}: nothing more is started")
                with open(part) as f:
                    rows += [dict(library=lib, run=run, tool=tool, **json.loads(line)) for line in f]
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    keys = {}
    for r in rows:
        if r["what"] != "torch":
            keys.setdefault((r["tool"], r["what"], r["case"]), []).append(r)
    outside = 0
    for (tool, what, case), rs in keys.items():
        par = [r for r in rs if r["library"] == "parent"]
        pm = [r["median_ms"] for r in par]
        centre, spread = 0.5 * (pm[0] + pm[1]), abs(pm[0] - pm[1])
        band = max(spread, max(r["max_ms"] - r["min_ms"] for r in par))
        new = [r["median_ms"] for r in rs if r["library"] == "tree"]
        ok = all(abs(m - centre) <= band for m in new)
        outside += not ok
        print(f"{what:18s} {case[:36]:36s} parent {pm[0]:9.4f} {pm[1]:9.4f} | tree {new[0]:9.4f} {new[1]:9.4f} | "
              f"{centre:9.4f} +- {band:.4f}  {'inside' if ok else 'OUTSIDE'}", flush=True)
    print("rows outside:", outside)
    return 1 if outside else 0


if __name__ == "__main__":
    sys.exit(main())
